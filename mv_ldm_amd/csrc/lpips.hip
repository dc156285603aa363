// LPIPS(net="vgg") around the implicit GEMM (include/mvldm.h, "LPIPS"): the glue between the thirteen 3x3 convolutions of the VGG-16 trunk,
// which mvldm_igemm_fwd runs, and the per-pixel distance of src/evaluation/metrics.py:43-54.
//
// A pair batch is 2n NHWC images in the compute dtype: rows [0, n) the first input, rows [n, 2n) the second, so that every conv is one
// launch for both and equal images take bit-identical paths (the distance of an image to itself is exactly 0).
//   lpips_prep   two fp32 NCHW inputs -> one NHWC [2n][h][w][c_pad] tensor, ((2x - 1) - shift_c) / scale_c, pad channels zero
//   lpips_relu   in-place ReLU of a conv output that is no tap, 16-byte accesses
//   lpips_tap    reads the PRE-activation output of a stage's last conv once: ReLU, the channel-normalised weighted squared difference of
//                pair (i, n + i) per pixel, and the 2x2 max-pooled ReLU map the next stage starts from -- the full-resolution ReLU map is
//                never written.  One fp64 partial per workgroup goes to the caller's workspace (no atomics).
//   lpips_fold   one workgroup per pair: out[i] = sum over the five taps of (sum of the tap's partials) / (h_l w_l), in a fixed order.
//
// The tap: a group of G lanes owns one 2x2 pixel quad of one pair (both images: 8 pixel rows of C channels); a lane holds the same
// 16-byte channel chunk(s) of all 8, so the channel norms are sums across the group, the distance and the quad's maximum stay in
// registers.  G = the chunks of a pixel (C / 4 in f32, C / 8 in 16 bit) rounded up to a power of two, at most 64; a wave takes 64 / G
// quads per pass.  An odd last row / column is half a quad: its pixels count in the distance and are not pooled.
#include <math.h>

#include "common.h"

namespace mvldm {

constexpr int kLpipsLayers = 5;
constexpr int kLpipsC[kLpipsLayers] = {64, 128, 256, 512, 512};     // relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
constexpr int kLpipsMinEdge = 16;                                   // four 2x2 pools must leave one pixel

struct LpipsScale {
    float shift[3], scale[3];
};

template <typename T>
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ in0, const float* __restrict__ in1, T* __restrict__ dst,
                                                         size_t n_px, int hw, LpipsScale k, int normalize) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // pixel of one input: image * hw + p
    if (idx >= n_px) return;
    const float* src = blockIdx.y ? in1 : in0;
    const size_t img = idx / (size_t)hw, p = idx % (size_t)hw;
    Chunk<T> c;
    c.zero();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float x = src[(img * 3 + ch) * (size_t)hw + p];
        if (normalize) x = 2.f * x - 1.f;
        c.set(ch, (x - k.shift[ch]) / k.scale[ch]);
    }
    store_chunk(dst + ((size_t)blockIdx.y * n_px + idx) * Chunk<T>::N, c);
}

template <typename T> __global__ __launch_bounds__(256) void lpips_relu_kernel(T* __restrict__ x, size_t chunks) {
    constexpr int E = Chunk<T>::N;
    const size_t i0 = (size_t)blockIdx.x * 1024 + threadIdx.x;
    Chunk<T> c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (i0 + u * 256 < chunks) c[u] = load_chunk(x + (i0 + u * 256) * E);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (i0 + u * 256 < chunks) {
#pragma unroll
            for (int e = 0; e < E; ++e) c[u].set(e, fmaxf(c[u].get(e), 0.f));
            store_chunk(x + (i0 + u * 256) * E, c[u]);
        }
}

__device__ __forceinline__ float group_sum(float v, int G) {        // butterfly over G (power of two) neighbouring lanes: every lane gets the sum
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// KC: 16-byte chunks of one pixel a lane holds (chunk sub + k G, k < KC)
template <typename T, int KC>
__global__ __launch_bounds__(256) void lpips_tap_kernel(const T* __restrict__ f, const float* __restrict__ lw, T* __restrict__ pooled, int n, int h,
                                                        int w, int C, int G, int qpb, int blocks_per_img, double* __restrict__ ws, int slot0,
                                                        int slots) {
    constexpr int E = Chunk<T>::N;
    __shared__ double s_red[4];
    const int img = blockIdx.x / blocks_per_img, blk = blockIdx.x % blocks_per_img;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / G, sub = lane % G, QW = 64 / G;
    const int CP = C / E;
    const int qcols = (w + 1) >> 1, Q = qcols * ((h + 1) >> 1);
    const int ph = h >> 1, pw = w >> 1;
    const int q0 = blk * qpb, q1 = min(q0 + qpb, Q);
    const T* fa = f + (size_t)img * h * w * C;
    const T* fb = f + (size_t)(n + img) * h * w * C;

    float wgt[KC][E];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int j = sub + k * G;
#pragma unroll
        for (int e = 0; e < E; e += 4) {
            const f32x4 v = j < CP ? *reinterpret_cast<const f32x4*>(lw + (size_t)j * E + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) wgt[k][e + i] = v[i];
        }
    }

    double acc = 0.0;
    for (int base = q0; base < q1; base += 4 * QW) {                // the same trip count for every lane of the workgroup
        const int q = base + wave * QW + grp;
        const bool qv = q < q1;
        const int qy = qv ? q / qcols : 0, qx = qv ? q % qcols : 0;
        float a[4][KC][E], b[4][KC][E];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int y = 2 * qy + (p >> 1), x = 2 * qx + (p & 1);
            const bool ok = qv && y < h && x < w;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const int j = sub + k * G;
                Chunk<T> ca, cb;
                ca.zero();
                cb.zero();
                if (ok && j < CP) {
                    const size_t off = ((size_t)y * w + x) * C + (size_t)j * E;
                    ca = load_chunk(fa + off);
                    cb = load_chunk(fb + off);
                }
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    a[p][k][e] = fmaxf(ca.get(e), 0.f);
                    b[p][k][e] = fmaxf(cb.get(e), 0.f);
                }
            }
        }
        float d = 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int k = 0; k < KC; ++k)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    sa += a[p][k][e] * a[p][k][e];
                    sb += b[p][k][e] * b[p][k][e];
                }
            sa = group_sum(sa, G);
            sb = group_sum(sb, G);
            // a pixel outside the map, or one whose channels are all <= 0, has norm 0: 0 * 1e10 = 0, never NaN
            const float ia = 1.f / (sqrtf(sa) + 1e-10f), ib = 1.f / (sqrtf(sb) + 1e-10f);
#pragma unroll
            for (int k = 0; k < KC; ++k)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float t = a[p][k][e] * ia - b[p][k][e] * ib;
                    d += wgt[k][e] * (t * t);
                }
        }
        if (pooled != nullptr && qv && 2 * qy + 1 < h && 2 * qx + 1 < w) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const int j = sub + k * G;
                if (j < CP) {
                    Chunk<T> ma, mb;
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        ma.set(e, fmaxf(fmaxf(a[0][k][e], a[1][k][e]), fmaxf(a[2][k][e], a[3][k][e])));
                        mb.set(e, fmaxf(fmaxf(b[0][k][e], b[1][k][e]), fmaxf(b[2][k][e], b[3][k][e])));
                    }
                    const size_t px = (size_t)qy * pw + qx, pc = (size_t)j * E;
                    store_chunk(pooled + ((size_t)img * ph * pw + px) * C + pc, ma);
                    store_chunk(pooled + ((size_t)(n + img) * ph * pw + px) * C + pc, mb);
                }
            }
        }
        acc += (double)wave_sum(d);
    }
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws[(size_t)img * slots + slot0 + blk] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

struct LpipsFold {
    int cnt[kLpipsLayers];
    double px[kLpipsLayers];
};

// one workgroup per pair: the partials of each tap strided over 256 threads, a fixed halving tree, the five layer means in layer order
__global__ __launch_bounds__(256) void lpips_fold_kernel(const double* __restrict__ ws, int slots, LpipsFold L, float* __restrict__ out) {
    __shared__ double s[256];
    const double* p = ws + (size_t)blockIdx.x * slots;
    double total = 0.0;
    for (int l = 0; l < kLpipsLayers; ++l) {
        double v = 0.0;
        for (int k = threadIdx.x; k < L.cnt[l]; k += 256) v += p[k];
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) total += s[0] / L.px[l];
        __syncthreads();
        p += L.cnt[l];
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)total;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int lpips_qpb(int c) { return max(8, (4096 / c) & ~7); }      // quads of one workgroup: 64 at C = 64 ... 8 at C = 512, whatever the dtype

int lpips_tap_slots(int h, int w, int c) {
    if (h < 1 || w < 1 || !channels_ok(c)) return 0;
    const long long Q = (long long)((h + 1) / 2) * ((w + 1) / 2);
    const long long blocks = (Q + lpips_qpb(c) - 1) / lpips_qpb(c);
    return blocks > 0x7FFFFFFF ? 0 : (int)blocks;
}

static long long lpips_slots(int h, int w, int* cnt) {
    long long total = 0;
    for (int l = 0; l < kLpipsLayers; ++l) {
        const int s = lpips_tap_slots(h >> l, w >> l, kLpipsC[l]);
        if (cnt) cnt[l] = s;
        total += s;
    }
    return total;
}

size_t lpips_workspace_bytes(int n_img, int h, int w) {
    if (n_img < 1 || h < kLpipsMinEdge || w < kLpipsMinEdge) return 0;
    const long long slots = lpips_slots(h, w, nullptr);
    return slots > 0x7FFFFFFF ? 0 : (size_t)n_img * slots * sizeof(double);
}

int lpips_prep_run(const float* in0, const float* in1, void* dst, int n_img, int h, int w, int c_pad, int dtype, int normalize, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "lpips_prep: n_img %d", n_img);
    MVLDM_REQUIRE(h >= kLpipsMinEdge && w >= kLpipsMinEdge, "lpips_prep: a %d x %d image leaves nothing after four 2x2 pool stages (at least %d x %d)",
                  h, w, kLpipsMinEdge, kLpipsMinEdge);
    MVLDM_REQUIRE(dtype_ok(dtype), "lpips_prep: unknown dtype %d", dtype);
    MVLDM_REQUIRE(c_pad == (dtype == MVLDM_F32 ? 4 : 8), "lpips_prep: c_pad %d is not the 16-byte padding of 3 channels in dtype %d", c_pad, dtype);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(in0 && in1 && dst, "lpips_prep: null pointer");
    const size_t n_px = (size_t)n_img * h * w, blocks = (n_px + 255) / 256;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "lpips_prep: %zu workgroups", blocks);
    const LpipsScale k = {{-0.030f, -0.088f, -0.188f}, {0.458f, 0.448f, 0.450f}};
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(lpips_prep_kernel<T>, dim3((unsigned)blocks, 2), dim3(256), 0, s, in0, in1, (T*)dst, n_px, h * w, k, normalize);
        return check_launch();
    });
}

int lpips_relu_run(void* x, size_t n, int dtype, hipStream_t s) {
    MVLDM_REQUIRE(dtype_ok(dtype), "lpips_relu: unknown dtype %d", dtype);
    const size_t epc = dtype == MVLDM_F32 ? 4 : 8;
    MVLDM_REQUIRE(n % epc == 0, "lpips_relu: %zu elements are no whole number of 16-byte chunks", n);
    if (n == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(x, 16), "lpips_relu: null or unaligned pointer");
    const size_t chunks = n / epc, blocks = (chunks + 1023) / 1024;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "lpips_relu: %zu workgroups", blocks);
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(lpips_relu_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (T*)x, chunks);
        return check_launch();
    });
}

int lpips_tap_run(const void* feat, const float* weight, void* pooled, int n_img, int h, int w, int c, int dtype, double* ws, size_t ws_bytes,
                  int slot0, int slots, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0 && h >= 1 && w >= 1, "lpips_tap: n_img %d, map %d x %d", n_img, h, w);
    MVLDM_REQUIRE(channels_ok(c), "lpips_tap: C = %d channels; multiples of 64 up to 512 are supported", c);
    MVLDM_REQUIRE(dtype_ok(dtype), "lpips_tap: unknown dtype %d", dtype);
    const int blocks_per_img = lpips_tap_slots(h, w, c);
    MVLDM_REQUIRE(blocks_per_img > 0, "lpips_tap: a %d x %d map is too large", h, w);
    MVLDM_REQUIRE(slot0 >= 0 && slots >= 1 && (long long)slot0 + blocks_per_img <= slots, "lpips_tap: partials [%d, %d + %d) of %d per image", slot0,
                  slot0, blocks_per_img, slots);
    const size_t need = (size_t)n_img * slots * sizeof(double);
    MVLDM_REQUIRE(ws_bytes >= need, "lpips_tap: workspace of %zu bytes, need %zu", ws_bytes, need);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(feat && weight && ws, "lpips_tap: null pointer");
    const size_t blocks = (size_t)n_img * blocks_per_img;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "lpips_tap: %zu workgroups", blocks);
    const int cp = c / (dtype == MVLDM_F32 ? 4 : 8);
    int G = 1;
    while (G < cp && G < 64) G <<= 1;
    const int kc = (cp + G - 1) / G;        // 1, or 2 for f32 above 256 channels
    const int qpb = lpips_qpb(c);
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        if constexpr (sizeof(T) == 4) {
            if (kc == 2) {
                hipLaunchKernelGGL((lpips_tap_kernel<T, 2>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)feat, weight, (T*)pooled, n_img, h, w, c,
                                   G, qpb, blocks_per_img, ws, slot0, slots);
                return check_launch();
            }
        }
        hipLaunchKernelGGL((lpips_tap_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)feat, weight, (T*)pooled, n_img, h, w, c, G,
                           qpb, blocks_per_img, ws, slot0, slots);
        return check_launch();
    });
}

int lpips_fold_run(const double* ws, size_t ws_bytes, int n_img, int h, int w, float* out, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "lpips_fold: n_img %d", n_img);
    MVLDM_REQUIRE(h >= kLpipsMinEdge && w >= kLpipsMinEdge, "lpips_fold: a %d x %d image leaves nothing after four 2x2 pool stages (at least %d x %d)",
                  h, w, kLpipsMinEdge, kLpipsMinEdge);
    LpipsFold L;
    const long long slots = lpips_slots(h, w, L.cnt);
    MVLDM_REQUIRE(slots <= 0x7FFFFFFF, "lpips_fold: %lld partials per image", slots);
    const size_t need = (size_t)n_img * slots * sizeof(double);
    MVLDM_REQUIRE(ws_bytes >= need, "lpips_fold: workspace of %zu bytes, need %zu", ws_bytes, need);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(ws && out, "lpips_fold: null pointer");
    for (int l = 0; l < kLpipsLayers; ++l) L.px[l] = (double)(h >> l) * (double)(w >> l);
    hipLaunchKernelGGL(lpips_fold_kernel, dim3(n_img), dim3(256), 0, s, ws, (int)slots, L, out);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_lpips_workspace_bytes(int n_img, int h, int w) { return lpips_workspace_bytes(n_img, h, w); }
extern "C" int mvldm_lpips_tap_slots(int h, int w, int c) { return lpips_tap_slots(h, w, c); }
extern "C" int mvldm_lpips_prep(const float* in0, const float* in1, void* dst, int n_img, int h, int w, int c_pad, int dtype, int normalize,
                                mvldm_stream_t stream) {
    return lpips_prep_run(in0, in1, dst, n_img, h, w, c_pad, dtype, normalize, (hipStream_t)stream);
}
extern "C" int mvldm_lpips_relu(void* x, size_t n, int dtype, mvldm_stream_t stream) { return lpips_relu_run(x, n, dtype, (hipStream_t)stream); }
extern "C" int mvldm_lpips_tap(const void* feat, const float* weight, void* pooled, int n_img, int h, int w, int c, int dtype, double* workspace,
                               size_t workspace_bytes, int slot0, int slots_per_image, mvldm_stream_t stream) {
    return lpips_tap_run(feat, weight, pooled, n_img, h, w, c, dtype, workspace, workspace_bytes, slot0, slots_per_image, (hipStream_t)stream);
}
extern "C" int mvldm_lpips_fold(const double* workspace, size_t workspace_bytes, int n_img, int h, int w, float* out, mvldm_stream_t stream) {
    return lpips_fold_run(workspace, workspace_bytes, n_img, h, w, out, (hipStream_t)stream);
}
