// DISTS around the implicit GEMM (include/mvldm.h, "DISTS"): the glue between the thirteen 3x3 convolutions of the VGG-16 trunk, which
// mvldm_igemm_fwd runs, and the structure / texture statistics of src/evaluation/metrics.py:27-40 (DISTS_pytorch.DISTS().forward).
//
// A pair batch is 2n NHWC images in the compute dtype: rows [0, n) the first input, rows [n, 2n) the second, so that every conv is one
// launch for both and equal images take bit-identical paths (the score of an image against itself is exactly 0).
//   dists_prep     two fp32 NCHW inputs -> one NHWC [2n][h][w][c_pad] tensor, (x - mean_c) / std_c, pad channels zero
//   dists_stats    reads the PRE-activation output of a stage's last conv: ReLU on load, then per pair and channel the five sums over the
//                  pixels  sum a, sum b, sum a^2, sum b^2, sum a b  in fp64 from the first product on.  A lane owns one 16-byte channel
//                  chunk and walks every `rows`-th pixel of the workgroup's band; the lanes that own the same chunk are added through
//                  LDS in row order.  One fp64 partial per (pair, workgroup, sum, channel) goes to the caller's workspace (no atomics).
//   dists_stats0   the same five sums of tap 0, the RAW fp32 NCHW inputs (3 channels), never a rounded copy
//   dists_l2pool   sqrt(sum_{3x3} g_ij relu(f)^2 + 1e-12), g = outer((1,2,1),(1,2,1)) / 16, stride 2, window origin (2y - 1, 2x - 1), zeros
//                  outside: the map the next stage starts from, [2n][ceil(h/2)][ceil(w/2)][C]; fp32, rounded once at the store
//   dists_fold     one workgroup per pair: the partials of each tap and channel in slot order, mean / variance / covariance, the
//                  weighted (1 - S1), (1 - S2) in the direct form, a fixed tree over channels, / (sum alpha + sum beta)
#include <math.h>

#include "common.h"

namespace mvldm {

constexpr int kDistsTaps = 6;
constexpr int kDistsC[kDistsTaps] = {3, 64, 128, 256, 512, 512};     // the raw image, relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
constexpr int kDistsChannels = 1475;
constexpr int kDistsSums = 5;                                        // sum a, sum b, sum a^2, sum b^2, sum a b
constexpr int kDistsPpb0 = 4096;                                     // pixels of one workgroup of tap 0

struct DistsScale {
    float mean[3], std[3];
};

template <typename T>
__global__ __launch_bounds__(256) void dists_prep_kernel(const float* __restrict__ in0, const float* __restrict__ in1, T* __restrict__ dst,
                                                         size_t n_px, int hw, DistsScale k) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // pixel of one input: image * hw + p
    if (idx >= n_px) return;
    const float* src = blockIdx.y ? in1 : in0;
    const size_t img = idx / (size_t)hw, p = idx % (size_t)hw;
    Chunk<T> c;
    c.zero();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c.set(ch, (src[(img * 3 + ch) * (size_t)hw + p] - k.mean[ch]) / k.std[ch]);
    store_chunk(dst + ((size_t)blockIdx.y * n_px + idx) * Chunk<T>::N, c);
}

// workgroup blk of pair img: pixels [blk ppb, min((blk + 1) ppb, hw)); thread t owns chunk t % CP of the pixels p0 + t / CP + k rows
template <typename T>
__global__ __launch_bounds__(256) void dists_stats_kernel(const T* __restrict__ f, int n, int hw, int C, int ppb, int blocks_per_img,
                                                          double* __restrict__ ws, int off, int stride) {
    constexpr int E = Chunk<T>::N;
    __shared__ double s_red[256 * E];
    const int img = blockIdx.x / blocks_per_img, blk = blockIdx.x % blocks_per_img;
    const int CP = C / E, rows = 256 / CP;
    const int j = threadIdx.x % CP, r = threadIdx.x / CP;
    const int p0 = blk * ppb, p1 = min(p0 + ppb, hw);
    const T* fa = f + (size_t)img * hw * C + (size_t)j * E;
    const T* fb = f + (size_t)(n + img) * hw * C + (size_t)j * E;

    double acc[kDistsSums][E];
#pragma unroll
    for (int s = 0; s < kDistsSums; ++s)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[s][e] = 0.0;
    if (r < rows)
        for (int p = p0 + r; p < p1; p += rows) {
            const Chunk<T> ca = load_chunk(fa + (size_t)p * C), cb = load_chunk(fb + (size_t)p * C);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double a = (double)fmaxf(ca.get(e), 0.f), b = (double)fmaxf(cb.get(e), 0.f);
                acc[0][e] += a;
                acc[1][e] += b;
                acc[2][e] += a * a;
                acc[3][e] += b * b;
                acc[4][e] += a * b;
            }
        }
    double* dst = ws + (size_t)img * stride + off + (size_t)blk * kDistsSums * C;
#pragma unroll
    for (int s = 0; s < kDistsSums; ++s) {
        if (r < rows) {
#pragma unroll
            for (int e = 0; e < E; ++e) s_red[r * C + j * E + e] = acc[s][e];
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            double v = s_red[c];
            for (int q = 1; q < rows; ++q) v += s_red[q * C + c];
            dst[s * C + c] = v;
        }
        __syncthreads();
    }
}

// tap 0: the raw inputs, fp32 NCHW [n][3][hw]; thread t walks the pixels p0 + t + 256 k of the workgroup's band
__global__ __launch_bounds__(256) void dists_stats0_kernel(const float* __restrict__ x, const float* __restrict__ y, int hw, int blocks_per_img,
                                                           double* __restrict__ ws, int off, int stride) {
    __shared__ double s_red[4][kDistsSums * 3];
    const int img = blockIdx.x / blocks_per_img, blk = blockIdx.x % blocks_per_img;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = blk * kDistsPpb0, p1 = min(p0 + kDistsPpb0, hw);
    const float* xa = x + (size_t)img * 3 * hw;
    const float* xb = y + (size_t)img * 3 * hw;
    double acc[kDistsSums][3];
#pragma unroll
    for (int s = 0; s < kDistsSums; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[s][c] = 0.0;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a = (double)xa[(size_t)c * hw + p], b = (double)xb[(size_t)c * hw + p];
            acc[0][c] += a;
            acc[1][c] += b;
            acc[2][c] += a * a;
            acc[3][c] += b * b;
            acc[4][c] += a * b;
        }
    }
#pragma unroll
    for (int s = 0; s < kDistsSums; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = wave_sum_d(acc[s][c]);
            if (lane == 0) s_red[wave][s * 3 + c] = v;
        }
    __syncthreads();
    if (threadIdx.x < kDistsSums * 3)
        ws[(size_t)img * stride + off + (size_t)blk * kDistsSums * 3 + threadIdx.x] =
            (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

// one thread per 16-byte chunk of the output: nine chunk loads (fewer at the border), fp32 sum in window order, one rounding at the store
template <typename T>
__global__ __launch_bounds__(256) void dists_l2pool_kernel(const T* __restrict__ f, T* __restrict__ out, size_t chunks, int h, int w, int oh, int ow,
                                                           int C) {
    constexpr int E = Chunk<T>::N;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // ((image * oh + oy) * ow + ox) * CP + j
    if (idx >= chunks) return;
    const int CP = C / E;
    const int j = (int)(idx % CP);
    size_t t = idx / CP;
    const int ox = (int)(t % ow);
    t /= ow;
    const int oy = (int)(t % oh);
    const size_t img = t / oh;
    const T* src = f + img * (size_t)h * w * C + (size_t)j * E;
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int y = 2 * oy - 1 + dy;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int x = 2 * ox - 1 + dx;
            if (y >= 0 && y < h && x >= 0 && x < w) {
                const float g = (float)((dy == 1 ? 2 : 1) * (dx == 1 ? 2 : 1)) * 0.0625f;
                const Chunk<T> c = load_chunk(src + ((size_t)y * w + x) * C);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float v = fmaxf(c.get(e), 0.f);
                    acc[e] += g * (v * v);
                }
            }
        }
    }
    Chunk<T> o;
#pragma unroll
    for (int e = 0; e < E; ++e) o.set(e, sqrtf(acc[e] + 1e-12f));
    store_chunk(out + idx * E, o);
}

struct DistsFold {
    int slots[kDistsTaps], off[kDistsTaps];     // workgroups of a tap, its first double within a pair's region
    double px[kDistsTaps];                      // pixels of its map
    int stride;                                 // doubles per pair
};

// one workgroup per pair.  Thread t takes the channels t, t + 256, ... of every tap in tap order; the 256 running sums meet in a halving tree.
__global__ __launch_bounds__(256) void dists_fold_kernel(const double* __restrict__ ws, DistsFold L, const float* __restrict__ alpha,
                                                         const float* __restrict__ beta, float* __restrict__ out) {
    __shared__ double s_num[256], s_w[256];
    const double* base = ws + (size_t)blockIdx.x * L.stride;
    const double c1 = 1e-6, c2 = 1e-6;
    double num = 0.0, wsum = 0.0;
    int ch0 = 0;
    for (int k = 0; k < kDistsTaps; ++k) {
        const int C = kDistsC[k];
        const double* p = base + L.off[k];
        for (int c = threadIdx.x; c < C; c += 256) {
            double sum[kDistsSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int b = 0; b < L.slots[k]; ++b)
#pragma unroll
                for (int s = 0; s < kDistsSums; ++s) sum[s] += p[((size_t)b * kDistsSums + s) * C + c];
            const double mx = sum[0] / L.px[k], my = sum[1] / L.px[k];
            const double vx = sum[2] / L.px[k] - mx * mx, vy = sum[3] / L.px[k] - my * my, cov = sum[4] / L.px[k] - mx * my;
            const double d1 = ((mx - my) * (mx - my)) / (mx * mx + my * my + c1);              // 1 - S1
            const double d2 = (vx + vy - 2.0 * cov) / (vx + vy + c2);                          // 1 - S2
            const double a = (double)alpha[ch0 + c], b = (double)beta[ch0 + c];
            num += a * d1 + b * d2;
            wsum += a + b;
        }
        ch0 += C;
    }
    s_num[threadIdx.x] = num;
    s_w[threadIdx.x] = wsum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            s_num[threadIdx.x] += s_num[threadIdx.x + o];
            s_w[threadIdx.x] += s_w[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(s_num[0] / s_w[0]);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int dists_ppb(int c) { return c == 3 ? kDistsPpb0 : max(256, 32768 / c); }     // pixels of one workgroup: 512 at C = 64, else 256

int dists_stat_slots(int h, int w, int c) {
    if (h < 1 || w < 1 || !(c == 3 || channels_ok(c))) return 0;
    const long long px = (long long)h * w;
    if (px > 0x7FFFFFFF) return 0;
    return (int)((px + dists_ppb(c) - 1) / dists_ppb(c));
}

// doubles per pair; fills the fold's table.  0: refused
static long long dists_layout(int h, int w, DistsFold* L) {
    if (h < 1 || w < 1) return 0;
    long long total = 0;
    int hk = h, wk = w;
    for (int k = 0; k < kDistsTaps; ++k) {
        if (k >= 2) {
            hk = (hk + 1) / 2;
            wk = (wk + 1) / 2;
        }
        const int s = dists_stat_slots(hk, wk, kDistsC[k]);
        if (s == 0) return 0;
        if (L) {
            L->slots[k] = s;
            L->off[k] = (int)total;
            L->px[k] = (double)hk * (double)wk;
        }
        total += (long long)s * kDistsSums * kDistsC[k];
        if (total > 0x7FFFFFFF) return 0;
    }
    if (L) L->stride = (int)total;
    return total;
}

size_t dists_workspace_bytes(int n_img, int h, int w) {
    if (n_img < 1) return 0;
    return (size_t)n_img * (size_t)dists_layout(h, w, nullptr) * sizeof(double);
}

int dists_prep_run(const float* in0, const float* in1, void* dst, int n_img, int h, int w, int c_pad, int dtype, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "dists_prep: n_img %d", n_img);
    MVLDM_REQUIRE(h >= 1 && w >= 1, "dists_prep: image %d x %d", h, w);
    MVLDM_REQUIRE(dtype_ok(dtype), "dists_prep: unknown dtype %d", dtype);
    MVLDM_REQUIRE(c_pad == (dtype == MVLDM_F32 ? 4 : 8), "dists_prep: c_pad %d is not the 16-byte padding of 3 channels in dtype %d", c_pad, dtype);
    MVLDM_REQUIRE((long long)h * w <= 0x7FFFFFFF, "dists_prep: a %d x %d image is too large", h, w);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(in0, 4) && aligned(in1, 4) && aligned(dst, 16), "dists_prep: null or unaligned pointer");
    const size_t n_px = (size_t)n_img * h * w, blocks = (n_px + 255) / 256;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "dists_prep: %zu workgroups", blocks);
    const DistsScale k = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dists_prep_kernel<T>, dim3((unsigned)blocks, 2), dim3(256), 0, s, in0, in1, (T*)dst, n_px, h * w, k);
        return check_launch();
    });
}

int dists_stats_run(const void* feat, const void* feat_b, int n_img, int h, int w, int c, int dtype, double* ws, size_t ws_bytes, int off,
                    int stride, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0 && h >= 1 && w >= 1, "dists_stats: n_img %d, map %d x %d", n_img, h, w);
    MVLDM_REQUIRE(c == 3 || channels_ok(c), "dists_stats: C = %d channels; multiples of 64 up to 512 (or the 3 of the raw image) are supported", c);
    MVLDM_REQUIRE(dtype_ok(dtype), "dists_stats: unknown dtype %d", dtype);
    MVLDM_REQUIRE(c != 3 || dtype == MVLDM_F32, "dists_stats: the raw image (C = 3) is fp32 NCHW, not dtype %d", dtype);
    const int blocks_per_img = dists_stat_slots(h, w, c);
    MVLDM_REQUIRE(blocks_per_img > 0, "dists_stats: a %d x %d map is too large", h, w);
    const long long mine = (long long)blocks_per_img * kDistsSums * c;
    MVLDM_REQUIRE(off >= 0 && stride >= 1 && off + mine <= stride, "dists_stats: partials [%d, %d + %lld) of %d doubles per pair", off, off, mine,
                  stride);
    const size_t need = (size_t)n_img * stride * sizeof(double);
    MVLDM_REQUIRE(ws_bytes >= need, "dists_stats: workspace of %zu bytes, need %zu", ws_bytes, need);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(ws, 8), "dists_stats: null or unaligned workspace pointer");
    const size_t blocks = (size_t)n_img * blocks_per_img;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "dists_stats: %zu workgroups", blocks);
    if (c == 3) {
        MVLDM_REQUIRE(aligned(feat, 4) && aligned(feat_b, 4), "dists_stats: null or unaligned pointer (C = 3 takes both fp32 NCHW inputs)");
        hipLaunchKernelGGL(dists_stats0_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)feat, (const float*)feat_b, h * w, blocks_per_img,
                           ws, off, stride);
        return check_launch();
    }
    MVLDM_REQUIRE(aligned(feat, 16), "dists_stats: null or unaligned pointer");
    MVLDM_REQUIRE(feat_b == nullptr, "dists_stats: a feature map is one [2 n_img] batch; the second pointer is for the raw image (C = 3) only");
    const int ppb = dists_ppb(c);
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dists_stats_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)feat, n_img, h * w, c, ppb, blocks_per_img, ws, off,
                           stride);
        return check_launch();
    });
}

int dists_l2pool_run(const void* feat, void* out, int n_img, int h, int w, int c, int dtype, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0 && h >= 1 && w >= 1, "dists_l2pool: n_img %d, map %d x %d", n_img, h, w);
    MVLDM_REQUIRE(channels_ok(c), "dists_l2pool: C = %d channels; multiples of 64 up to 512 are supported", c);
    MVLDM_REQUIRE(dtype_ok(dtype), "dists_l2pool: unknown dtype %d", dtype);
    MVLDM_REQUIRE((long long)h * w <= 0x7FFFFFFF, "dists_l2pool: a %d x %d map is too large", h, w);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(feat, 16) && aligned(out, 16), "dists_l2pool: null or unaligned pointer");
    const int oh = (h + 1) / 2, ow = (w + 1) / 2;
    const size_t chunks = (size_t)2 * n_img * oh * ow * (c / (dtype == MVLDM_F32 ? 4 : 8)), blocks = (chunks + 255) / 256;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "dists_l2pool: %zu workgroups", blocks);
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dists_l2pool_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)feat, (T*)out, chunks, h, w, oh, ow, c);
        return check_launch();
    });
}

int dists_fold_run(const double* ws, size_t ws_bytes, int n_img, int h, int w, const float* alpha, const float* beta, float* out, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "dists_fold: n_img %d", n_img);
    MVLDM_REQUIRE(h >= 1 && w >= 1, "dists_fold: image %d x %d", h, w);
    DistsFold L;
    const long long stride = dists_layout(h, w, &L);
    MVLDM_REQUIRE(stride > 0, "dists_fold: a %d x %d image is too large", h, w);
    const size_t need = (size_t)n_img * stride * sizeof(double);
    MVLDM_REQUIRE(ws_bytes >= need, "dists_fold: workspace of %zu bytes, need %zu", ws_bytes, need);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(ws, 8) && aligned(alpha, 4) && aligned(beta, 4) && aligned(out, 4), "dists_fold: null or unaligned pointer");
    hipLaunchKernelGGL(dists_fold_kernel, dim3(n_img), dim3(256), 0, s, ws, L, alpha, beta, out);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_dists_workspace_bytes(int n_img, int h, int w) { return dists_workspace_bytes(n_img, h, w); }
extern "C" int mvldm_dists_stat_slots(int h, int w, int c) { return dists_stat_slots(h, w, c); }
extern "C" int mvldm_dists_prep(const float* in0, const float* in1, void* dst, int n_img, int h, int w, int c_pad, int dtype, mvldm_stream_t stream) {
    return dists_prep_run(in0, in1, dst, n_img, h, w, c_pad, dtype, (hipStream_t)stream);
}
extern "C" int mvldm_dists_stats(const void* feat, const void* feat_b, int n_img, int h, int w, int c, int dtype, double* workspace,
                                 size_t workspace_bytes, int offset, int doubles_per_pair, mvldm_stream_t stream) {
    return dists_stats_run(feat, feat_b, n_img, h, w, c, dtype, workspace, workspace_bytes, offset, doubles_per_pair, (hipStream_t)stream);
}
extern "C" int mvldm_dists_l2pool(const void* feat, void* out, int n_img, int h, int w, int c, int dtype, mvldm_stream_t stream) {
    return dists_l2pool_run(feat, out, n_img, h, w, c, dtype, (hipStream_t)stream);
}
extern "C" int mvldm_dists_fold(const double* workspace, size_t workspace_bytes, int n_img, int h, int w, const float* alpha, const float* beta,
                                float* out, mvldm_stream_t stream) {
    return dists_fold_run(workspace, workspace_bytes, n_img, h, w, alpha, beta, out, (hipStream_t)stream);
}
