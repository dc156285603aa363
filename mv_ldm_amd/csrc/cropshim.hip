// The crop shim (include/mvldm.h, "Crop shim"): what `rescale_and_crop` (src/dataset/shims/crop_shim.py:11-75) does to every image a
// dataset reader hands on -- quantise to bytes, PIL's Image.resize(LANCZOS) on the 8-bit image, centre crop, / 255 -- with the crop
// folded into the two passes, so that only the pixels that survive it are computed.
//   PIL's 8-bit resample is integer arithmetic: per axis the Lanczos-3 weights of output i (precompute_coeffs, in double) are rounded to
//   22 fractional bits (normalize_coeffs_8bpc), a pixel is clip((2^21 + sum_t px[xmin + t] k[t]) >> 22, 0, 255) in int32, horizontally
//   first with a uint8 image between the passes.  The tables are built on the host, operation for operation as PIL builds them
//   (-ffp-contract=off), and kept on the device per (device, in, out, first output, outputs): the first use of a geometry uploads them,
//   every later call is two launches and nothing else.  A pass whose size stays runs on the identity table (one tap of weight 2^22:
//   (2^21 + px 2^22) >> 22 = px), i.e. as the copy / crop PIL's skipped pass amounts to.
//   crop_h_kernel   one workgroup per (image, source row the vertical pass reads): the row's bytes under the crop window's taps go to
//                   LDS by channel (a uint8 NHWC row in whole dwords, a float NCHW row quantised as the reference does: x 255 in fp32,
//                   clamp, truncate), then every thread makes 4 adjacent bytes of one channel and stores them as one dword of the
//                   workspace [n][3][rows][roundup(w_out, 4)].  An image flagged in `flip` (mvldm_crop_shim_flip: the augmentation shim's
//                   image.flip(-1) before the resize) is staged mirrored -- the same bytes, reversed slots -- and nothing else changes:
//                   PIL's tables are not mirror-symmetric (xmin truncates, an odd crop margin is floored), so the flip cannot follow
//                   the resize
//   crop_v_kernel   one workgroup per (image, output row): a thread reads one dword of every tap row, keeps 4 int32 sums and writes
//                   4 floats byte / 255 (one 16-byte store where the row length and the pointer allow)
#include <math.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "common.h"

namespace mvldm {

constexpr int kCsBits = 22;                 // PIL's PRECISION_BITS (32 - 8 - 2)
constexpr int kCsMaxW = 16384;              // widest source row: its three channels fill 48 KiB of LDS
constexpr int kCsMaxH = 65536;

// ---- geometry and tables (host) --------------------------------------------------------------------------------------------------
struct CropGeom {
    int h_s, w_s, row, col;
};
// rescale_and_crop's sizes: scale = max(h_out / h, w_out / w), rounded half to even as Python's round() does
static bool crop_geometry(int h, int w, int h_out, int w_out, CropGeom* g) {
    if (h < 1 || w < 1 || h_out < 1 || w_out < 1 || h_out > h || w_out > w) return false;
    const double sh = (double)h_out / (double)h, sw = (double)w_out / (double)w;
    const double scale = sh > sw ? sh : sw;
    g->h_s = (int)nearbyint((double)h * scale);
    g->w_s = (int)nearbyint((double)w * scale);
    if (g->h_s != h_out && g->w_s != w_out) return false;
    if (g->h_s < h_out || g->w_s < w_out) return false;
    g->row = (g->h_s - h_out) / 2;
    g->col = (g->w_s - w_out) / 2;
    return true;
}

static double pil_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static double pil_lanczos(double x) {
    if (-3.0 <= x && x < 3.0) return pil_sinc(x) * pil_sinc(x / 3);
    return 0.0;
}

struct CropAxis {                           // outputs [off, off + count) of an axis resized n_in -> n_out
    int ksize = 0, lo = 0, hi = 0;          // taps per output; the source indices any output reads: [lo, hi)
    std::vector<int32_t> bounds, coefs;     // [count][2] (first tap, taps), [count][ksize]
};
static CropAxis crop_axis_build(int n_in, int n_out, int off, int count) {
    CropAxis a;
    a.bounds.resize((size_t)count * 2);
    if (n_in == n_out) {                    // the pass PIL skips
        a.ksize = 1;
        a.coefs.assign((size_t)count, 1 << kCsBits);
        for (int i = 0; i < count; ++i) {
            a.bounds[2 * i] = off + i;
            a.bounds[2 * i + 1] = 1;
        }
        a.lo = off;
        a.hi = off + count;
        return a;
    }
    const double scale = (double)n_in / (double)n_out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale, ss = 1.0 / filterscale;
    a.ksize = (int)ceil(support) * 2 + 1;
    a.coefs.assign((size_t)count * a.ksize, 0);
    std::vector<double> k(a.ksize);
    a.lo = n_in;
    a.hi = 0;
    for (int i = 0; i < count; ++i) {
        const double center = ((double)(off + i) + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            k[x] = pil_lanczos(((double)(x + xmin) - center + 0.5) * ss);
            ww += k[x];
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            a.coefs[(size_t)i * a.ksize + x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (double)(1 << kCsBits)) : (int32_t)(0.5 + k[x] * (double)(1 << kCsBits));
        }
        a.bounds[2 * i] = xmin;
        a.bounds[2 * i + 1] = xmax;
        if (xmin < a.lo) a.lo = xmin;
        if (xmin + xmax > a.hi) a.hi = xmin + xmax;
    }
    return a;
}

struct CropTable {                          // a CropAxis on a device: bounds then coefs in one allocation, kept for the process
    int ksize, lo, hi;
    const int32_t *bounds, *coefs;
};
static std::mutex g_cs_mutex;
static std::map<std::tuple<int, int, int, int, int>, CropTable> g_cs_tables;

static int crop_table(int n_in, int n_out, int off, int count, hipStream_t s, CropTable* out) {
    int dev = 0;
    MVLDM_CHECK_HIP(hipGetDevice(&dev));
    const auto key = std::make_tuple(dev, n_in, n_out, off, count);
    std::lock_guard<std::mutex> lock(g_cs_mutex);
    auto it = g_cs_tables.find(key);
    if (it != g_cs_tables.end()) {
        *out = it->second;
        return MVLDM_OK;
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    MVLDM_CHECK_HIP(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return set_error(MVLDM_ERR_UNSUPPORTED, "crop_shim: the tables of axis %d -> %d [%d, %d) are not on the device yet; call once outside the capture",
                         n_in, n_out, off, off + count);
    const CropAxis a = crop_axis_build(n_in, n_out, off, count);
    const size_t nb = a.bounds.size(), nc = a.coefs.size();
    int32_t* d = nullptr;
    MVLDM_CHECK_HIP(hipMalloc((void**)&d, (nb + nc) * sizeof(int32_t)));
    hipError_t e = hipMemcpy(d, a.bounds.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + nb, a.coefs.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return set_error(MVLDM_ERR_HIP, "crop_shim: table upload: %s", hipGetErrorString(e));
    }
    const CropTable t{a.ksize, a.lo, a.hi, d, d + nb};
    g_cs_tables.emplace(key, t);
    *out = t;
    return MVLDM_OK;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cs_pixel(int acc) {
    acc >>= kCsBits;                        // arithmetic: the negative lobes can take a sum below zero
    return (uint32_t)min(max(acc, 0), 255);
}

// Workgroup b: image b / rows, source row y0 + b % rows.  x0, x1: the source columns the window's taps read; LDS [3][x1 - x0] bytes.
// flip (may be null): one byte per image; an image whose byte is set is read mirrored along w -- the window [x0, x1) is taken in flipped
// coordinates, i.e. source columns [w - x1, w - x0) are staged and column p lands in slot w - 1 - p - x0, so LDS holds the row of
// image.flip(-1) and everything after the staging is the same.
template <bool U8>
__global__ __launch_bounds__(256) void crop_h_kernel(const void* __restrict__ src, size_t src_bytes, uint8_t* __restrict__ tmp, int h, int w, int rows,
                                                     int y0, int x0, int x1, int w_out, int wp, int ksize, const int32_t* __restrict__ bounds,
                                                     const int32_t* __restrict__ coefs, const uint8_t* __restrict__ flip) {
    extern __shared__ uint8_t cs_row[];
    const int wl = x1 - x0;
    const size_t img = blockIdx.x / (unsigned)rows;
    const int yy = (int)(blockIdx.x % (unsigned)rows), y = y0 + yy;
    const bool mirror = flip != nullptr && flip[img] != 0;
    const int s0 = mirror ? w - x1 : x0;    // the first source column staged
    if (U8) {                               // bytes [lo, hi) of the interleaved image, fetched as the dwords that cover them
        const size_t base = (img * h + y) * (size_t)w * 3, lo = base + (size_t)s0 * 3, hi = lo + (size_t)wl * 3;
        const uint8_t* p = (const uint8_t*)src;
        for (size_t d = lo / 4 + threadIdx.x; d * 4 < hi; d += 256) {
            uint32_t v;
            if (d * 4 + 4 <= src_bytes) {
                v = ((const uint32_t*)src)[d];
            } else {                        // the buffer's last, partial dword
                v = 0;
                for (size_t j = d * 4; j < src_bytes; ++j) v |= (uint32_t)p[j] << (8 * (j - d * 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t o = d * 4 + j;
                if (o >= lo && o < hi) {
                    const unsigned q = (unsigned)(o - base);
                    const int x = (int)(q / 3) - s0;
                    cs_row[(q % 3) * wl + (mirror ? wl - 1 - x : x)] = (uint8_t)(v >> (8 * j));
                }
            }
        }
    } else {
        const float* p = (const float*)src;
        for (int e = threadIdx.x; e < 3 * wl; e += 256) {
            const int ch = e / wl, x = e % wl;
            float v = p[((img * 3 + ch) * h + y) * (size_t)w + s0 + x] * 255.f;     // (image * 255).clip(0, 255).type(torch.uint8)
            v = fminf(fmaxf(v, 0.f), 255.f);
            cs_row[ch * wl + (mirror ? wl - 1 - x : x)] = (uint8_t)(int)v;
        }
    }
    __syncthreads();
    const int wq = wp / 4;
    for (int e = threadIdx.x; e < 3 * wq; e += 256) {
        const int ch = e / wq, q = e % wq;
        const uint8_t* line = cs_row + ch * wl;
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = q * 4 + j;
            if (ox < w_out) {
                const int xmin = bounds[2 * ox] - x0, n = bounds[2 * ox + 1];
                const int32_t* k = coefs + (size_t)ox * ksize;
                int acc = 1 << (kCsBits - 1);
                for (int t = 0; t < n; ++t) acc += (int)line[xmin + t] * k[t];
                packed |= cs_pixel(acc) << (8 * j);
            }
        }
        *(uint32_t*)(tmp + ((img * 3 + ch) * rows + yy) * (size_t)wp + q * 4) = packed;
    }
}

// Workgroup b: image b / h_out, output row b % h_out; its taps are rows [ymin - y0, ymin - y0 + n) of the workspace
template <bool VEC>
__global__ __launch_bounds__(256) void crop_v_kernel(const uint8_t* __restrict__ tmp, float* __restrict__ dst, int rows, int y0, int h_out, int w_out,
                                                     int wp, int ksize, const int32_t* __restrict__ bounds, const int32_t* __restrict__ coefs) {
    const size_t img = blockIdx.x / (unsigned)h_out;
    const int oy = (int)(blockIdx.x % (unsigned)h_out);
    const int ymin = bounds[2 * oy], n = bounds[2 * oy + 1];
    const int32_t* k = coefs + (size_t)oy * ksize;
    const int wq = wp / 4;
    for (int e = threadIdx.x; e < 3 * wq; e += 256) {
        const int ch = e / wq, q = e % wq;
        const uint8_t* col = tmp + ((img * 3 + ch) * rows + (ymin - y0)) * (size_t)wp + q * 4;
        int acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = 1 << (kCsBits - 1);
        for (int t = 0; t < n; ++t) {
            const uint32_t v = *(const uint32_t*)(col + (size_t)t * wp);
            const int kt = k[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (int)((v >> (8 * j)) & 255u) * kt;
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)cs_pixel(acc[j]) / 255.f;          // np.array(image) / 255: a correctly rounded divide
        float* out = dst + ((img * 3 + ch) * h_out + oy) * (size_t)w_out + q * 4;
        if (VEC) {
            *(f32x4*)out = f32x4{o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (q * 4 + j < w_out) out[j] = o[j];
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static bool cs_shape_ok(int n_img, int h, int w) { return n_img >= 0 && h >= 1 && w >= 1 && h <= kCsMaxH && w <= kCsMaxW; }

// the rows of the source the vertical pass reads: needs no device (the workspace is sized without one), built once per geometry
static void cs_row_window(int h, const CropGeom& g, int h_out, int* y0, int* y1) {
    static std::map<std::tuple<int, int, int, int>, std::pair<int, int>> windows;
    const auto key = std::make_tuple(h, g.h_s, g.row, h_out);
    std::lock_guard<std::mutex> lock(g_cs_mutex);
    auto it = windows.find(key);
    if (it == windows.end()) {
        const CropAxis a = crop_axis_build(h, g.h_s, g.row, h_out);
        it = windows.emplace(key, std::make_pair(a.lo, a.hi)).first;
    }
    *y0 = it->second.first;
    *y1 = it->second.second;
}

size_t crop_shim_workspace_bytes(int n_img, int h, int w, int h_out, int w_out) {
    CropGeom g;
    if (!cs_shape_ok(n_img, h, w) || n_img == 0 || !crop_geometry(h, w, h_out, w_out, &g)) return 0;
    int y0, y1;
    cs_row_window(h, g, h_out, &y0, &y1);
    return (size_t)n_img * 3 * (size_t)(y1 - y0) * (size_t)((w_out + 3) / 4 * 4);
}

int crop_shim_run(const void* src, int src_u8, float* dst, int n_img, int h, int w, int h_out, int w_out, const uint8_t* flip, void* ws,
                  size_t ws_bytes, int* scaled_hw, hipStream_t s) {
    MVLDM_REQUIRE(src_u8 == 0 || src_u8 == 1, "crop_shim: src_u8 %d", src_u8);
    MVLDM_REQUIRE(n_img >= 0, "crop_shim: n_img %d", n_img);
    MVLDM_REQUIRE(h >= 1 && w >= 1 && h_out >= 1 && w_out >= 1, "crop_shim: image %d x %d -> %d x %d: an edge below 1", h, w, h_out, w_out);
    MVLDM_REQUIRE(h_out <= h && w_out <= w, "crop_shim: %d x %d is larger than the source's %d x %d (the shim only shrinks)", h_out, w_out, h, w);
    if (h > kCsMaxH || w > kCsMaxW) return set_error(MVLDM_ERR_UNSUPPORTED, "crop_shim: source %d x %d; up to %d x %d is supported", h, w, kCsMaxH, kCsMaxW);
    CropGeom g;
    MVLDM_REQUIRE(crop_geometry(h, w, h_out, w_out, &g), "crop_shim: %d x %d -> %d x %d: neither scaled edge meets its target", h, w, h_out, w_out);
    if (scaled_hw) {
        scaled_hw[0] = g.h_s;
        scaled_hw[1] = g.w_s;
    }
    if (n_img == 0) return MVLDM_OK;
    const int wp = (w_out + 3) / 4 * 4;
    const size_t need = crop_shim_workspace_bytes(n_img, h, w, h_out, w_out);
    MVLDM_REQUIRE(ws_bytes >= need, "crop_shim: workspace of %zu bytes, need %zu", ws_bytes, need);
    MVLDM_REQUIRE(src != nullptr && dst != nullptr && ws != nullptr && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)ws & 3) == 0,
                  "crop_shim: null or unaligned pointer (4 bytes)");
    CropTable tx, ty;
    int rc = crop_table(w, g.w_s, g.col, w_out, s, &tx);
    if (rc != MVLDM_OK) return rc;
    rc = crop_table(h, g.h_s, g.row, h_out, s, &ty);
    if (rc != MVLDM_OK) return rc;
    const int rows = ty.hi - ty.lo;
    const size_t b1 = (size_t)n_img * rows, b2 = (size_t)n_img * h_out;
    MVLDM_REQUIRE(b1 <= 0x7FFFFFFFu && b2 <= 0x7FFFFFFFu, "crop_shim: %zu workgroups", b1 > b2 ? b1 : b2);
    const size_t src_bytes = (size_t)n_img * h * w * 3 * (src_u8 ? 1 : 4);
    const unsigned lds = (unsigned)(3 * (tx.hi - tx.lo) + 3) / 4 * 4;        // <= 3 kCsMaxW = 48 KiB
    uint8_t* tmp = (uint8_t*)ws;
    if (src_u8)
        hipLaunchKernelGGL(crop_h_kernel<true>, dim3((unsigned)b1), dim3(256), lds, s, src, src_bytes, tmp, h, w, rows, ty.lo, tx.lo, tx.hi, w_out, wp,
                           tx.ksize, tx.bounds, tx.coefs, flip);
    else
        hipLaunchKernelGGL(crop_h_kernel<false>, dim3((unsigned)b1), dim3(256), lds, s, src, src_bytes, tmp, h, w, rows, ty.lo, tx.lo, tx.hi, w_out, wp,
                           tx.ksize, tx.bounds, tx.coefs, flip);
    if (w_out % 4 == 0 && ((uintptr_t)dst & 15) == 0)
        hipLaunchKernelGGL(crop_v_kernel<true>, dim3((unsigned)b2), dim3(256), 0, s, (const uint8_t*)tmp, dst, rows, ty.lo, h_out, w_out, wp, ty.ksize,
                           ty.bounds, ty.coefs);
    else
        hipLaunchKernelGGL(crop_v_kernel<false>, dim3((unsigned)b2), dim3(256), 0, s, (const uint8_t*)tmp, dst, rows, ty.lo, h_out, w_out, wp, ty.ksize,
                           ty.bounds, ty.coefs);
    return check_launch();
}

int crop_shim_axis(int n_in, int n_out, int off, int count, int32_t* bounds, int32_t* coefs, int coefs_len) {
    MVLDM_REQUIRE(n_in >= 1 && n_in <= kCsMaxH && n_out >= 1 && n_out <= n_in, "crop_shim_axis: axis %d -> %d", n_in, n_out);
    MVLDM_REQUIRE(off >= 0 && count >= 1 && off + count <= n_out, "crop_shim_axis: outputs [%d, %d) of %d", off, off + count, n_out);
    const CropAxis a = crop_axis_build(n_in, n_out, off, count);
    if (bounds)
        for (size_t i = 0; i < a.bounds.size(); ++i) bounds[i] = a.bounds[i];
    if (coefs) {
        MVLDM_REQUIRE((size_t)coefs_len >= a.coefs.size(), "crop_shim_axis: room for %d coefficients, need %zu", coefs_len, a.coefs.size());
        for (size_t i = 0; i < a.coefs.size(); ++i) coefs[i] = a.coefs[i];
    }
    return a.ksize;
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_crop_shim_workspace_bytes(int n_img, int h, int w, int h_out, int w_out) {
    return crop_shim_workspace_bytes(n_img, h, w, h_out, w_out);
}
extern "C" int mvldm_crop_shim(const void* src, int src_u8, float* dst, int n_img, int h, int w, int h_out, int w_out, void* workspace, size_t workspace_bytes,
                               int* scaled_hw, mvldm_stream_t stream) {
    return crop_shim_run(src, src_u8, dst, n_img, h, w, h_out, w_out, nullptr, workspace, workspace_bytes, scaled_hw, (hipStream_t)stream);
}
extern "C" int mvldm_crop_shim_flip(const void* src, int src_u8, float* dst, int n_img, int h, int w, int h_out, int w_out, const uint8_t* flip, void* workspace,
                                    size_t workspace_bytes, int* scaled_hw, mvldm_stream_t stream) {
    return crop_shim_run(src, src_u8, dst, n_img, h, w, h_out, w_out, flip, workspace, workspace_bytes, scaled_hw, (hipStream_t)stream);
}
extern "C" int mvldm_crop_shim_axis(int n_in, int n_out, int offset, int count, int32_t* bounds, int32_t* coefs, int coefs_len) {
    return crop_shim_axis(n_in, n_out, offset, count, bounds, coefs, coefs_len);
}
