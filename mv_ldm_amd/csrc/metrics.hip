// Image quality of sampled views (include/mvldm.h, "Image metrics"): PSNR and Gaussian-window SSIM of n_img image pairs, fp32 NCHW,
// in one launch plus a small fold.  The SSIM is skimage.metrics.structural_similarity(win_size=11, gaussian_weights=True,
// data_range=1.0) restated: its crop of 5 pixels per side makes the border mode of the filter unobservable, so the map is a VALID
// 11 x 11 separable convolution of the five moments x, y, x^2, y^2, xy over (h - 10) x (w - 10) outputs.
//
// A workgroup owns a kTile x kTile output tile of one (image, channel): it stages the tile plus the 10-pixel halo of both images in
// LDS, runs the horizontal pass of the five moments into LDS (a thread slides over 4 neighbouring columns of one row), the vertical
// pass into registers (a thread slides over 4 neighbouring rows of one column), forms S in fp32 and sums it in fp64.  The clipped
// squared error of the PSNR is summed, in fp64, over the input pixels the workgroup owns (its tile's footprint; the last tile of a
// row / column also takes the 10 halo pixels, so the footprints partition the image).  One fp64 pair per workgroup goes to the
// caller's workspace; the fold adds an image's pairs in a fixed order -- no atomics, the same bits on every run, and an image's
// scores depend on nothing but its own pixels.
//
// Conditioning: the variances are differences f(x^2) - f(x)^2 of nearly equal numbers wherever the image is flat, and C2 = 9e-4 puts
// an fp32 round-off of 1e-7 there straight into the 4th digit of S.  Variance and covariance do not change when a constant is
// subtracted, so the tile stages x - x0 and y - y0 (x0, y0: each image's own pixel at the centre of the staged footprint) and adds the
// constants back to the means: on natural images the staged values are small and the cancellation loses 1-2 digits fewer.
#include <math.h>

#include "common.h"

namespace mvldm {

constexpr int kTile = 32;             // output tile edge (mv_ldm_amd/ops.py IMAGE_METRICS_TILE mirrors it for the tests)
constexpr int kWin = 11;              // taps; radius 5 = int(truncate 3.5 * sigma 1.5 + 0.5)
constexpr int kIn = kTile + kWin - 1; // staged edge: 42
constexpr int kInLd = kIn + 1;        // 43: odd pitch, the horizontal pass walks rows with consecutive lanes
constexpr int kHLd = kTile + 1;       // 33

struct SsimTaps {
    float w[kWin];
};

__global__ __launch_bounds__(256) void image_metrics_kernel(const float* __restrict__ a, const float* __restrict__ b, int c, int h, int w,
                                                            int tiles_x, int tiles_y, SsimTaps taps, float cov_norm, double* __restrict__ ws) {
    __shared__ float s_a[kIn * kInLd], s_b[kIn * kInLd];
    __shared__ float s_h[5][kIn * kHLd];
    __shared__ double s_red[2][4];
    const int tiles = tiles_x * tiles_y;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x % tiles;        // plane = img * c + channel
    const int ty0 = (tile / tiles_x) * kTile, tx0 = (tile % tiles_x) * kTile;
    const int oh = h - (kWin - 1), ow = w - (kWin - 1);
    const int vh = min(kTile, oh - ty0), vw = min(kTile, ow - tx0);         // valid outputs of this tile
    // input pixels whose squared error this workgroup sums
    const int own_h = (ty0 + kTile >= oh) ? h - ty0 : kTile, own_w = (tx0 + kTile >= ow) ? w - tx0 : kTile;
    const float* pa = a + (size_t)plane * h * w;
    const float* pb = b + (size_t)plane * h * w;

    const size_t centre = (size_t)(ty0 + (vh + kWin - 1) / 2) * w + tx0 + (vw + kWin - 1) / 2;
    const float a0 = pa[centre], b0 = pb[centre];
    double err = 0.0;
    for (int i = threadIdx.x; i < kIn * kIn; i += 256) {
        const int r = i / kIn, q = i % kIn;
        const int y = ty0 + r, x = tx0 + q;
        float va = a0, vb = b0;
        if (y < h && x < w) {
            va = pa[(size_t)y * w + x];
            vb = pb[(size_t)y * w + x];
            if (r < own_h && q < own_w) {
                const double d = (double)fminf(fmaxf(va, 0.f), 1.f) - (double)fminf(fmaxf(vb, 0.f), 1.f);
                err += d * d;
            }
        }
        s_a[r * kInLd + q] = va - a0;
        s_b[r * kInLd + q] = vb - b0;
    }
    __syncthreads();

    // horizontal pass: item = (row, group of 4 output columns); consecutive lanes take consecutive rows (pitch 43: no bank conflict)
    for (int i = threadIdx.x; i < kIn * (kTile / 4); i += 256) {
        const int r = i % kIn, q0 = (i / kIn) * 4;
        float m[4][5];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int k = 0; k < 5; ++k) m[o][k] = 0.f;
#pragma unroll
        for (int t = 0; t < kWin + 3; ++t) {
            const float x = s_a[r * kInLd + q0 + t], y = s_b[r * kInLd + q0 + t];
            const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int k = t - o;
                if (k >= 0 && k < kWin) {
                    const float g = taps.w[k];
                    m[o][0] += g * x;
                    m[o][1] += g * y;
                    m[o][2] += g * xx;
                    m[o][3] += g * yy;
                    m[o][4] += g * xy;
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int k = 0; k < 5; ++k) s_h[k][r * kHLd + q0 + o] = m[o][k];
    }
    __syncthreads();

    // vertical pass: thread = (column, group of 4 output rows)
    const int col = threadIdx.x % kTile, r0 = (threadIdx.x / kTile) * 4;
    float m[4][5];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int k = 0; k < 5; ++k) m[o][k] = 0.f;
#pragma unroll
    for (int t = 0; t < kWin + 3; ++t) {
        float v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = s_h[k][(r0 + t) * kHLd + col];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = t - o;
            if (k >= 0 && k < kWin) {
                const float g = taps.w[k];
#pragma unroll
                for (int j = 0; j < 5; ++j) m[o][j] += g * v[j];
            }
        }
    }
    const float C1 = 1e-4f, C2 = 9e-4f;       // (0.01 * data_range)^2, (0.03 * data_range)^2 with data_range = 1
    double ssum = 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (r0 + o < vh && col < vw) {
            const float dx = m[o][0], dy = m[o][1], ux = a0 + dx, uy = b0 + dy;
            const float vx = cov_norm * (m[o][2] - dx * dx), vy = cov_norm * (m[o][3] - dy * dy), vxy = cov_norm * (m[o][4] - dx * dy);
            const float num = (2.f * ux * uy + C1) * (2.f * vxy + C2);
            const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
            ssum += (double)(num / den);
        }
    }

    ssum = wave_sum_d(ssum);
    err = wave_sum_d(err);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[0][wave] = ssum;
        s_red[1][wave] = err;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double* p = s_red[threadIdx.x];
        ws[(size_t)blockIdx.x * 2 + threadIdx.x] = (p[0] + p[1]) + (p[2] + p[3]);
    }
}

// one workgroup per image: its P = c * tiles pairs, strided over 256 threads, then a fixed halving tree
__global__ __launch_bounds__(256) void image_metrics_fold_kernel(const double* __restrict__ ws, int P, double inv_ssim_n, double inv_mse_n,
                                                                 float* __restrict__ psnr, float* __restrict__ ssim) {
    __shared__ double s_s[256], s_e[256];
    const double* p = ws + (size_t)blockIdx.x * P * 2;
    double s = 0.0, e = 0.0;
    for (int k = threadIdx.x; k < P; k += 256) {
        s += p[2 * k];
        e += p[2 * k + 1];
    }
    s_s[threadIdx.x] = s;
    s_e[threadIdx.x] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            s_s[threadIdx.x] += s_s[threadIdx.x + o];
            s_e[threadIdx.x] += s_e[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ssim[blockIdx.x] = (float)(s_s[0] * inv_ssim_n);
        psnr[blockIdx.x] = (float)(-10.0 * log10(s_e[0] * inv_mse_n));       // identical images: log10(0) = -inf -> +inf, as torch
    }
}

static int metrics_tiles(int h, int w, int* tx, int* ty) {
    *tx = (w - (kWin - 1) + kTile - 1) / kTile;
    *ty = (h - (kWin - 1) + kTile - 1) / kTile;
    return *tx * *ty;
}

size_t image_metrics_workspace_bytes(int n_img, int c, int h, int w) {
    if (n_img < 1 || c < 1 || h < kWin || w < kWin) return 0;
    int tx, ty;
    return (size_t)n_img * c * metrics_tiles(h, w, &tx, &ty) * 2 * sizeof(double);
}

int image_metrics_run(const float* pred, const float* gt, int n_img, int c, int h, int w, int use_sample_covariance, float* psnr, float* ssim,
                      double* ws, size_t ws_bytes, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0 && c >= 1, "image_metrics: n_img %d, c %d", n_img, c);
    MVLDM_REQUIRE(h >= kWin && w >= kWin, "image_metrics: %d x %d image is smaller than the %d x %d window", h, w, kWin, kWin);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(pred && gt && psnr && ssim && ws, "image_metrics: null pointer");
    int tx, ty;
    const int tiles = metrics_tiles(h, w, &tx, &ty);
    const size_t blocks = (size_t)n_img * c * tiles;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu && (size_t)c * tiles <= 0x7FFFFFFFu, "image_metrics: %zu workgroups", blocks);
    const size_t need = blocks * 2 * sizeof(double);
    MVLDM_REQUIRE(ws_bytes >= need, "image_metrics: workspace of %zu bytes, need %zu", ws_bytes, need);
    SsimTaps taps;
    double g[kWin], sum = 0.0;
    for (int k = 0; k < kWin; ++k) sum += g[k] = exp(-0.5 * (k - kWin / 2) * (k - kWin / 2) / (1.5 * 1.5));
    for (int k = 0; k < kWin; ++k) taps.w[k] = (float)(g[k] / sum);
    const float cov_norm = use_sample_covariance ? (float)(121.0 / 120.0) : 1.0f;
    hipLaunchKernelGGL(image_metrics_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pred, gt, c, h, w, tx, ty, taps, cov_norm, ws);
    int rc = check_launch();
    if (rc) return rc;
    const double ssim_n = (double)c * (h - (kWin - 1)) * (w - (kWin - 1)), mse_n = (double)c * h * w;
    hipLaunchKernelGGL(image_metrics_fold_kernel, dim3(n_img), dim3(256), 0, s, ws, c * tiles, 1.0 / ssim_n, 1.0 / mse_n, psnr, ssim);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_image_metrics_workspace_bytes(int n_img, int c, int h, int w) { return image_metrics_workspace_bytes(n_img, c, h, w); }
extern "C" int mvldm_image_metrics(const float* pred, const float* gt, int n_img, int c, int h, int w, int use_sample_covariance, float* psnr,
                                   float* ssim, double* workspace, size_t workspace_bytes, mvldm_stream_t stream) {
    return image_metrics_run(pred, gt, n_img, c, h, w, use_sample_covariance, psnr, ssim, workspace, workspace_bytes, (hipStream_t)stream);
}
