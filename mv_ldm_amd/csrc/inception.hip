// Clean-FID around the implicit GEMM (include/mvldm.h, "Clean-FID"): what `cleanfid.fid.compute_fid` (src/scripts/compute_fid.py:44-47)
// needs besides the convolutions, which mvldm_igemm_fwd runs with BatchNorm folded into weight and bias.
//   inception_prep      uint8 or fp32 [0, 1] NCHW [n][3][h][w] -> NHWC [n][oh][ow][c_pad] in the compute dtype: the package's "clean" resize,
//                       PIL's antialiased bicubic on float32 planes (a = -0.5, horizontally first, a pass whose size stays is skipped; the
//                       coefficients and the sum over the taps in double, in tap order, rounded to float32 at the end of each pass),
//                       clip to [0, 255], (v - 128) / 128; pad channels zero.  The horizontal pass writes [n][3][h][ow] float32 to the workspace.
//   inception_unfold    NHWC [n][h][w][c] -> [n][h][w][kh kw c]: the kh x kw window around each pixel (stride 1, same size), tap-major then
//                       channel, zero outside the map: a 1 x 7, 7 x 1, 1 x 3, 3 x 1 or 5 x 5 convolution is then a 1 x 1 one
//   inception_maxpool   3 x 3, stride 1 or 2, padding 0 or 1 (as -inf), floored size; inception_avgpool 3 x 3 / 1 / padding 1, divided by
//                       the taps inside the map; inception_concat copies a contiguous map (with ReLU if asked): all three write a channel
//                       slice of a wider NHWC buffer, so a block's concatenation costs no pass of its own
//   inception_features  NHWC [n][h][w][c] -> fp64 means [n][c]: one thread per (image, channel), pixels in order, fp64 from the first add
//   frechet_accumulate  state (count, sum f, sum f^T f) += n feature rows of width d, images in order: one thread per entry of the state adds the
//                       images and then adds that to the state.  fid_accumulate (fid.hip) ends in it too, at width 64
//   frechet_compute     the Frechet distance at d <= 2048 with the matrices in global memory: Sigma1 = V D V^T and the spectrum of
//                       D^1/2 V^T Sigma2 V D^1/2 by ONE-SIDED Jacobi (Hestenes): G = A V is kept by columns, a workgroup owns one pair of
//                       columns of a round (round-robin ordering, d / 2 disjoint pairs, one launch a round), takes the rotation from three
//                       dot products and applies it to both columns (and to V's).  Every sum has a fixed order; no atomics.  The host
//                       enqueues kFrSweepCap sweeps and reads nothing back: a sweep whose largest |g_p . g_q| / (|g_p| |g_q|) stayed
//                       below the tolerance sets a flag in the workspace that turns the launches behind it into no-ops.
#include <math.h>

#include "common.h"

namespace mvldm {

// ---- the resize ---------------------------------------------------------------------------------------------------------------------
// PIL's bicubic_filter (a = -0.5) and precompute_coeffs, operation for operation (the library is built with -ffp-contract=off)
__device__ __forceinline__ double pil_cubic(double x) {
    constexpr double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct PilAxis {
    double scale, support, ss;      // in / out; 2 max(scale, 1); 1 / max(scale, 1)
    int n_in, same;
};
static PilAxis pil_axis(int n_in, int n_out) {
    PilAxis a;
    a.scale = (double)n_in / (double)n_out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * fs;
    a.ss = 1.0 / fs;
    a.n_in = n_in;
    a.same = n_in == n_out;
    return a;
}

// the taps of output index i: [xmin, xmin + n), and the sum of their weights
__device__ __forceinline__ void pil_window(const PilAxis& ax, int i, int* xmin, int* n, double* center, double* ww) {
    const double c = ((double)i + 0.5) * ax.scale;
    int lo = (int)(c - ax.support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(c + ax.support + 0.5);
    if (hi > ax.n_in) hi = ax.n_in;
    double w = 0.0;
    for (int x = 0; x < hi - lo; ++x) w += pil_cubic(((double)(x + lo) - c + 0.5) * ax.ss);
    *xmin = lo;
    *n = hi - lo;
    *center = c;
    *ww = w;
}

template <bool U8>
__device__ __forceinline__ float prep_load(const void* src, size_t at) {
    if (U8) return (float)((const uint8_t*)src)[at];
    return ((const float*)src)[at] * 255.f;         // a float image is scaled, not quantised
}

// horizontal pass: one thread per element of tmp [n 3 h][ow]
template <bool U8>
__global__ __launch_bounds__(256) void inception_prep_h_kernel(const void* __restrict__ src, float* __restrict__ tmp, size_t total, int w, int ow,
                                                               PilAxis ax) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % ow);
    const size_t row = idx / ow;
    if (ax.same) {
        tmp[idx] = prep_load<U8>(src, row * w + ox);
        return;
    }
    int xmin, n;
    double center, ww;
    pil_window(ax, ox, &xmin, &n, &center, &ww);
    double ss = 0.0;
    for (int x = 0; x < n; ++x) {
        double k = pil_cubic(((double)(x + xmin) - center + 0.5) * ax.ss);
        if (ww != 0.0) k /= ww;
        ss += (double)prep_load<U8>(src, row * w + xmin + x) * k;
    }
    tmp[idx] = (float)ss;
}

// vertical pass, clip, (v - 128) / 128: one thread per output pixel
template <typename T>
__global__ __launch_bounds__(256) void inception_prep_v_kernel(const float* __restrict__ tmp, T* __restrict__ dst, size_t n_px, int h, int oh, int ow,
                                                               PilAxis ax) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // (image * oh + oy) * ow + ox
    if (idx >= n_px) return;
    const int ox = (int)(idx % ow);
    const size_t t = idx / ow;
    const int oy = (int)(t % oh);
    const size_t img = t / oh;
    int ymin = oy, n = 1;
    double center = 0.0, ww = 0.0;
    if (!ax.same) pil_window(ax, oy, &ymin, &n, &center, &ww);
    Chunk<T> c;
    c.zero();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* plane = tmp + (img * 3 + ch) * (size_t)h * ow + ox;
        float v;
        if (ax.same) {
            v = plane[(size_t)oy * ow];
        } else {
            double ss = 0.0;
            for (int y = 0; y < n; ++y) {
                double k = pil_cubic(((double)(y + ymin) - center + 0.5) * ax.ss);
                if (ww != 0.0) k /= ww;
                ss += (double)plane[(size_t)(ymin + y) * ow] * k;
            }
            v = (float)ss;
        }
        v = fminf(fmaxf(v, 0.f), 255.f);
        c.set(ch, (v - 128.f) / 128.f);
    }
    store_chunk(dst + idx * Chunk<T>::N, c);
}

// ---- unfold, pools, concat: one thread per 16-byte chunk of the output ---------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void inception_unfold_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t total, int h, int w, int cp,
                                                               int kh, int kw, int ph, int pw) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // ((image h + y) w + x) (kh kw cp) + tap cp + chunk
    if (idx >= total) return;
    const int j = (int)(idx % cp);
    size_t t = idx / cp;
    const int tap = (int)(t % (kh * kw));
    t /= kh * kw;
    const int x = (int)(t % w);
    t /= w;
    const int y = (int)(t % h);
    const size_t img = t / h;
    const int sy = y + tap / kw - ph, sx = x + tap % kw - pw;
    Chunk<T> c;
    c.zero();
    if (sy >= 0 && sy < h && sx >= 0 && sx < w) c = load_chunk(src + (((img * h + sy) * w + sx) * cp + j) * Chunk<T>::N);
    store_chunk(dst + idx * Chunk<T>::N, c);
}

template <typename T, bool kMax>
__global__ __launch_bounds__(256) void inception_pool_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t total, int h, int w, int cp, int oh,
                                                             int ow, int stride, int pad, int dst_ld, int dst_c_off) {
    constexpr int E = Chunk<T>::N;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // ((image oh + oy) ow + ox) cp + chunk
    if (idx >= total) return;
    const int j = (int)(idx % cp);
    size_t t = idx / cp;
    const int ox = (int)(t % ow);
    t /= ow;
    const int oy = (int)(t % oh);
    const size_t img = t / oh;
    double acc[E];                              // the average adds in double: nine terms that may cancel, rounded once at the end
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = kMax ? -INFINITY : 0.0;
    int taps = 0;
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
            const int sy = oy * stride + dy - pad, sx = ox * stride + dx - pad;
            if (sy < 0 || sy >= h || sx < 0 || sx >= w) continue;
            const Chunk<T> c = load_chunk(src + (((img * h + sy) * w + sx) * cp + j) * E);
            ++taps;
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] = kMax ? fmax(acc[e], (double)c.get(e)) : acc[e] + (double)c.get(e);
        }
    Chunk<T> o;
    const double div = (double)taps;
#pragma unroll
    for (int e = 0; e < E; ++e) o.set(e, (float)(kMax ? acc[e] : acc[e] / div));
    store_chunk(dst + (idx / cp) * (size_t)dst_ld + dst_c_off + (size_t)j * E, o);
}

template <typename T>
__global__ __launch_bounds__(256) void inception_concat_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t total, int cp, int dst_ld,
                                                               int dst_c_off, int relu) {
    constexpr int E = Chunk<T>::N;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // pixel cp + chunk
    if (idx >= total) return;
    Chunk<T> c = load_chunk(src + idx * E);
    if (relu) {
#pragma unroll
        for (int e = 0; e < E; ++e) c.set(e, fmaxf(c.get(e), 0.f));
    }
    store_chunk(dst + (idx / cp) * (size_t)dst_ld + dst_c_off + (idx % cp) * E, c);
}

template <typename T>
__global__ __launch_bounds__(256) void inception_features_kernel(const T* __restrict__ f, int hw, int c, double* __restrict__ out) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    const T* p = f + (size_t)blockIdx.y * hw * c + ch;
    double v = 0.0;
    for (int q = 0; q < hw; ++q) v += (double)to_f32<T>(p[(size_t)q * c]);
    out[(size_t)blockIdx.y * c + ch] = v / (double)hw;
}

// entry 0: the count; 1 + a: sum_i f[i][a]; 1 + d + a d + b: sum_i f[i][a] f[i][b] -- the images in order, then one add to the state
__global__ __launch_bounds__(256) void frechet_state_kernel(const double* __restrict__ feat, int n, int d, double* __restrict__ state) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)1 + d + (size_t)d * d) return;
    double v = 0.0;
    if (e == 0) {
        v = (double)n;
    } else if (e <= (size_t)d) {
        for (int i = 0; i < n; ++i) v += feat[(size_t)i * d + (e - 1)];
    } else {
        const size_t a = (e - 1 - d) / d, b = (e - 1 - d) % d;
        for (int i = 0; i < n; ++i) v += feat[(size_t)i * d + a] * feat[(size_t)i * d + b];
    }
    state[e] += v;
}

// ---- the Frechet distance -----------------------------------------------------------------------------------------------------------
constexpr int kFrMaxD = 2048;
constexpr int kFrSweepCap = 30;             // the host enqueues this many sweeps of each solve; 10 - 14 do the work at d = 2048
constexpr int kFrCtl = 16;                  // doubles of control record in front of the workspace
// ctl: [0] the running solve has converged, [1] its sweeps, [2] the residual of its last sweep; [3] |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2;
// [4 .. 6] sweeps, residual and flag of the first solve, kept while the second runs; [7] |A|_F^2 of the running solve's matrix
struct FrWs {
    double *ctl, *mu1, *mu2, *lam, *slot, *G, *V, *B, *T;
};
static size_t frechet_ws_doubles(int d) { return (size_t)kFrCtl + 4 * (size_t)d + 4 * (size_t)d * d; }
static FrWs frechet_ws(double* ws, int d) {
    FrWs w;
    w.ctl = ws;
    w.mu1 = ws + kFrCtl;
    w.mu2 = w.mu1 + d;
    w.lam = w.mu2 + d;
    w.slot = w.lam + d;                     // d / 2 running maxima of the sweep, one per workgroup of a round
    w.G = w.slot + d;
    w.V = w.G + (size_t)d * d;
    w.B = w.V + (size_t)d * d;
    w.T = w.B + (size_t)d * d;
    return w;
}

// every thread gets the sum of the 256 values, added in one fixed tree
__device__ __forceinline__ double fr_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void frechet_mean_kernel(const double* __restrict__ s1, const double* __restrict__ s2, int d, FrWs w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < d) {
        w.mu1[i] = s1[1 + i] / s1[0];
        w.mu2[i] = s2[1 + i] / s2[0];
        if (i < d / 2) w.slot[i] = 0.0;
    }
    if (i < kFrCtl) w.ctl[i] = 0.0;
}

// Sigma1 -> G, Sigma2 -> B, I -> V (all symmetric: a row is a column)
__global__ __launch_bounds__(256) void frechet_sigma_kernel(const double* __restrict__ s1, const double* __restrict__ s2, int d, FrWs w) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)d * d) return;
    const int i = (int)(e / d), j = (int)(e % d);
    const double n1 = s1[0], n2 = s2[0];
    w.G[e] = (s1[1 + d + e] - n1 * (w.mu1[i] * w.mu1[j])) / (n1 - 1.0);
    w.B[e] = (s2[1 + d + e] - n2 * (w.mu2[i] * w.mu2[j])) / (n2 - 1.0);
    w.V[e] = i == j ? 1.0 : 0.0;
}

// one workgroup: head = |mu1 - mu2|^2 + (tr Sigma1 + tr Sigma2); thread t takes indices t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(256) void frechet_head_kernel(int d, FrWs w) {
    __shared__ double red[256];
    double dm = 0.0, t1 = 0.0, t2 = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) {
        const double x = w.mu1[i] - w.mu2[i];
        dm += x * x;
        t1 += w.G[(size_t)i * d + i];
        t2 += w.B[(size_t)i * d + i];
    }
    dm = fr_block_sum(dm, red);
    t1 = fr_block_sum(t1, red);
    t2 = fr_block_sum(t2, red);
    if (threadIdx.x == 0) w.ctl[3] = dm + (t1 + t2);
}

// One round of one-sided Jacobi.  Workgroup k owns the pair of round r: (d - 1, r) for k = 0, else ((r + k) % (d - 1), (r - k) % (d - 1)),
// p the smaller index.  G[p], G[q] are columns p and q of A V (contiguous: G is stored by columns).  With app = g_p . g_p, aqq = g_q . g_q,
// apq = g_p . g_q the rotation that makes the two columns orthogonal is Rutishauser's: zeta = (aqq - app) / (2 apq),
// t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t; g_p <- c g_p - s g_q, g_q <- s g_p + c g_q (V alike; see below for c).
// It is applied when |apq| > tol sqrt(app) sqrt(aqq), unless sqrt(app) sqrt(aqq) <= tol^2 |A|_F^2 (two columns of round-off: without this
// floor a rank-deficient Sigma spends as many sweeps again on orthogonalising its null space's noise); the ratio's largest value of the
// sweep stays in slot[k].
template <bool kVectors>
__global__ __launch_bounds__(256) void frechet_round_kernel(int d, int r, double tol, const double* __restrict__ ctl, double* __restrict__ slot,
                                                            double* __restrict__ G, double* __restrict__ V) {
    __shared__ double red[256];
    if (ctl[0] != 0.0) return;                  // the solve has converged: every thread reads the same word
    const int k = blockIdx.x, R = d - 1;
    const int a = k == 0 ? d - 1 : (r + k) % R, b = k == 0 ? r : (r - k + R) % R;
    const int p = min(a, b), q = max(a, b);
    double* gp = G + (size_t)p * d;
    double* gq = G + (size_t)q * d;
    double x[kFrMaxD / 256], y[kFrMaxD / 256];
    double spp = 0.0, sqq = 0.0, spq = 0.0;
#pragma unroll
    for (int m = 0; m < kFrMaxD / 256; ++m) {
        const int i = m * 256 + threadIdx.x;
        x[m] = i < d ? gp[i] : 0.0;
        y[m] = i < d ? gq[i] : 0.0;
        spp += x[m] * x[m];
        sqq += y[m] * y[m];
        spq += x[m] * y[m];
    }
    const double app = fr_block_sum(spp, red), aqq = fr_block_sum(sqq, red), apq = fr_block_sum(spq, red);
    const double den = sqrt(app) * sqrt(aqq);
    const double floor = tol * tol * ctl[7];    // |g_p| |g_q| <= tol^2 |A|_F^2: both columns are round-off of a null space, left alone
    const double ratio = den > floor ? fabs(apq) / den : 0.0;
    if (threadIdx.x == 0) slot[k] = fmax(slot[k], ratio);
    if (!(ratio > tol)) return;                 // block-uniform: all threads hold the same sums
    const double zeta = (aqq - app) / (2.0 * apq);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
    // c - 1 = -t^2 / (rt (1 + rt)), rt = sqrt(1 + t^2), and x + ((c - 1) x - s y): with c itself, rounded next to 1 where the grid below is
    // twice as fine as the grid above, c^2 + s^2 - 1 averages +2^-53 for small t and every rotation stretches its columns by that
    // (measured in the numpy model: a relative error of the eigenvalues that grows with d, 5e-14 at d = 256)
    const double h = t * t, rt = sqrt(h + 1.0), s = (1.0 / rt) * t, cm1 = -h / (rt * (1.0 + rt));
#pragma unroll
    for (int m = 0; m < kFrMaxD / 256; ++m) {
        const int i = m * 256 + threadIdx.x;
        if (i < d) {
            gp[i] = x[m] + (cm1 * x[m] - s * y[m]);
            gq[i] = y[m] + (s * x[m] + cm1 * y[m]);
            if (kVectors) {
                const double vx = V[(size_t)p * d + i], vy = V[(size_t)q * d + i];
                V[(size_t)p * d + i] = vx + (cm1 * vx - s * vy);
                V[(size_t)q * d + i] = vy + (s * vx + cm1 * vy);
            }
        }
    }
}

// one workgroup: |A|_F^2 = the sum of squares of G (thread t takes entries t, t + 256, ... in order, then the tree) -> ctl[7]; rotations keep it
__global__ __launch_bounds__(256) void frechet_fro_kernel(int d, const double* __restrict__ G, double* __restrict__ ctl) {
    __shared__ double red[256];
    double v = 0.0;
    for (size_t e = threadIdx.x; e < (size_t)d * d; e += 256) v += G[e] * G[e];
    v = fr_block_sum(v, red);
    if (threadIdx.x == 0) ctl[7] = v;
}

// the end of a sweep, one workgroup: the largest ratio of the sweep (a maximum: no order to fix) -> residual; converged -> the flag
__global__ __launch_bounds__(256) void frechet_sweep_kernel(int d, double tol, double* __restrict__ ctl, double* __restrict__ slot) {
    __shared__ double red[256];
    if (ctl[0] != 0.0) return;
    double v = 0.0;
    for (int i = threadIdx.x; i < d / 2; i += 256) {
        v = fmax(v, slot[i]);
        slot[i] = 0.0;
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ctl[1] += 1.0;
        ctl[2] = red[0];
        if (red[0] <= tol) ctl[0] = 1.0;
    }
}

// workgroup i: lam[i] = v_i . g_i (the Rayleigh quotient of the unit vector v_i: the eigenvalue with its sign) or |g_i| (no vectors kept)
template <bool kVectors>
__global__ __launch_bounds__(256) void frechet_lambda_kernel(int d, const double* __restrict__ G, const double* __restrict__ V, double* __restrict__ lam) {
    __shared__ double red[256];
    const double* g = G + (size_t)blockIdx.x * d;
    const double* v = V + (size_t)blockIdx.x * d;
    double sum = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) sum += kVectors ? v[i] * g[i] : g[i] * g[i];
    sum = fr_block_sum(sum, red);
    if (threadIdx.x == 0) lam[blockIdx.x] = kVectors ? sum : sqrt(sum);
}

// C[a][b] = sum_k X[a][k] Y[b][k], k in order: 64 x 64 of C per workgroup, 4 x 4 per thread, d a multiple of 64
__global__ __launch_bounds__(256) void frechet_nt_kernel(int d, const double* __restrict__ X, const double* __restrict__ Y, double* __restrict__ Cm) {
    __shared__ double sx[16][65], sy[16][65];
    const int a0 = blockIdx.y * 64, b0 = blockIdx.x * 64;
    const int ta = threadIdx.x / 16, tb = threadIdx.x % 16;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int k0 = 0; k0 < d; k0 += 16) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int e = m * 256 + threadIdx.x, row = e / 16, kk = e % 16;
            sx[kk][row] = X[(size_t)(a0 + row) * d + k0 + kk];
            sy[kk][row] = Y[(size_t)(b0 + row) * d + k0 + kk];
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            double xa[4], yb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xa[i] = sx[kk][ta * 4 + i];
                yb[i] = sy[kk][tb * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += xa[i] * yb[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Cm[(size_t)(a0 + ta * 4 + i) * d + b0 + tb * 4 + j] = acc[i][j];
}

// S = D^1/2 sym(M) D^1/2 -> G: one thread per unordered pair writes both halves, so S is symmetric to the bit
__global__ __launch_bounds__(256) void frechet_scale_kernel(int d, const double* __restrict__ lam, const double* __restrict__ M, double* __restrict__ G) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)d * d) return;
    const int i = (int)(e / d), j = (int)(e % d);
    if (i > j) return;
    const double si = sqrt(fmax(lam[i], 0.0)), sj = sqrt(fmax(lam[j], 0.0));
    const double v = (si * (0.5 * (M[(size_t)i * d + j] + M[(size_t)j * d + i]))) * sj;
    G[(size_t)i * d + j] = v;
    G[(size_t)j * d + i] = v;
}

// the first solve's record moves to ctl[4 .. 6], the control words are cleared for the second
__global__ void frechet_next_kernel(double* __restrict__ ctl) {
    if (threadIdx.x == 0) {
        ctl[4] = ctl[1];
        ctl[5] = ctl[2];
        ctl[6] = ctl[0];
        ctl[0] = ctl[1] = ctl[2] = 0.0;
    }
}

__global__ __launch_bounds__(256) void frechet_score_kernel(int d, const double* __restrict__ s1, const double* __restrict__ s2, const double* __restrict__ ctl,
                                                            const double* __restrict__ lam, float* __restrict__ score, double* __restrict__ info) {
    __shared__ double red[256];
    double c = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) c += sqrt(fmax(lam[i], 0.0));
    c = fr_block_sum(c, red);
    if (threadIdx.x == 0) {
        const double head = ctl[3], fid = head - 2.0 * c;
        const bool ok1 = ctl[6] != 0.0, ok2 = ctl[0] != 0.0;
        const bool good = ok1 && ok2 && s1[0] >= 2.0 && s2[0] >= 2.0;
        *score = good ? (float)fid : __builtin_nanf("");
        info[0] = ctl[4];
        info[1] = ctl[5];
        info[2] = ctl[1];
        info[3] = ctl[2];
        info[4] = (double)((ok1 ? 0 : 1) + (ok2 ? 0 : 1));
        info[5] = fid;
        info[6] = c;
        info[7] = head;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool frechet_d_ok(int d) { return d >= 64 && d <= kFrMaxD && d % 64 == 0; }
constexpr long long kOffsetMax = 0x7FFFFFFFll;      // bytes of an operand the convolutions behind these kernels can address

size_t inception_workspace_bytes(int n_img, int h, int ow) {
    if (n_img < 1 || h < 1 || ow < 1) return 0;
    return (size_t)n_img * 3 * h * ow * sizeof(float);
}

int inception_prep_run(const void* src, int src_u8, void* dst, int n_img, int h, int w, int oh, int ow, int c_pad, int dtype, void* ws, size_t ws_bytes,
                       hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "inception_prep: n_img %d", n_img);
    MVLDM_REQUIRE(h >= 1 && w >= 1 && oh >= 1 && ow >= 1, "inception_prep: image %d x %d -> %d x %d: an edge below 1", h, w, oh, ow);
    MVLDM_REQUIRE(src_u8 == 0 || src_u8 == 1, "inception_prep: src_u8 %d", src_u8);
    MVLDM_REQUIRE(dtype_ok(dtype), "inception_prep: unknown dtype %d", dtype);
    MVLDM_REQUIRE(c_pad == (dtype == MVLDM_F32 ? 4 : 8), "inception_prep: c_pad %d is not the 16-byte padding of 3 channels in dtype %d", c_pad, dtype);
    MVLDM_REQUIRE((long long)h * w <= kOffsetMax && (long long)oh * ow <= kOffsetMax && (long long)h * ow <= kOffsetMax,
                  "inception_prep: %d x %d -> %d x %d is too large", h, w, oh, ow);
    if (n_img == 0) return MVLDM_OK;
    const size_t need = inception_workspace_bytes(n_img, h, ow);
    MVLDM_REQUIRE(ws_bytes >= need, "inception_prep: workspace of %zu bytes, need %zu", ws_bytes, need);
    MVLDM_REQUIRE((double)n_img * oh * ow * c_pad * (double)dtype_size(dtype) <= (double)kOffsetMax,
                  "inception_prep: the output of %d images is past the 32-bit offset range", n_img);
    MVLDM_REQUIRE(aligned(src, src_u8 ? 1 : 4) && aligned(dst, 16) && aligned(ws, 4), "inception_prep: null or unaligned pointer");
    const size_t total = (size_t)n_img * 3 * h * ow, n_px = (size_t)n_img * oh * ow;
    const size_t b1 = (total + 255) / 256, b2 = (n_px + 255) / 256;
    MVLDM_REQUIRE(b1 <= 0x7FFFFFFFu && b2 <= 0x7FFFFFFFu, "inception_prep: %zu workgroups", b1 > b2 ? b1 : b2);
    const PilAxis ax = pil_axis(w, ow), ay = pil_axis(h, oh);
    if (src_u8) hipLaunchKernelGGL(inception_prep_h_kernel<true>, dim3((unsigned)b1), dim3(256), 0, s, src, (float*)ws, total, w, ow, ax);
    else hipLaunchKernelGGL(inception_prep_h_kernel<false>, dim3((unsigned)b1), dim3(256), 0, s, src, (float*)ws, total, w, ow, ax);
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(inception_prep_v_kernel<T>, dim3((unsigned)b2), dim3(256), 0, s, (const float*)ws, (T*)dst, n_px, h, oh, ow, ay);
        return check_launch();
    });
}

// the checks shared by the chunk kernels: a map [n][h][w][c] of 16-byte channel chunks within the 32-bit offset range
static int inc_map_ok(const char* who, int n_img, int h, int w, int c, int dtype) {
    MVLDM_REQUIRE(n_img >= 0, "%s: n_img %d", who, n_img);
    MVLDM_REQUIRE(h >= 1 && w >= 1, "%s: map %d x %d: an edge below 1", who, h, w);
    MVLDM_REQUIRE(dtype_ok(dtype), "%s: unknown dtype %d", who, dtype);
    MVLDM_REQUIRE(c >= 1 && c % (16 / (int)dtype_size(dtype)) == 0, "%s: C = %d channels are no whole 16-byte chunks", who, c);
    MVLDM_REQUIRE((double)n_img * h * w * c * (double)dtype_size(dtype) <= (double)kOffsetMax, "%s: %d x %d x %d x %d is past the 32-bit offset range", who,
                  n_img, h, w, c);
    return MVLDM_OK;
}
static int inc_slice_ok(const char* who, int c, int dst_ld, int dst_c_off, int dtype, double rows) {
    const int e = 16 / (int)dtype_size(dtype);
    MVLDM_REQUIRE(dst_ld >= c && dst_c_off >= 0 && dst_c_off + c <= dst_ld && dst_ld % e == 0 && dst_c_off % e == 0,
                  "%s: channels [%d, %d) do not fit rows of %d (in whole 16-byte chunks)", who, dst_c_off, dst_c_off + c, dst_ld);
    MVLDM_REQUIRE(rows * dst_ld * (double)dtype_size(dtype) <= (double)kOffsetMax, "%s: the destination is past the 32-bit offset range", who);
    return MVLDM_OK;
}

int inception_unfold_run(const void* src, void* dst, int n_img, int h, int w, int c, int kh, int kw, int ph, int pw, int dtype, hipStream_t s) {
    int rc = inc_map_ok("inception_unfold", n_img, h, w, c, dtype);
    if (rc != MVLDM_OK) return rc;
    MVLDM_REQUIRE(kh >= 1 && kw >= 1 && kh <= 7 && kw <= 7 && kh % 2 == 1 && kw % 2 == 1, "inception_unfold: kernel %d x %d; odd edges up to 7 are supported", kh, kw);
    MVLDM_REQUIRE(ph == kh / 2 && pw == kw / 2, "inception_unfold: padding (%d, %d) of a %d x %d kernel does not keep the map's size", ph, pw, kh, kw);
    MVLDM_REQUIRE((double)n_img * h * w * c * kh * kw * (double)dtype_size(dtype) <= (double)kOffsetMax,
                  "inception_unfold: the unfolded map is past the 32-bit offset range");
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(src, 16) && aligned(dst, 16), "inception_unfold: null or unaligned pointer");
    const int cp = c / (16 / (int)dtype_size(dtype));
    const size_t total = (size_t)n_img * h * w * kh * kw * cp, blocks = (total + 255) / 256;
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(inception_unfold_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)src, (T*)dst, total, h, w, cp, kh, kw, ph, pw);
        return check_launch();
    });
}

int inception_pool_run(bool is_max, const void* src, void* dst, int n_img, int h, int w, int c, int stride, int pad, int dst_ld, int dst_c_off, int dtype,
                       hipStream_t s) {
    const char* who = is_max ? "inception_maxpool" : "inception_avgpool";
    int rc = inc_map_ok(who, n_img, h, w, c, dtype);
    if (rc != MVLDM_OK) return rc;
    MVLDM_REQUIRE((stride == 1 || stride == 2) && (pad == 0 || pad == 1), "%s: stride %d, padding %d; 1 or 2 and 0 or 1 are supported", who, stride, pad);
    MVLDM_REQUIRE(h + 2 * pad >= 3 && w + 2 * pad >= 3, "%s: a %d x %d map with padding %d holds no 3 x 3 window", who, h, w, pad);
    const int oh = (h + 2 * pad - 3) / stride + 1, ow = (w + 2 * pad - 3) / stride + 1;
    rc = inc_slice_ok(who, c, dst_ld, dst_c_off, dtype, (double)n_img * oh * ow);
    if (rc != MVLDM_OK) return rc;
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(src, 16) && aligned(dst, 16), "%s: null or unaligned pointer", who);
    const int cp = c / (16 / (int)dtype_size(dtype));
    const size_t total = (size_t)n_img * oh * ow * cp, blocks = (total + 255) / 256;
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        if (is_max) hipLaunchKernelGGL((inception_pool_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)src, (T*)dst, total, h, w, cp, oh, ow, stride, pad, dst_ld, dst_c_off);
        else hipLaunchKernelGGL((inception_pool_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)src, (T*)dst, total, h, w, cp, oh, ow, stride, pad, dst_ld, dst_c_off);
        return check_launch();
    });
}

int inception_concat_run(const void* src, void* dst, size_t rows, int c, int dst_ld, int dst_c_off, int relu, int dtype, hipStream_t s) {
    MVLDM_REQUIRE(dtype_ok(dtype), "inception_concat: unknown dtype %d", dtype);
    MVLDM_REQUIRE(c >= 1 && c % (16 / (int)dtype_size(dtype)) == 0, "inception_concat: C = %d channels are no whole 16-byte chunks", c);
    MVLDM_REQUIRE(relu == 0 || relu == 1, "inception_concat: relu %d", relu);
    int rc = inc_slice_ok("inception_concat", c, dst_ld, dst_c_off, dtype, (double)rows);
    if (rc != MVLDM_OK) return rc;
    if (rows == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(src, 16) && aligned(dst, 16), "inception_concat: null or unaligned pointer");
    const int cp = c / (16 / (int)dtype_size(dtype));
    const size_t total = rows * cp, blocks = (total + 255) / 256;
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(inception_concat_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)src, (T*)dst, total, cp, dst_ld, dst_c_off, relu);
        return check_launch();
    });
}

int inception_features_run(const void* feat, int n_img, int h, int w, int c, int dtype, double* out, hipStream_t s) {
    int rc = inc_map_ok("inception_features", n_img, h, w, c, dtype);
    if (rc != MVLDM_OK) return rc;
    MVLDM_REQUIRE((long long)h * w <= kOffsetMax && n_img <= 65535, "inception_features: %d maps of %d x %d are too many or too large", n_img, h, w);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(feat, 16) && aligned(out, 8), "inception_features: null or unaligned pointer");
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(inception_features_kernel<T>, dim3((c + 255) / 256, n_img), dim3(256), 0, s, (const T*)feat, h * w, c, out);
        return check_launch();
    });
}

int frechet_accumulate_run(const double* features, int n, int d, double* state, hipStream_t s) {
    MVLDM_REQUIRE(n >= 0, "frechet_accumulate: n %d", n);
    MVLDM_REQUIRE(frechet_d_ok(d), "frechet_accumulate: d = %d features; multiples of 64 up to %d are supported", d, kFrMaxD);
    if (n == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(features, 8) && aligned(state, 8), "frechet_accumulate: null or unaligned pointer");
    const size_t entries = (size_t)1 + d + (size_t)d * d;
    hipLaunchKernelGGL(frechet_state_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, features, n, d, state);
    return check_launch();
}

size_t frechet_workspace_bytes(int d) { return frechet_d_ok(d) ? frechet_ws_doubles(d) * sizeof(double) : 0; }

template <bool kVectors>
static void frechet_solve(int d, double tol, const FrWs& w, hipStream_t s) {
    hipLaunchKernelGGL(frechet_fro_kernel, dim3(1), dim3(256), 0, s, d, (const double*)w.G, w.ctl);
    for (int sw = 0; sw < kFrSweepCap; ++sw) {
        for (int r = 0; r < d - 1; ++r)
            hipLaunchKernelGGL(frechet_round_kernel<kVectors>, dim3(d / 2), dim3(256), 0, s, d, r, tol, (const double*)w.ctl, w.slot, w.G, w.V);
        hipLaunchKernelGGL(frechet_sweep_kernel, dim3(1), dim3(256), 0, s, d, tol, w.ctl, w.slot);
    }
}

int frechet_compute_run(const double* s1, const double* s2, int d, double* ws, size_t ws_bytes, float* score, double* info, hipStream_t s) {
    MVLDM_REQUIRE(frechet_d_ok(d), "frechet_compute: d = %d features; multiples of 64 up to %d are supported", d, kFrMaxD);
    MVLDM_REQUIRE(ws_bytes >= frechet_workspace_bytes(d), "frechet_compute: workspace of %zu bytes, need %zu", ws_bytes, frechet_workspace_bytes(d));
    MVLDM_REQUIRE(aligned(s1, 8) && aligned(s2, 8) && aligned(ws, 8) && aligned(score, 4) && aligned(info, 8),
                  "frechet_compute: null or unaligned pointer");
    const FrWs w = frechet_ws(ws, d);
    const double tol = sqrt((double)d) * 2.220446049250313e-16;     // dgesvj's: the round-off of a d-term dot product of unit vectors
    const unsigned sq = (unsigned)(((size_t)d * d + 255) / 256);
    hipLaunchKernelGGL(frechet_mean_kernel, dim3((d + 255) / 256), dim3(256), 0, s, s1, s2, d, w);
    hipLaunchKernelGGL(frechet_sigma_kernel, dim3(sq), dim3(256), 0, s, s1, s2, d, w);
    hipLaunchKernelGGL(frechet_head_kernel, dim3(1), dim3(256), 0, s, d, w);
    frechet_solve<true>(d, tol, w, s);
    hipLaunchKernelGGL(frechet_lambda_kernel<true>, dim3(d), dim3(256), 0, s, d, (const double*)w.G, (const double*)w.V, w.lam);
    // T[j] = Sigma2 v_j (B symmetric: T[j][i] = sum_k V[j][k] B[i][k]); M[i][j] = v_i . T[j] -> G's storage is free again after the scale
    hipLaunchKernelGGL(frechet_nt_kernel, dim3(d / 64, d / 64), dim3(256), 0, s, d, (const double*)w.V, (const double*)w.B, w.T);
    hipLaunchKernelGGL(frechet_nt_kernel, dim3(d / 64, d / 64), dim3(256), 0, s, d, (const double*)w.V, (const double*)w.T, w.B);
    hipLaunchKernelGGL(frechet_scale_kernel, dim3(sq), dim3(256), 0, s, d, (const double*)w.lam, (const double*)w.B, w.G);
    hipLaunchKernelGGL(frechet_next_kernel, dim3(1), dim3(64), 0, s, w.ctl);
    frechet_solve<false>(d, tol, w, s);
    hipLaunchKernelGGL(frechet_lambda_kernel<false>, dim3(d), dim3(256), 0, s, d, (const double*)w.G, (const double*)w.V, w.lam);
    hipLaunchKernelGGL(frechet_score_kernel, dim3(1), dim3(256), 0, s, d, s1, s2, (const double*)w.ctl, (const double*)w.lam, score, info);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_inception_workspace_bytes(int n_img, int h, int ow) { return inception_workspace_bytes(n_img, h, ow); }
extern "C" int mvldm_inception_prep(const void* src, int src_u8, void* dst, int n_img, int h, int w, int oh, int ow, int c_pad, int dtype, void* workspace,
                                    size_t workspace_bytes, mvldm_stream_t stream) {
    return inception_prep_run(src, src_u8, dst, n_img, h, w, oh, ow, c_pad, dtype, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int mvldm_inception_unfold(const void* src, void* dst, int n_img, int h, int w, int c, int kh, int kw, int pad_h, int pad_w, int dtype,
                                      mvldm_stream_t stream) {
    return inception_unfold_run(src, dst, n_img, h, w, c, kh, kw, pad_h, pad_w, dtype, (hipStream_t)stream);
}
extern "C" int mvldm_inception_maxpool(const void* src, void* dst, int n_img, int h, int w, int c, int stride, int pad, int dst_ld, int dst_c_off, int dtype,
                                       mvldm_stream_t stream) {
    return inception_pool_run(true, src, dst, n_img, h, w, c, stride, pad, dst_ld, dst_c_off, dtype, (hipStream_t)stream);
}
extern "C" int mvldm_inception_avgpool(const void* src, void* dst, int n_img, int h, int w, int c, int dst_ld, int dst_c_off, int dtype, mvldm_stream_t stream) {
    return inception_pool_run(false, src, dst, n_img, h, w, c, 1, 1, dst_ld, dst_c_off, dtype, (hipStream_t)stream);
}
extern "C" int mvldm_inception_concat(const void* src, void* dst, size_t rows, int c, int dst_ld, int dst_c_off, int relu, int dtype, mvldm_stream_t stream) {
    return inception_concat_run(src, dst, rows, c, dst_ld, dst_c_off, relu, dtype, (hipStream_t)stream);
}
extern "C" int mvldm_inception_features(const void* feat, int n_img, int h, int w, int c, int dtype, double* features, mvldm_stream_t stream) {
    return inception_features_run(feat, n_img, h, w, c, dtype, features, (hipStream_t)stream);
}
extern "C" int mvldm_frechet_accumulate(const double* features, int n, int d, double* state, mvldm_stream_t stream) {
    return frechet_accumulate_run(features, n, d, state, (hipStream_t)stream);
}
extern "C" size_t mvldm_frechet_workspace_bytes(int d) { return frechet_workspace_bytes(d); }
extern "C" int mvldm_frechet_compute(const double* state1, const double* state2, int d, double* workspace, size_t workspace_bytes, float* score, double* info,
                                     mvldm_stream_t stream) {
    return frechet_compute_run(state1, state2, d, workspace, workspace_bytes, score, info, (hipStream_t)stream);
}
