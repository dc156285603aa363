// FID (feature = 64) around the implicit GEMM (include/mvldm.h, "FID"): the glue between the three 3x3 convolutions of the Inception-v3 stem,
// which mvldm_igemm_fwd runs with BatchNorm folded into weight and bias, and torchmetrics' FrechetInceptionDistance(feature=64,
// normalize=True) as src/evaluation/metric_computer.py:22,65-68 uses it.
//   fid_prep        fp32 [0, 1] or uint8 NCHW [n][3][h][w] -> NHWC [n][oh][ow][c_pad] in the compute dtype: the package's byte quantisation
//                   (x * 255 in fp32, clamped to [0, 255], truncated), torch-fidelity's TensorFlow-1 bilinear resize (source coordinate
//                   float(i) * (in / out) in fp32, no half-pixel centres, lerp along x first), (v - 128) / 128; pad channels zero
//   fid_pool        reads the PRE-activation output of the third conv: ReLU, max-pool 3x3 / stride 2 / no padding / floor, and the sum of
//                   the pooled map per channel in fp64 from the first add.  The pooled map is never written.  A lane owns one 16-byte
//                   channel chunk and walks every `rows`-th output pixel of the workgroup's band of output rows; the lanes that own the same
//                   chunk are added through LDS in row order.  One fp64 partial per (image, band, channel), no atomics.
//   fid_accumulate  the partials of each image in band order / pixels -> the fp64 features [n][c]; then frechet_accumulate (inception.hip)
//                   adds them to the state (count, sum f, sum f^T f)
//   fid_compute     ONE workgroup: mu and Sigma of both states in fp64, Sigma1 = V D V^T by cyclic Jacobi in LDS, the eigenvalues of
//                   S = D^1/2 V^T Sigma2 V D^1/2 (the spectrum of Sigma1^1/2 Sigma2 Sigma1^1/2) the same way,
//                   fid = |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2 - 2 sum sqrt(max(lambda_i, 0))
#include <math.h>

#include "common.h"

namespace mvldm {

constexpr int kFidD = 64;               // the width fid_compute is built for
constexpr int kFidLd = 65;              // doubles per LDS matrix row: a column walk (stride 520 bytes) then covers the 32 even banks of the
                                        // 64-dword bank row once per half wave, a row walk is contiguous -- both free of conflicts
constexpr int kFidPairs = kFidD / 2;    // disjoint rotations of one round
constexpr int kFidRounds = kFidD - 1;   // rounds of one sweep (round-robin: every pair once)
constexpr int kFidSweepCap = 30;        // a solve needs 7 - 12 sweeps, 19 on eigenvalues over 12 decades; the loop bound is this constant
constexpr double kFidTol = 1e-22;       // a solve has converged when off(A)^2 <= kFidTol^2 * |A|_F^2
constexpr int kFidBandPx = 512;         // output pixels of one pool workgroup, rounded up to whole output rows

template <typename T, bool U8>
__global__ __launch_bounds__(256) void fid_prep_kernel(const void* __restrict__ src, T* __restrict__ dst, size_t n_px, int h, int w, int oh, int ow,
                                                       float scale_h, float scale_w) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // (image * oh + oy) * ow + ox
    if (idx >= n_px) return;
    const int ox = (int)(idx % ow);
    const size_t t = idx / ow;
    const int oy = (int)(t % oh);
    const size_t img = t / oh;
    const float sy = (float)oy * scale_h, sx = (float)ox * scale_w;
    const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);   // the min never binds (oy < oh): it keeps the loads inside whatever fp32 does
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float dy = sy - (float)y0, dx = sx - (float)x0;
    Chunk<T> c;
    c.zero();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const size_t plane = (img * 3 + ch) * (size_t)h * w;
        float a[4];
        const size_t at[4] = {plane + (size_t)y0 * w + x0, plane + (size_t)y0 * w + x1, plane + (size_t)y1 * w + x0, plane + (size_t)y1 * w + x1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (U8) a[k] = (float)((const uint8_t*)src)[at[k]];
            else a[k] = truncf(fminf(fmaxf(((const float*)src)[at[k]] * 255.f, 0.f), 255.f));      // .byte() of a value in range; clamped outside it
        }
        const float v0 = a[0] + (a[1] - a[0]) * dx, v1 = a[2] + (a[3] - a[2]) * dx;
        c.set(ch, ((v0 + (v1 - v0) * dy) - 128.f) / 128.f);
    }
    store_chunk(dst + idx * Chunk<T>::N, c);
}

// workgroup blk of image img: output rows [blk band, min((blk + 1) band, oh)); thread t owns chunk t % CP of the band's output pixels t / CP + k rows
template <typename T>
__global__ __launch_bounds__(256) void fid_pool_kernel(const T* __restrict__ f, int h, int w, int C, int oh, int ow, int band, int slots,
                                                       double* __restrict__ ws) {
    constexpr int E = Chunk<T>::N;
    __shared__ double s_red[256 * E];
    const int img = blockIdx.x / slots, blk = blockIdx.x % slots;
    const int CP = C / E, rows = 256 / CP;
    const int j = threadIdx.x % CP, r = threadIdx.x / CP;
    const int oy0 = blk * band, n_q = (min(oy0 + band, oh) - oy0) * ow;
    const T* src = f + (size_t)img * h * w * C + (size_t)j * E;
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0;
    if (r < rows)
        for (int q = r; q < n_q; q += rows) {
            const int oy = oy0 + q / ow, ox = q % ow;
            float m[E];
#pragma unroll
            for (int e = 0; e < E; ++e) m[e] = 0.f;                // the ReLU: max(0, window)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const Chunk<T> c = load_chunk(src + ((size_t)(2 * oy + dy) * w + (2 * ox + dx)) * C);
#pragma unroll
                    for (int e = 0; e < E; ++e) m[e] = fmaxf(m[e], c.get(e));
                }
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += (double)m[e];
        }
    if (r < rows) {
#pragma unroll
        for (int e = 0; e < E; ++e) s_red[r * C + j * E + e] = acc[e];
    }
    __syncthreads();
    double* dst = ws + ((size_t)img * slots + blk) * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        double v = s_red[c];
        for (int q = 1; q < rows; ++q) v += s_red[q * C + c];
        dst[c] = v;
    }
}

__global__ __launch_bounds__(256) void fid_features_kernel(const double* __restrict__ part, int slots, int C, double px, double* __restrict__ feat,
                                                           double* __restrict__ feat_out) {
    const double* p = part + (size_t)blockIdx.x * slots * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        double v = 0.0;
        for (int b = 0; b < slots; ++b) v += p[(size_t)b * C + c];
        v /= px;
        feat[(size_t)blockIdx.x * C + c] = v;
        if (feat_out) feat_out[(size_t)blockIdx.x * C + c] = v;
    }
}

// ---- the Frechet distance: one workgroup of 256 threads -------------------------------------------------------------------------------
struct FidLds {
    double *A, *V, *B;                      // three [64][kFidLd] matrices
    double *c, *s, *pp, *qq, *red;          // a round's rotations and new diagonal entries; the reduction tree
    int *p, *q;
};

// every thread gets the sum of the 256 values, added in one fixed tree
__device__ __forceinline__ double fid_block_sum(double v, double* red) {
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

// sum of squares of A: thread t takes row t / 4, columns (t % 4) 16 ... + 16
__device__ __forceinline__ double fid_sumsq(const double* A, bool with_diagonal, double* red) {
    const int i = threadIdx.x >> 2, j0 = (threadIdx.x & 3) * 16;
    double v = 0.0;
#pragma unroll 4
    for (int j = j0; j < j0 + 16; ++j) {
        const double a = A[i * kFidLd + j];
        if (with_diagonal || i != j) v += a * a;
    }
    return fid_block_sum(v, red);
}

// Cyclic Jacobi on the symmetric A (LDS), round-robin ordering: round r pairs 63 with r and (r + k) % 63 with (r - k) % 63, k = 1 ... 31.
// One round: threads 0 ... 31 compute the 32 rotations from A as it stands; then A <- A J (thread = row x 8 pairs, and V <- V J with it);
// then A <- J^T A (thread = column x 8 pairs), where the 2 x 2 blocks of the pairs get their closed form (a_pq = 0 exactly).  Every branch
// around a barrier depends on values all threads read from LDS: the loop is block-uniform.  At most kFidSweepCap sweeps.
template <bool kVectors>
__device__ void fid_jacobi(const FidLds& L, int* sweeps, double* off_rel, bool* converged) {
    const int t = threadIdx.x;
    double* A = L.A;
    const double fro2 = fid_sumsq(A, true, L.red);
    double off2 = fid_sumsq(A, false, L.red);
    const double thresh = kFidTol * kFidTol * fro2;
    int sw = 0;
    while (!(off2 <= thresh) && sw < kFidSweepCap) {
        for (int r = 0; r < kFidRounds; ++r) {
            if (t < kFidPairs) {
                const int a = t == 0 ? kFidD - 1 : (r + t) % kFidRounds, b = t == 0 ? r : (r - t + kFidRounds) % kFidRounds;
                const int p = min(a, b), q = max(a, b);
                const double app = A[p * kFidLd + p], aqq = A[q * kFidLd + q], apq = A[p * kFidLd + q];
                double c = 1.0, s = 0.0, tt = 0.0;
                if (apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(tt * tt + 1.0);
                    s = tt * c;
                }
                L.p[t] = p;
                L.q[t] = q;
                L.c[t] = c;
                L.s[t] = s;
                L.pp[t] = app - tt * apq;
                L.qq[t] = aqq + tt * apq;
            }
            __syncthreads();
            {
                const int i = t & 63, k0 = (t >> 6) * 8;
#pragma unroll 4
                for (int k = k0; k < k0 + 8; ++k) {
                    const int p = L.p[k], q = L.q[k];
                    const double c = L.c[k], s = L.s[k];
                    const double x = A[i * kFidLd + p], y = A[i * kFidLd + q];
                    A[i * kFidLd + p] = c * x - s * y;
                    A[i * kFidLd + q] = s * x + c * y;
                    if (kVectors) {
                        const double vx = L.V[i * kFidLd + p], vy = L.V[i * kFidLd + q];
                        L.V[i * kFidLd + p] = c * vx - s * vy;
                        L.V[i * kFidLd + q] = s * vx + c * vy;
                    }
                }
            }
            __syncthreads();
            {
                const int j = t & 63, k0 = (t >> 6) * 8;
#pragma unroll 4
                for (int k = k0; k < k0 + 8; ++k) {
                    const int p = L.p[k], q = L.q[k];
                    const double c = L.c[k], s = L.s[k];
                    const double x = A[p * kFidLd + j], y = A[q * kFidLd + j];
                    double nx = c * x - s * y, ny = s * x + c * y;
                    if (j == p) {
                        nx = L.pp[k];
                        ny = 0.0;
                    } else if (j == q) {
                        nx = 0.0;
                        ny = L.qq[k];
                    }
                    A[p * kFidLd + j] = nx;
                    A[q * kFidLd + j] = ny;
                }
            }
            __syncthreads();
        }
        ++sw;
        off2 = fid_sumsq(A, false, L.red);
    }
    *sweeps = sw;
    *off_rel = fro2 > 0.0 ? sqrt(off2 / fro2) : 0.0;
    *converged = off2 <= thresh;
}

constexpr int kFidSmemDoubles = 3 * kFidD * kFidLd + 4 * kFidPairs + 256 + 3 * kFidD;
constexpr int kFidSmemBytes = kFidSmemDoubles * 8 + 2 * kFidPairs * 4;

__global__ __launch_bounds__(256) void fid_compute_kernel(const double* __restrict__ s1, const double* __restrict__ s2, float* __restrict__ score,
                                                          double* __restrict__ info) {
    extern __shared__ double smem[];
    constexpr int D = kFidD, LD = kFidLd;
    FidLds L;
    L.A = smem;
    L.V = L.A + D * LD;
    L.B = L.V + D * LD;
    L.c = L.B + D * LD;
    L.s = L.c + kFidPairs;
    L.pp = L.s + kFidPairs;
    L.qq = L.pp + kFidPairs;
    L.red = L.qq + kFidPairs;
    double* mu1 = L.red + 256;
    double* mu2 = mu1 + D;
    double* sd = mu2 + D;
    L.p = (int*)(sd + D);
    L.q = L.p + kFidPairs;
    const int t = threadIdx.x;
    const double n1 = s1[0], n2 = s2[0];
    if (t < D) {
        mu1[t] = s1[1 + t] / n1;
        mu2[t] = s2[1 + t] / n2;
    }
    __syncthreads();
    for (int e = t; e < D * D; e += 256) {
        const int i = e / D, j = e % D;
        L.A[i * LD + j] = (s1[1 + D + e] - n1 * (mu1[i] * mu1[j])) / (n1 - 1.0);
        L.B[i * LD + j] = (s2[1 + D + e] - n2 * (mu2[i] * mu2[j])) / (n2 - 1.0);
        L.V[i * LD + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    double head = 0.0;                          // thread 0: |mu1 - mu2|^2 + (tr Sigma1 + tr Sigma2), each in index order
    if (t == 0) {
        double dm = 0.0, tr1 = 0.0, tr2 = 0.0;
        for (int i = 0; i < D; ++i) {
            const double d = mu1[i] - mu2[i];
            dm += d * d;
            tr1 += L.A[i * LD + i];
            tr2 += L.B[i * LD + i];
        }
        head = dm + (tr1 + tr2);
    }
    int sw1, sw2;
    double off1, off2;
    bool ok1, ok2;
    fid_jacobi<true>(L, &sw1, &off1, &ok1);
    if (t < D) sd[t] = sqrt(fmax(L.A[t * LD + t], 0.0));
    // T = Sigma2 V -> A (thread: column j, 16 rows), then M = V^T T -> B
    {
        const int j = t & 63, i0 = (t >> 6) * 16;
        __syncthreads();
#pragma nounroll
        for (int i = i0; i < i0 + 16; ++i) {
            double v = 0.0;
#pragma unroll 8
            for (int k = 0; k < D; ++k) v += L.B[i * LD + k] * L.V[k * LD + j];
            L.A[i * LD + j] = v;
        }
        __syncthreads();
#pragma nounroll
        for (int i = i0; i < i0 + 16; ++i) {
            double v = 0.0;
#pragma unroll 8
            for (int k = 0; k < D; ++k) v += L.V[k * LD + i] * L.A[k * LD + j];
            L.B[i * LD + j] = v;
        }
        __syncthreads();
    }
    // S = D^1/2 sym(M) D^1/2 -> A: one thread per unordered pair writes both halves, so S is symmetric to the bit
    for (int e = t; e < D * D; e += 256) {
        const int i = e / D, j = e % D;
        if (i <= j) {
            const double v = (sd[i] * (0.5 * (L.B[i * LD + j] + L.B[j * LD + i]))) * sd[j];
            L.A[i * LD + j] = v;
            L.A[j * LD + i] = v;
        }
    }
    __syncthreads();
    fid_jacobi<false>(L, &sw2, &off2, &ok2);
    if (t == 0) {
        double c = 0.0;
        for (int i = 0; i < D; ++i) c += sqrt(fmax(L.A[i * LD + i], 0.0));
        const double fid = head - 2.0 * c;
        const bool good = ok1 && ok2 && n1 >= 2.0 && n2 >= 2.0;
        *score = good ? (float)fid : __builtin_nanf("");
        info[0] = (double)sw1;
        info[1] = off1;
        info[2] = (double)sw2;
        info[3] = off2;
        info[4] = (double)((ok1 ? 0 : 1) + (ok2 ? 0 : 1));     // solves that stopped at the sweep cap
        info[5] = fid;                                          // the score before its rounding to fp32
        info[6] = c;
        info[7] = head;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int frechet_accumulate_run(const double* features, int n, int d, double* state, hipStream_t s);      // inception.hip: d a multiple of 64 up to 2048
static int fid_band(int ow) { return (kFidBandPx + ow - 1) / ow; }      // output rows of one workgroup

int fid_pool_slots(int h, int w, int c) {
    if (h < 3 || w < 3 || !channels_ok(c) || (long long)h * w > 0x7FFFFFFF) return 0;
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1, band = fid_band(ow);
    return (oh + band - 1) / band;
}

size_t fid_workspace_bytes(int n_img, int h, int w, int c) {
    const int slots = fid_pool_slots(h, w, c);
    if (n_img < 1 || slots == 0) return 0;
    return (size_t)n_img * ((size_t)slots + 1) * c * sizeof(double);      // the partials, then the features
}

int fid_prep_run(const void* src, int src_u8, void* dst, int n_img, int h, int w, int oh, int ow, int c_pad, int dtype, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "fid_prep: n_img %d", n_img);
    MVLDM_REQUIRE(h >= 1 && w >= 1 && oh >= 1 && ow >= 1, "fid_prep: image %d x %d -> %d x %d: an edge below 1", h, w, oh, ow);
    MVLDM_REQUIRE(src_u8 == 0 || src_u8 == 1, "fid_prep: src_u8 %d", src_u8);
    MVLDM_REQUIRE(dtype_ok(dtype), "fid_prep: unknown dtype %d", dtype);
    MVLDM_REQUIRE(c_pad == (dtype == MVLDM_F32 ? 4 : 8), "fid_prep: c_pad %d is not the 16-byte padding of 3 channels in dtype %d", c_pad, dtype);
    MVLDM_REQUIRE((long long)h * w <= 0x7FFFFFFF && (long long)oh * ow <= 0x7FFFFFFF, "fid_prep: %d x %d -> %d x %d is too large", h, w, oh, ow);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(src, src_u8 ? 1 : 4) && aligned(dst, 16), "fid_prep: null or unaligned pointer");
    const size_t n_px = (size_t)n_img * oh * ow, blocks = (n_px + 255) / 256;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "fid_prep: %zu workgroups", blocks);
    const float scale_h = (float)h / (float)oh, scale_w = (float)w / (float)ow;
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        if (src_u8) hipLaunchKernelGGL((fid_prep_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, src, (T*)dst, n_px, h, w, oh, ow, scale_h, scale_w);
        else hipLaunchKernelGGL((fid_prep_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, src, (T*)dst, n_px, h, w, oh, ow, scale_h, scale_w);
        return check_launch();
    });
}

int fid_pool_run(const void* feat, int n_img, int h, int w, int c, int dtype, double* ws, size_t ws_bytes, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "fid_pool: n_img %d", n_img);
    MVLDM_REQUIRE(h >= 3 && w >= 3, "fid_pool: a %d x %d map holds no 3 x 3 window", h, w);
    MVLDM_REQUIRE(channels_ok(c), "fid_pool: C = %d channels; multiples of 64 up to 512 are supported", c);
    MVLDM_REQUIRE(dtype_ok(dtype), "fid_pool: unknown dtype %d", dtype);
    const int slots = fid_pool_slots(h, w, c);
    MVLDM_REQUIRE(slots > 0, "fid_pool: a %d x %d map is too large", h, w);
    const size_t need = (size_t)n_img * slots * c * sizeof(double);
    MVLDM_REQUIRE(ws_bytes >= need, "fid_pool: workspace of %zu bytes, need %zu", ws_bytes, need);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(feat, 16) && aligned(ws, 8), "fid_pool: null or unaligned pointer");
    const size_t blocks = (size_t)n_img * slots;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFu, "fid_pool: %zu workgroups", blocks);
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    return dispatch_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(fid_pool_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)feat, h, w, c, oh, ow, fid_band(ow), slots, ws);
        return check_launch();
    });
}

int fid_accumulate_run(double* ws, size_t ws_bytes, int n_img, int h, int w, int c, double* features, double* state, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "fid_accumulate: n_img %d", n_img);
    const int slots = fid_pool_slots(h, w, c);
    MVLDM_REQUIRE(slots > 0, "fid_accumulate: a %d x %d map of %d channels is refused (an edge below 3, C no multiple of 64 up to 512, or too large)", h, w, c);
    const size_t need = (size_t)n_img * ((size_t)slots + 1) * c * sizeof(double);
    MVLDM_REQUIRE(ws_bytes >= need, "fid_accumulate: workspace of %zu bytes, need %zu", ws_bytes, need);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(ws, 8) && (state == nullptr || aligned(state, 8)) && (features == nullptr || aligned(features, 8)),
                  "fid_accumulate: null or unaligned pointer");
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    double* feat = ws + (size_t)n_img * slots * c;
    hipLaunchKernelGGL(fid_features_kernel, dim3(n_img), dim3(256), 0, s, (const double*)ws, slots, c, (double)oh * (double)ow, feat, features);
    return state ? frechet_accumulate_run(feat, n_img, c, state, s) : check_launch();
}

int fid_compute_run(const double* s1, const double* s2, int c, float* score, double* info, hipStream_t s) {
    MVLDM_REQUIRE(c == kFidD, "fid_compute: C = %d features; the solve is built for 64 (feature=64)", c);
    MVLDM_REQUIRE(aligned(s1, 8) && aligned(s2, 8) && aligned(score, 4) && aligned(info, 8), "fid_compute: null or unaligned pointer");
    static std::atomic<uint64_t> mask{0};
    const int rc = ensure_dyn_smem((const void*)fid_compute_kernel, kFidSmemBytes, mask);
    if (rc != MVLDM_OK) return rc;
    hipLaunchKernelGGL(fid_compute_kernel, dim3(1), dim3(256), kFidSmemBytes, s, s1, s2, score, info);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_fid_workspace_bytes(int n_img, int h, int w, int c) { return fid_workspace_bytes(n_img, h, w, c); }
extern "C" int mvldm_fid_pool_slots(int h, int w, int c) { return fid_pool_slots(h, w, c); }
extern "C" int mvldm_fid_prep(const void* src, int src_u8, void* dst, int n_img, int h, int w, int oh, int ow, int c_pad, int dtype,
                              mvldm_stream_t stream) {
    return fid_prep_run(src, src_u8, dst, n_img, h, w, oh, ow, c_pad, dtype, (hipStream_t)stream);
}
extern "C" int mvldm_fid_pool(const void* feat, int n_img, int h, int w, int c, int dtype, double* workspace, size_t workspace_bytes,
                              mvldm_stream_t stream) {
    return fid_pool_run(feat, n_img, h, w, c, dtype, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int mvldm_fid_accumulate(double* workspace, size_t workspace_bytes, int n_img, int h, int w, int c, double* features, double* state,
                                    mvldm_stream_t stream) {
    return fid_accumulate_run(workspace, workspace_bytes, n_img, h, w, c, features, state, (hipStream_t)stream);
}
extern "C" int mvldm_fid_compute(const double* state1, const double* state2, int c, float* score, double* info, mvldm_stream_t stream) {
    return fid_compute_run(state1, state2, c, score, info, (hipStream_t)stream);
}
