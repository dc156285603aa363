// Clean-KID (include/mvldm.h, "Clean-KID"): cleanfid.fid.kernel_distance on the fp64 features, the subsets given as index lists.
//   kid_tile     one workgroup = one 64 x 64 tile of one of the three Grams of one subset (x x^T, y y^T, x y^T; x = rows idx2 of f2, y = rows
//                idx1 of f1).  The two symmetric Grams launch only the tile pairs a <= b and count a < b twice.  256 threads = 4 waves in a
//                2 x 2 grid, each wave a 32 x 32 quadrant as 2 x 2 blocks of v_mfma_f64_16x16x4_f64.  d is walked in chunks of 16 doubles:
//                the row index is gathered (and clamped to [0, n)) once per row, then every chunk is one contiguous 128-byte piece of the
//                row, fetched to registers one chunk ahead and staged through LDS.  The epilogue applies (g / d + 1)^3 in registers, zeroes
//                rows and columns at or beyond m and the diagonal of the symmetric Grams, and adds the tile in one fixed tree (16 values a
//                lane in order, a butterfly over the wave, the four waves in order) to ONE double of the workspace.  No m x m matrix exists.
//   kid_subset   one workgroup a subset: the tile partials in index order -> A_s (the two symmetric Grams) and B_s (the cross Gram);
//                per_subset[s] = A_s / (m - 1) - 2 B_s / m, or NaN when one of the subset's indices lies outside [0, n) (the lists are
//                scanned again here: no flag is shared with kid_tile); scale_s = |A_s| / (m - 1) + 2 |B_s| / m.
//   kid_final    one thread: the subsets in order -> info and score.
// No floating-point atomics anywhere: two calls give the same bits.
#include <math.h>

#include "common.h"

namespace mvldm {

typedef __attribute__((ext_vector_type(4))) double f64x4;
typedef __attribute__((ext_vector_type(2))) double f64x2;

constexpr int kKidTile = 64;            // rows and columns of a workgroup's tile
constexpr int kKidBk = 16;              // doubles of a row per K-chunk: 128 bytes
constexpr int kKidLd = kKidBk + 1;      // doubles per LDS row: rows r and r + 1 are 34 banks apart, so the 16 rows x 2 k of half a wave's
                                        // 8-byte fragment read cover the 64 banks once
constexpr int kKidMaxD = 2048;          // the widths mvldm_frechet_* takes

static bool kid_d_ok(int d) { return d >= 64 && d <= kKidMaxD && d % 64 == 0; }
static long long kid_tiles(int m) { return (m + kKidTile - 1) / kKidTile; }
// tiles of one subset: the pairs a <= b of the two symmetric Grams, then every tile of the cross Gram
static long long kid_tiles_per_subset(int m) {
    const long long t = kid_tiles(m);
    return t * (t + 1) + t * t;
}

__global__ __launch_bounds__(256) void kid_tile_kernel(const double* __restrict__ f1, int n1, const double* __restrict__ f2, int n2, int d,
                                                       const int32_t* __restrict__ idx1, const int32_t* __restrict__ idx2, int m, int T,
                                                       int tiles_per_subset, double* __restrict__ partial) {
    __shared__ double s_a[kKidTile * kKidLd];
    __shared__ double s_b[kKidTile * kKidLd];
    __shared__ int s_row[2 * kKidTile];
    __shared__ double s_red[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int subset = blockIdx.x / tiles_per_subset;
    int r = blockIdx.x % tiles_per_subset;
    const int pairs = T * (T + 1) / 2;
    // which Gram, which tile: 0 = x x^T, 1 = y y^T (pairs a <= b, row-major over the upper triangle), 2 = x y^T
    int gram, ta = 0, tb;
    if (r < 2 * pairs) {
        gram = r / pairs;
        r %= pairs;
        while (r >= T - ta) {
            r -= T - ta;
            ++ta;
        }
        tb = ta + r;
    } else {
        gram = 2;
        r -= 2 * pairs;
        ta = r / T;
        tb = r % T;
    }
    const bool sym = gram != 2;
    const bool a_is_x = gram != 1, b_is_x = gram == 0;
    const double* fa = a_is_x ? f2 : f1;
    const double* fb = b_is_x ? f2 : f1;
    // the rows of both operands, clamped before they become addresses; a row at or beyond m reads row 0 and is zeroed in the epilogue
    if (t < 2 * kKidTile) {
        const bool is_a = t < kKidTile;
        const bool from_x = is_a ? a_is_x : b_is_x;
        const int row = (is_a ? ta : tb) * kKidTile + (t & (kKidTile - 1));
        const int n = from_x ? n2 : n1;
        int v = 0;
        if (row < m) v = (from_x ? idx2 : idx1)[(size_t)subset * m + row];
        s_row[t] = min(max(v, 0), n - 1);
    }
    __syncthreads();
    // staging: thread t moves 16 bytes (2 doubles) of rows t / 8 and t / 8 + 32 of each operand per chunk
    const int lr = t >> 3, lc = (t & 7) * 2;
    const double* pa0 = fa + (size_t)s_row[lr] * d + lc;
    const double* pa1 = fa + (size_t)s_row[lr + 32] * d + lc;
    const double* pb0 = fb + (size_t)s_row[kKidTile + lr] * d + lc;
    const double* pb1 = fb + (size_t)s_row[kKidTile + lr + 32] * d + lc;
    f64x2 ra0 = *(const f64x2*)pa0, ra1 = *(const f64x2*)pa1, rb0 = *(const f64x2*)pb0, rb1 = *(const f64x2*)pb1;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;         // the wave's quadrant
    const int fr = lane & 15, fk = lane >> 4;                      // fragment: A[row fr][k fk], B[k fk][col fr]
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += kKidBk) {
        s_a[lr * kKidLd + lc] = ra0.x;
        s_a[lr * kKidLd + lc + 1] = ra0.y;
        s_a[(lr + 32) * kKidLd + lc] = ra1.x;
        s_a[(lr + 32) * kKidLd + lc + 1] = ra1.y;
        s_b[lr * kKidLd + lc] = rb0.x;
        s_b[lr * kKidLd + lc + 1] = rb0.y;
        s_b[(lr + 32) * kKidLd + lc] = rb1.x;
        s_b[(lr + 32) * kKidLd + lc + 1] = rb1.y;
        __syncthreads();
        if (k0 + kKidBk < d) {                                      // the next chunk is in flight while this one is multiplied
            ra0 = *(const f64x2*)(pa0 + k0 + kKidBk);
            ra1 = *(const f64x2*)(pa1 + k0 + kKidBk);
            rb0 = *(const f64x2*)(pb0 + k0 + kKidBk);
            rb1 = *(const f64x2*)(pb1 + k0 + kKidBk);
        }
#pragma unroll
        for (int kk = 0; kk < kKidBk; kk += 4) {
            const double a0 = s_a[(wr + fr) * kKidLd + kk + fk], a1 = s_a[(wr + 16 + fr) * kKidLd + kk + fk];
            const double b0 = s_b[(wc + fr) * kKidLd + kk + fk], b1 = s_b[(wc + 16 + fr) * kKidLd + kk + fk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // result register q of block (i, j): column lane & 15, row (lane >> 4) + 4 q -- the f64 map, not the one of the 16-bit forms
    const double dd = (double)d;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = ta * kKidTile + wr + i * 16 + fk + 4 * q, col = tb * kKidTile + wc + j * 16 + fr;
                const double v = acc[i][j][q] / dd + 1.0;
                const double c = v * v * v;
                sum += (row < m && col < m && !(sym && row == col)) ? c : 0.0;
            }
    sum = wave_sum_d(sum);
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    if (t == 0) {
        const double v = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        partial[blockIdx.x] = (sym && ta < tb) ? 2.0 * v : v;
    }
}

// workspace: [num_subsets][tiles_per_subset] partials, [num_subsets] per-subset values (used when per_subset is NULL), [num_subsets] scales
__global__ __launch_bounds__(256) void kid_subset_kernel(const double* __restrict__ partial, int tiles_per_subset, int pairs,
                                                         const int32_t* __restrict__ idx1, int n1, const int32_t* __restrict__ idx2, int n2, int m,
                                                         double* __restrict__ per, double* __restrict__ scale) {
    __shared__ int s_bad;
    const int s = blockIdx.x, t = threadIdx.x;
    if (t == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int i = t; i < m; i += 256) {
        const int a = idx1[(size_t)s * m + i], b = idx2[(size_t)s * m + i];
        bad = bad || a < 0 || a >= n1 || b < 0 || b >= n2;
    }
    if (bad) s_bad = 1;                                             // every writer stores the same value
    __syncthreads();
    if (t == 0) {
        const double* p = partial + (size_t)s * tiles_per_subset;
        double A = 0.0, B = 0.0;
        for (int i = 0; i < 2 * pairs; ++i) A += p[i];
        for (int i = 2 * pairs; i < tiles_per_subset; ++i) B += p[i];
        const double m1 = (double)(m - 1), mm = (double)m;
        per[s] = s_bad ? __builtin_nan("") : A / m1 - B * 2.0 / mm;
        scale[s] = fabs(A) / m1 + fabs(B) * 2.0 / mm;
    }
}

__global__ __launch_bounds__(64) void kid_final_kernel(const double* __restrict__ per, const double* __restrict__ scale, int num_subsets, int m,
                                                       float* __restrict__ score, double* __restrict__ info) {
    if (threadIdx.x != 0) return;
    double tsum = 0.0, ssum = 0.0;
    int bad = 0;
    for (int s = 0; s < num_subsets; ++s) {
        const double v = per[s];
        tsum += v;
        ssum += scale[s];
        bad += v != v ? 1 : 0;
    }
    const double kid = tsum / (double)num_subsets / (double)m;
    info[0] = kid;
    info[1] = ssum / (double)num_subsets / (double)m;
    info[2] = (double)m;
    info[3] = (double)bad;
    *score = (float)kid;
}

size_t kid_workspace_bytes(int m, int num_subsets) {
    if (m < 2 || num_subsets < 1) return 0;
    return (size_t)num_subsets * ((size_t)kid_tiles_per_subset(m) + 2) * sizeof(double);
}

int kid_compute_run(const double* f1, int n1, const double* f2, int n2, int d, const int32_t* idx1, const int32_t* idx2, int num_subsets, int m,
                    double* ws, size_t ws_bytes, float* score, double* per_subset, double* info, hipStream_t s) {
    MVLDM_REQUIRE(num_subsets >= 1, "kid_compute: %d subsets", num_subsets);
    MVLDM_REQUIRE(m >= 2, "kid_compute: subsets of m = %d rows; KID needs two a side", m);
    MVLDM_REQUIRE(m <= n1 && m <= n2, "kid_compute: subsets of m = %d rows out of n1 = %d, n2 = %d", m, n1, n2);
    if (!kid_d_ok(d)) return set_error(MVLDM_ERR_UNSUPPORTED, "kid_compute: d = %d features; multiples of 64 up to %d are supported", d, kKidMaxD);
    const long long tps = kid_tiles_per_subset(m), blocks = tps * num_subsets;
    MVLDM_REQUIRE(blocks <= 0x7FFFFFFFll && (long long)num_subsets * m <= 0x7FFFFFFFll, "kid_compute: %d subsets of %d rows are too many", num_subsets, m);
    MVLDM_REQUIRE(ws_bytes >= kid_workspace_bytes(m, num_subsets), "kid_compute: workspace of %zu bytes, need %zu", ws_bytes,
                  kid_workspace_bytes(m, num_subsets));
    MVLDM_REQUIRE(aligned(f1, 16) && aligned(f2, 16) && aligned(idx1, 4) && aligned(idx2, 4) && aligned(ws, 8) &&
                      aligned(score, 4) && aligned(info, 8) && (per_subset == nullptr || aligned(per_subset, 8)),
                  "kid_compute: null or unaligned pointer");
    const int T = (int)kid_tiles(m), pairs = T * (T + 1) / 2;
    double* per = per_subset ? per_subset : ws + (size_t)blocks;
    double* scale = ws + (size_t)blocks + num_subsets;
    hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, f1, n1, f2, n2, d, idx1, idx2, m, T, (int)tps, ws);
    hipLaunchKernelGGL(kid_subset_kernel, dim3(num_subsets), dim3(256), 0, s, (const double*)ws, (int)tps, pairs, idx1, n1, idx2, n2, m, per, scale);
    hipLaunchKernelGGL(kid_final_kernel, dim3(1), dim3(64), 0, s, (const double*)per, (const double*)scale, num_subsets, m, score, info);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_kid_workspace_bytes(int m, int num_subsets) { return kid_workspace_bytes(m, num_subsets); }
extern "C" int mvldm_kid_compute(const double* f1, int n1, const double* f2, int n2, int d, const int32_t* idx1, const int32_t* idx2, int num_subsets,
                                 int m, double* workspace, size_t workspace_bytes, float* score, double* per_subset, double* info,
                                 mvldm_stream_t stream) {
    return kid_compute_run(f1, n1, f2, n2, d, idx1, idx2, num_subsets, m, workspace, workspace_bytes, score, per_subset, info, (hipStream_t)stream);
}
