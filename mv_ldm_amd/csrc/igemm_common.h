// What the implicit-GEMM files have in common (igemm.hip: host rules, split-K reduce and the entry points; igemm_small.hip /
// igemm_large.hip / igemm_xl.hip: igemm_kernel and igemm_bl_kernel from igemm_bl.h, by tile; igemm_halo.hip: the pixel-halo tiles 11 and 17;
// pack.hip: the weight packers): the parameter struct, the MFMA + LDS policy, the workgroup -> tile map, the two epilogues, the
// fragment helpers of the LDS-DMA kernels, and the host pieces that more than one file reads (tile table, LDS sizes, launch).
// Every kernel instantiation is compiled in exactly one of those files; each file exposes one plain launch function (at the end).
// The rule, as in linear_common.h: moving a helper here must leave the device code of every kernel as it was.
// tools/kernel_hashes.py checks it -- it hashes every kernel's assembly, whichever file it is compiled in -- and a helper whose
// hoisting changes one instruction of any kernel stays where it was, with a comment line there.
#pragma once
#include <algorithm>

#include "common.h"

namespace mvldm {

struct IgemmParams {
    const void* src0; const void* src1; const void* weight;
    const float* bias; const float* row_bias; const void* residual; void* dst; float* ws;
    int c0, c1, ctot;
    int n_img, h_in, w_in, h_out, w_out, hw_out;
    int ksize, stride, pad, upsample;
    int M, n_out, n_pad, n_dst, k_pad, taps;
    int row_bias_ld, epilogue, dst_f32, dst_ld;
    float out_scale;
    int splitk, k_tiles, k_tiles_per_split;
    int tiles_m, tiles_n;
    int korder;                 // 0: k = (tap, channel)   1: k = (channel block of BK, tap, channel in block)
    int px, sub_m, sub_n, m_fast;  // XCD-aware 2-D tile partition
    int grp_m, grp_n;              // > 1: inside an XCD's partition consecutive workgroups form grp_m x grp_n blocks of tiles (map_block)
    int rb_vec;                    // row_bias rows are 16-byte addressable (base and leading dimension)
    int bias_vec;                  // bias is 16-byte aligned
    int ty0, tx0, cy, cx;          // tap origin relative to (oy*stride, ox*stride), and the always-inside reference tap
    int scatter, ph_y, ph_x;       // sub-pixel phase of a decomposed nearest-2x upsampling conv: output row m -> (2i+py, 2j+px)
    int fake;                      // EXPERIMENT knob (MVLDM_IGEMM_FAKE): bit 2 = no global stores / residual loads, bit 3 = no epilogue
    unsigned src0_bytes, src1_bytes, w_bytes;   // buffer-descriptor extents (lean 16-bit loop)
    int use_bl, stage_epi;
    int nt_store;                  // staged epilogue: streaming (non-temporal) output stores
};

// ---- per-dtype MFMA + LDS policy -------------------------------------------------------------------
template <typename T> struct Mma;

// 16-bit: the 32x32x16 MFMA of common.h over 128-byte XOR-swizzled LDS rows
template <typename T16> struct Mma16 : Mfma16<T16> {
    static constexpr int KI = 16;        // K per MFMA
    static constexpr int BK = 64;        // K per LDS tile
    static constexpr int PITCH = 128;    // bytes per LDS row
    using Frag = typename Mfma16<T16>::Frag;
    static __device__ __forceinline__ void store(char* tile, int r, int kc, u32x4 v) {
        *reinterpret_cast<u32x4*>(tile + r * PITCH + ((kc ^ ((r >> 1) & 7)) << 4)) = v;
    }
    static __device__ __forceinline__ Frag load(const char* tile, int r, int kk, int hi) {
        const int kc = kk * 2 + hi;
        return *reinterpret_cast<const Frag*>(tile + r * PITCH + ((kc ^ ((r >> 1) & 7)) << 4));
    }
};
template <> struct Mma<bf16_t> : Mma16<bf16_t> {};
template <> struct Mma<f16_t> : Mma16<f16_t> {};
template <> struct Mma<float> {
    static constexpr int KI = 2;
    static constexpr int BK = 32;
    static constexpr int PITCH = 33 * 4;
    using Frag = float;
    static __device__ __forceinline__ void store(char* tile, int r, int kc, u32x4 v) {
        uint32_t* p = reinterpret_cast<uint32_t*>(tile + r * PITCH + kc * 16);
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
    static __device__ __forceinline__ Frag load(const char* tile, int r, int kk, int hi) {
        return *reinterpret_cast<const float*>(tile + r * PITCH + (kk * 2 + hi) * 4);
    }
    static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
};

// packed weight row -> original output column (GEGLU rows alternate [value|gate] in blocks of 32)
__device__ __forceinline__ int orig_col(int n_packed, int n_out, bool geglu) {
    if (!geglu) return n_packed;
    const int blk = n_packed >> 5, w = n_packed & 31;
    return (blk & 1) ? (n_out >> 1) + (blk >> 1) * 32 + w : (blk >> 1) * 32 + w;
}

// SCATTER false: the per-element fallback epilogue inside the GEMM kernels -- phase convs never take it (fill_params), and with
// the two divisions in its 64-fold unrolled body hipcc stops unrolling and demotes the accumulators to scratch
template <typename T, bool SCATTER = false>
__device__ __forceinline__ void epilogue_store(const IgemmParams& p, int m, int n_dst_col, float v) {
    // v already includes bias/row_bias/activation
    v *= p.out_scale;
    if (p.residual) v += to_f32<T>(reinterpret_cast<const T*>(p.residual)[(size_t)m * p.n_dst + n_dst_col]);
    size_t drow = (size_t)m;
    if (SCATTER && p.scatter) {   // sub-pixel phase of a decomposed nearest-2x upsampling conv (the split-K reduce of a phase lands here)
        const int img = m / p.hw_out, rem = m - img * p.hw_out;
        const int i = rem / p.w_out, j = rem - i * p.w_out;
        drow = ((size_t)img * (2 * p.h_out) + 2 * i + p.ph_y) * (size_t)(2 * p.w_out) + 2 * j + p.ph_x;
    }
    const size_t o = drow * p.dst_ld + n_dst_col;
    if (p.dst_f32) reinterpret_cast<float*>(p.dst)[o] = v;
    else reinterpret_cast<T*>(p.dst)[o] = from_f32<T>(v);
}

// Workgroup -> (split, m-tile, n-tile).  The hardware places workgroup b on XCD b % 8 (observed; used for
// speed only): the 8 XCDs form a px x py grid over the tile space so that each XCD's private 4 MB L2
// sees one slice of A and one slice of W -- the host picks (px, py) minimising py*bytes(A) + px*bytes(W),
// the traffic that crosses the fabric.  Inside an XCD, tiles that share the larger operand are adjacent.
__device__ __forceinline__ bool map_block(const IgemmParams& p, int& split, int& tm, int& tn) {
    const int b = blockIdx.x, xcd = b & 7, idx = b >> 3;
    const int xm = xcd % p.px, xn = xcd / p.px;
    const int per = p.sub_m * p.sub_n;
    split = idx / per;
    const int r = idx - split * per;
    int tml, tnl;
    if (p.grp_m * p.grp_n > 1) {
        // The ~32 workgroups an XCD runs at the same time stream their operands in step: a tile row of A is fetched once for the grp_n
        // column tiles that share it, a W panel once for the grp_m row tiles -- fabric traffic of the XCD's partition ~
        // A * (sub_n / grp_n) + W * (sub_m / grp_m).  One row (or column) of 32 tiles re-reads the other operand once per tile:
        // measured 4.8x / 7.7x the algorithmic bytes on the level-1 / level-2 GEGLU projections (4.5 GB at 3.9 TB/s: bandwidth-bound).
        // Order: super-rows of grp_m row tiles; inside, chunks of grp_n columns; inside a chunk the row index runs fastest.
        const int gm = p.grp_m, gn = p.grp_n;
        const int nfull = p.sub_m / gm, per_super = gm * p.sub_n;
        int mg, gm_eff, rr;
        if (r < nfull * per_super) { mg = r / per_super; rr = r - mg * per_super; gm_eff = gm; }
        else { mg = nfull; rr = r - nfull * per_super; gm_eff = p.sub_m - nfull * gm; }
        const int ng = rr / (gm_eff * gn), r2 = rr - ng * gm_eff * gn;
        tnl = ng * gn + r2 / gm_eff;
        tml = mg * gm + r2 % gm_eff;
    } else if (p.m_fast) { tnl = r / p.sub_m; tml = r - tnl * p.sub_m; }
    else { tml = r / p.sub_n; tnl = r - tml * p.sub_n; }
    tm = xm * p.sub_m + tml;
    tn = xn * p.sub_n + tnl;
    return tm < p.tiles_m && tn < p.tiles_n;
}

// ---- epilogue shared by both main-loop variants ---------------------------------------------------
template <typename T, int BM, int BN, int WM, int WN>
__device__ __forceinline__ void igemm_epilogue(const IgemmParams& p, f32x16 (&acc)[BM / WM / 32][BN / WN / 32], int tm, int tn,
                                               int split, int wm, int wn, int hi, int l31) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    const bool geglu = p.epilogue == MVLDM_EPI_GEGLU;
    if (p.splitk > 1) {
        float* ws = p.ws + (size_t)split * p.M * p.n_pad;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = tn * BN + wn * (BN / WN) + j * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = tm * BM + wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (m < p.M && n < p.n_pad) ws[(size_t)m * p.n_pad + n] = acc[i][j][r];
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        if (geglu) {
            if constexpr (TN % 2 == 0) {
#pragma unroll
                for (int j = 0; j < TN; j += 2) {
                    const int nb = tn * BN + wn * (BN / WN) + j * 32;  // packed col of the value block
                    const int col = (nb >> 6) * 32 + l31;             // output column
                    if (col >= p.n_dst) continue;
                    const float bv = p.bias ? p.bias[col] : 0.f;
                    const float bg = p.bias ? p.bias[p.n_dst + col] : 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = tm * BM + wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        if (m >= p.M) continue;
                        epilogue_store<T>(p, m, col, (acc[i][j][r] + bv) * gelu_erf_fast(acc[i][j + 1][r] + bg));
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = tn * BN + wn * (BN / WN) + j * 32 + l31;
                if (n >= p.n_out) continue;
                const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = tm * BM + wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (m >= p.M) continue;
                    float v = acc[i][j][r] + bv;
                    if (p.row_bias) v += p.row_bias[(size_t)(m / p.hw_out) * p.row_bias_ld + n];
                    if (p.epilogue == MVLDM_EPI_SILU) v = silu_f(v);
                    else if (p.epilogue == MVLDM_EPI_GELU) v = gelu_erf_fast(v);
                    epilogue_store<T>(p, m, n, v);
                }
            }
        }
    }
}

// ---- LDS-staged epilogue (16-bit loops) --------------------------------------------------------------
// The MFMA accumulator layout gives a lane ONE column and 16 scattered rows: storing from it means 2-byte
// stores in 64-byte runs (and the residual is read the same way).  Here every wave parks a finished 32-row
// block of its tile in LDS as RAW fp32 accumulators (16 ds_write_b32 per block, nothing else), then re-reads it
// row-major: a lane owns 8 consecutive output columns of one row, so bias, time-embedding row and residual
// arrive as 16/32-byte loads, the activation / GEGLU product runs on 8 values at a time, and one 16-byte store
// leaves; a store instruction covers 8 full 128-byte lines.  The epilogue mode is decided once per group,
// outside the element loops (the first version branched and waited on a bias load per accumulator block: PMC /
// `MVLDM_IGEMM_FAKE=8` showed the epilogue costing as much as the whole main loop at K = 320).  Split-K partial
// slabs take the same route with 16-byte fp32 stores.
// A wave tile wider than 4 column blocks is parked in groups of <= 4 blocks (the 8 park buffers must fit the ring).
constexpr int park_blocks(int tn) { return tn <= 4 ? tn : 4; }

enum { EPI_PLAIN = 0, EPI_ACT_SILU = 1, EPI_PAIR_GEGLU = 2, EPI_PARTIAL = 3, EPI_ACT_GELU = 4 };

// one parked group: JN column blocks of one 32-row block.  m0: global row of block row 0; pcol0: first packed
// column of the group.
template <typename T, int JN, int MODE, int PITCH>
__device__ __forceinline__ void epi_rows(const IgemmParams& p, const float* st, int m0, int pcol0, int split, int lane) {
    constexpr bool PAIR = MODE == EPI_PAIR_GEGLU;
    constexpr int WC = PAIR ? JN * 16 : JN * 32;      // output columns of the group
    constexpr int CPR = WC / 8;                       // 8-column chunks per row
    static_assert(64 % CPR == 0 && (32 * CPR) % 64 == 0, "row-major mapping");
    constexpr int RSTEP = 64 / CPR, ITERS = 32 / RSTEP;
    const int ch = lane % CPR, row0 = lane / CPR;     // a lane keeps its columns over the rows it visits
    const int ncol0 = PAIR ? (pcol0 >> 1) : pcol0;
    const int n0 = ncol0 + ch * 8;
    const int n_lim = MODE == EPI_PARTIAL ? p.n_pad : p.n_dst;
    if (n0 >= n_lim) return;
    // value (and, for GEGLU, gate) position of this lane's chunk inside a parked row
    const int voff = PAIR ? (2 * (ch >> 2)) * 32 + (ch & 3) * 8 : ch * 8;
    float bv[8], bg[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = bg[e] = 0.f;
    if (MODE != EPI_PARTIAL && p.bias) {
        if (p.bias_vec) {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + n0), b1 = *reinterpret_cast<const f32x4*>(p.bias + n0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { bv[e] = b0[e]; bv[4 + e] = b1[e]; }
            if constexpr (PAIR) {
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(p.bias + p.n_dst + n0);
                const f32x4 g1 = *reinterpret_cast<const f32x4*>(p.bias + p.n_dst + n0 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { bg[e] = g0[e]; bg[4 + e] = g1[e]; }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bv[e] = p.bias[n0 + e];
                if constexpr (PAIR) bg[e] = p.bias[p.n_dst + n0 + e];
            }
        }
    }
    const bool rb_on = MODE != EPI_PARTIAL && MODE != EPI_PAIR_GEGLU && p.row_bias != nullptr;
    // The residual rows of ALL the lane's iterations are requested here, before the first store: inside the loop below every
    // load sits behind the previous iteration's store to `dst` (which the compiler must assume may alias it), i.e. one full
    // memory latency PER ITERATION -- measured on the level-0 output projection (K = 320, 256 x 320 tile): 25 us of epilogue
    // per tile against 13 us of main loop.  <= 8 chunks = 32 registers (the accumulators of the later row blocks are still live).
    Chunk<T> rpre[ITERS];
    if constexpr (MODE != EPI_PARTIAL) {
        if (p.residual && !(p.fake & 4)) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int m = m0 + row0 + it * RSTEP;
                if (m < p.M) rpre[it] = load_chunk<T>(reinterpret_cast<const T*>(p.residual) + (size_t)m * p.n_dst + n0);
            }
        }
    }
    // ... and the time-embedding row when the whole 32-row block lies in one image (always, unless an image ends inside it)
    float rbv[8];
    bool rb_pre = false;
    if (rb_on) {
        const int img0 = m0 / p.hw_out;
        rb_pre = p.rb_vec && (min(m0 + 31, p.M - 1) / p.hw_out) == img0;
        if (rb_pre) {
            const float* rb = p.row_bias + (size_t)img0 * p.row_bias_ld + n0;
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(rb), r1 = *reinterpret_cast<const f32x4*>(rb + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { rbv[e] = r0[e]; rbv[4 + e] = r1[e]; }
        }
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int row = row0 + it * RSTEP;
        const int m = m0 + row;
        if (m >= p.M) continue;
        const f32x4 a = *reinterpret_cast<const f32x4*>(st + row * PITCH + voff);
        const f32x4 b = *reinterpret_cast<const f32x4*>(st + row * PITCH + voff + 4);
        if constexpr (MODE == EPI_PARTIAL) {
            float* o = p.ws + (size_t)split * p.M * p.n_pad + (size_t)m * p.n_pad + n0;
            *reinterpret_cast<f32x4*>(o) = a;
            *reinterpret_cast<f32x4*>(o + 4) = b;
        } else {
            float v[8] = {a[0] + bv[0], a[1] + bv[1], a[2] + bv[2], a[3] + bv[3], b[0] + bv[4], b[1] + bv[5], b[2] + bv[6], b[3] + bv[7]};
            if constexpr (PAIR) {
                const f32x4 ga = *reinterpret_cast<const f32x4*>(st + row * PITCH + voff + 32);
                const f32x4 gb = *reinterpret_cast<const f32x4*>(st + row * PITCH + voff + 36);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] *= gelu_erf_16(ga[e] + bg[e]);
                    v[4 + e] *= gelu_erf_16(gb[e] + bg[4 + e]);
                }
            } else {
                if (rb_on && rb_pre) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += rbv[e];
                } else if (rb_on) {   // per-image row (time embedding): one division per 8 outputs
                    const float* rb = p.row_bias + (size_t)(m / p.hw_out) * p.row_bias_ld + n0;
                    if (p.rb_vec) {
                        const f32x4 r0 = *reinterpret_cast<const f32x4*>(rb), r1 = *reinterpret_cast<const f32x4*>(rb + 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[e] += r0[e]; v[4 + e] += r1[e]; }
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += rb[e];
                    }
                }
                if constexpr (MODE == EPI_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
                }
                if constexpr (MODE == EPI_ACT_GELU) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = gelu_erf_fast(v[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= p.out_scale;
            if (p.fake & 4) { if (v[0] == 1.2345e33f) p.ws[0] = v[1]; continue; }
            if (p.residual) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += rpre[it].get(e);
            }
            Chunk<T> oc;
#pragma unroll
            for (int e = 0; e < 8; ++e) oc.set(e, v[e]);
            size_t drow = (size_t)m;
            if (p.scatter) {   // sub-pixel phase: low-resolution pixel (i, j) of image `img` -> (2i+py, 2j+px) of the 2x output
                const int img = m / p.hw_out, rem = m - img * p.hw_out;
                const int i = rem / p.w_out, j = rem - i * p.w_out;
                drow = ((size_t)img * (2 * p.h_out) + 2 * i + p.ph_y) * (size_t)(2 * p.w_out) + 2 * j + p.ph_x;
            }
            T* const dptr = reinterpret_cast<T*>(p.dst) + drow * p.dst_ld + n0;
            if (p.nt_store) __builtin_nontemporal_store(oc.raw, reinterpret_cast<u32x4*>(dptr));
            else store_chunk<T>(dptr, oc);
        }
    }
}

// park JN column blocks (from J0) of row block I of the wave's accumulators: raw fp32, [row][col].  The accumulators are named by
// template indices, never through a reference to a sub-array: with five epilogue modes behind it hipcc otherwise stops promoting
// the 64 x 64 wave tile's `acc` to registers (320 bytes of scratch per lane, written and re-read once per tile: 3-4x slower)
template <int TM, int TN, int I, int J0, int JN, int PITCH>
__device__ __forceinline__ void epi_park(const f32x16 (&acc)[TM][TN], float* st, int lane) {
    const int hi = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[((r & 3) + 8 * (r >> 2) + 4 * hi) * PITCH + j * 32 + l31] = acc[I][J0 + j][r];
    // (same wave wrote and reads: LDS serves a wave's requests in order; the compiler's own lgkmcnt wait covers
    //  the data dependence through `st`)
}

template <typename T, int JN, int PITCH>
__device__ __forceinline__ void epi_group_rows(const IgemmParams& p, const float* st, int m0, int pcol0, int split, int mode, int lane) {
    if (mode == EPI_PARTIAL) epi_rows<T, JN, EPI_PARTIAL, PITCH>(p, st, m0, pcol0, split, lane);
    else if (mode == EPI_PAIR_GEGLU) {
        if constexpr (JN % 2 == 0) epi_rows<T, JN, EPI_PAIR_GEGLU, PITCH>(p, st, m0, pcol0, split, lane);
    } else if (mode == EPI_ACT_SILU) epi_rows<T, JN, EPI_ACT_SILU, PITCH>(p, st, m0, pcol0, split, lane);
    else if (mode == EPI_ACT_GELU) epi_rows<T, JN, EPI_ACT_GELU, PITCH>(p, st, m0, pcol0, split, lane);
    else epi_rows<T, JN, EPI_PLAIN, PITCH>(p, st, m0, pcol0, split, lane);
}

template <typename T, int BM, int BN, int WM, int WN, int I>
__device__ __forceinline__ void igemm_epilogue_rowblock(const IgemmParams& p, const f32x16 (&acc)[BM / WM / 32][BN / WN / 32], float* st, int tm, int tn,
                                                        int split, int wm, int wn, int mode, int lane) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int WCOLS = BN / WN;          // packed columns of a wave tile
    constexpr int JG = park_blocks(TN);
    constexpr int PITCH = JG * 32 + 4;      // floats
    const int m0 = tm * BM + wm * (BM / WM) + I * 32;
    const int pcol0 = tn * BN + wn * WCOLS;
    epi_park<TM, TN, I, 0, JG, PITCH>(acc, st, lane);
    epi_group_rows<T, JG, PITCH>(p, st, m0, pcol0, split, mode, lane);
    if constexpr (TN > JG) {
        epi_park<TM, TN, I, JG, TN - JG, PITCH>(acc, st, lane);
        epi_group_rows<T, TN - JG, PITCH>(p, st, m0, pcol0 + JG * 32, split, mode, lane);
    }
    if constexpr (I + 1 < TM) igemm_epilogue_rowblock<T, BM, BN, WM, WN, I + 1>(p, acc, st, tm, tn, split, wm, wn, mode, lane);
}

template <typename T, int BM, int BN, int WM, int WN>
__device__ __forceinline__ void igemm_epilogue_staged(const IgemmParams& p, f32x16 (&acc)[BM / WM / 32][BN / WN / 32], int tm,
                                                      int tn, int split, int wm, int wn, int wave, int lane, char* smem) {
    constexpr int TN = BN / WN / 32;
    constexpr int JG = park_blocks(TN);
    constexpr int PITCH = JG * 32 + 4;      // floats
    static_assert(TN <= 2 * JG, "at most two park groups");
    if (p.fake & 8) return;
    float* st = reinterpret_cast<float*>(smem) + wave * (32 * PITCH);
    const int mode = p.splitk > 1 ? EPI_PARTIAL
                                  : (p.epilogue == MVLDM_EPI_GEGLU ? EPI_PAIR_GEGLU
                                     : (p.epilogue == MVLDM_EPI_SILU ? EPI_ACT_SILU : (p.epilogue == MVLDM_EPI_GELU ? EPI_ACT_GELU : EPI_PLAIN)));
    __syncthreads();   // every wave is done with the operand ring
    igemm_epilogue_rowblock<T, BM, BN, WM, WN, 0>(p, acc, st, tm, tn, split, wm, wn, mode, lane);
}

// LDS-DMA kernels: who this lane is.  `wave` is wave-uniform (it indexes LDS pieces and feeds scalar address arithmetic); wave (wm, wn) of
// the WM x WN grid; hi / l31: the lane's half and row inside a 32-row MFMA fragment
struct WaveLane { int lane, wave, wm, wn, hi, l31; };
template <int WN> __device__ __forceinline__ WaveLane wave_lane() {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    return {lane, wave, wave / WN, wave % WN, lane >> 5, lane & 31};
}

// One k-sub-step (16 of the tile's 64 K values) of operand fragments, and the MFMAs that consume them.  The
// main loop keeps TWO of these live and always has the next one's ds_reads in flight while the current
// one's MFMAs run -- including across the ring barrier (the first fragments of tile t+1 are fetched under
// the last MFMAs of tile t), so one wave alone covers the LDS latency instead of leaning on occupancy.
template <typename T, int TM, int TN> struct BlFrags {
    typename Mma<T>::Frag a[TM], b[TN];
};

template <typename T, int BM, int BN, int WM, int WN>
__device__ __forceinline__ void bl_load(const char* stage_base, BlFrags<T, BM / WM / 32, BN / WN / 32>& f, int kk, int wm, int wn,
                                        int hi, int l31) {
    using M_ = Mma<T>;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    const char* at = stage_base;
    const char* bt = at + BM * 128;
#pragma unroll
    for (int i = 0; i < TM; ++i) f.a[i] = M_::load(at, wm * (BM / WM) + i * 32 + l31, kk, hi);
#pragma unroll
    for (int j = 0; j < TN; ++j) f.b[j] = M_::load(bt, wn * (BN / WN) + j * 32 + l31, kk, hi);
}

template <typename T, int TM, int TN>
__device__ __forceinline__ void bl_mma(const BlFrags<T, TM, TN>& f, f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::mma(f.a[i], f.b[j], acc[i][j]);
}

// ---- host side ------------------------------------------------------------------------------------
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
struct TileCfg { int bm, bn, threads; };
constexpr TileCfg kTiles[] = {{0, 0, 0}, {128, 128, 256}, {128, 64, 256}, {64, 128, 256}, {64, 64, 128}, {32, 64, 64},
                                 {256, 64, 256},     // tile 6: 64x64 wave tile, lean 16-bit loop only
                                 {256, 128, 512},    // tile 7: 8 waves of 64x64 -- half the L2->LDS bytes per flop of tile 2
                                 {128, 256, 512},    // tile 8
                                 {256, 256, 512},    // tile 9: 8 waves of 64x128, 2-deep ring (128 KB): 128 flop per L2->LDS byte
                                 {256, 320, 512},    // tile 10: 8 waves of 64x160 -- every channel count of this UNet is a
                                                     // multiple of 320 (no N padding); 142 flop per L2->LDS byte
                                 {256, 128, 512},    // tile 11: 256x128 with the LDS-resident pixel halo (3x3 stride-1 convs)
                                 {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0},      // 12 - 14: linear_pp / linear_pw / linear_ws (own files); 15 unused
                                 {0, 0, 0},          // 16: unused (deep-ring form of tile 2, measured slower, not built)
                                 {256, 320, 512},    // tile 17: 256x320 with the LDS-resident pixel halo (3x3 stride-1 convs on maps <= 24 wide)
                                 // deep-ring tile for launches of a few hundred rows (weight-bound: levels 2 - 4 at a few scenes):
                                 {192, 128, 512}};   // tile 18: 8 waves of 96x32, 4 slots (160 KB): <= 192 rows read every weight byte once
constexpr int kNumTiles = 11;
inline bool deep_tile(int tile) { return tile == 18; }

template <typename KernT> inline int launch_kernel(KernT kern, std::atomic<uint64_t>& attr_done, int smem, int blocks, int threads,
                                                   const IgemmParams& p, hipStream_t s) {
    if (int rc0 = ensure_dyn_smem(reinterpret_cast<const void*>(kern), smem, attr_done)) return rc0;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), smem, s, p);
    return check_launch();
}

// LDS of the pixel-halo tiles: two halo buffers of halo_rows_for() 128-byte rows, the weight ring (tile 11: 3 x 128 rows, tile 17: 2 x 320),
// the zero row and a 1 KiB dump for the pieces past the end
inline int halo_rows_for(int w_in) { return (256 + 2 * (w_in + 1) + 7) / 8 * 8; }
inline int halo_smem(int w_in) { return 2 * halo_rows_for(w_in) * 128 + 3 * 128 * 128 + 128 + 1024; }
inline int halow_smem(int w_in) { return 2 * halo_rows_for(w_in) * 128 + 2 * 320 * 128 + 128 + 1024; }

// tiles 6 - 11 and 17 exist for the 16-bit block-major path only
inline int require_bl(const IgemmParams& p, int tile, int act_dtype) {
    if (act_dtype != MVLDM_F32 && p.use_bl) return MVLDM_OK;
    return set_error(MVLDM_ERR_ARG, "igemm: tile %d needs the 16-bit block-major path", tile);
}
// the two 16-bit activation types (callers have checked for them: require_bl)
template <typename F> inline int dispatch_16bit(int dtype, F&& f) { return dtype == MVLDM_BF16 ? f(bf16_t{}) : f(f16_t{}); }

// one launch entry point per kernel file (each compiles the instantiations of its tiles, and no other file does)
int igemm_launch_small(const IgemmParams& p, int tile, int act_dtype, hipStream_t s);   // igemm_small.hip: tiles 1 - 5 (4 waves or fewer)
int igemm_launch_large(const IgemmParams& p, int tile, int act_dtype, hipStream_t s);   // igemm_large.hip: tiles 6 - 8
int igemm_launch_xl(const IgemmParams& p, int tile, int act_dtype, hipStream_t s);      // igemm_xl.hip: tiles 9, 10 and 18
int igemm_launch_halo(const IgemmParams& p, int tile, int act_dtype, hipStream_t s);    // igemm_halo.hip: tiles 11 and 17

}  // namespace mvldm
