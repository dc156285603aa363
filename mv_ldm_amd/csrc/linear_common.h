// What the Linear kernel files (linear_pp.hip, linear_pw.hip, linear_ws.hip, linear_rs.hip: tiles 12, 13, 14, 19) have in common: the
// MFMA trait, the permuted-column transposed product and its park-free epilogue helpers, the persistent tile walk of an XCD, and the host
// code that turns a mvldm_igemm_desc into the fields every Linear parameter struct carries.  A file keeps what is its own: the extra
// fields of its parameter struct, ring layout, issue / wait schedule, main loop, epilogue order, applicability rule and launch.
// The helpers read parameter structs by FIELD NAME (templates on the struct type) or take the fields themselves: there is no common base
// struct, so every kernel's argument block keeps its layout.  Moving a helper here must leave the device code of every kernel as it was
// (compare `hipcc --cuda-device-only -S` of a file before and after, `__hip_cuid_` lines aside).
#pragma once
#include <algorithm>

#include "common.h"

namespace mvldm {

constexpr unsigned kLinRowNone = 0xFFFFFFFFu;      // byte offset of a row past M (lin_off turns it into kBufOob)

// MFMA 32x32x16 on 16-bit operands (common.h)
template <typename T> using LinMma = Mfma16<T>;

// one fragment (16 bytes = 8 K values of a row) from its LDS address
template <typename T> __device__ __forceinline__ typename LinMma<T>::Frag lin_frag(const char* p) {
    return *reinterpret_cast<const typename LinMma<T>::Frag*>(p);
}

// The product is computed TRANSPOSED (W fragment = MFMA A operand), so a lane holds ONE output row, and the W rows a wave feeds to the
// MFMA's M index are PERMUTED: M index mu = 8a + 4h + e (= lane & 31 of the W-fragment read) is fed from column
// 16 (a >> 1) + 8h + 4 (a & 1) + e of the 32-column block.  That costs nothing (it is the lane's LDS read address) and leaves accumulator
// registers 0..7 / 8..15 of a lane = 8 + 8 CONSECUTIVE output columns (8h .. 8h+7 and 16 + 8h ..): two 16-byte stores per 32 x 32 block
// straight from registers -- no LDS park, no v_permlane swaps.  The permutation maps each 16-lane group of a ds_read_b128 onto the same SET
// of rows as the identity, so the XOR swizzle stays conflict-free.  GEGLU: value and gate blocks use the same permutation, so a lane holds
// a column's value AND gate.
__device__ __forceinline__ int lin_perm(int mu) {
    const int a = mu >> 3, h = (mu >> 2) & 1, e = mu & 3;
    return 16 * (a >> 1) + 8 * h + 4 * (a & 1) + e;
}

// byte offset of column `col` in the row at byte offset `row` of dst / the residual; out of range past M or the layer's width
__device__ __forceinline__ unsigned lin_off(unsigned row, int col, int n_dst) {
    return (row != kLinRowNone && col < n_dst) ? row + (unsigned)col * 2u : kBufOob;
}

// one 32 x 32 block (GEGLU: one value / gate pair) of the finished tile -> two packed 16-byte chunks.  c[k]: the lane's 16 columns
// in output order (registers 0..7 = columns 8h .. 8h+7, 8..15 = 16 + 8h .. of the block).  RES: residual chunks of the same columns
template <typename T, bool RES>
__device__ __forceinline__ void lin_pack(const float (&c)[16], float scale, const u32x4 (&res)[2], u32x4 (&out)[2]) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        Chunk<T> oc;
        if constexpr (RES) {
            Chunk<T> rc;
            rc.raw = res[g];
#pragma unroll
            for (int e = 0; e < 8; ++e) oc.set(e, c[8 * g + e] * scale + rc.get(e));
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) oc.set(e, c[8 * g + e] * scale);
        }
        out[g] = oc.raw;
    }
}

// (buffer descriptors only in free functions: an opaque __amdgpu_buffer_rsrc_t inside a lambda trips hipcc's host pass)
// bias of the BN packed columns of tile column tn: thread t fetches packed columns 4t .. 4t+3 (zeros past the tile / the layer / without a
// bias).  GEGLU: the packed weight alternates [32 value | 32 gate] columns, the torch-layout bias keeps the value columns first and the gate
// columns at n_dst.  P: a parameter struct with bias, bias_bytes, n_dst, n_out (the struct, not the four fields: passed as values they
// changed the operand order of an add in linear_rs.hip's kernels).
// The SAME column mapping is written out in three helpers that belong to one file each -- lp_issue_bias (linear_pp.hip: LDS-DMA into the
// slab), pw_bias_off (linear_pw.hip: inline-asm load) and the slab fill of linear_ws.hip: a shared offset function called from them and from
// here reordered instructions in their kernels, and a helper that changes a kernel's code is not hoisted.  A change to the mapping goes to
// all four.
template <int BN, typename P> __device__ __forceinline__ u32x4 lin_load_bias(const P& p, bool geglu, bool valid, int tn, int t) {
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias_bytes, 0x00020000);
    const int pc = tn * BN + 4 * t;                             // packed column
    int oc = pc;                                                // column of the torch-layout bias
    if (geglu) {
        const int blk = pc >> 5, w = pc & 31;
        oc = ((blk & 1) ? p.n_dst : 0) + (blk >> 1) * 32 + w;
    }
    const unsigned off = (valid && 4 * t < BN && pc < p.n_out) ? (unsigned)oc * 4u : kBufOob;
    return __builtin_amdgcn_raw_buffer_load_b128(rb, off, 0, 0);
}
// one 16-byte chunk of the residual (zeros at kBufOob / without a residual)
__device__ __forceinline__ u32x4 lin_load_res(const void* residual, unsigned res_bytes, unsigned off) {
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(residual), 0, res_bytes, 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0);
}

// Walks the tiles of a persistent workgroup (all wave-uniform).  XCD x owns row blocks [x * m_per, (x+1) * m_per) and all column tiles.  Its
// tiles form ONE list in block order -- gm x gn blocks of tiles, column chunks (nbn of them) fastest, inside a block the row fastest; ragged
// blocks at the edges are packed densely -- and its wgx workgroups take list entries lid, lid + wgx, lid + 2 wgx ...: the workgroups an XCD
// runs at the same time share about gm activation row blocks and gn weight panels in its L2 (with one row of 32 column tiles in flight the
// 6.5 MB weight of the level-1 GEGLU projection streamed through the 4 MB L2 once per row block), and a round leaves no CU idle unless
// the list ends.  (Rounds 4-5 walked whole blocks, one per round: a block shape that did not divide the XCD's tile grid idled workgroups
// in EVERY round -- 27 of 32 on the 8 x 8 level QKV, 8 rounds for 6.75 rounds of work.)
// P: a parameter struct with wgx, gm, gn, tiles_n (lin_block_shape picks gm and gn).
template <typename P> struct LinTileIter {
    int r, tm, tn;
    bool valid;
    __device__ __forceinline__ void set(const P& p, int r0, int lid, int m_lo, int m_cnt) {
        r = r0;
        const int i = r0 * p.wgx + lid;
        valid = i < m_cnt * p.tiles_n;
        if (valid) {
            const int strip = p.gm * p.tiles_n;                          // tiles of a full strip of gm row blocks
            const int sm = min(i / strip, (m_cnt + p.gm - 1) / p.gm - 1);
            const int hm = min(p.gm, m_cnt - sm * p.gm);                 // rows of this strip (the last one may be lower)
            const int is = i - sm * strip;
            const int cn = is / (hm * p.gn);                             // column chunk (the last one may be narrower)
            const int j = is - cn * hm * p.gn;
            const int ln = j / hm;
            tm = m_lo + sm * p.gm + (j - ln * hm);
            tn = cn * p.gn + ln;
        }
    }
};

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// CUs of the current device, queried once per process; 256 when the query fails
inline int cu_count() {
    static const int n_cu = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            return prop.multiProcessorCount;
        return 256;
    }();
    return n_cu;
}

// descriptor -> the fields every Linear parameter struct has.  Byte ranges are those of the buffer descriptors (the applicability rules keep
// them below 4 GB).  `fake` (roofline experiments, 0 in the product build; results are WRONG): 1 = the activation pieces read as zeros
// without memory traffic, 2 = same for the weight, 4 = no stores
template <typename P> inline void lin_fill_params(P& p, const mvldm_igemm_desc& d, int fake) {
    p.a = d.src0; p.w = d.weight; p.bias = d.bias; p.residual = d.residual; p.dst = d.dst;
    p.M = d.n_img * d.h_out * d.w_out; p.n_out = d.n_out; p.n_pad = d.n_pad;
    p.n_dst = d.epilogue == MVLDM_EPI_GEGLU ? d.n_out / 2 : d.n_out;
    p.dst_ld = d.dst_ld > 0 ? d.dst_ld : p.n_dst;
    p.out_scale = d.out_scale;
    p.a_bytes = (unsigned)((double)p.M * d.c0 * 2.0); p.w_bytes = (unsigned)((double)d.n_pad * d.k_pad * 2.0);
    p.bias_bytes = d.bias ? (unsigned)d.n_out * 4u : 0u;
    p.res_bytes = d.residual ? (unsigned)((double)p.M * p.n_dst * 2.0) : 0u;
    p.dst_bytes = (unsigned)((double)p.M * p.dst_ld * 2.0);
    if (fake & 1) p.a_bytes = 0;
    if (fake & 2) p.w_bytes = 0;
    if (fake & 4) p.dst_bytes = 0;
}
// ... and those of the kernels that take the channel concat of two sources (tiles 12, 13, 19): K-tiles [0, kt0) come from `a`, the rest from `a1`
template <typename P> inline void lin_fill_params2(P& p, const mvldm_igemm_desc& d, int fake) {
    lin_fill_params(p, d, fake);
    p.a1 = d.src1;
    p.K = d.c0 + d.c1; p.c0 = d.c0; p.c1 = d.c1; p.kt0 = d.c0 / 64;
    p.a1_bytes = (fake & 1) ? 0u : (unsigned)((double)p.M * p.c1 * 2.0);
}

// Block shape of LinTileIter's list, for an XCD whose wgx workgroups (set by the caller: one per CU, fewer when it has fewer tiles) walk m_per
// row blocks x tiles_n column tiles: the shape of about one round's tiles that moves the fewest bytes into the XCD's L2 per tile -- gm
// activation row blocks of a_t bytes + gn weight panels of w_t bytes
template <typename P> inline void lin_block_shape(P& p, double a_t, double w_t) {
    double best_cost = 1e300;
    p.gm = p.gn = 1;
    for (int gm = 1; gm <= std::min(p.wgx, p.m_per); ++gm) {
        const int gn = std::max(1, std::min(p.wgx / gm, p.tiles_n));
        // (cost per tile of the block: a block smaller than a round shares less)
        const double cost = (gm * a_t + gn * w_t) / (gm * gn);
        if (cost < best_cost) { best_cost = cost; p.gm = gm; p.gn = gn; }
    }
}

}  // namespace mvldm
