// Implicit-GEMM convolution / Linear on CDNA4 matrix cores (see include/mvldm.h: mvldm_igemm_fwd).
//
//   out[m][n] = epi( sum_k A[m][k] * W[n][k] + bias[n] + row_bias[img(m)][n] ) * scale + residual[m][n]
//
// m = (image, oy, ox) output pixel, k = (tap, channel).  A is never materialised: every 16-byte
// chunk of a K-tile row is fetched straight from the NHWC activation(s) -- zero for padding taps,
// from the second source for the skip-concat channels, from (iy>>1, ix>>1) for the fused nearest
// upsample.  W is the pre-packed K-major weight.  Both tiles are staged through LDS (double
// buffered, register prefetch of the next K-tile while MFMAs run on the current one) and consumed by
// v_mfma_f32_32x32x16_{bf16,f16} / v_mfma_f32_32x32x2_f32 with fp32 accumulation.
//
// LDS layout (16-bit types): 128-byte rows of 8 x 16-byte chunks, chunk index XOR-swizzled with
// (row>>1)&7 so that the 16-lane groups of a ds_read_b128 fragment read hit 16 distinct 16-byte
// slots of the 256-byte bank row (conflict-free); fp32: rows of 32 floats at pitch 33.
// Workgroup -> tile mapping is XCD-aware: each of the 8 XCDs owns a contiguous range of
// (split, n-tile, m-tile) ids with m fastest, so one weight tile is streamed from HBM by one XCD only.
//
// This file is the host side -- the rules that pick tile, split-K and the XCD partition (choose_config, fill_params), the split-K reduce
// kernels and the entry points.  The GEMM kernels are compiled by tile family in igemm_small.hip / igemm_large.hip / igemm_xl.hip (igemm_bl.h) and
// igemm_halo.hip, the weight packers in pack.hip; igemm_common.h holds what they share.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "igemm_common.h"

namespace mvldm {

// split-K: sum the fp32 partial slabs and run the same epilogue (deterministic, no atomics)
template <typename T> __global__ __launch_bounds__(256) void igemm_splitk_reduce(const IgemmParams p) {
    const bool geglu = p.epilogue == MVLDM_EPI_GEGLU;
    const size_t total = (size_t)p.M * p.n_dst;
    const size_t slab = (size_t)p.M * p.n_pad;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int m = (int)(idx / p.n_dst), col = (int)(idx - (size_t)m * p.n_dst);
        float v;
        if (geglu) {
            const int nv = (col >> 5) * 64 + (col & 31), ng = nv + 32;
            float a = 0.f, g = 0.f;
            for (int s = 0; s < p.splitk; ++s) {
                a += p.ws[s * slab + (size_t)m * p.n_pad + nv];
                g += p.ws[s * slab + (size_t)m * p.n_pad + ng];
            }
            if (p.bias) { a += p.bias[col]; g += p.bias[p.n_dst + col]; }
            v = a * gelu_erf_fast(g);
        } else {
            float a = 0.f;
            for (int s = 0; s < p.splitk; ++s) a += p.ws[s * slab + (size_t)m * p.n_pad + col];
            if (p.bias) a += p.bias[col];
            if (p.row_bias) a += p.row_bias[(size_t)(m / p.hw_out) * p.row_bias_ld + col];
            if (p.epilogue == MVLDM_EPI_SILU) a = silu_f(a);
            else if (p.epilogue == MVLDM_EPI_GELU) a = gelu_erf_fast(a);
            v = a;
        }
        epilogue_store<T, true>(p, m, col, v);
    }
}

// the same reduction, 8 output columns per thread (16-bit output, 8-column-aligned rows): 16-byte slab / bias / residual loads
// and one 16-byte store instead of eight scalar round trips and eight index divisions.  At one scene a DDIM step runs ~125
// split-K launches and the scalar form (7.8 us per launch on average) was 11 % of the GPU time.
template <typename T> __global__ __launch_bounds__(256) void igemm_splitk_reduce_vec(const IgemmParams p) {
    const bool geglu = p.epilogue == MVLDM_EPI_GEGLU;
    const int cpr = p.n_dst / 8;                                  // 8-column chunks per output row
    const size_t total = (size_t)p.M * cpr;
    const size_t slab = (size_t)p.M * p.n_pad;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int m = (int)(idx / cpr), col = (int)(idx - (size_t)m * cpr) * 8;
        const int nv = geglu ? (col >> 5) * 64 + (col & 31) : col;
        const float* w0 = p.ws + (size_t)m * p.n_pad + nv;
        float a[8], g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = g[e] = 0.f;
        // the slabs are summed in split order (fixed: same bits on every run), FOUR slabs' loads in flight at a time: with one slab per
        // iteration every add waited for its own L2 round trip -- 10 splits = 10 dependent latencies = 5-6 us for a 7 MB read
        // (rocprofv3, the 4x4-level convs of one scene), as long as a third of the GEMM it finishes
        int s = 0;
        for (; s + 4 <= p.splitk; s += 4) {
            f32x4 lo[4], hi[4], gl[4], gh[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                lo[u] = *reinterpret_cast<const f32x4*>(w0 + (s + u) * slab);
                hi[u] = *reinterpret_cast<const f32x4*>(w0 + (s + u) * slab + 4);
                if (geglu) {
                    gl[u] = *reinterpret_cast<const f32x4*>(w0 + (s + u) * slab + 32);
                    gh[u] = *reinterpret_cast<const f32x4*>(w0 + (s + u) * slab + 36);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { a[e] += lo[u][e]; a[4 + e] += hi[u][e]; }
                if (geglu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { g[e] += gl[u][e]; g[4 + e] += gh[u][e]; }
                }
            }
        }
        for (; s < p.splitk; ++s) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(w0 + s * slab), hi = *reinterpret_cast<const f32x4*>(w0 + s * slab + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] += lo[e]; a[4 + e] += hi[e]; }
            if (geglu) {
                const f32x4 gl = *reinterpret_cast<const f32x4*>(w0 + s * slab + 32), gh = *reinterpret_cast<const f32x4*>(w0 + s * slab + 36);
#pragma unroll
                for (int e = 0; e < 4; ++e) { g[e] += gl[e]; g[4 + e] += gh[e]; }
            }
        }
        if (p.bias) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += p.bias[col + e];
        }
        if (geglu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] *= gelu_erf_fast(g[e] + (p.bias ? p.bias[p.n_dst + col + e] : 0.f));
        } else {
            if (p.row_bias) {
                const float* rb = p.row_bias + (size_t)(m / p.hw_out) * p.row_bias_ld + col;
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += rb[e];
            }
            if (p.epilogue == MVLDM_EPI_SILU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] = silu_f(a[e]);
            } else if (p.epilogue == MVLDM_EPI_GELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] = gelu_erf_fast(a[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] *= p.out_scale;
        if (p.residual) {
            const Chunk<T> rc = load_chunk<T>(reinterpret_cast<const T*>(p.residual) + (size_t)m * p.n_dst + col);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += rc.get(e);
        }
        size_t drow = (size_t)m;
        if (p.scatter) {
            const int img = m / p.hw_out, rem = m - img * p.hw_out;
            const int i = rem / p.w_out, j = rem - i * p.w_out;
            drow = ((size_t)img * (2 * p.h_out) + 2 * i + p.ph_y) * (size_t)(2 * p.w_out) + 2 * j + p.ph_x;
        }
        Chunk<T> oc;
#pragma unroll
        for (int e = 0; e < 8; ++e) oc.set(e, a[e]);
        store_chunk<T>(reinterpret_cast<T*>(p.dst) + drow * p.dst_ld + col, oc);
    }
}

// ---- host side ------------------------------------------------------------------------------------
// tuning knobs (read once): MVLDM_IGEMM_STAGES (0 = heuristic), MVLDM_IGEMM_TARGET (split-K workgroup
// target), MVLDM_IGEMM_SYNC=1 (force the register-prefetch main loop for 16-bit types: A/B testing)
static int env_int(const char* name, int dflt) { return knob_int(name, dflt); }      // (experiment builds only: common.h)
static const int kEnvTarget = env_int("MVLDM_IGEMM_TARGET", 0);
static const int kEnvSync = env_int("MVLDM_IGEMM_SYNC", 0);
static const int kEnvPx = env_int("MVLDM_IGEMM_PX", 0);
static const int kEnvNoStage = env_int("MVLDM_IGEMM_NOSTAGE", 0);
// MVLDM_IGEMM_FAKE makes every conv/linear return WRONG results (operands read as zeros, epilogue skipped): it exists
// for the roofline experiments of tools/fake_probe.sh only and is compiled in only with -DMVLDM_EXPERIMENTS
// (MVLDM_EXPERIMENTS=1 python -m mv_ldm_amd._build --force); the product library ignores the variable.
#ifdef MVLDM_EXPERIMENTS
static const int kEnvFake = env_int("MVLDM_IGEMM_FAKE", 0);
#else
static constexpr int kEnvFake = 0;
#endif

// per-call tuning overrides ride in the upper bits of desc.tile: bits 8-11 px (XCD grid), bit 12 register-prefetch
// loop instead of the LDS-DMA one (A/B testing)
static thread_local int t_force_sync = 0;

// every kernel-bearing file launches its own tiles (igemm_common.h)
static int launch_igemm(const IgemmParams& p, int tile, int act_dtype, hipStream_t s) {
    if (tile >= 1 && tile <= 5) return igemm_launch_small(p, tile, act_dtype, s);
    if (tile >= 6 && tile <= 8) return igemm_launch_large(p, tile, act_dtype, s);
    if (tile == 9 || tile == 10 || tile == 18) return igemm_launch_xl(p, tile, act_dtype, s);
    if (tile == 11 || tile == 17) return igemm_launch_halo(p, tile, act_dtype, s);
    return set_error(MVLDM_ERR_ARG, "igemm: bad tile %d", tile);
}


// Pick tile + split-K.  Target: >= ~2 workgroups per CU (256 CUs) without shredding K below 4 tiles.
static void choose_config(const mvldm_igemm_desc& d, int M, int k_tiles, int& tile, int& splitk, size_t ws_bytes) {
    const int target = kEnvTarget ? kEnvTarget : 512;
    if (tile == 0) {
        // measured on MI355X (tools/igemm_sweep.py, profiles/r01_igemm_sweep_*.json): the 32x64 wave tile
        // wins everywhere at these sizes (3 workgroups per CU with a 2-deep ring); 128x64 for 3x3 convs
        // and narrow N, 64x128 for wide Linear layers; tiny M gets the small tiles.
        // Large problems are bound by the L2 -> LDS fill rate (PMC: ~18 TB/s at 43 flop/byte with 128x64
        // tiles): the 8-wave 256x128 / 128x256 tiles halve the bytes per flop and take a 3-deep ring.  They
        // need >= ~300 workgroups to keep 256 CUs busy (profiles/r01_igemm_sweep2_*.json).
        // 256x320: no N padding at this UNet's channel counts (320/640/960/1280) and the best bytes-per-flop, but
        // only ~1 workgroup per CU: needs whole rounds of 256 workgroups (sweep5: +14..33 % on the 32x32-level
        // convs / Linears at 32 scenes, a loss below ~2 rounds)
        const bool can10 = d.act_dtype != MVLDM_F32 && d.k_order == 1 && d.dst_dtype != MVLDM_F32 && d.n_pad % 320 == 0 &&
                           d.epilogue != MVLDM_EPI_GEGLU && d.upsample != 1 && d.n_out % 8 == 0 && (d.dst_ld <= 0 || d.dst_ld % 8 == 0) &&
                           !(d.ksize == 3 && d.src1);
        const int wgs10 = cdiv(M, 256) * (d.n_pad / 320);
        const double eff10 = (double)wgs10 / (256.0 * cdiv(wgs10, 256));
        // (Linears keep winning down to 2 ragged rounds: 908 vs 850 TFLOP/s at 576 workgroups; 3x3 convs do not)
        if (can10 && (wgs10 >= 1024 || (wgs10 >= 512 && (eff10 >= 0.9 || d.ksize == 1)))) tile = 10;
        else if (M <= 32) tile = 5;
        else if (M <= 64) tile = 4;
        else if (d.ksize >= 2) tile = cdiv(M, 256) * cdiv(d.n_pad, 128) >= 300 ? 7 : 2;
        else if (d.n_pad >= 768 && d.act_dtype != MVLDM_F32 && d.k_order == 1 && d.dst_dtype != MVLDM_F32 &&
                 cdiv(M, 256) * cdiv(d.n_pad, 256) >= 1024)
            tile = 9;   // wide Linear (QKV, GEGLU) with >= 4 rounds of workgroups: 256x256 measured +10-15 % over
                        // 128x256 / 64x128 (sweep4); at 1-2 rounds its quantisation loses 2x (N=1280 at 8x8)
        else if (d.k_pad >= 1024 && d.n_pad >= 1024 && cdiv(M, 128) * cdiv(d.n_pad, 256) >= 300) tile = 8;
        else tile = d.n_pad < 640 ? 2 : 3;
    }
    const int tm = cdiv(M, kTiles[tile].bm), tn = cdiv(d.n_pad, kTiles[tile].bn);
    if (splitk == 0) {
        splitk = 1;
        const int wgs = tm * tn;
        if (wgs < target) splitk = std::min(std::max(k_tiles / 4, 1), cdiv(target, wgs));
        if (d.workspace == nullptr) splitk = 1;
        while (splitk > 1 && (size_t)splitk * M * d.n_pad * sizeof(float) > ws_bytes) --splitk;
    }
    splitk = std::max(1, std::min(splitk, k_tiles));
}

static int fill_params(const mvldm_igemm_desc& d, IgemmParams& p, int& tile) {
    const int epc = d.act_dtype == MVLDM_F32 ? 4 : 8;
    const int bk = d.act_dtype == MVLDM_F32 ? 32 : 64;
    MVLDM_REQUIRE(d.src0 && d.weight && d.dst, "igemm: null pointer");
    // upsample: 0 none, 1 nearest-2x before a 3x3 conv (gather form), 2..5 = sub-pixel phase (py, px) = ((u-2)>>1, (u-2)&1) of the
    // same conv decomposed into four 2x2 convs on the low-resolution image (weights pre-summed by the caller)
    const bool phase = d.upsample >= 2;
    MVLDM_REQUIRE(d.upsample >= 0 && d.upsample <= 5, "igemm: upsample %d", d.upsample);
    MVLDM_REQUIRE(phase ? (d.ksize == 2 && d.stride == 1 && d.h_out == d.h_in && d.w_out == d.w_in && !d.src1 && !d.residual &&
                           !d.row_bias && d.act_dtype != MVLDM_F32 && d.dst_dtype == d.act_dtype && d.k_order == 1)
                        : (d.ksize == 1 || d.ksize == 3),
                  "igemm: ksize %d / upsample %d", d.ksize, d.upsample);
    MVLDM_REQUIRE(d.stride == 1 || d.stride == 2, "igemm: stride %d", d.stride);
    MVLDM_REQUIRE(d.c0 % epc == 0 && d.c1 % epc == 0 && d.c0 > 0, "igemm: channels (%d,%d) must be multiples of %d", d.c0, d.c1, epc);
    MVLDM_REQUIRE((d.c1 == 0) == (d.src1 == nullptr), "igemm: src1/c1 mismatch");
    MVLDM_REQUIRE(d.k_pad % bk == 0 && d.k_pad >= d.ksize * d.ksize * (d.c0 + d.c1), "igemm: k_pad %d", d.k_pad);
    MVLDM_REQUIRE(d.n_pad % 64 == 0 && d.n_pad >= d.n_out, "igemm: n_pad %d (n_out %d)", d.n_pad, d.n_out);
    MVLDM_REQUIRE(d.dst_dtype == d.act_dtype || d.dst_dtype == MVLDM_F32, "igemm: dst dtype");
    if (d.epilogue == MVLDM_EPI_GEGLU)
        MVLDM_REQUIRE(d.n_out % 64 == 0 && !d.row_bias, "igemm: GEGLU needs n_out %% 64 == 0");
    p.src0 = d.src0; p.src1 = d.src1; p.weight = d.weight; p.bias = d.bias; p.row_bias = d.row_bias;
    p.residual = d.residual; p.dst = d.dst; p.ws = d.workspace;
    p.c0 = d.c0; p.c1 = d.c1; p.ctot = d.c0 + d.c1;
    p.n_img = d.n_img; p.h_in = d.h_in; p.w_in = d.w_in; p.h_out = d.h_out; p.w_out = d.w_out;
    p.hw_out = d.h_out * d.w_out;
    p.ksize = d.ksize; p.stride = d.stride; p.pad = d.pad; p.upsample = phase ? 0 : d.upsample; p.taps = d.ksize * d.ksize;
    p.scatter = phase; p.ph_y = phase ? (d.upsample - 2) >> 1 : 0; p.ph_x = phase ? (d.upsample - 2) & 1 : 0;
    // tap t reads input pixel (oy*stride + ty0 + t/ks, ox*stride + tx0 + t%ks); (cy, cx) is a tap offset that is inside the image
    // for every output pixel: the centre of a padded 3x3 / the pixel itself for a 2x2 phase (whose taps start at py-1, px-1)
    p.ty0 = phase ? p.ph_y - 1 : -d.pad; p.tx0 = phase ? p.ph_x - 1 : -d.pad;
    p.cy = phase ? 1 - p.ph_y : d.ksize / 2; p.cx = phase ? 1 - p.ph_x : d.ksize / 2;
    p.M = d.n_img * p.hw_out; p.n_out = d.n_out; p.n_pad = d.n_pad; p.k_pad = d.k_pad;
    p.n_dst = d.epilogue == MVLDM_EPI_GEGLU ? d.n_out / 2 : d.n_out;
    p.rb_vec = d.row_bias && ((uintptr_t)d.row_bias % 16 == 0) && d.row_bias_ld % 4 == 0;
    p.bias_vec = d.bias && ((uintptr_t)d.bias % 16 == 0);
    p.row_bias_ld = d.row_bias_ld; p.epilogue = d.epilogue; p.dst_f32 = d.dst_dtype == MVLDM_F32;
    p.out_scale = d.out_scale;
    p.dst_ld = d.dst_ld > 0 ? d.dst_ld : p.n_dst;
    MVLDM_REQUIRE(p.dst_ld >= p.n_dst, "igemm: dst_ld %d < n_dst %d", p.dst_ld, p.n_dst);
    p.k_tiles = d.k_pad / bk;
    tile = d.tile & 63;
    t_force_sync = (d.tile >> 12) & 1;
    const int force_px = (d.tile >> 8) & 15;
    int splitk = d.splitk;
    MVLDM_REQUIRE(((tile >= 0 && tile <= kNumTiles) || tile == 17 || deep_tile(tile)) && splitk >= 0, "igemm: tile/splitk");
    choose_config(d, p.M, p.k_tiles, tile, splitk, d.workspace_bytes);
    // (a phase conv may split K like any other: its partial slabs are indexed by the LOW-resolution row and the reduce kernel scatters)
    if (splitk > 1)
        MVLDM_REQUIRE(d.workspace && (size_t)splitk * p.M * d.n_pad * sizeof(float) <= d.workspace_bytes,
                      "igemm: split-K workspace too small");
    // lean 16-bit loop: block-major K, extents addressable by a 32-bit buffer offset
    const double es = 2.0;
    const double b0 = (double)d.n_img * d.h_in * d.w_in * d.c0 * es, b1 = (double)d.n_img * d.h_in * d.w_in * d.c1 * es;
    const double bw = (double)d.n_pad * d.k_pad * es;
    p.use_bl = d.act_dtype != MVLDM_F32 && d.k_order == 1 && !t_force_sync && !kEnvSync &&
               b0 < 4.0e9 && b1 < 4.0e9 && bw < 4.0e9;
    if (d.act_dtype != MVLDM_F32 && d.k_order == 1 && !t_force_sync && !kEnvSync && !p.use_bl) {
        // a source or the weight is beyond the 32-bit buffer-offset range of the LDS-DMA loop: the launch is still correct
        // on the 64-bit-pointer register-prefetch loop, but 3-5x slower -- say so once (callers chunk the batch: vae._chunks)
        static bool warned = false;
        if (!warned) {
            warned = true;
            fprintf(stderr, "[mvldm] igemm: operand of %.2f GB exceeds the 4 GB range of the fast 16-bit loop; using the slower "
                            "64-bit-address loop (split the batch to avoid this)\n", std::max(std::max(b0, b1), bw) / 1e9);
        }
    }
    p.src0_bytes = (unsigned)b0; p.src1_bytes = (unsigned)b1; p.w_bytes = (unsigned)bw;
    p.fake = kEnvFake;
    // An output of half the 256 MB Infinity Cache or more is gone from every cache before its consumer starts: written with
    // streaming stores it does not evict the operand tiles the other workgroups are re-reading (-0.4 % per DDIM step at 64 scenes,
    // same-box A/B); small outputs (a few scenes) stay cacheable for the next op.  MVLDM_STREAM_STORES=0 / 1 forces it.
    p.nt_store = stream_stores((size_t)p.M * (size_t)p.n_dst * (p.dst_f32 || d.act_dtype == MVLDM_F32 ? 4 : 2));
    if (kEnvFake & 1) p.src0_bytes = p.src1_bytes = 0;   // EXPERIMENT ONLY: every A piece fails the range check (zeros, no L2 traffic)
    if (kEnvFake & 2) p.w_bytes = 0;                     // same for W
    if (tile >= 6 && !p.use_bl) tile = 2;
    if (deep_tile(tile) && d.upsample) tile = 2;      // (no per-tap tables / phase scatter in the deep-ring instantiations)
    p.splitk = splitk;
    if (p.use_bl) {   // splits own whole channel blocks (all taps of a block stay together)
        const int cbs = p.k_tiles / p.taps;
        const int per = cdiv(cbs, std::min(splitk, cbs));
        p.k_tiles_per_split = per * p.taps;
        p.splitk = cdiv(cbs, per);
    } else {
        p.k_tiles_per_split = cdiv(p.k_tiles, splitk);
        p.splitk = cdiv(p.k_tiles, p.k_tiles_per_split);  // drop empty splits
    }
    // LDS-staged epilogue: 16-byte rows need 8-column alignment of the 16-bit output (or a split-K slab)
    p.stage_epi = d.act_dtype != MVLDM_F32 && !kEnvNoStage && (p.splitk > 1 || (!p.dst_f32 && p.n_dst % 8 == 0 && p.dst_ld % 8 == 0));
    if (tile >= 9 && tile <= 10 && (!p.stage_epi || (tile == 10 && d.epilogue == MVLDM_EPI_GEGLU))) tile = 7;   // no per-element epilogue there; odd TN cannot pair GEGLU columns
    if (tile == 11 && !(p.use_bl && p.stage_epi && p.splitk == 1 && d.ksize == 3 && d.stride == 1 && d.pad == 1 && !d.upsample &&
                        d.h_out == d.h_in && d.w_out == d.w_in && halo_rows_for(d.w_in) <= 384 && halo_smem(d.w_in) <= 160 * 1024))
        tile = 7;   // the halo kernel only does 3x3 / stride 1 / pad 1 on images up to 63 pixels wide, one K pass
    if (tile == 17 && !(p.use_bl && p.stage_epi && p.splitk == 1 && d.ksize == 3 && d.stride == 1 && d.pad == 1 && !d.upsample && d.c1 == 0 &&
                        d.h_out == d.h_in && d.w_out == d.w_in && d.epilogue != MVLDM_EPI_GEGLU && halow_smem(d.w_in) <= 160 * 1024))
        tile = 7;   // the wide halo kernel: one-source 3x3 / stride 1 / pad 1 on maps up to 24 pixels wide, one K pass
    if (phase) {
        MVLDM_REQUIRE(p.use_bl && p.stage_epi, "igemm: 2x2 phase conv needs the lean 16-bit loop and an 8-aligned 16-bit output");
        if (tile != 7 && tile != 10) tile = 2;
    }
    if (p.use_bl && d.upsample == 1 && tile != 7) tile = 2;
    if (p.use_bl && d.upsample != 1) {
        // the lean loop addresses every tap relative to the centre tap: it must lie inside the image
        const int hc = (d.h_out - 1) * d.stride + p.ty0 + p.cy, wc = (d.w_out - 1) * d.stride + p.tx0 + p.cx;
        MVLDM_REQUIRE(p.ty0 + p.cy >= 0 && p.tx0 + p.cx >= 0 && hc < d.h_in && wc < d.w_in,
                      "igemm: conv geometry (pad %d, stride %d) not supported", d.pad, d.stride);
    }
    p.tiles_m = cdiv(p.M, kTiles[tile].bm);
    p.tiles_n = cdiv(d.n_pad, kTiles[tile].bn);
    p.korder = d.k_order;
    if (d.k_order)
        MVLDM_REQUIRE(d.k_order == 1 && p.ctot % bk == 0 && d.c0 % bk == 0 && d.k_pad == p.taps * p.ctot,
                      "igemm: k_order 1 needs channel counts (%d,%d) multiples of %d", d.c0, d.c1, bk);
    // XCD grid px x py (px * py = 8): fabric traffic ~ py * bytes(A) + px * bytes(W), idle tiles penalised
    {
        const double a_bytes = (double)d.n_img * d.h_in * d.w_in * p.ctot, w_bytes = (double)d.n_pad * d.k_pad;
        double best = 1e300;
        for (int px = 1; px <= 8; px *= 2) {
            const int py = 8 / px;
            const int sm = cdiv(p.tiles_m, px), sn = cdiv(p.tiles_n, py);
            const double waste = (double)(8 * sm * sn) / ((double)p.tiles_m * p.tiles_n);
            const double cost = (py * a_bytes + px * w_bytes) * waste * waste;
            if (cost < best) { best = cost; p.px = px; p.sub_m = sm; p.sub_n = sn; }
        }
        p.m_fast = w_bytes >= a_bytes;
        const int fpx = force_px ? force_px : kEnvPx;
        if (fpx > 0 && fpx <= 8 && (8 % fpx) == 0) {
            p.px = fpx; p.sub_m = cdiv(p.tiles_m, p.px); p.sub_n = cdiv(p.tiles_n, 8 / p.px);
        }
        // block of tiles the XCD's concurrently running workgroups cover (8-wave tiles: one workgroup per CU, 32 CUs): the shape that
        // minimises the partition's fabric traffic A_x * ceil(sub_n / gn) + W_x * ceil(sub_m / gm) with gm * gn = 32.
        // MVLDM_IGEMM_GROUP=0 keeps the one-row / one-column order (A/B knob), "gm" forces the row count.
        p.grp_m = p.grp_n = 1;
        static const int kGroup = knob_int("MVLDM_IGEMM_GROUP", -1);
        if (kGroup != 0 && ((tile >= 7 && tile <= 10) || tile == 17) && p.sub_m * p.sub_n > 32) {
            const double ax = a_bytes / p.px, wx = w_bytes / (8 / p.px);
            double bestc = 1e300;
            for (int gm = 1; gm <= 32; gm *= 2) {
                if (kGroup > 0 && gm != kGroup) continue;
                const int gme = std::min(gm, p.sub_m), gne = std::min(32 / gm, p.sub_n);
                const double c = ax * cdiv(p.sub_n, gne) + wx * cdiv(p.sub_m, gme);
                if (c < bestc) { bestc = c; p.grp_m = gme; p.grp_n = gne; }
            }
        }
    }
    return MVLDM_OK;
}

// tile 12: the persistent, epilogue-pipelined Linear kernel of linear_pp.hip; tile 13: the persistent wide Linear of linear_pw.hip
int linear_pp_run(const mvldm_igemm_desc& d, hipStream_t s);
int linear_pw_run(const mvldm_igemm_desc& d, hipStream_t s);
int linear_ws_run(const mvldm_igemm_desc& d, hipStream_t s);      // tile 14: weight-stationary Linear for K = 320 (linear_ws.hip)
int skinny_run(const mvldm_igemm_desc& d, hipStream_t s);         // tile 15: skinny-M weight-streaming GEMM on the fragment-order pack (skinny.hip)
int linear_rs_run(const mvldm_igemm_desc& d, hipStream_t s);      // tile 19: register-staged persistent Linear, 4 waves of 128 x 128 (linear_rs.hip)

int igemm_run(const mvldm_igemm_desc& d, hipStream_t s) {
    IgemmParams p;
    int tile = 0;
    if (d.n_img == 0 || d.h_out == 0 || d.w_out == 0) return MVLDM_OK;   // empty batch: nothing to do (its buffers may be null)
    const int req = d.tile & 63;
    if (req == 15) return skinny_run(d, s);
    if (req == 12 || req == 13 || req == 14 || req == 19) {      // the Linear tiles of the other files
        MVLDM_REQUIRE(d.src0 && d.weight && d.dst, "igemm: null pointer");
        return req == 12 ? linear_pp_run(d, s) : req == 13 ? linear_pw_run(d, s) : req == 14 ? linear_ws_run(d, s) : linear_rs_run(d, s);
    }
    MVLDM_REQUIRE(d.k_order != 2, "igemm: the fragment-order pack (k_order 2) is read by tile 15 only");
    int rc = fill_params(d, p, tile);
    if (rc) return rc;
    if (p.M == 0) return MVLDM_OK;
    rc = dispatch_dtype(d.act_dtype, [&](auto t) {
        using T = decltype(t);
        int r = launch_igemm(p, tile, Elt<T>::DT, s);
        if (r) return r;
        if (p.splitk > 1) {
            if constexpr (sizeof(T) == 2) {
                if (!p.dst_f32 && p.n_dst % 8 == 0 && p.dst_ld % 8 == 0 && ((uintptr_t)p.ws % 16) == 0 &&
                    (!p.residual || ((uintptr_t)p.residual % 16) == 0) && ((uintptr_t)p.dst % 16) == 0) {
                    const size_t chunks = (size_t)p.M * (p.n_dst / 8);
                    hipLaunchKernelGGL(igemm_splitk_reduce_vec<T>, dim3((unsigned)std::min<size_t>((chunks + 255) / 256, 4096)), dim3(256), 0, s, p);
                    return check_launch();
                }
            }
            const size_t total = (size_t)p.M * p.n_dst;
            const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
            hipLaunchKernelGGL(igemm_splitk_reduce<T>, dim3(blocks), dim3(256), 0, s, p);
            return check_launch();
        }
        return (int)MVLDM_OK;
    });
    return rc;
}

}  // namespace mvldm

using namespace mvldm;

extern "C" int mvldm_igemm_fwd(const mvldm_igemm_desc* d, mvldm_stream_t stream) {
    MVLDM_REQUIRE(d != nullptr, "igemm: null desc");
    return igemm_run(*d, (hipStream_t)stream);
}

extern "C" size_t mvldm_igemm_workspace_bytes(const mvldm_igemm_desc* d) {
    if (!d) return 0;
    const size_t M = (size_t)d->n_img * d->h_out * d->w_out;
    // the heuristic never splits deeper than ~512 workgroups' worth; 16 slabs is a safe ceiling
    return (size_t)16 * M * d->n_pad * sizeof(float);
}

