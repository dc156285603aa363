// The two general implicit-GEMM kernels and their launchers: igemm_kernel (register prefetch: f32, and the 16-bit problems the lean loop
// cannot take) and igemm_bl_kernel (LDS-DMA, every tile / tap / source / upsample form).  Included by igemm_small.hip, igemm_large.hip and
// igemm_xl.hip only, which divide the tiles between them -- a quick-compile experiment on one tile compiles one of those files.
#pragma once
#include "igemm_common.h"

namespace mvldm {

template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void igemm_kernel(const IgemmParams p) {
    using M_ = Mma<T>;
    constexpr int NT = WM * WN * 64;
    constexpr int EPC = Elt<T>::EPC;
    constexpr int BK = M_::BK;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int A_BYTES = BM * M_::PITCH, B_BYTES = BN * M_::PITCH;
    constexpr int A_IT = BM * 8 / NT, B_IT = BN * 8 / NT;
    static_assert(A_IT >= 1 && B_IT >= 1 && TM >= 1 && TN >= 1, "bad tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int hi = lane >> 5, l31 = lane & 31;

    int split, tm, tn;
    if (!map_block(p, split, tm, tn)) return;   // uniform per workgroup, before any barrier
    const int kt0 = split * p.k_tiles_per_split;
    const int kt1 = min(kt0 + p.k_tiles_per_split, p.k_tiles);

    // ---- loader coordinates (fixed per thread across the K loop) ----
    const int kc = tid & 7, r0 = tid >> 3;
    int a_img[A_IT], a_y[A_IT], a_x[A_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int m = tm * BM + r0 + it * (NT / 8);
        if (m < p.M) {
            const int img = m / p.hw_out, rem = m - img * p.hw_out;
            const int oy = rem / p.w_out;
            a_img[it] = img;
            a_y[it] = oy * p.stride - p.pad;
            a_x[it] = (rem - oy * p.w_out) * p.stride - p.pad;
        } else {
            a_img[it] = -1; a_y[it] = 0; a_x[it] = 0;
        }
    }
    const T* wbase = reinterpret_cast<const T*>(p.weight) + (size_t)(tn * BN + r0) * p.k_pad + kc * EPC;
    const int hs = p.upsample ? 2 * p.h_in : p.h_in, wsz = p.upsample ? 2 * p.w_in : p.w_in;

    u32x4 areg[A_IT], breg[B_IT];
    auto load_tile = [&](int kt) {
        int tap, c;
        if (p.korder) {
            const int cb = kt / p.taps;
            tap = kt - cb * p.taps;
            c = cb * BK + kc * EPC;
        } else {
            const int ke = kt * BK + kc * EPC;
            tap = ke / p.ctot;
            c = ke - tap * p.ctot;
        }
        const bool tap_ok = tap < p.taps;
        const int ky = tap / p.ksize, kx = tap - ky * p.ksize;
        const bool from0 = c < p.c0;
        const T* sbase = from0 ? reinterpret_cast<const T*>(p.src0) + c
                               : reinterpret_cast<const T*>(p.src1) + (c - p.c0);
        const int cs = from0 ? p.c0 : p.c1;
#pragma unroll
        for (int it = 0; it < A_IT; ++it) {
            int iy = a_y[it] + ky, ix = a_x[it] + kx;
            const bool ok = tap_ok && a_img[it] >= 0 && iy >= 0 && iy < hs && ix >= 0 && ix < wsz;
            if (p.upsample) { iy >>= 1; ix >>= 1; }
            if (ok) {
                const size_t off = ((size_t)(a_img[it] * p.h_in + iy) * p.w_in + ix) * cs;
                areg[it] = *reinterpret_cast<const u32x4*>(sbase + off);
            } else {
                areg[it] = u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int it = 0; it < B_IT; ++it) {
            const int n = tn * BN + r0 + it * (NT / 8);
            if (n < p.n_pad)
                breg[it] = *reinterpret_cast<const u32x4*>(wbase + (size_t)it * (NT / 8) * p.k_pad + (size_t)kt * BK);
            else
                breg[it] = u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store_tile = [&](int stage) {
        char* at = smem + stage * (A_BYTES + B_BYTES);
        char* bt = at + A_BYTES;
#pragma unroll
        for (int it = 0; it < A_IT; ++it) M_::store(at, r0 + it * (NT / 8), kc, areg[it]);
#pragma unroll
        for (int it = 0; it < B_IT; ++it) M_::store(bt, r0 + it * (NT / 8), kc, breg[it]);
    };

    f32x16 acc[TM][TN];      // (cleared in place: a shared zero_acc(acc) helper changes the code of 74 kernels -- igemm_common.h)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (kt0 < kt1) {
        load_tile(kt0);
        store_tile(0);
    }
    __syncthreads();
    int cur = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        const bool more = kt + 1 < kt1;
        if (more) load_tile(kt + 1);
        const char* at = smem + cur * (A_BYTES + B_BYTES);
        const char* bt = at + A_BYTES;
#pragma unroll
        for (int kk = 0; kk < BK / M_::KI; ++kk) {
            typename M_::Frag a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = M_::load(at, wm * (BM / WM) + i * 32 + l31, kk, hi);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = M_::load(bt, wn * (BN / WN) + j * 32 + l31, kk, hi);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = M_::mma(a[i], b[j], acc[i][j]);
        }
        if (more) store_tile(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // 16-bit problems that cannot take the lean loop (conv_in of the UNet and of the VAE encoder: 3 / 11 input channels) still write
    // 16-byte rows through the LDS-staged epilogue: the per-element form stores 2-byte values 64 B per row and instruction -- the VAE's
    // conv_in at 32 images of 256 x 256 (537 MB of output, 14 GFLOP) took 2.3 ms of a 68 ms training step, 0.23 TB/s
    if constexpr (sizeof(T) == 2) {
        if (p.stage_epi) {
            igemm_epilogue_staged<T, BM, BN, WM, WN>(p, acc, tm, tn, split, wm, wn, wave, lane, smem);
            return;
        }
    }
    igemm_epilogue<T, BM, BN, WM, WN>(p, acc, tm, tn, split, wm, wn, hi, l31);
}

// ---- 16-bit main loop, lean form: buffer-load LDS-DMA, unrolled taps -----------------------------------
// For the block-major K order every K-tile is (64-channel block cb, tap): the tap loop is unrolled, so each
// lane's pixel offset for each tap is a REGISTER computed once per workgroup (out-of-image taps and rows
// beyond M hold an out-of-range offset: the buffer descriptor's bounds check returns zeros, which the DMA
// writes to LDS -- no zero page, no select).  Inside the loop a tile costs per wave: A_IT + B_IT
// `buffer_load_dwordx4 ... lds` with a scalar soffset (channel block / K position), the M0 updates, the
// fragment ds_reads and the MFMAs -- no vector address arithmetic at all (PMC of the previous loop: 11
// VALU + 16 SALU instructions per MFMA).

// Per-lane source addressing of the A pieces.  Without upsampling every tap of a pixel is the centre tap's
// byte offset plus a displacement that is the same for all lanes, so a lane keeps ONE offset per piece and
// a 9-bit validity mask; the displacement rides in the scalar offset of the buffer load (the descriptor's
// base is moved back by one row + one pixel so that it is never negative).  Nearest-2x upsampling makes the
// displacement depend on the parity of the lane's pixel: those (few) launches keep a per-tap table.
template <int TAPS, int A_IT, bool DUAL, bool UPS> struct BlAddr {
    unsigned a0[UPS ? TAPS : 1][A_IT];
    unsigned a1[DUAL ? (UPS ? TAPS : 1) : 1][DUAL ? A_IT : 1];
    unsigned mask[UPS ? 1 : A_IT];
};

// issue K-tile (channel block cb, tap t) into the ring slot at `stage_base`
// (STAGES is carried only to give every kernel instantiation its own copy: sharing one specialization
//  between two kernels trips the host pass of hipcc 7.2)
// (LO, HI: the pieces [LO, HI) of the tile's A_IT + B_IT, activation pieces first -- the spread issue of the main loops)
template <typename T, int BM, int BN, int NW, int KS, bool DUAL, int A_IT, int B_IT, int STAGES, bool UPS, int t, int LO = 0, int HI = 1 << 20>
__device__ __forceinline__ void bl_issue(const IgemmParams& p, char* stage_base, int wave, int cb,
                                         const BlAddr<KS * KS, A_IT, DUAL, UPS>& ad, const unsigned (&vb)[B_IT]) {
    constexpr int BK = 64, TAPS = KS * KS;
    const int lead = (!UPS && KS > 1) ? p.w_in + 1 : 0;                                         // pixels
    const int disp = UPS ? 0 : (t / KS - p.cy) * p.w_in + (t % KS - p.cx) + lead;               // >= 0
    const unsigned lead0 = (unsigned)lead * (unsigned)p.c0 * 2u, lead1 = (unsigned)lead * (unsigned)p.c1 * 2u;
    const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.src0)) - lead0, 0, p.src0_bytes + lead0, 0x00020000);
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(DUAL ? p.src1 : p.src0)) - (DUAL ? lead1 : lead0), 0,
        DUAL ? p.src1_bytes + lead1 : p.src0_bytes + lead0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.weight), 0, p.w_bytes, 0x00020000);
    char* at = stage_base;
    char* bt = at + BM * 128;
    const int c = cb * BK;
    const bool from0 = !DUAL || c < p.c0;
    const int soff = ((from0 ? c : c - p.c0) + disp * (from0 ? p.c0 : p.c1)) * 2;
#pragma unroll
    for (int it = (LO > 0 ? LO : 0); it < (HI < A_IT ? HI : A_IT); ++it) {
        __attribute__((address_space(3))) void* dst = (__attribute__((address_space(3))) void*)(at + (wave + NW * it) * 1024);
        unsigned v0, v1;
        if constexpr (UPS) {
            v0 = ad.a0[t][it];
            v1 = ad.a1[DUAL ? t : 0][DUAL ? it : 0];
        } else {
            const bool ok = (ad.mask[it] >> t) & 1u;
            v0 = ok ? ad.a0[0][it] : kBufOob;
            v1 = ok ? ad.a1[0][DUAL ? it : 0] : kBufOob;
        }
        if (from0) __builtin_amdgcn_raw_ptr_buffer_load_lds(r0, dst, 16, v0, soff, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(r1, dst, 16, v1, soff, 0, 0);
    }
    const int koff = (cb * TAPS + t) * (BK * 2);
#pragma unroll
    for (int it = (LO > A_IT ? LO - A_IT : 0); it < (HI - A_IT < B_IT ? HI - A_IT : B_IT); ++it)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(bt + (wave + NW * it) * 1024), 16,
                                                 vb[it], koff, 0, 0);
}

// whole K-tile, fragments fetched right before use: the 4-wave tiles run 2-4 workgroups per CU and hide the LDS
// latency with occupancy (the pipelined form above costs them registers and measured 10-20 % slower)
template <typename T, int BM, int BN, int WM, int WN>
__device__ __forceinline__ void bl_compute(const char* stage_base, f32x16 (&acc)[BM / WM / 32][BN / WN / 32], int wm, int wn,
                                           int hi, int l31) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
#pragma unroll
    for (int kk = 0; kk < 64 / Mma<T>::KI; ++kk) {
        BlFrags<T, TM, TN> f;
        bl_load<T, BM, BN, WM, WN>(stage_base, f, kk, wm, wn, hi, l31);
        bl_mma<T, TM, TN>(f, acc);
    }
}

// s_waitcnt vmcnt(min(young, MAXY) * LPT) lgkmcnt(0): `young` tiles of LPT loads per wave may stay in flight behind the awaited one
template <int LPT, int MAXY>
__device__ __forceinline__ void bl_wait_young(int young) {
    if constexpr (MAXY >= 1) {
        if (young >= MAXY) {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(MAXY * LPT) : "memory");
            return;
        }
        bl_wait_young<LPT, MAXY - 1>(young);
    } else {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
}

template <typename T, int BM, int BN, int WM, int WN, int KS, bool DUAL, int STAGES, bool UPS>
__global__ __launch_bounds__(WM* WN * 64) void igemm_bl_kernel(const IgemmParams p) {
    using M_ = Mma<T>;
    static_assert(sizeof(T) == 2, "16-bit activation types only");
    constexpr int NW = WM * WN, TAPS = KS * KS;
    constexpr int BK = 64, EPC = 8;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int A_IT = BM / 8 / NW, B_IT = BN / 8 / NW, LPT = A_IT + B_IT;
    static_assert(A_IT >= 1 && B_IT >= 1 && (BM / 8) % NW == 0 && (BN / 8) % NW == 0, "bad tile");
    static_assert(STAGES >= 2 && STAGES <= 8, "ring depth");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const auto [lane, wave, wm, wn, hi, l31] = wave_lane<WN>();
    int split, tm, tn;
    if (!map_block(p, split, tm, tn)) return;
    // split-K partitions channel blocks (k_tiles_per_split is a multiple of TAPS for this kernel)
    const int cb0 = split * (p.k_tiles_per_split / TAPS);
    const int cb1 = min(cb0 + p.k_tiles_per_split / TAPS, p.k_tiles / TAPS);

    const int slot = lane & 7, rsub = lane >> 3;
    BlAddr<TAPS, A_IT, DUAL, UPS> ad;
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int row = (wave + NW * it) * 8 + rsub;
        const int m = tm * BM + row;
        const unsigned chunk = (unsigned)((slot ^ ((row >> 1) & 7)) * EPC);
        const bool live = m < p.M;
        const int img = live ? m / p.hw_out : 0, rem = live ? m - img * p.hw_out : 0;
        const int oy = rem / p.w_out, ox = rem - oy * p.w_out;
        if constexpr (UPS) {
            const unsigned hs = 2 * p.h_in, wsz = 2 * p.w_in;
            const int y0 = live ? oy * p.stride - p.pad : -(1 << 20), x0 = ox * p.stride - p.pad;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int iy = y0 + t / KS, ix = x0 + t % KS;
                const bool ok = (unsigned)iy < hs && (unsigned)ix < wsz;
                const unsigned pix = (unsigned)(img * p.h_in + (iy >> 1)) * (unsigned)p.w_in + (unsigned)(ix >> 1);
                ad.a0[t][it] = ok ? (pix * (unsigned)p.c0 + chunk) * 2u : kBufOob;
                if constexpr (DUAL) ad.a1[t][it] = ok ? (pix * (unsigned)p.c1 + chunk) * 2u : kBufOob;
            }
        } else {
            // centre tap (inside the image for every live row: checked on the host)
            const int yc = oy * p.stride + p.ty0 + p.cy, xc = ox * p.stride + p.tx0 + p.cx;
            const unsigned pix = (unsigned)(img * p.h_in + yc) * (unsigned)p.w_in + (unsigned)xc;
            unsigned msk = 0;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int iy = yc + t / KS - p.cy, ix = xc + t % KS - p.cx;
                msk |= (live && (unsigned)iy < (unsigned)p.h_in && (unsigned)ix < (unsigned)p.w_in) ? (1u << t) : 0u;
            }
            ad.a0[0][it] = (pix * (unsigned)p.c0 + chunk) * 2u;
            if constexpr (DUAL) ad.a1[0][it] = (pix * (unsigned)p.c1 + chunk) * 2u;
            ad.mask[it] = msk;
        }
    }
    unsigned vb[B_IT];      // (in place, as in the two halo kernels: a shared weight_row_offsets helper changes the code of these kernels)
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int row = (wave + NW * it) * 8 + rsub;
        const int n = tn * BN + row;
        const unsigned chunk = (unsigned)((slot ^ ((row >> 1) & 7)) * EPC);
        vb[it] = n < p.n_pad ? ((unsigned)n * (unsigned)p.k_pad + chunk) * 2u : kBufOob;
    }

    f32x16 acc[TM][TN];      // (cleared in place: a shared zero_acc(acc) helper changes the code of 74 kernels -- igemm_common.h)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // (no lambdas around the buffer builtins: an opaque __amdgpu_buffer_rsrc_t inside a lambda makes the
    //  host pass drop the kernel's stub -- free function templates instead)
#define MVLDM_BL_ISSUE(stage_, cb_, t_) \
    bl_issue<T, BM, BN, NW, KS, DUAL, A_IT, B_IT, STAGES, UPS, t_>(p, smem + (stage_) * STAGE_BYTES, wave, cb_, ad, vb)
#define MVLDM_BL_ISSUE_R(stage_, cb_, t_, lo_, hi_) \
    bl_issue<T, BM, BN, NW, KS, DUAL, A_IT, B_IT, STAGES, UPS, t_, lo_, hi_>(p, smem + (stage_) * STAGE_BYTES, wave, cb_, ad, vb)
#define MVLDM_BL_NEXT(t_, d_) (((t_) + (d_)) % TAPS)
#define MVLDM_BL_LOAD(f_, slot_, kk_) bl_load<T, BM, BN, WM, WN>(smem + (slot_) * STAGE_BYTES, f_, kk_, wm, wn, hi, l31)
#define MVLDM_BL_MMA(f_)                  \
    __builtin_amdgcn_sched_barrier(0);    \
    bl_mma<T, TM, TN>(f_, acc);           \
    __builtin_amdgcn_sched_barrier(0);
    // One K-tile.  On entry f0 holds (in flight) the kk=0 fragments of the tile in slot_c and tiles
    // T+1 .. T+STAGES-1 are in the ring.  After the last fragments of tile T are read, every wave waits for
    // its pieces of tile T+1, the barrier publishes them and retires slot_c, which is refilled with tile
    // T+STAGES at once; the kk=0 fragments of tile T+1 are then fetched under tile T's last MFMAs.
    // (round 6: the spread issue of MVLDM_BL_STEP_SIMPLE below was built here too -- 4/9 of the pieces behind the barrier, the rest in front of sub-steps
    //  1 and 2 of the next step -- and is neutral in the step's op table: up1 / down2 +1 ... +1.5 %, up2 / down1 -1 ... -1.5 %; not kept)
#define MVLDM_BL_STEP(t_)                                                                                         \
    {                                                                                                             \
        static_assert(64 / M_::KI == 4, "four k-sub-steps per K-tile");                                          \
        MVLDM_BL_LOAD(f1, slot_c, 1);                                                                             \
        MVLDM_BL_MMA(f0)                                                                                          \
        MVLDM_BL_LOAD(f0, slot_c, 2);                                                                             \
        MVLDM_BL_MMA(f1)                                                                                          \
        MVLDM_BL_LOAD(f1, slot_c, 3);                                                                             \
        MVLDM_BL_MMA(f0)                                                                                          \
        /* tile T+1 must have landed: behind it only tile T+2 can be in flight (3-deep ring, and only if it */    \
        /* exists -- nothing is issued past the end of K, so the tail drains with vmcnt(0)) */                     \
        if (STAGES == 3 && cb + ((t_) + 2) / TAPS < cb1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPT) : "memory"); \
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                          \
        __builtin_amdgcn_s_barrier();                                                                             \
        {                                                                                                         \
            /* (no constexpr locals as template arguments: the host pass rejects them inside a kernel) */       \
            const int cbn_ = cb + ((t_) + STAGES) / TAPS;                                                         \
            if (cbn_ < cb1) { MVLDM_BL_ISSUE(slot_c, cbn_, MVLDM_BL_NEXT(t_, STAGES)); }                          \
        }                                                                                                         \
        slot_c = slot_c + 1 == STAGES ? 0 : slot_c + 1;                                                           \
        MVLDM_BL_LOAD(f0, slot_c, 0);                                                                             \
        MVLDM_BL_MMA(f1)                                                                                          \
    }
    // 4-wave tiles: 2-slot ring, one barrier per tile, fragments fetched right before use
    // (round 6, SPREAD ISSUE: the next tile's LPT pieces used to go out in one burst behind the barrier -- every wave of the CU in the address path at
    //  once, ~ 70 cycles per piece with the matrix pipe idle (the same finding as tile 13's).  Now 4/9 of the pieces go out behind the
    //  barrier and the rest in front of sub-steps 1 and 2 (in front of their fragment reads: with the fragments live next to the piece offsets the
    //  256 x 320 3x3 kernel spilled); the last piece still has two sub-steps of MFMAs in front of the wait that needs it.  8-wave tiles only (tile 10: the 256 x 320
    //  convs of the 32 x 32 level, -3 % in the step's op table).  -DMVLDM_BL_BURST: the old order, A/B.)
#ifdef MVLDM_BL_BURST
    constexpr bool SPREAD_S = false;
#elif defined(MVLDM_BL_SPREAD_ALL)
    constexpr bool SPREAD_S = true;         // (experiment: the 4-wave tiles too)
#else
    constexpr bool SPREAD_S = NW == 8;      // (the 4-wave tiles run 2 - 4 workgroups per CU whose bursts already interleave: with it, -DMVLDM_BL_SPREAD_ALL, the 1 / 4-scene steps are 0.6 - 1 % slower)
#endif
#define MVLDM_BL_STEP_SIMPLE(t_)                                                                                  \
    {                                                                                                             \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                               \
        __builtin_amdgcn_s_barrier();                                                                             \
        if constexpr (!SPREAD_S) {                                                                                \
            const int cbn_ = cb + ((t_) + 1) / TAPS;                                                              \
            if (cbn_ < cb1) { MVLDM_BL_ISSUE(slot_c ^ 1, cbn_, MVLDM_BL_NEXT(t_, 1)); }                           \
            bl_compute<T, BM, BN, WM, WN>(smem + slot_c * STAGE_BYTES, acc, wm, wn, hi, l31);                     \
        } else {                                                                                                  \
            constexpr int Q0_ = (4 * LPT + 8) / 9, Q1_ = Q0_ + (LPT - Q0_ + 1) / 2;                              \
            const int cbn_ = cb + ((t_) + 1) / TAPS;                                                              \
            const bool more_ = cbn_ < cb1;                                                                        \
            if (more_) { MVLDM_BL_ISSUE_R(slot_c ^ 1, cbn_, MVLDM_BL_NEXT(t_, 1), 0, Q0_); }                      \
            {                                                                                                     \
                BlFrags<T, TM, TN> fs_;                                                                           \
                MVLDM_BL_LOAD(fs_, slot_c, 0);                                                                    \
                bl_mma<T, TM, TN>(fs_, acc);                                                                      \
            }                                                                                                     \
            if (more_) { MVLDM_BL_ISSUE_R(slot_c ^ 1, cbn_, MVLDM_BL_NEXT(t_, 1), Q0_, Q1_); }                    \
            {                                                                                                     \
                BlFrags<T, TM, TN> fs_;                                                                           \
                MVLDM_BL_LOAD(fs_, slot_c, 1);                                                                    \
                bl_mma<T, TM, TN>(fs_, acc);                                                                      \
            }                                                                                                     \
            if (more_) { MVLDM_BL_ISSUE_R(slot_c ^ 1, cbn_, MVLDM_BL_NEXT(t_, 1), Q1_, LPT); }                    \
            {                                                                                                     \
                BlFrags<T, TM, TN> fs_;                                                                           \
                MVLDM_BL_LOAD(fs_, slot_c, 2);                                                                    \
                bl_mma<T, TM, TN>(fs_, acc);                                                                      \
                MVLDM_BL_LOAD(fs_, slot_c, 3);                                                                    \
                bl_mma<T, TM, TN>(fs_, acc);                                                                      \
            }                                                                                                     \
        }                                                                                                         \
        slot_c ^= 1;                                                                                              \
    }
    // Deep ring (STAGES >= 4, the small-launch tiles 16 - 18): tiles t+1 .. t+STAGES-1 are in flight while tile t is consumed.  With a
    // few hundred output rows a K-tile is a handful of MFMAs, so a step of the 2-slot loop costs one exposed L2 / HBM round trip
    // (the 4x4-level convs of one scene: 18 steps x ~0.8 us for 30 MB of weights); here the round trip is shared by STAGES - 1 steps.
#define MVLDM_BL_STEP_DEEP(t_)                                                                                    \
    {                                                                                                             \
        bl_wait_young<LPT, STAGES - 2>((cb1 - cb) * TAPS - (t_) - 1);      /* tile t has landed (younger ones stay in flight) */ \
        __builtin_amdgcn_s_barrier();                                      /* ... for every wave, and tile t-1's slot is free */ \
        {                                                                                                         \
            const int cbn_ = cb + ((t_) + STAGES - 1) / TAPS;                                                     \
            if (cbn_ < cb1) { MVLDM_BL_ISSUE(slot_c == 0 ? STAGES - 1 : slot_c - 1, cbn_, MVLDM_BL_NEXT(t_, STAGES - 1)); } \
        }                                                                                                         \
        bl_compute<T, BM, BN, WM, WN>(smem + slot_c * STAGE_BYTES, acc, wm, wn, hi, l31);                         \
        slot_c = slot_c + 1 == STAGES ? 0 : slot_c + 1;                                                           \
    }
#define MVLDM_BL_PRO(j_)                                                                                          \
    if constexpr (STAGES - 1 > (j_)) {                                                                            \
        if (cb0 + (j_) / TAPS < cb1) { MVLDM_BL_ISSUE((j_), cb0 + (j_) / TAPS, ((j_) % TAPS)); }                  \
    }
    // (the pipelined form needs 2 x (TM + TN) fragments next to the accumulators: not with 10 accumulator blocks)
    // (round 5 re-tried it for tile 10 with the per-tap offsets kept out of registers: the 1x1 form fits -- and measures +-0 on every Linear --,
    //  the 3x3 form still spills 52 B per lane into the loop: 870 -> 993 us)
    constexpr bool PIPE = NW == 8 && TM * TN <= 8 && STAGES <= 3;
    if constexpr (STAGES > 3) {
        static_assert((STAGES - 2) * LPT <= 63, "vmcnt is a 6-bit counter");
        if (cb0 < cb1) {
            MVLDM_BL_ISSUE(0, cb0, 0);
            MVLDM_BL_PRO(1) MVLDM_BL_PRO(2) MVLDM_BL_PRO(3) MVLDM_BL_PRO(4) MVLDM_BL_PRO(5) MVLDM_BL_PRO(6)
            int slot_c = 0;
            for (int cb = cb0; cb < cb1; ++cb) {
                MVLDM_BL_STEP_DEEP(0)
                if constexpr (TAPS == 4) { MVLDM_BL_STEP_DEEP(1) MVLDM_BL_STEP_DEEP(2) MVLDM_BL_STEP_DEEP(3) }
                if constexpr (TAPS == 9) {
                    MVLDM_BL_STEP_DEEP(1) MVLDM_BL_STEP_DEEP(2) MVLDM_BL_STEP_DEEP(3) MVLDM_BL_STEP_DEEP(4)
                    MVLDM_BL_STEP_DEEP(5) MVLDM_BL_STEP_DEEP(6) MVLDM_BL_STEP_DEEP(7) MVLDM_BL_STEP_DEEP(8)
                }
            }
        }
    } else if constexpr (!PIPE) {
        static_assert(STAGES == 2, "the plain loop uses the 2-slot ring");
        if (cb0 < cb1) {
            MVLDM_BL_ISSUE(0, cb0, 0);
            int slot_c = 0;
            for (int cb = cb0; cb < cb1; ++cb) {
                MVLDM_BL_STEP_SIMPLE(0)
                if constexpr (TAPS == 4) { MVLDM_BL_STEP_SIMPLE(1) MVLDM_BL_STEP_SIMPLE(2) MVLDM_BL_STEP_SIMPLE(3) }
                if constexpr (TAPS == 9) {
                    MVLDM_BL_STEP_SIMPLE(1) MVLDM_BL_STEP_SIMPLE(2) MVLDM_BL_STEP_SIMPLE(3) MVLDM_BL_STEP_SIMPLE(4)
                    MVLDM_BL_STEP_SIMPLE(5) MVLDM_BL_STEP_SIMPLE(6) MVLDM_BL_STEP_SIMPLE(7) MVLDM_BL_STEP_SIMPLE(8)
                }
            }
        }
    } else if (cb0 < cb1) {
        // prologue: fill the whole ring (up to STAGES tiles in flight), wait for the first
        MVLDM_BL_ISSUE(0, cb0, 0);
        const bool has1 = cb0 + 1 / TAPS < cb1, has2 = STAGES == 3 && cb0 + 2 / TAPS < cb1;
        if (has1) { MVLDM_BL_ISSUE(1, cb0 + 1 / TAPS, (1 % TAPS)); }
        if constexpr (STAGES == 3) {
            if (has2) { MVLDM_BL_ISSUE(2, cb0 + 2 / TAPS, (2 % TAPS)); }
        }
        if (has2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
        else if (has1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        int slot_c = 0;
        BlFrags<T, TM, TN> f0, f1;
        MVLDM_BL_LOAD(f0, 0, 0);
        for (int cb = cb0; cb < cb1; ++cb) {
            MVLDM_BL_STEP(0)
            if constexpr (TAPS == 4) { MVLDM_BL_STEP(1) MVLDM_BL_STEP(2) MVLDM_BL_STEP(3) }
            if constexpr (TAPS == 9) {
                MVLDM_BL_STEP(1) MVLDM_BL_STEP(2) MVLDM_BL_STEP(3) MVLDM_BL_STEP(4)
                MVLDM_BL_STEP(5) MVLDM_BL_STEP(6) MVLDM_BL_STEP(7) MVLDM_BL_STEP(8)
            }
        }
    }
#undef MVLDM_BL_STEP_SIMPLE
#undef MVLDM_BL_STEP_DEEP
#undef MVLDM_BL_PRO
#undef MVLDM_BL_LOAD
#undef MVLDM_BL_MMA
#undef MVLDM_BL_NEXT
#undef MVLDM_BL_STEP
#undef MVLDM_BL_ISSUE
#undef MVLDM_BL_ISSUE_R
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (TM * TN > 4) {
        // (the per-element fallback does not unroll at 8 accumulator blocks and would push them to scratch:
        //  the host only picks such a tile when the staged epilogue applies)
        igemm_epilogue_staged<T, BM, BN, WM, WN>(p, acc, tm, tn, split, wm, wn, wave, lane, smem);
    } else {
        if (p.stage_epi) igemm_epilogue_staged<T, BM, BN, WM, WN>(p, acc, tm, tn, split, wm, wn, wave, lane, smem);
        else igemm_epilogue<T, BM, BN, WM, WN>(p, acc, tm, tn, split, wm, wn, hi, l31);
    }
}

template <typename T, int BM, int BN, int WM, int WN> static int launch_sync(const IgemmParams& p, hipStream_t s) {
    static std::atomic<uint64_t> done{0};
    constexpr int ring = 2 * (BM + BN) * Mma<T>::PITCH, park = WM * WN * 32 * (park_blocks(BN / WN / 32) * 32 + 4) * 4;
    return launch_kernel(igemm_kernel<T, BM, BN, WM, WN>, done, (sizeof(T) == 2 && park > ring) ? park : ring,
                         8 * p.sub_m * p.sub_n * p.splitk, WM * WN * 64, p, s);
}

template <typename T, int BM, int BN, int WM, int WN, int KS, bool DUAL, int STAGES, bool UPS>
static int launch_bl_s(const IgemmParams& p, hipStream_t s) {
    static std::atomic<uint64_t> done{0};
    // the epilogue parks one 32-row fp32 block per wave in the (then idle) ring
    constexpr int ring = STAGES * (BM + BN) * 128, park = WM * WN * 32 * (park_blocks(BN / WN / 32) * 32 + 4) * 4;
    return launch_kernel(igemm_bl_kernel<T, BM, BN, WM, WN, KS, DUAL, STAGES, UPS>, done, ring > park ? ring : park,
                         8 * p.sub_m * p.sub_n * p.splitk, WM * WN * 64, p, s);
}
template <typename T, int BM, int BN, int WM, int WN, int KS, bool DUAL, int DEPTH = 0>
static int launch_bl(const IgemmParams& p, hipStream_t s) {
    // ring depth is fixed per tile (sweeps in profiles/r01_igemm_sweep*.json): the 4-wave tiles run 2-3
    // workgroups per CU and lose more to a third slot than they gain; the 8-wave 256x128 / 128x256 tiles own
    // the CU and take 3 slots; 256x256 only has room for 2.  DEPTH > 0: the deep-ring tiles (16 - 18) name theirs.
    constexpr int STAGES = DEPTH ? DEPTH : ((WM * WN == 8 && 3 * (BM + BN) * 128 <= 160 * 1024) ? 3 : 2);
    if (p.upsample) {
        // per-tap address tables: only built for the two tiles the host maps upsampling convs to
        if constexpr (KS == 3 && !DUAL && ((BM == 128 && BN == 64) || (BM == 256 && BN == 128)))
            return launch_bl_s<T, BM, BN, WM, WN, KS, DUAL, STAGES, true>(p, s);
        else
            return set_error(MVLDM_ERR_ARG, "igemm: upsampling 3x3 conv needs tile 2 or 7 on the 16-bit path");
    }
    return launch_bl_s<T, BM, BN, WM, WN, KS, DUAL, STAGES, false>(p, s);
}
// the deep-ring tiles: 1x1 / 3x3, one or two sources, no upsampling forms (fill_params maps those to tile 2)
template <typename T, int BM, int BN, int WM, int WN, int DEPTH> static int launch_bl_deep(const IgemmParams& p, hipStream_t s) {
    const bool dual = p.c1 > 0;
    if (p.ksize == 3) return dual ? launch_bl<T, BM, BN, WM, WN, 3, true, DEPTH>(p, s) : launch_bl<T, BM, BN, WM, WN, 3, false, DEPTH>(p, s);
    if (p.ksize == 1) return dual ? launch_bl<T, BM, BN, WM, WN, 1, true, DEPTH>(p, s) : launch_bl<T, BM, BN, WM, WN, 1, false, DEPTH>(p, s);
    return set_error(MVLDM_ERR_ARG, "igemm: the deep-ring tiles take 1x1 and 3x3 convs");
}

template <typename T, int BM, int BN, int WM, int WN> static int launch_bl_any(const IgemmParams& p, hipStream_t s) {
    const bool dual = p.c1 > 0;
    if (p.ksize == 2) {   // the four 2x2 phases of a decomposed nearest-2x upsampling conv: tiles 2, 7 and 10 only
        if constexpr ((BM == 128 && BN == 64) || (BM == 256 && BN == 128) || (BM == 256 && BN == 320))
            return launch_bl<T, BM, BN, WM, WN, 2, false>(p, s);
        else
            return set_error(MVLDM_ERR_ARG, "igemm: 2x2 phase conv needs tile 2, 7 or 10");
    }
    if (p.ksize == 3) {
        if (!dual) return launch_bl<T, BM, BN, WM, WN, 3, false>(p, s);
        // two-source 3x3 convs: the 256x256 / 256x320 tiles do not fit the register file with a second set of per-piece offsets
        // (hipcc: 31-33 spilled registers, 128-136 B of scratch per lane) and are not instantiated; the rules never pick them
        // (choose_config) and an explicit request is refused.  (The UNet has no such conv: GroupNorm materialises the skip
        // concat before conv1; only the 1x1 shortcuts read two sources.)
        if constexpr (BM == 256 && BN >= 256)
            return set_error(MVLDM_ERR_UNSUPPORTED, "igemm: tiles 9 / 10 do not take a two-source 3x3 conv (use tile 7 or 11)");
        else
            return launch_bl<T, BM, BN, WM, WN, 3, true>(p, s);
    }
    return dual ? launch_bl<T, BM, BN, WM, WN, 1, true>(p, s) : launch_bl<T, BM, BN, WM, WN, 1, false>(p, s);
}

template <typename T, int BM, int BN, int WM, int WN> static int launch_tile(const IgemmParams& p, hipStream_t s) {
    if constexpr (sizeof(T) == 2) {
        if (p.use_bl) return launch_bl_any<T, BM, BN, WM, WN>(p, s);
    }
    // f32, and the few 16-bit problems whose channel counts are not multiples of 64 (conv_in, VAE conv_in/out,
    // quant convs): register-prefetch loop
    return launch_sync<T, BM, BN, WM, WN>(p, s);
}

}  // namespace mvldm
