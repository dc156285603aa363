// Implicit GEMM, tiles 11 and 17: 3x3 stride-1 convolutions with an LDS-resident pixel halo (16-bit types only).
#include "igemm_common.h"

namespace mvldm {

// (buffer descriptors live in free functions, never in a kernel body: see the note at igemm_bl_kernel in igemm_bl.h)
template <bool DUAL>
__device__ __forceinline__ void halo_issue_a(const IgemmParams& p, char* dst, unsigned v0, unsigned v1, int cb) {
    const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.src0), 0, p.src0_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(DUAL ? p.src1 : p.src0), 0,
                                                                         DUAL ? p.src1_bytes : p.src0_bytes, 0x00020000);
    const int c = cb * 64;
    const bool from0 = !DUAL || c < p.c0;
    const int soff = (from0 ? c : c - p.c0) * 2;
    if (from0) __builtin_amdgcn_raw_ptr_buffer_load_lds(r0, (__attribute__((address_space(3))) void*)dst, 16, v0, soff, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(r1, (__attribute__((address_space(3))) void*)dst, 16, v1, soff, 0, 0);
}
__device__ __forceinline__ void halo_issue_w(const IgemmParams& p, char* dst, unsigned v, int koff) {
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.weight), 0, p.w_bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)dst, 16, v, koff, 0, 0);
}

// The two kernels below write their set-up (LDS carve-out, halo-piece offsets, weight-row offsets, per-row tap mask, accumulator clear)
// and their issue macros out in full, twice.  Each of these was tried as one shared __forceinline__ helper -- weight_row_offsets,
// tap_mask_3x3, halo_piece_offsets, an issue pair on B_IT / DUAL over a carve-out struct, zero_acc -- and every one of them, alone,
// changed the code of all six kernels (tools/kernel_hashes.py), so by the rule of igemm_common.h none is hoisted; only the wave / lane
// preamble (wave_lane) leaves the code as it was.  A change to one kernel's set-up goes to the other.

// ---- 3x3 stride-1 convolution with an LDS-resident pixel halo ------------------------------------------------
// The 9 taps of a 3x3 conv read the same 64-channel slice of the same pixels, shifted by dy*W + dx rows of the
// NHWC pixel array.  Instead of fetching a shifted 256-row A tile per tap (9 x 32 KB per channel block through the
// L2 -> LDS path, which bounds the loop above), this kernel fetches ONE contiguous range of
// 256 + 2*(W+1) pixel rows per channel block (the tile's pixels plus W+1 rows of halo on either side) and serves all
// 9 taps from it: tap (dy,dx) of tile row r is halo row r + (W+1) + dy*W + dx -- a lane-uniform displacement.
// Image borders are per-lane 9-bit masks; a masked lane reads a 128-byte row of zeros.  Only the W tiles (16 KB per
// tap) still stream per K-tile, through a 3-slot ring; the halo of the next channel block arrives piecewise under
// the 9 taps of the current one (2 slots).  L2 -> LDS bytes per channel block: 41 + 9*16 = 185 KB instead of 432 KB.
template <typename T, bool DUAL>
__global__ __launch_bounds__(512) void igemm_halo_kernel(const IgemmParams p, int halo_rows) {
    using M_ = Mma<T>;
    constexpr int BM = 256, BN = 128, WM = 4, WN = 2, NW = 8, TM = 2, TN = 2, B_IT = 2, KA = 6, EPC = 8;
    constexpr int W_BYTES = BN * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int a_bytes = halo_rows * 128;
    char* const wring = smem + 2 * a_bytes;
    char* const zrow = wring + 3 * W_BYTES;
    char* const dummy = zrow + 128;

    const auto [lane, wave, wm, wn, hi, l31] = wave_lane<WN>();
    int split, tm, tn;
    if (!map_block(p, split, tm, tn)) return;
    const int cb1 = p.k_tiles / 9;
    const int lead = p.w_in + 1;
    const int m0 = tm * BM;
    const int np = halo_rows / 8;                       // 1 KiB pieces of a halo tile
    const int slot = lane & 7, rsub = lane >> 3;
    const int m_tot = p.n_img * p.h_in * p.w_in;

    if (threadIdx.x < 8) *reinterpret_cast<u32x4*>(zrow + threadIdx.x * 16) = u32x4{0u, 0u, 0u, 0u};

    // halo pieces of this wave: q = wave + 8k
    unsigned off0[KA], off1[DUAL ? KA : 1];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
        const int q = wave + NW * k;
        const int hr = q * 8 + rsub;
        const int pm = m0 - lead + hr;
        const bool ok = q < np && pm >= 0 && pm < m_tot;
        const unsigned chunk = (unsigned)((slot ^ ((hr >> 1) & 7)) * EPC);
        off0[k] = ok ? ((unsigned)pm * (unsigned)p.c0 + chunk) * 2u : kBufOob;
        if constexpr (DUAL) off1[k] = ok ? ((unsigned)pm * (unsigned)p.c1 + chunk) * 2u : kBufOob;
    }
    unsigned vb[B_IT];
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int row = (wave + NW * it) * 8 + rsub;
        const int n = tn * BN + row;
        const unsigned chunk = (unsigned)((slot ^ ((row >> 1) & 7)) * EPC);
        vb[it] = n < p.n_pad ? ((unsigned)n * (unsigned)p.k_pad + chunk) * 2u : kBufOob;
    }
    // per-row tap validity
    unsigned mask[TM];
    int rloc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        rloc[i] = wm * (BM / WM) + i * 32 + l31;
        const int m = m0 + rloc[i];
        unsigned msk = 0;
        if (m < p.M) {
            const int rem = m % p.hw_out;
            const int y = rem / p.w_out, x = rem - y * p.w_out;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
                msk |= ((unsigned)iy < (unsigned)p.h_in && (unsigned)ix < (unsigned)p.w_in) ? (1u << t) : 0u;
            }
        }
        mask[i] = msk;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // one halo piece (index k of this wave) of channel block cb into halo slot cb & 1; out-of-range: zeros into `dummy`
#define MVLDM_HALO_A(k_, cb_)                                                                                          \
    {                                                                                                                  \
        const int q_ = wave + NW * (k_);                                                                               \
        const bool real_ = (cb_) < cb1 && q_ < np;                                                                     \
        halo_issue_a<DUAL>(p, real_ ? smem + ((cb_) & 1) * a_bytes + q_ * 1024 : dummy, real_ ? off0[k_] : kBufOob,     \
                           real_ ? off1[DUAL ? (k_) : 0] : kBufOob, (cb_) < cb1 ? (cb_) : 0);                           \
    }
    // W tile of K-tile index kt_ (= cb*9 + tap) into ring slot ws_; past the end of K: zeros
#define MVLDM_HALO_W(kt_, ws_)                                                                                         \
    {                                                                                                                  \
        const bool real_ = (kt_) < cb1 * 9;                                                                            \
        _Pragma("unroll") for (int it = 0; it < B_IT; ++it)                                                            \
            halo_issue_w(p, wring + (ws_) * W_BYTES + (wave + NW * it) * 1024, real_ ? vb[it] : kBufOob, real_ ? (kt_) * 128 : 0); \
    }

    // prologue: the whole halo of block 0, W tiles 0..2
#pragma unroll
    for (int k = 0; k < KA; ++k) MVLDM_HALO_A(k, 0)
    MVLDM_HALO_W(0, 0)
    MVLDM_HALO_W(1, 1)
    MVLDM_HALO_W(2, 2)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // fragment addressing of one tap: masked lanes read the zero row
    const char* abase[TM];
    int arow[TM];
    const char* bt;
#define MVLDM_HALO_ADDR(cb_, t_, ws_)                                                                                  \
    {                                                                                                                  \
        const int disp_ = lead + ((t_) / 3 - 1) * p.w_in + ((t_) % 3 - 1);   /* lane-uniform row displacement */        \
        const char* as_ = smem + ((cb_) & 1) * a_bytes;                                                                \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                               \
            const bool ok_ = (mask[i] >> (t_)) & 1u;                                                                   \
            abase[i] = ok_ ? as_ : zrow;                                                                               \
            arow[i] = ok_ ? rloc[i] + disp_ : 0;                                                                       \
        }                                                                                                              \
        bt = wring + (ws_) * W_BYTES;                                                                                  \
    }
#define MVLDM_HALO_LOAD(f_, kk_)                                                                                       \
    {                                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) f_.a[i] = M_::load(abase[i], arow[i], kk_, hi);                 \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) f_.b[j] = M_::load(bt, wn * (BN / WN) + j * 32 + l31, kk_, hi); \
    }
#define MVLDM_HALO_MMA(f_)                \
    __builtin_amdgcn_sched_barrier(0);    \
    bl_mma<T, TM, TN>(f_, acc);           \
    __builtin_amdgcn_sched_barrier(0);

    int wslot = 0, kt = 0;
    BlFrags<T, TM, TN> f0, f1;
    MVLDM_HALO_ADDR(0, 0, 0)
    MVLDM_HALO_LOAD(f0, 0)
    for (int cb = 0; cb < cb1; ++cb) {
#pragma unroll
        for (int t = 0; t < 9; ++t, ++kt) {
            MVLDM_HALO_LOAD(f1, 1)
            MVLDM_HALO_MMA(f0)
            MVLDM_HALO_LOAD(f0, 2)
            MVLDM_HALO_MMA(f1)
            MVLDM_HALO_LOAD(f1, 3)
            MVLDM_HALO_MMA(f0)
            // W tile kt+1 must have landed; behind it at most {halo piece, W tile kt+2, halo piece} = 4 loads are in flight
            asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            MVLDM_HALO_W(kt + 3, wslot)
            if (t < KA) { MVLDM_HALO_A(t, cb + 1) }
            else { MVLDM_HALO_A(0, cb1) }                                     // (keeps the per-step load count uniform)
            wslot = wslot == 2 ? 0 : wslot + 1;
            // first fragments of the next K-tile under the last MFMAs of this one (past the end: harmless reads)
            if (t < 8) { MVLDM_HALO_ADDR(cb, t + 1, wslot) }
            else { MVLDM_HALO_ADDR(cb + 1, 0, wslot) }
            MVLDM_HALO_LOAD(f0, 0)
            MVLDM_HALO_MMA(f1)
        }
    }
#undef MVLDM_HALO_ADDR
#undef MVLDM_HALO_LOAD
#undef MVLDM_HALO_MMA
#undef MVLDM_HALO_A
#undef MVLDM_HALO_W
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    igemm_epilogue_staged<T, BM, BN, WM, WN>(p, acc, tm, tn, split, wm, wn, wave, lane, smem);
}

// ---- tile 17 (round 5): the pixel halo under a 256 x 320 tile, for maps up to 24 pixels wide ------------------------------------
// Tile 10 (256 x 320, the headline's 3x3 convs) idles its matrix pipes 31 % of the time with both waves of a SIMD parked on the next
// K-tile's round trip: 72 KB per CU per step through the 2-slot ring.  With the halo resident (one fill of 256 + 2 (W + 1) pixel
// rows per channel block serves the 9 taps) a step moves 40 KB of weights + 1/9 of the 37 KB halo = 44 KB.  LDS: two halo buffers +
// a 2-slot weight ring = 2 x 37 + 2 x 40 KB at W = 16 (156 KB); a 32-wide map needs 164 KB -- level 0 stays on tile 10.
// 8 waves of 64 x 160 like tile 10 (10 accumulator blocks: fragments are fetched right before use, the two waves of a SIMD cover each
// other's LDS latency); per step a wave issues 5 weight pieces + 1 halo piece behind the barrier, and the counted wait in front of
// the next barrier (vmcnt(1): only the halo piece may still be in flight) is for the weights issued one step earlier.
template <typename T>
__global__ __launch_bounds__(512) void igemm_halow_kernel(const IgemmParams p, int halo_rows) {
    using M_ = Mma<T>;
    constexpr int BM = 256, BN = 320, WM = 4, WN = 2, NW = 8, TM = 2, TN = 5, B_IT = 5, KA = 6, EPC = 8;
    constexpr int W_BYTES = BN * 128;
    static_assert(64 / M_::KI == 4, "four k-sub-steps per K-tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int a_bytes = halo_rows * 128;
    char* const wring = smem + 2 * a_bytes;
    char* const zrow = wring + 2 * W_BYTES;
    char* const dummy = zrow + 128;

    const auto [lane, wave, wm, wn, hi, l31] = wave_lane<WN>();
    int split, tm, tn;
    if (!map_block(p, split, tm, tn)) return;
    const int cb1 = p.k_tiles / 9;
    const int lead = p.w_in + 1;
    const int m0 = tm * BM;
    const int np = halo_rows / 8;                       // 1 KiB pieces of a halo tile
    const int slot = lane & 7, rsub = lane >> 3;
    const int m_tot = p.n_img * p.h_in * p.w_in;

    if (threadIdx.x < 8) *reinterpret_cast<u32x4*>(zrow + threadIdx.x * 16) = u32x4{0u, 0u, 0u, 0u};

    unsigned off0[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
        const int q = wave + NW * k;
        const int hr = q * 8 + rsub;
        const int pm = m0 - lead + hr;
        const bool ok = q < np && pm >= 0 && pm < m_tot;
        const unsigned chunk = (unsigned)((slot ^ ((hr >> 1) & 7)) * EPC);
        off0[k] = ok ? ((unsigned)pm * (unsigned)p.c0 + chunk) * 2u : kBufOob;
    }
    unsigned vb[B_IT];
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int row = (wave + NW * it) * 8 + rsub;
        const int n = tn * BN + row;
        const unsigned chunk = (unsigned)((slot ^ ((row >> 1) & 7)) * EPC);
        vb[it] = n < p.n_pad ? ((unsigned)n * (unsigned)p.k_pad + chunk) * 2u : kBufOob;
    }
    unsigned mask[TM];
    int rloc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        rloc[i] = wm * (BM / WM) + i * 32 + l31;
        const int m = m0 + rloc[i];
        unsigned msk = 0;
        if (m < p.M) {
            const int rem = m % p.hw_out;
            const int y = rem / p.w_out, x = rem - y * p.w_out;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
                msk |= ((unsigned)iy < (unsigned)p.h_in && (unsigned)ix < (unsigned)p.w_in) ? (1u << t) : 0u;
            }
        }
        mask[i] = msk;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#define MVLDM_HW_A(k_, cb_)                                                                                            \
    {                                                                                                                  \
        const int q_ = wave + NW * (k_);                                                                               \
        const bool real_ = (cb_) < cb1 && q_ < np;                                                                     \
        halo_issue_a<false>(p, real_ ? smem + ((cb_) & 1) * a_bytes + q_ * 1024 : dummy, real_ ? off0[k_] : kBufOob, kBufOob,  \
                            (cb_) < cb1 ? (cb_) : 0);                                                                  \
    }
#define MVLDM_HW_W(kt_, ws_)                                                                                           \
    {                                                                                                                  \
        const bool real_ = (kt_) < cb1 * 9;                                                                            \
        _Pragma("unroll") for (int it = 0; it < B_IT; ++it)                                                            \
            halo_issue_w(p, wring + (ws_) * W_BYTES + (wave + NW * it) * 1024, real_ ? vb[it] : kBufOob, real_ ? (kt_) * 128 : 0); \
    }

    // prologue: the whole halo of block 0, W tiles 0 and 1
#pragma unroll
    for (int k = 0; k < KA; ++k) MVLDM_HW_A(k, 0)
    MVLDM_HW_W(0, 0)
    MVLDM_HW_W(1, 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int kt = 0;
    for (int cb = 0; cb < cb1; ++cb) {
        const char* as = smem + (cb & 1) * a_bytes;
        // (the per-tap row offsets are loop-invariant: hipcc hoists all 9 x TM of them and spills 46 registers to scratch, whose reloads
        //  count in vmcnt like the DMA pieces.  Opaque per-iteration values keep the two selects per tap inside the loop.)
        asm volatile("" : "+v"(mask[0]), "+v"(mask[1]), "+v"(rloc[0]), "+v"(rloc[1]));
#pragma unroll
        for (int t = 0; t < 9; ++t, ++kt) {
            const int ws = kt & 1;
            const int disp = lead + (t / 3 - 1) * p.w_in + (t % 3 - 1);      // lane-uniform row displacement of the tap
            const char* abase[TM];
            int arow[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const bool ok = (mask[i] >> t) & 1u;
                abase[i] = ok ? as : zrow;
                arow[i] = ok ? rloc[i] + disp : 0;
            }
            const char* bt = wring + ws * W_BYTES;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                BlFrags<T, TM, TN> f;
#pragma unroll
                for (int i = 0; i < TM; ++i) f.a[i] = M_::load(abase[i], arow[i], kk, hi);
#pragma unroll
                for (int j = 0; j < TN; ++j) f.b[j] = M_::load(bt, wn * (BN / WN) + j * 32 + l31, kk, hi);
                bl_mma<T, TM, TN>(f, acc);
            }
            // W tile kt+1 has landed (behind it only the halo piece issued with it may still be in flight); every wave is done with
            // W slot `ws` -- and, after tap 8, with this block's halo buffer
            asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            MVLDM_HW_W(kt + 2, ws)
            if (t < KA) { MVLDM_HW_A(t, cb + 1) }
            else { MVLDM_HW_A(0, cb1) }                                       // (keeps the per-step load count uniform)
        }
    }
#undef MVLDM_HW_A
#undef MVLDM_HW_W
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    igemm_epilogue_staged<T, BM, BN, WM, WN>(p, acc, tm, tn, split, wm, wn, wave, lane, smem);
}

template <typename T> static int launch_halo(const IgemmParams& p, hipStream_t s) {
    const int hr = halo_rows_for(p.w_in), smem = halo_smem(p.w_in);
    const int blocks = 8 * p.sub_m * p.sub_n;
    static std::atomic<uint64_t> done0{0}, done1{0};
    if (p.c1 > 0) {
        if (int rc0 = ensure_dyn_smem(reinterpret_cast<const void*>(igemm_halo_kernel<T, true>), 160 * 1024, done1)) return rc0;
        hipLaunchKernelGGL((igemm_halo_kernel<T, true>), dim3(blocks), dim3(512), smem, s, p, hr);
    } else {
        if (int rc0 = ensure_dyn_smem(reinterpret_cast<const void*>(igemm_halo_kernel<T, false>), 160 * 1024, done0)) return rc0;
        hipLaunchKernelGGL((igemm_halo_kernel<T, false>), dim3(blocks), dim3(512), smem, s, p, hr);
    }
    return check_launch();
}

template <typename T> static int launch_halow(const IgemmParams& p, hipStream_t s) {
    static std::atomic<uint64_t> done{0};
    if (int rc0 = ensure_dyn_smem(reinterpret_cast<const void*>(igemm_halow_kernel<T>), 160 * 1024, done)) return rc0;
    hipLaunchKernelGGL((igemm_halow_kernel<T>), dim3(8 * p.sub_m * p.sub_n), dim3(512), halow_smem(p.w_in), s, p, halo_rows_for(p.w_in));
    return check_launch();
}

int igemm_launch_halo(const IgemmParams& p, int tile, int act_dtype, hipStream_t s) {
    if (int rc = require_bl(p, tile, act_dtype)) return rc;
    return dispatch_16bit(act_dtype, [&](auto t) {
        using T = decltype(t);
        return tile == 11 ? launch_halo<T>(p, s) : launch_halow<T>(p, s);
    });
}

}  // namespace mvldm
