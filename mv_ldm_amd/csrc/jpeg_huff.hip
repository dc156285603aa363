// The Huffman-coded scan of a JPEG frame decoded on the device (include/mvldm.h, "JPEG frames: the scan on the device" and "JPEG frames:
// restart intervals on the device"): a self-synchronising decoder (Klein and Wiseman; Weissenberger and Schmidt) in the form whose
// correctness does not depend on synchronisation ever happening, as a plain form (one stream per frame) and a restart form (the stream cut
// at its restart intervals).  The step function, the bit window, a lane's description of its subsequence and the coefficient sink are
// jpeg_huff_common.h's, shared with the two host emulations.  What the two forms share on the device is written once below: the table load,
// the workgroup scan, the cold pass with its rounds, the write pass, the end of the DC kernels and the launch.  What differs is how a
// chunk's lanes get their streams (the batch walk and the interval table checks) and the segmented scan of the DC differences.
//   jpeg_huff_kernel      one workgroup of 1024 per frame, one subsequence of `sb` bits per thread, the frame's chunks of 1024
//                         subsequences in order.  LDS: the six Huffman tables (8544 B), the exit states twice (16 KiB: a round reads one
//                         copy and writes the other, so one barrier a round), the zigzag table, wave totals.  Per chunk: the cold pass;
//                         rounds until no entry changed (__syncthreads_or) or n_act rounds ran; an exclusive scan of the completed-block
//                         counts; the write pass.  A lane's loop runs at most sb symbols (a symbol is at least one bit), a chunk at most
//                         n_act rounds, a frame ceil(bits / sb / 1024) chunks: every bound comes from sizes.  No kernel waits for
//                         another workgroup.  The coefficient slots are zeroed by a memset node in front of this kernel on the same
//                         stream: stream order puts every store of the write pass after it.
//   jpeg_rst_scan_kernel  the same for a frame WITH restart intervals (a frame without DRI is one interval).  An interval starts
//                         byte-aligned at block 0 of an MCU with the predictors at 0, so its first subsequence has a true entry without a
//                         round, and no subsequence crosses an interval.  The kernel checks the descriptor and every pair of the interval
//                         table before it reads a scan bit, then walks the intervals in batches: the longest run of whole intervals whose
//                         subsequence counts sum to at most 1024, found by a workgroup scan of the counts (kept in LDS; a lane finds its
//                         interval by binary search).  An interval of more than 1024 subsequences is walked alone, in chunks with the
//                         carry, as jpeg_huff_kernel walks a frame.  Per chunk as above, except that a lane that opens an interval never
//                         takes its neighbour's exit, a lane subtracts from the scan of the completed blocks its value at the interval's
//                         first lane, and every store of the write pass is guarded by block < end of the interval.
//   jpeg_huff_dc_kernel   one workgroup per frame: per component the DC differences in scan order (luma MCU-major) become predictions
//                         through a 64-bit workgroup scan with a carry, and every block's S = sum |coef q| is formed from eight 16-byte
//                         loads; the largest S and the reason go to status.
//   jpeg_rst_dc_kernel    the same with a SEGMENTED scan: a block that opens an interval starts from 0.
// Divergent by nature and bound by each lane's serial chain (window -> table lookup in LDS -> next bit position), not by bandwidth.
#include "common.h"
#include "jpeg_huff_common.h"

namespace mvldm {

namespace {

// inclusive scan of one value per lane over the workgroup: within the wave by shuffles, across the 16 waves through LDS (one barrier; the
// caller's next barrier frees wave_tot).  *all: the workgroup's sum.
__device__ __forceinline__ uint32_t huff_scan_u32(uint32_t v, uint32_t* wave_tot, unsigned tid, uint32_t* all) {
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, WAVE);
        if ((int)(tid & (WAVE - 1)) >= o) incl += up;
    }
    if ((tid & (WAVE - 1)) == WAVE - 1) wave_tot[tid / WAVE] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (unsigned u = 0; u < (unsigned)kHuffChunk / WAVE; ++u) {
        const uint32_t t = wave_tot[u];
        before += u < tid / WAVE ? t : 0u;
        sum += t;
    }
    *all = sum;
    return before + incl;
}

// The frame's tables into LDS and its quantiser rows into qt; the caller's next barrier publishes them.
__device__ __forceinline__ void huff_load_tables(const uint8_t* tables, uint16_t* qt, unsigned img, unsigned tid, uint8_t* tab, uint8_t* zigzag) {
    const u32x4* blob = (const u32x4*)(tables + (size_t)img * kHuffBlobBytes);
    for (unsigned i = tid; i < (unsigned)kHuffTabsBytes / 16; i += kHuffChunk) ((u32x4*)tab)[i] = blob[i];
    if (tid < 24) ((u32x4*)(qt + (size_t)img * 192))[tid] = blob[kHuffTabsBytes / 16 + tid];
    if (tid < 64) zigzag[tid] = huff_zigzag(tid);
}

// One chunk's cold pass and rounds for the lane whose subsequence of the stream (sc, bits) ends at `end`: it starts from `cold`, and
// unless `first` -- the lane takes no neighbour's exit: its cold entry is true -- it decodes again whenever its left neighbour's exit
// differs from the entry it used, until no lane of the chunk changed or n_act rounds ran.  *entry: the entry the rounds settled on,
// *done: the blocks the lane completes from it; the exits are in buf[*cur].  Returns the rounds.
__device__ __forceinline__ uint32_t huff_settle(const uint8_t* sc, uint32_t bits, uint32_t end, HuffState cold, bool first, bool active, uint32_t n_act,
                                                const uint8_t* tab, const HuffGeom& G, uint32_t sb, HuffState (*buf)[kHuffChunk], unsigned tid, HuffState* entry,
                                                uint32_t* done, int* cur) {
    HuffNoSink none;
    HuffState exit = {0u, 0u};
    *entry = exit;
    *done = 0;
    if (active) {                                           // cold pass
        *entry = exit = cold;
        huff_run(sc, bits, tab, G.nl, G.nb, end, sb, &exit, done, &none);
        buf[0][tid] = exit;
    }
    __syncthreads();
    int c = 0;
    uint32_t rounds = 0;
    for (uint32_t r = 0; r < n_act; ++r) {
        int changed = 0;
        if (active) {
            if (!first) {
                const HuffState e = buf[c][tid - 1];
                if (!huff_same(e, *entry)) {
                    *entry = exit = e;
                    huff_run(sc, bits, tab, G.nl, G.nb, end, sb, &exit, done, &none);
                    changed = 1;
                }
            }
            buf[c ^ 1][tid] = exit;
        }
        const int any = __syncthreads_or(changed);          // the round's barrier: readers of buf[c] are done, buf[c ^ 1] is complete
        c ^= 1;
        ++rounds;
        if (!any) break;
    }
    *cur = c;
    return rounds;
}

// The write pass of one lane, from the entry the rounds settled on: block n of the frame is the first it decodes into, `limit` the end
// of its stream's blocks.  *ended counts the streams whose last block was completed.
__device__ __forceinline__ void huff_write(const uint8_t* sc, uint32_t bits, uint32_t end, HuffState entry, uint32_t n, uint32_t limit, const uint8_t* tab,
                                           const HuffGeom& G, uint32_t sb, int16_t* cf, const uint8_t* zigzag, uint32_t* bad, uint32_t* ended) {
    HuffCoefSink sink{cf, zigzag, G, n, limit, bits, 0u, bad, nullptr};
    sink.open();
    uint32_t again = 0;
    huff_run(sc, bits, tab, G.nl, G.nb, end, sb, &entry, &again, &sink);
    if (sink.ended) atomicAdd(ended, 1u);
}

// Block j of component c in scan order (luma MCU-major): its 64 coefficients in the frame's slot
__device__ __forceinline__ int16_t* huff_dc_block(int16_t* cf, const HuffGeom& G, uint32_t c, uint32_t j) {
    const uint32_t m = c == 0 ? j / G.nl : j, b = c == 0 ? j - m * G.nl : G.nl + c - 1;
    return cf + (size_t)huff_block_index(G, m, b) * 64;
}

// The end of both DC kernels: the workgroup's largest S and the reason into the frame's status
__device__ __forceinline__ void huff_dc_finish(int bad, int32_t worst, int32_t* wave_max, int32_t* st, unsigned tid) {
    const unsigned lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int any_bad = __syncthreads_or(bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t other = __shfl_xor(worst, o, WAVE);
        worst = other > worst ? other : worst;
    }
    if (lane == 0) wave_max[wave] = worst;
    __syncthreads();
    if (tid == 0) {
        for (unsigned u = 0; u < (unsigned)kHuffChunk / WAVE; ++u) worst = wave_max[u] > worst ? wave_max[u] : worst;
        st[0] = any_bad ? MVLDM_JPEG_CORRUPT : worst > kJpegGuard ? MVLDM_JPEG_RANGE : MVLDM_JPEG_OK;
        st[1] = any_bad ? 0 : worst;
    }
}

}  // namespace

__global__ __launch_bounds__(kHuffChunk) void jpeg_huff_kernel(const uint8_t* __restrict__ scan, size_t scan_bytes, const int32_t* __restrict__ desc,
                                                                const uint8_t* __restrict__ tables, int16_t* __restrict__ coef, uint16_t* __restrict__ qt,
                                                                int32_t* __restrict__ status, HuffGeom G, uint32_t sb) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[kHuffTabsBytes];
    __shared__ HuffState buf[2][kHuffChunk];
    __shared__ uint32_t wave_tot[kHuffChunk / WAVE];
    __shared__ uint8_t zigzag[64];
    __shared__ uint32_t ended, bad;
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    huff_load_tables(tables, qt, img, tid, tab, zigzag);
    if (tid == 0) ended = 0u, bad = 0u;
    int32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = desc[(size_t)img * 4 + i];
    const bool ok = huff_desc_ok(d, scan_bytes);            // a descriptor that does not fit the buffer: no bit is read, the frame is refused
    const uint8_t* sc = scan + (ok ? (size_t)d[0] : 0);
    const uint32_t bit_len = ok ? (uint32_t)d[1] : 0u;
    const uint32_t nsub = huff_rst_count(bit_len, sb);
    int16_t* cf = coef + (size_t)img * G.total * 64;
    __syncthreads();

    HuffState carry = {0u, 0u};
    uint32_t base = 0, rounds_max = 0;
    for (uint32_t ch0 = 0; ch0 < nsub; ch0 += kHuffChunk) {
        const uint32_t n_act = nsub - ch0 < (uint32_t)kHuffChunk ? nsub - ch0 : (uint32_t)kHuffChunk;
        const bool active = tid < n_act;
        const uint64_t e64 = ((uint64_t)(ch0 + tid) + 1) * sb;
        const uint32_t end = e64 < bit_len ? (uint32_t)e64 : bit_len;
        HuffState entry;
        uint32_t done, chunk_blocks;
        int cur;
        const uint32_t rounds = huff_settle(sc, bit_len, end, tid == 0 ? carry : HuffState{(ch0 + tid) * sb, 0u}, tid == 0, active, n_act, tab, G, sb, buf, tid,
                                            &entry, &done, &cur);
        rounds_max = rounds > rounds_max ? rounds : rounds_max;
        const uint32_t incl = huff_scan_u32(done, wave_tot, tid, &chunk_blocks);       // the completed blocks up to and with this lane
        if (active) huff_write(sc, bit_len, end, entry, base + incl - done, G.total, tab, G, sb, cf, zigzag, &bad, &ended);
        carry = buf[cur][n_act - 1];
        base += chunk_blocks;
        __syncthreads();                                    // buf and wave_tot are free for the next chunk; ended and bad are visible
    }
    if (tid == 0) {
        status[(size_t)img * 4 + 0] = bad == 0u && ended == 1u ? MVLDM_JPEG_OK : MVLDM_JPEG_CORRUPT;
        status[(size_t)img * 4 + 1] = 0;
        status[(size_t)img * 4 + 2] = (int32_t)rounds_max;
        status[(size_t)img * 4 + 3] = 0;
    }
}

__global__ __launch_bounds__(kHuffChunk) void jpeg_rst_scan_kernel(const uint8_t* __restrict__ scan, size_t scan_bytes, const int32_t* __restrict__ desc,
                                                                    const uint8_t* __restrict__ tables, int16_t* __restrict__ coef, uint16_t* __restrict__ qt,
                                                                    int32_t* __restrict__ status, HuffGeom G, uint32_t sb) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[kHuffTabsBytes];
    __shared__ HuffState buf[2][kHuffChunk];
    __shared__ uint32_t pre[kHuffChunk];                    // a batch's inclusive subsequence counts; then a chunk's exclusive block counts
    __shared__ uint32_t wave_tot[kHuffChunk / WAVE];
    __shared__ uint8_t zigzag[64];
    __shared__ uint32_t ended, bad;
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    huff_load_tables(tables, qt, img, tid, tab, zigzag);
    if (tid == 0) ended = 0u, bad = 0u;
    int32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = desc[(size_t)img * 4 + i];
    const bool ok = huff_rst_desc_ok(d, scan_bytes, G.mcus);        // a descriptor that does not fit the buffer: nothing of the frame is read
    const uint8_t* region = scan + (ok ? (size_t)d[0] : 0);
    const int32_t* tbl = (const int32_t*)region;                   // 16-byte aligned: scan is, and so is d[0]
    const uint32_t n_all = ok ? (uint32_t)d[1] : 0u, ri = ok ? (uint32_t)d[3] : 1u;
    int wrong = 0;                                                  // the whole table against the descriptor before any scan bit is read
    for (uint32_t g = tid; g < n_all; g += kHuffChunk) wrong |= huff_rst_entry_ok(tbl[2 * g], tbl[2 * g + 1], d) ? 0 : 1;
    wrong = __syncthreads_or(wrong);                                // also: tab, zigzag, ended and bad are set
    const uint32_t n_int = wrong ? 0u : n_all;
    int16_t* cf = coef + (size_t)img * G.total * 64;

    uint32_t rounds_max = 0;
    for (uint32_t g0 = 0; g0 < n_int;) {
        // the batch: the longest run of whole intervals from g0 whose subsequences fit the workgroup
        uint32_t cnt = 0, all;
        if (g0 + tid < n_int) cnt = huff_rst_count_capped((uint32_t)tbl[2 * (g0 + tid) + 1], sb, (uint32_t)kHuffChunk);
        const uint32_t incl = huff_scan_u32(cnt, wave_tot, tid, &all);
        pre[tid] = incl;
        const uint32_t nbi = (uint32_t)__syncthreads_count(cnt != 0u && incl <= (uint32_t)kHuffChunk);      // the sums only grow: a prefix of the lanes
        const bool big = nbi == 0u;                         // interval g0 alone is more than a chunk
        uint32_t j = 0, n_act = 0, n_chunks = 1;
        HuffRstLane ln;
        ln.entry0 = HuffState{0u, 0u};
        if (big) {
            ln.start = 0u;
        } else {
            n_act = pre[nbi - 1];
            j = huff_rst_find(pre, nbi, tid < n_act ? tid : 0u);
            ln.start = j ? pre[j - 1] : 0u;
        }
        const uint32_t g = g0 + j;
        ln.sc = region + tbl[2 * g];
        ln.bits = (uint32_t)tbl[2 * g + 1];
        huff_rst_blocks(G, g, ri, &ln.base, &ln.limit);
        const uint32_t subs = huff_rst_count(ln.bits, sb);
        if (big) n_chunks = (subs + (uint32_t)kHuffChunk - 1) / (uint32_t)kHuffChunk;
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            if (big) {
                const uint32_t left = subs - ch * (uint32_t)kHuffChunk;
                n_act = left < (uint32_t)kHuffChunk ? left : (uint32_t)kHuffChunk;
            }
            const bool active = tid < n_act;
            ln.s = ch * (uint32_t)kHuffChunk + tid - ln.start;
            ln.first = tid == ln.start;
            const uint32_t end = huff_rst_end(ln, sb);
            HuffState entry;
            uint32_t done, chunk_blocks;
            int cur;                                        // the first barrier of huff_settle: every lane has read pre[] of the batch
            const uint32_t rounds = huff_settle(ln.sc, ln.bits, end, huff_rst_cold(ln, sb), ln.first, active, n_act, tab, G, sb, buf, tid, &entry, &done, &cur);
            rounds_max = rounds > rounds_max ? rounds : rounds_max;
            // the blocks completed in front of this lane INSIDE its interval: the workgroup's exclusive scan minus its value at the
            // interval's first lane
            const uint32_t excl = huff_scan_u32(done, wave_tot, tid, &chunk_blocks) - done;
            pre[tid] = excl;
            __syncthreads();
            if (active) huff_write(ln.sc, ln.bits, end, entry, ln.base + excl - pre[ln.start], ln.limit, tab, G, sb, cf, zigzag, &bad, &ended);
            ln.entry0 = buf[cur][n_act - 1];                // the carry of an interval longer than a chunk
            ln.base += chunk_blocks;
            __syncthreads();                                // buf, pre and wave_tot are free for the next chunk; ended and bad are visible
        }
        g0 += big ? 1u : nbi;
    }
    if (tid == 0) {
        status[(size_t)img * 4 + 0] = ok && !wrong && bad == 0u && ended == n_int ? MVLDM_JPEG_OK : MVLDM_JPEG_CORRUPT;
        status[(size_t)img * 4 + 1] = 0;
        status[(size_t)img * 4 + 2] = (int32_t)rounds_max;
        status[(size_t)img * 4 + 3] = (int32_t)n_all;
    }
}

// The two DC kernels keep their scans and the S sum in their own text.  One body (a template on the segmented scan, or the S sum as a
// function) was tried: jpeg_huff_dc_kernel sits at 126 of 128 registers, and every such form took it to 128 with 8 to 132 bytes of
// scratch a lane.  Shared are the block's address and the end of the kernel.  desc is the restart form's; jpeg_huff_dc_kernel takes it
// unread so that one launch function serves both.
__global__ __launch_bounds__(kHuffChunk) void jpeg_huff_dc_kernel(int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, const int32_t* __restrict__ desc,
                                                                   int32_t* __restrict__ status, HuffGeom G) {
    __shared__ uint32_t q[96];                              // uint16 [3][64] as pairs
    __shared__ long long wave_sum[kHuffChunk / WAVE];
    __shared__ int32_t wave_max[kHuffChunk / WAVE];
    const unsigned img = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    int32_t* st = status + (size_t)img * 4;
    if (st[0] != MVLDM_JPEG_OK) return;                     // the same in every lane: refused by the first kernel
    if (tid < 96) q[tid] = ((const uint32_t*)(qt + (size_t)img * 192))[tid];
    __syncthreads();
    int16_t* cf = coef + (size_t)img * G.total * 64;
    int bad = 0;
    int32_t worst = 0;
    for (uint32_t c = 0; c < G.ncomp; ++c) {
        const uint32_t nc = c == 0 ? G.mcus * G.nl : G.mcus;
        long long carry = 0;
        for (uint32_t j0 = 0; j0 < nc; j0 += kHuffChunk) {
            const uint32_t j = j0 + tid;
            const bool live = j < nc;
            int16_t* blk = cf;
            int diff = 0;
            if (live) {
                blk = huff_dc_block(cf, G, c, j);
                diff = blk[0];
            }
            long long incl = diff;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const long long up = __shfl_up(incl, o, WAVE);
                if ((int)lane >= o) incl += up;
            }
            if (lane == WAVE - 1) wave_sum[wave] = incl;
            __syncthreads();
            long long before = 0, all = 0;
#pragma unroll
            for (unsigned u = 0; u < (unsigned)kHuffChunk / WAVE; ++u) {
                const long long t = wave_sum[u];
                before += u < wave ? t : 0;
                all += t;
            }
            const long long pred = carry + before + incl;
            carry += all;
            if (live) {
                if (pred < -32768 || pred > 32767) {
                    bad = 1;
                } else {
                    int32_t sum = (int32_t)(pred < 0 ? -pred : pred) * (int32_t)(q[c * 32] & 0xFFFFu);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const u32x4 v = ((const u32x4*)blk)[i];         // loaded here, not held across the scan: 1024 lanes leave 128 registers
                        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const uint32_t qq = q[c * 32 + i * 4 + e];
                            const int32_t lo = (int32_t)(int16_t)(w4[e] & 0xFFFFu), hi = (int32_t)w4[e] >> 16;
                            if (i != 0 || e != 0) sum += (lo < 0 ? -lo : lo) * (int32_t)(qq & 0xFFFFu);
                            sum += (hi < 0 ? -hi : hi) * (int32_t)(qq >> 16);
                        }
                    }
                    worst = sum > worst ? sum : worst;
                    blk[0] = (int16_t)pred;
                }
            }
            __syncthreads();                                // wave_sum is free for the next 1024 blocks
        }
    }
    huff_dc_finish(bad, worst, wave_max, st, tid);
}

// jpeg_huff_dc_kernel with a SEGMENTED scan: a (head, sum) pair through the shuffles and the wave totals
__global__ __launch_bounds__(kHuffChunk) void jpeg_rst_dc_kernel(int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, const int32_t* __restrict__ desc,
                                                                  int32_t* __restrict__ status, HuffGeom G) {
    __shared__ uint32_t q[96];                              // uint16 [3][64] as pairs
    __shared__ long long wave_sum[kHuffChunk / WAVE];
    __shared__ int32_t wave_head[kHuffChunk / WAVE];
    __shared__ int32_t wave_max[kHuffChunk / WAVE];
    const unsigned img = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    int32_t* st = status + (size_t)img * 4;
    if (st[0] != MVLDM_JPEG_OK) return;                     // the same in every lane: refused by the first kernel
    const uint32_t ri = (uint32_t)desc[(size_t)img * 4 + 3];        // checked by the first kernel: 1 .. MCUs of the frame
    if (tid < 96) q[tid] = ((const uint32_t*)(qt + (size_t)img * 192))[tid];
    __syncthreads();
    int16_t* cf = coef + (size_t)img * G.total * 64;
    int bad = 0;
    int32_t worst = 0;
    for (uint32_t c = 0; c < G.ncomp; ++c) {
        const uint32_t per = c == 0 ? G.nl : 1u, nc = G.mcus * per, period = ri * per;
        long long carry = 0;
        for (uint32_t j0 = 0; j0 < nc; j0 += kHuffChunk) {
            const uint32_t j = j0 + tid;
            const bool live = j < nc;
            int16_t* blk = cf;
            int diff = 0;
            bool f = false;
            if (live) {
                blk = huff_dc_block(cf, G, c, j);
                diff = blk[0];
                f = j % period == 0u;                       // the first block of a restart interval
            }
            long long v = diff;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const long long up = __shfl_up(v, o, WAVE);
                const int upf = __shfl_up((int)f, o, WAVE);
                if ((int)lane >= o) huff_rst_join(upf != 0, up, &f, &v);
            }
            if (lane == WAVE - 1) wave_sum[wave] = v, wave_head[wave] = (int32_t)f;
            __syncthreads();
            long long before = carry, all = carry;
#pragma unroll
            for (unsigned u = 0; u < (unsigned)kHuffChunk / WAVE; ++u) {
                const long long t = wave_sum[u];
                const bool tf = wave_head[u] != 0;
                all = tf ? t : all + t;
                if (u < wave) before = all;
            }
            const long long pred = f ? v : before + v;
            carry = all;
            if (live) {
                if (pred < -32768 || pred > 32767) {
                    bad = 1;
                } else {
                    int32_t sum = (int32_t)(pred < 0 ? -pred : pred) * (int32_t)(q[c * 32] & 0xFFFFu);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const u32x4 x = ((const u32x4*)blk)[i];         // loaded here, not held across the scan: 1024 lanes leave 128 registers
                        const uint32_t w4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const uint32_t qq = q[c * 32 + i * 4 + e];
                            const int32_t lo = (int32_t)(int16_t)(w4[e] & 0xFFFFu), hi = (int32_t)w4[e] >> 16;
                            if (i != 0 || e != 0) sum += (lo < 0 ? -lo : lo) * (int32_t)(qq & 0xFFFFu);
                            sum += (hi < 0 ? -hi : hi) * (int32_t)(qq >> 16);
                        }
                    }
                    worst = sum > worst ? sum : worst;
                    blk[0] = (int16_t)pred;
                }
            }
            __syncthreads();                                // wave_sum and wave_head are free for the next 1024 blocks
        }
    }
    huff_dc_finish(bad, worst, wave_max, st, tid);
}

namespace {

using HuffScanKernel = void (*)(const uint8_t*, size_t, const int32_t*, const uint8_t*, int16_t*, uint16_t*, int32_t*, HuffGeom, uint32_t);
using HuffDcKernel = void (*)(int16_t*, const uint16_t*, const int32_t*, int32_t*, HuffGeom);

// A memset and the two launches of either form; `name` opens every error text.
int huff_launch(const char* name, HuffScanKernel scan_kernel, HuffDcKernel dc_kernel, const uint8_t* scan, size_t scan_bytes, const int32_t* desc,
                const uint8_t* tables, int n_img, int h, int w, int sampling, int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "%s: n_img %d", name, n_img);
    JpegLayout L;
    MVLDM_REQUIRE(jpeg_layout(h, w, sampling, &L), "%s: frame %d x %d, sampling %d (edges 1 .. %d, sampling 0 .. 3)", name, h, w, sampling, kJpegMaxDim);
    MVLDM_REQUIRE(huff_bits_ok(subseq_bits), "%s: subseq_bits %d (0, or a multiple of 32 in 32 .. %d)", name, subseq_bits, kHuffMaxBits);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(scan, 16) && aligned(tables, 16) && aligned(coef, 16) && aligned(qt, 16) && aligned(desc, 4) && aligned(status, 4),
                  "%s: null or unaligned pointer (scan, tables, coef, qt: 16 bytes; desc, status: 4)", name);
    MVLDM_REQUIRE(scan_bytes <= 0x7FFFFFFFu, "%s: %zu bytes of scans (below 2^31)", name, scan_bytes);
    const HuffGeom G = huff_geom(L);
    const uint32_t sb = subseq_bits ? (uint32_t)subseq_bits : (uint32_t)kHuffDefaultBits;
    MVLDM_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)n_img * L.blocks * 64 * sizeof(int16_t), s));
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n_img), dim3(kHuffChunk), 0, s, scan, scan_bytes, desc, tables, coef, qt, status, G, sb);
    hipLaunchKernelGGL(dc_kernel, dim3((unsigned)n_img), dim3(kHuffChunk), 0, s, coef, (const uint16_t*)qt, desc, status, G);
    return check_launch();
}

}  // namespace

int jpeg_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w, int sampling, int16_t* coef,
                        uint16_t* qt, int32_t* status, int subseq_bits, hipStream_t s) {
    return huff_launch("jpeg_entropy_device", jpeg_huff_kernel, jpeg_huff_dc_kernel, scan, scan_bytes, desc, tables, n_img, h, w, sampling, coef, qt, status,
                       subseq_bits, s);
}

int jpeg_rst_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w, int sampling, int16_t* coef,
                            uint16_t* qt, int32_t* status, int subseq_bits, hipStream_t s) {
    return huff_launch("jpeg_rst_entropy_device", jpeg_rst_scan_kernel, jpeg_rst_dc_kernel, scan, scan_bytes, desc, tables, n_img, h, w, sampling, coef, qt, status,
                       subseq_bits, s);
}

}  // namespace mvldm

using namespace mvldm;
extern "C" int mvldm_jpeg_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w, int sampling,
                                         int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, mvldm_stream_t stream) {
    return jpeg_entropy_device(scan, scan_bytes, desc, tables, n_img, h, w, sampling, coef, qt, status, subseq_bits, (hipStream_t)stream);
}

extern "C" int mvldm_jpeg_rst_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w,
                                             int sampling, int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, mvldm_stream_t stream) {
    return jpeg_rst_entropy_device(scan, scan_bytes, desc, tables, n_img, h, w, sampling, coef, qt, status, subseq_bits, (hipStream_t)stream);
}
