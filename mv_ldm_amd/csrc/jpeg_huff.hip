// The Huffman-coded scan of a JPEG frame decoded on the device (include/mvldm.h, "JPEG frames: the scan on the device"): a
// self-synchronising decoder (Klein and Wiseman; Weissenberger and Schmidt) in the form whose correctness does not depend on
// synchronisation ever happening.  The step function, the bit window and the coefficient store are jpeg_huff_common.h's, shared with
// mvldm_jpeg_entropy_emul_host.
//   jpeg_huff_kernel     one workgroup of 1024 per frame, one subsequence of `sb` bits per thread, the frame's chunks of 1024
//                        subsequences in order.  LDS: the six Huffman tables (8544 B), the exit states twice (16 KiB: a round reads one
//                        copy and writes the other, so one barrier a round), the zigzag table, wave totals.  Per chunk: the cold pass;
//                        rounds until no entry changed (__syncthreads_or) or n_act rounds ran; an exclusive scan of the completed-block
//                        counts; the write pass.  A lane's loop runs at most sb symbols (a symbol is at least one bit), a chunk at most
//                        n_act rounds, a frame ceil(bits / sb / 1024) chunks: every bound comes from sizes.  No kernel waits for
//                        another workgroup.  The coefficient slots are zeroed by a memset node in front of this kernel on the same
//                        stream: stream order puts every store of the write pass after it.
//   jpeg_huff_dc_kernel  one workgroup per frame: per component the DC differences in scan order (luma MCU-major) become predictions
//                        through a 64-bit workgroup scan with a carry, and every block's S = sum |coef q| is formed from eight 16-byte
//                        loads; the largest S and the reason go to status.
// Divergent by nature and bound by each lane's serial chain (window -> table lookup in LDS -> next bit position), not by bandwidth.
#include "common.h"
#include "jpeg_huff_common.h"

namespace mvldm {

__global__ __launch_bounds__(kHuffChunk) void jpeg_huff_kernel(const uint8_t* __restrict__ scan, size_t scan_bytes, const int32_t* __restrict__ desc,
                                                                const uint8_t* __restrict__ tables, int16_t* __restrict__ coef, uint16_t* __restrict__ qt,
                                                                int32_t* __restrict__ status, HuffGeom G, uint32_t sb) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[kHuffTabsBytes];
    __shared__ HuffState buf[2][kHuffChunk];
    __shared__ uint32_t wave_blocks[kHuffChunk / WAVE];
    __shared__ uint8_t zigzag[64];
    __shared__ uint32_t end_p, bad;
    const unsigned img = blockIdx.x, tid = threadIdx.x;
    const u32x4* blob = (const u32x4*)(tables + (size_t)img * kHuffBlobBytes);
    for (unsigned i = tid; i < (unsigned)kHuffTabsBytes / 16; i += kHuffChunk) ((u32x4*)tab)[i] = blob[i];
    if (tid < 24) ((u32x4*)(qt + (size_t)img * 192))[tid] = blob[kHuffTabsBytes / 16 + tid];
    if (tid < 64) zigzag[tid] = huff_zigzag(tid);
    if (tid == 0) end_p = 0xFFFFFFFFu, bad = 0u;
    int32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = desc[(size_t)img * 4 + i];
    const bool ok = huff_desc_ok(d, scan_bytes);            // a descriptor that does not fit the buffer: no bit is read, the frame is refused
    const uint8_t* sc = scan + (ok ? (size_t)d[0] : 0);
    const uint32_t bit_len = ok ? (uint32_t)d[1] : 0u;
    const uint32_t nsub = (uint32_t)(((uint64_t)bit_len + sb - 1) / sb);
    __syncthreads();

    HuffState carry = {0u, 0u};
    uint32_t base = 0, rounds_max = 0;
    for (uint32_t ch0 = 0; ch0 < nsub; ch0 += kHuffChunk) {
        const uint32_t n_act = nsub - ch0 < (uint32_t)kHuffChunk ? nsub - ch0 : (uint32_t)kHuffChunk;
        const bool active = tid < n_act;
        const uint64_t e64 = ((uint64_t)(ch0 + tid) + 1) * sb;
        const uint32_t end = e64 < bit_len ? (uint32_t)e64 : bit_len;
        HuffNoSink none;
        HuffState entry = {0u, 0u}, exit = {0u, 0u};
        uint32_t done = 0;
        if (active) {                                       // cold pass
            entry = tid == 0 ? carry : HuffState{(ch0 + tid) * sb, 0u};
            exit = entry;
            huff_run(sc, bit_len, tab, G.nl, G.nb, end, sb, &exit, &done, &none);
            buf[0][tid] = exit;
        }
        __syncthreads();
        int cur = 0;
        uint32_t rounds = 0;
        for (uint32_t r = 0; r < n_act; ++r) {
            int changed = 0;
            if (active) {
                if (tid >= 1) {
                    const HuffState e = buf[cur][tid - 1];
                    if (!huff_same(e, entry)) {
                        entry = exit = e;
                        huff_run(sc, bit_len, tab, G.nl, G.nb, end, sb, &exit, &done, &none);
                        changed = 1;
                    }
                }
                buf[cur ^ 1][tid] = exit;
            }
            const int any = __syncthreads_or(changed);      // the round's barrier: readers of buf[cur] are done, buf[cur ^ 1] is complete
            cur ^= 1;
            ++rounds;
            if (!any) break;
        }
        rounds_max = rounds > rounds_max ? rounds : rounds_max;
        // exclusive scan of the completed-block counts: within the wave by shuffles, across the 16 waves through LDS
        uint32_t incl = done;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, WAVE);
            if ((int)(tid & (WAVE - 1)) >= o) incl += up;
        }
        if ((tid & (WAVE - 1)) == WAVE - 1) wave_blocks[tid / WAVE] = incl;
        __syncthreads();
        uint32_t before = 0, chunk_blocks = 0;
#pragma unroll
        for (unsigned v = 0; v < (unsigned)kHuffChunk / WAVE; ++v) {
            const uint32_t t = wave_blocks[v];
            before += v < tid / WAVE ? t : 0u;
            chunk_blocks += t;
        }
        if (active) {                                       // write pass, from the entry the rounds settled on
            HuffCoefSink sink{coef + (size_t)img * G.total * 64, zigzag, G, base + before + incl - done, &end_p, &bad, nullptr};
            sink.open();
            HuffState st = entry;
            uint32_t again = 0;
            huff_run(sc, bit_len, tab, G.nl, G.nb, end, sb, &st, &again, &sink);
        }
        carry = buf[cur][n_act - 1];
        base += chunk_blocks;
        __syncthreads();                                    // buf and wave_blocks are free for the next chunk; end_p and bad are visible
    }
    if (tid == 0) {
        const uint32_t at = end_p;
        status[(size_t)img * 4 + 0] = bad == 0u && at != 0xFFFFFFFFu && bit_len - at < 8u ? MVLDM_JPEG_OK : MVLDM_JPEG_CORRUPT;
        status[(size_t)img * 4 + 1] = 0;
        status[(size_t)img * 4 + 2] = (int32_t)rounds_max;
        status[(size_t)img * 4 + 3] = 0;
    }
}

__global__ __launch_bounds__(kHuffChunk) void jpeg_huff_dc_kernel(int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, int32_t* __restrict__ status,
                                                                   HuffGeom G) {
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
                const uint32_t m = c == 0 ? j / G.nl : j, b = c == 0 ? j - m * G.nl : G.nl + c - 1;
                blk = cf + (size_t)huff_block_index(G, m, b) * 64;
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

int jpeg_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w, int sampling, int16_t* coef,
                        uint16_t* qt, int32_t* status, int subseq_bits, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "jpeg_entropy_device: n_img %d", n_img);
    JpegLayout L;
    MVLDM_REQUIRE(jpeg_layout(h, w, sampling, &L), "jpeg_entropy_device: frame %d x %d, sampling %d (edges 1 .. %d, sampling 0 .. 3)", h, w, sampling, kJpegMaxDim);
    MVLDM_REQUIRE(huff_bits_ok(subseq_bits), "jpeg_entropy_device: subseq_bits %d (0, or a multiple of 32 in 32 .. %d)", subseq_bits, kHuffMaxBits);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(scan, 16) && aligned(tables, 16) && aligned(coef, 16) && aligned(qt, 16) && aligned(desc, 4) && aligned(status, 4),
                  "jpeg_entropy_device: null or unaligned pointer (scan, tables, coef, qt: 16 bytes; desc, status: 4)");
    MVLDM_REQUIRE(scan_bytes <= 0x7FFFFFFFu, "jpeg_entropy_device: %zu bytes of scans (below 2^31)", scan_bytes);
    const HuffGeom G = huff_geom(L);
    const uint32_t sb = subseq_bits ? (uint32_t)subseq_bits : (uint32_t)kHuffDefaultBits;
    MVLDM_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)n_img * L.blocks * 64 * sizeof(int16_t), s));
    hipLaunchKernelGGL(jpeg_huff_kernel, dim3((unsigned)n_img), dim3(kHuffChunk), 0, s, scan, scan_bytes, desc, tables, coef, qt, status, G, sb);
    hipLaunchKernelGGL(jpeg_huff_dc_kernel, dim3((unsigned)n_img), dim3(kHuffChunk), 0, s, coef, (const uint16_t*)qt, status, G);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" int mvldm_jpeg_entropy_device(const uint8_t* scan, size_t scan_bytes, const int32_t* desc, const uint8_t* tables, int n_img, int h, int w, int sampling,
                                         int16_t* coef, uint16_t* qt, int32_t* status, int subseq_bits, mvldm_stream_t stream) {
    return jpeg_entropy_device(scan, scan_bytes, desc, tables, n_img, h, w, sampling, coef, qt, status, subseq_bits, (hipStream_t)stream);
}
