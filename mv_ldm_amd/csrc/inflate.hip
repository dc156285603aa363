// PNG frames: IDAT inflated on the device (include/mvldm.h, "PNG frames: IDAT inflated on the device").  One wave per frame.  DEFLATE is
// one serial chain of symbols, so one lane decodes: it runs the sequential step (inflate_common.h) until the wave has something to do --
// a code set to turn into tables, a stored block to copy, a queue of up to 64 symbols to write -- and the 64 lanes do that together: the
// tables of a dynamic block (a length per lane), a stored block and every match as parallel copies, a run of literals one per lane.
// Matches read a 32 KiB sliding window in LDS, never the frame's slot, which is written only; __syncthreads() orders every group of
// writes before the reads that follow it.  At the end the wave reads the slot back once (after a workgroup-scope fence) for the
// Adler-32 and the rows' filter bytes.  No wait on another workgroup, no allocation, no read-back: the call can be captured.
// The kernel is latency-bound by construction, like the unfilter kernel behind it: a batch of frames is that many waves.
#include "common.h"
#include "inflate_common.h"

namespace mvldm {

static_assert(kInfLanes == WAVE, "one lane of the step functions per lane of the wave");

__global__ __launch_bounds__(WAVE) void png_inflate_kernel(const uint8_t* __restrict__ z, size_t z_bytes, const int32_t* __restrict__ zdesc, uint8_t* streams,
                                                           size_t stream_bytes, const int32_t* __restrict__ desc, int h, int w, int32_t* __restrict__ zstatus) {
    __shared__ InfShared S;
    const size_t img = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int32_t* d = desc + img * kPngDescInts;
    const int32_t* zd = zdesc + img * kInfZdescInts;
    if (!png_desc_ok(d, stream_bytes, (size_t)0x7FFFFFFF, h, w) || !inflate_zdesc_ok(zd, z_bytes)) {     // uniform: nothing of the frame is read or written
        if (lane == 0) zstatus[img] = MVLDM_PNG_DESC;
        return;
    }
    const uint32_t row = (uint32_t)(1 + png_stride(w, d[1], d[2]));
    const uint32_t need = (uint32_t)h * row;                // fits: png_desc_ok placed it inside stream_bytes, which is below 2^31
    const uint32_t len = (uint32_t)zd[1];
    const uint8_t* zp = z + (size_t)zd[0];
    uint8_t* out = streams + (size_t)d[0];
    InfState st;
    inf_init(st, len, need);
    if (lane == 0) {
        S.status = MVLDM_PNG_INFLATE;
        S.act = INF_ACT_NONE;
    }
    __syncthreads();
    const uint64_t bound = (uint64_t)len * 8 + 16;
    for (uint64_t it = 0; it < bound; ++it) {
        if (lane == 0) inf_step(st, S, zp);
        __syncthreads();
        const int act = S.act;
        if (act == INF_ACT_DONE) break;
        if (act == INF_ACT_BUILD_CL) {
            inf_build_count(S.dst, S.cl, 19, lane);
            __syncthreads();
            if (lane == 0) inf_build_offsets(S.dst);
            __syncthreads();
            inf_build_place(S.dst, S.cl, 19, lane);
        } else if (act == INF_ACT_BUILD) {
            const int n_lit = S.n_lit, n_dst = S.n_dst;     // at most 288 + 32: the step set them
            inf_build_count(S.lit, S.lens, n_lit, lane);
            inf_build_count(S.dst, S.lens + n_lit, n_dst, lane);
            __syncthreads();
            if (lane == 0) inf_build_offsets(S.lit);
            if (lane == 1) inf_build_offsets(S.dst);
            __syncthreads();
            inf_build_place(S.lit, S.lens, n_lit, lane);
            inf_build_place(S.dst, S.lens + n_lit, n_dst, lane);
        } else if (act == INF_ACT_STORED) {
            inf_copy_stored(S, zp, len, out, need, lane);
        } else if (act == INF_ACT_BATCH) {
            const uint32_t n = S.a0 < (uint32_t)kInfBatch ? S.a0 : (uint32_t)kInfBatch;
            uint32_t i = 0;
            while (i < n) {                                 // uniform: the queue is read from LDS by every lane alike
                const uint32_t v = S.q_val[i];
                if (v >= kInfMatch) {
                    const uint32_t start = S.q_pos[i], length = v & 0xFFFFu, dist = v >> 16;
                    const uint64_t bytes = inf_match_read(S, start, length, dist, lane);
                    __syncthreads();
                    inf_match_write(S, out, need, start, length, dist, lane, bytes);
                    i += 1;
                } else {
                    uint32_t j = i + 1;
                    while (j < n && S.q_val[j] < kInfMatch) ++j;
                    inf_put_literals(S, out, need, i, j, lane);
                    i = j;
                }
                __syncthreads();
            }
        } else if (act == INF_ACT_FINISH) {
            __threadfence_block();                          // the slot was written by other lanes: release / acquire at workgroup scope
            __syncthreads();
            inf_sum_lane(S, out, S.a0, need, row, lane);
            __syncthreads();
            if (lane == 0) S.status = inf_verdict(S, S.a0, need);
            break;
        }
        __syncthreads();
    }
    if (lane == 0) zstatus[img] = S.status;
}

int png_inflate(const uint8_t* z, size_t z_bytes, const int32_t* zdesc, uint8_t* streams, size_t stream_bytes, const int32_t* desc, int n_img, int h, int w,
                int32_t* zstatus, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "png_inflate: n_img %d", n_img);
    MVLDM_REQUIRE(png_dims_ok(h, w), "png_inflate: frame %d x %d (edges 1 .. %d)", h, w, kPngMaxDim);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(aligned(z, 16) && streams != nullptr && aligned(zdesc, 4) && aligned(desc, 4) && aligned(zstatus, 4),
                  "png_inflate: null or unaligned pointer (z: 16 bytes; zdesc, desc, zstatus: 4 bytes)");
    MVLDM_REQUIRE(z_bytes <= 0x7FFFFFFFu && stream_bytes <= 0x7FFFFFFFu, "png_inflate: %zu bytes of zlib streams, %zu of inflated streams (below 2^31)", z_bytes,
                  stream_bytes);
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n_img), dim3(WAVE), 0, s, z, z_bytes, zdesc, streams, stream_bytes, desc, h, w, zstatus);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_png_inflate_room(size_t bytes) { return inflate_room(bytes); }
extern "C" int mvldm_png_inflate(const uint8_t* z, size_t z_bytes, const int32_t* zdesc, uint8_t* streams, size_t stream_bytes, const int32_t* desc, int n_img,
                                 int h, int w, int32_t* zstatus, mvldm_stream_t stream) {
    return png_inflate(z, z_bytes, zdesc, streams, stream_bytes, desc, n_img, h, w, zstatus, (hipStream_t)stream);
}
