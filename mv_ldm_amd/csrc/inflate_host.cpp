// The inflate kernel's host twin: the same step and the same per-lane functions (inflate_common.h), with a loop over the 64 lanes where
// the kernel has a wave and nothing where it has a barrier (include/mvldm.h, "PNG frames: IDAT inflated on the device").  What the CPU
// tests pin to zlib, byte for byte and refusal for refusal, and what `png_decode(device="cpu", inflate="device")` runs.  Its input comes
// from untrusted files: a frame passes png_desc_ok and inflate_zdesc_ok before a byte of it is read.
#include <memory>

#include "common.h"
#include "inflate_common.h"

namespace mvldm {

static int inflate_frame_host(InfShared& S, const uint8_t* zp, uint32_t len, uint8_t* out, uint32_t need, uint32_t row) {
    InfState st;
    inf_init(st, len, need);
    S.status = MVLDM_PNG_INFLATE;
    S.act = INF_ACT_NONE;
    const uint64_t bound = (uint64_t)len * 8 + 16;
    for (uint64_t it = 0; it < bound; ++it) {
        const int act = inf_step(st, S, zp);
        if (act == INF_ACT_DONE) break;
        if (act == INF_ACT_BUILD_CL) {
            for (int lane = 0; lane < kInfLanes; ++lane) inf_build_count(S.dst, S.cl, 19, lane);
            inf_build_offsets(S.dst);
            for (int lane = 0; lane < kInfLanes; ++lane) inf_build_place(S.dst, S.cl, 19, lane);
        } else if (act == INF_ACT_BUILD) {
            const int n_lit = S.n_lit, n_dst = S.n_dst;
            for (int lane = 0; lane < kInfLanes; ++lane) {
                inf_build_count(S.lit, S.lens, n_lit, lane);
                inf_build_count(S.dst, S.lens + n_lit, n_dst, lane);
            }
            inf_build_offsets(S.lit);
            inf_build_offsets(S.dst);
            for (int lane = 0; lane < kInfLanes; ++lane) {
                inf_build_place(S.lit, S.lens, n_lit, lane);
                inf_build_place(S.dst, S.lens + n_lit, n_dst, lane);
            }
        } else if (act == INF_ACT_STORED) {
            for (int lane = 0; lane < kInfLanes; ++lane) inf_copy_stored(S, zp, len, out, need, lane);
        } else if (act == INF_ACT_BATCH) {
            const uint32_t n = S.a0 < (uint32_t)kInfBatch ? S.a0 : (uint32_t)kInfBatch;
            uint32_t i = 0;
            while (i < n) {
                const uint32_t v = S.q_val[i];
                if (v >= kInfMatch) {
                    const uint32_t start = S.q_pos[i], length = v & 0xFFFFu, dist = v >> 16;
                    uint64_t bytes[kInfLanes];
                    for (int lane = 0; lane < kInfLanes; ++lane) bytes[lane] = inf_match_read(S, start, length, dist, lane);
                    for (int lane = 0; lane < kInfLanes; ++lane) inf_match_write(S, out, need, start, length, dist, lane, bytes[lane]);
                    i += 1;
                } else {
                    uint32_t j = i + 1;
                    while (j < n && S.q_val[j] < kInfMatch) ++j;
                    for (int lane = 0; lane < kInfLanes; ++lane) inf_put_literals(S, out, need, i, j, lane);
                    i = j;
                }
            }
        } else if (act == INF_ACT_FINISH) {
            const uint32_t n = S.a0;
            for (int lane = 0; lane < kInfLanes; ++lane) inf_sum_lane(S, out, n, need, row, lane);
            S.status = inf_verdict(S, n, need);
            break;
        }
    }
    return S.status;
}

}  // namespace mvldm

using namespace mvldm;
extern "C" int mvldm_png_inflate_host(const uint8_t* z, size_t z_bytes, const int32_t* zdesc, uint8_t* streams, size_t stream_bytes, const int32_t* desc, int n_img,
                                      int h, int w, int32_t* zstatus) {
    if (n_img < 0 || !png_dims_ok(h, w)) return set_error(MVLDM_ERR_ARG, "png_inflate_host: %d frames of %d x %d (edges 1 .. %d)", n_img, h, w, kPngMaxDim);
    if (n_img == 0) return MVLDM_OK;
    if (z == nullptr || zdesc == nullptr || streams == nullptr || desc == nullptr || zstatus == nullptr) return set_error(MVLDM_ERR_ARG, "png_inflate_host: null pointer");
    if (z_bytes > 0x7FFFFFFFu || stream_bytes > 0x7FFFFFFFu)
        return set_error(MVLDM_ERR_ARG, "png_inflate_host: %zu bytes of zlib streams, %zu of inflated streams (below 2^31)", z_bytes, stream_bytes);
    std::unique_ptr<InfShared> S(new InfShared);
    for (int i = 0; i < n_img; ++i) {
        const int32_t* d = desc + (size_t)i * kPngDescInts;
        const int32_t* zd = zdesc + (size_t)i * kInfZdescInts;
        if (!png_desc_ok(d, stream_bytes, (size_t)0x7FFFFFFF, h, w) || !inflate_zdesc_ok(zd, z_bytes)) {
            zstatus[i] = MVLDM_PNG_DESC;
            continue;
        }
        const uint32_t row = (uint32_t)(1 + png_stride(w, d[1], d[2]));
        zstatus[i] = inflate_frame_host(*S, z + (size_t)zd[0], (uint32_t)zd[1], streams + (size_t)d[0], (uint32_t)h * row, row);
    }
    return MVLDM_OK;
}
