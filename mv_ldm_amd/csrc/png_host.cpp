// The PNG kernel's host twin: the same reconstruction and expansion (png_common.h) row by row in plain C++ on host pointers
// (include/mvldm.h, "PNG frames").  What the CPU tests pin to Pillow, and what tools use where no device is at hand.  Its sizes come from
// untrusted files: every frame passes png_desc_ok before a byte of it is read, and a frame that does not is left alone.
#include <vector>

#include "common.h"
#include "png_common.h"

namespace mvldm {

template <int BPP>
static int png_frame_host(const uint8_t* src, int ctype, int depth, void* dst, int kind, size_t img, int h, int w, const uint32_t* pal, uint32_t* above) {
    const size_t stride = png_stride(w, ctype, depth);
    const int units = (int)(stride / BPP);
    int miss = 0;
    for (int u = 0; u < units; ++u) above[u] = 0;           // the row above the first row
    for (int row = 0; row < h; ++row) {
        const uint8_t* rowp = src + (size_t)row * (1 + stride);
        uint32_t ft = rowp[0];
        ft = ft > 4u ? 0u : ft;
        uint32_t last = 0, c = 0;                           // left of the first pixel
        for (int u = 0; u < units; ++u) {
            uint32_t x = 0;
            for (int k = 0; k < BPP; ++k) x |= (uint32_t)rowp[1 + (size_t)u * BPP + k] << (8 * k);
            const uint32_t b = above[u];
            last = png_recon_unit<BPP>(ft, x, last, b, c);
            c = b;
            above[u] = last;
            miss |= png_emit_unit(dst, kind, img, h, w, row, u, last, ctype, depth, pal);
        }
    }
    return miss;
}

}  // namespace mvldm

using namespace mvldm;
extern "C" int mvldm_png_unfilter_host(const uint8_t* streams, size_t stream_bytes, const int32_t* desc, const uint8_t* palettes, size_t palette_bytes, void* dst,
                                       int dst_kind, int n_img, int h, int w, int32_t* status) {
    if (n_img < 0 || !png_dims_ok(h, w)) return set_error(MVLDM_ERR_ARG, "png_unfilter_host: %d frames of %d x %d (edges 1 .. %d)", n_img, h, w, kPngMaxDim);
    if (dst_kind != MVLDM_PNG_DST_U8 && dst_kind != MVLDM_PNG_DST_F32) return set_error(MVLDM_ERR_ARG, "png_unfilter_host: dst_kind %d", dst_kind);
    if (n_img == 0) return MVLDM_OK;
    if (streams == nullptr || desc == nullptr || dst == nullptr || status == nullptr || (palettes == nullptr && palette_bytes != 0))
        return set_error(MVLDM_ERR_ARG, "png_unfilter_host: null pointer");
    if (stream_bytes > 0x7FFFFFFFu || palette_bytes > 0x7FFFFFFFu)
        return set_error(MVLDM_ERR_ARG, "png_unfilter_host: %zu bytes of streams, %zu of palettes (below 2^31)", stream_bytes, palette_bytes);
    std::vector<uint32_t> above((size_t)w), pal(256);
    for (int i = 0; i < n_img; ++i) {
        const int32_t* d = desc + (size_t)i * kPngDescInts;
        if (!png_desc_ok(d, stream_bytes, palette_bytes, h, w)) {
            status[i] = MVLDM_PNG_DESC;
            continue;
        }
        const int ctype = d[1], depth = d[2];
        if (ctype == 3)
            for (int k = 0; k < 256; ++k) pal[k] = png_pal_slot(palettes + d[3], d[4], k);
        const uint8_t* src = streams + (size_t)d[0];
        int miss;
        switch (png_bpp(ctype, depth)) {
            case 1: miss = png_frame_host<1>(src, ctype, depth, dst, dst_kind, (size_t)i, h, w, pal.data(), above.data()); break;
            case 2: miss = png_frame_host<2>(src, ctype, depth, dst, dst_kind, (size_t)i, h, w, pal.data(), above.data()); break;
            case 3: miss = png_frame_host<3>(src, ctype, depth, dst, dst_kind, (size_t)i, h, w, pal.data(), above.data()); break;
            default: miss = png_frame_host<4>(src, ctype, depth, dst, dst_kind, (size_t)i, h, w, pal.data(), above.data()); break;
        }
        status[i] = miss ? MVLDM_PNG_PALETTE_INDEX : MVLDM_PNG_OK;
    }
    return MVLDM_OK;
}
