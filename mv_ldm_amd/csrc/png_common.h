// What the PNG row-unfiltering kernel (png.hip) and its host twin (png_host.cpp, mvldm_png_unfilter_host) share: the geometry of an
// inflated stream, the descriptor check, the reconstruction of one filtered unit and the expansion of a reconstructed unit to RGB --
// written once, so that the kernel and the twin run the same statements (include/mvldm.h, "PNG frames").
// No HIP call and no other header of the library.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mvldm.h"

#ifndef MVLDM_HD
#if defined(__HIPCC__)
#define MVLDM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MVLDM_HD inline
#endif
#endif

namespace mvldm {

constexpr int kPngMaxDim = 16384;               // edges 1 .. 16384: a row of units fits the kernel's LDS row, every offset fits size_t sums of int32
constexpr int kPngDescInts = MVLDM_PNG_DESC_INTS;
constexpr uint32_t kPngPalMiss = 1u << 24;      // a palette slot beyond the PLTE entries: looked up as black, and the frame is flagged

// colour type x bit depth the kernel expands: RGB, RGBA, grey, grey + alpha at 8 bits; palette at 1, 2, 4, 8
MVLDM_HD bool png_format_ok(int ctype, int depth) {
    if (ctype == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    return (ctype == 0 || ctype == 2 || ctype == 4 || ctype == 6) && depth == 8;
}
MVLDM_HD int png_channels(int ctype) { return ctype == 2 ? 3 : ctype == 6 ? 4 : ctype == 4 ? 2 : 1; }
// bytes of a row behind its filter byte
MVLDM_HD size_t png_stride(int w, int ctype, int depth) { return ((size_t)w * (size_t)(png_channels(ctype) * depth) + 7) >> 3; }
// the filters' distance to "the byte to the left": bytes of a whole pixel, 1 below 8 bits.  Also the kernel's unit: one pixel, or one byte of pixels.
MVLDM_HD int png_bpp(int ctype, int depth) { return depth < 8 ? 1 : png_channels(ctype); }
MVLDM_HD bool png_dims_ok(int h, int w) { return h >= 1 && w >= 1 && h <= kPngMaxDim && w <= kPngMaxDim; }

// desc[0..7] = offset of the inflated stream in the packed buffer, colour type, bit depth, offset of the palette in the packed palettes
// (bytes), palette entries, 0, 0, 0.  false: nothing of the frame is read and nothing is written for it.
MVLDM_HD bool png_desc_ok(const int32_t* d, size_t stream_bytes, size_t palette_bytes, int h, int w) {
    if (!png_dims_ok(h, w) || d[0] < 0 || !png_format_ok(d[1], d[2])) return false;
    const size_t need = (size_t)h * (1 + png_stride(w, d[1], d[2]));
    if ((size_t)d[0] > stream_bytes || stream_bytes - (size_t)d[0] < need) return false;
    if (d[1] == 3) {
        if (d[3] < 0 || d[4] < 1 || d[4] > 256) return false;
        if ((size_t)d[3] > palette_bytes || palette_bytes - (size_t)d[3] < (size_t)d[4] * 3) return false;
    }
    return true;
}

// slot i of a frame's 256-entry palette table: R | G << 8 | B << 16, or kPngPalMiss beyond the PLTE entries
MVLDM_HD uint32_t png_pal_slot(const uint8_t* pal, int count, int i) {
    return i < count ? (uint32_t)pal[3 * i] | (uint32_t)pal[3 * i + 1] << 8 | (uint32_t)pal[3 * i + 2] << 16 : kPngPalMiss;
}

// ---- reconstruction ---------------------------------------------------------------------------------------------------------------
// One byte: x the filtered byte, a the reconstructed byte one pixel to the left, b the one above, c the one above a (all 0 outside the
// image).  Every predictor is computed and one is selected: the lanes of a wave hold rows of different filters, a branch would run all
// five anyway.  Average floors the 9-bit sum; Paeth is p = a + b - c in integers, ties in the order a, b, c.  A filter byte above 4 is None.
MVLDM_HD uint32_t png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc) ? b : c);
}
MVLDM_HD uint32_t png_recon_byte(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t avg = (a + b) >> 1, pae = png_paeth((int)a, (int)b, (int)c);
    const uint32_t pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? avg : ft == 4 ? pae : 0u;
    return (x + pred) & 255u;
}
// One unit of BPP bytes, byte k in bits 8k .. 8k + 7
template <int BPP> MVLDM_HD uint32_t png_recon_unit(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < BPP; ++k)
        r |= png_recon_byte(ft, (x >> (8 * k)) & 255u, (a >> (8 * k)) & 255u, (b >> (8 * k)) & 255u, (c >> (8 * k)) & 255u) << (8 * k);
    return r;
}

// ---- expansion --------------------------------------------------------------------------------------------------------------------
// k / 255 in fp32, correctly rounded: the bits of torch's `k.float() / 255`
MVLDM_HD float png_unit_float(uint32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)k, 255.0f);
#else
    return (float)k / 255.0f;
#endif
}
// pixel x of row `row` of frame `img` <- rgb (R | G << 8 | B << 16).  kind MVLDM_PNG_DST_U8: uint8 [n][h][w][3]; _F32: fp32 [n][3][h][w]
MVLDM_HD void png_store_pixel(void* dst, int kind, size_t img, int h, int w, int row, int x, uint32_t rgb) {
    if (kind == MVLDM_PNG_DST_U8) {
        uint8_t* p = (uint8_t*)dst + (((img * (size_t)h + (size_t)row) * (size_t)w + (size_t)x) * 3);
        p[0] = (uint8_t)(rgb & 255u);
        p[1] = (uint8_t)((rgb >> 8) & 255u);
        p[2] = (uint8_t)((rgb >> 16) & 255u);
    } else {
        const size_t plane = (size_t)h * (size_t)w;
        float* p = (float*)dst + (img * 3 * plane + (size_t)row * (size_t)w + (size_t)x);
        p[0] = png_unit_float(rgb & 255u);
        p[plane] = png_unit_float((rgb >> 8) & 255u);
        p[2 * plane] = png_unit_float((rgb >> 16) & 255u);
    }
}
// The reconstructed unit u of a row -> its pixels: alpha dropped, grey replicated, palette entries looked up in `pal` (256 slots of
// png_pal_slot).  Returns 1 if a palette index lies beyond the PLTE entries (stored as black), else 0.
MVLDM_HD int png_emit_unit(void* dst, int kind, size_t img, int h, int w, int row, int u, uint32_t r, int ctype, int depth, const uint32_t* pal) {
    if (ctype == 2 || ctype == 6) {
        png_store_pixel(dst, kind, img, h, w, row, u, r & 0xFFFFFFu);
        return 0;
    }
    if (ctype == 0 || ctype == 4) {
        png_store_pixel(dst, kind, img, h, w, row, u, (r & 255u) * 0x010101u);
        return 0;
    }
    int miss = 0;
    const int per = 8 / depth;                  // pixels of a byte, the leftmost in the high bits
    for (int p = 0; p < per; ++p) {
        const int x = u * per + p;
        if (x < w) {
            const uint32_t e = pal[(r >> (8 - depth * (p + 1))) & ((1u << depth) - 1u)];
            miss |= (int)(e >> 24);
            png_store_pixel(dst, kind, img, h, w, row, x, e & 0xFFFFFFu);
        }
    }
    return miss;
}

}  // namespace mvldm
