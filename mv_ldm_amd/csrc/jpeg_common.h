// What the JPEG decoder's host half (jpeg_host.cpp) and device half (jpeg.hip) share: the frame layout, the range guard and the integer
// arithmetic of libjpeg's parallel half -- jidctint's ISLOW inverse DCT, the "fancy" triangle upsampling of jdsample.c and the
// YCbCr -> RGB tables of jdcolor.c -- written once, so that mvldm_jpeg_idct_host and the two kernels run the same statements.
// No HIP call and no other header of the library: jpeg_host.cpp also compiles on its own with a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mvldm.h"

#if defined(__HIPCC__)
#define MVLDM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MVLDM_HD inline
#endif

namespace mvldm {

// ---- the range guard -------------------------------------------------------------------------------------------------------------
// S = sum_k |coef_k q_k| over the 64 dequantised values of a block.  A frame is decoded here only when every block has S <= kJpegGuard;
// otherwise libjpeg's C code (64-bit `long`, the result masked to 10 bits), libjpeg-turbo's SIMD code (dequantised values and pass-1
// outputs stored in 16 bits with saturation, 16-bit adds in front of the multiplies) and a plain int32 kernel stop agreeing.
//
// One 1-D pass is linear in its inputs until its single DESCALE: out_x = DESCALE(sum_k M[x][k] in_k, n) with integer M.  Feeding unit
// vectors through jpeg_idct_1d gives max_x |M[x][k]| = 8192, 11363, 10703, 11362, 8192, 11362, 10704, 11363 for k = 0 .. 7, so
// kJpegGain1 = 11363 = round(2^13 sqrt(2) cos(pi / 16)), the 1.3870 of the cosine basis; and over every partial sum the pass forms --
// each product, tmp and z in front of the final butterflies -- the largest |coefficient| of any input is kJpegPartial = 27431.
//   (a) a dequantised value fits 16 bits:                  |coef q| <= S <= 32767.
//   (b) a pass-1 output fits 16 bits without saturation:   |ws| <= (11363 S_col + 2^10) >> 11 <= 11363 S_col / 2048 + 1 <= 32767
//                                                          <=> S_col <= 32766 * 2048 / 11363 = 5905.5, and S_col <= S.
//       The SIMD code also adds in0 + in4 (and in0 - in4) of a ROW of pass-1 outputs in 16 bits before it widens: |ws_0| + |ws_4| <=
//       11363 (S_col0 + S_col4) / 2048 + 2 <= 11363 S / 2048 + 2, which (b) on the whole block's S keeps below 32768 as well -- the
//       reason the guard is on the block's S and not per column.
//   (c) every int32 partial sum of pass 2 stays below 2^31: the inputs of a row satisfy sum_k |ws_k| <= 11363 S / 2048 + 8, so a
//       partial sum is at most 27431 (11363 * 5905 / 2048 + 8) = 9.0e8 < 2^31 = 2.1e9; the final sums are at most
//       11363 * 32772 + 2^17 = 3.7e8.  Pass 1's partial sums are at most 27431 * 5905 = 1.6e8.
// (b) binds: B = 5905.  Within it the three implementations compute the same int32 values, and the last step is libjpeg-turbo's
// saturating pack, clip(x + 128, 0, 255).  (libjpeg's C table lookup masks x to 10 bits first and equals the clip for |x| <= 511;
// |x| <= 0.2405 S reaches that only above S = 2124, i.e. for blocks whose pixels would already lie four times outside [0, 255].)
constexpr int kJpegGuard = 5905;
constexpr int kJpegGain1 = 11363;
constexpr int kJpegPartial = 27431;

// ---- layout ------------------------------------------------------------------------------------------------------------------------
// A frame of h x w in one of the four sampling layouts: per component the size in samples (ceil(h v / vmax) x ceil(w hs / hmax), what
// the upsampler's edges use), the MCU-padded block grid and the offset of its first block.  Coefficients: int16 [blocks][64];
// planes (the workspace): uint8, component c at 64 off[c], [8 bh][8 bw].
struct JpegLayout {
    int ncomp, hmax, vmax;
    int mcux, mcuy;
    int bw[3], bh[3];       // blocks per row / column of the component's padded grid
    int cw[3], ch[3];       // real samples per row / column
    int off[3];             // first block of the component within the frame
    int blocks;             // all components
};
constexpr int kJpegMaxDim = 16384;          // per edge: keeps every index of a frame inside int32

MVLDM_HD bool jpeg_layout(int h, int w, int sampling, JpegLayout* L) {
    if (h < 1 || w < 1 || h > kJpegMaxDim || w > kJpegMaxDim || sampling < MVLDM_JPEG_GRAY || sampling > MVLDM_JPEG_420) return false;
    L->ncomp = sampling == MVLDM_JPEG_GRAY ? 1 : 3;
    L->hmax = sampling >= MVLDM_JPEG_422 ? 2 : 1;
    L->vmax = sampling == MVLDM_JPEG_420 ? 2 : 1;
    L->mcux = (w + 8 * L->hmax - 1) / (8 * L->hmax);
    L->mcuy = (h + 8 * L->vmax - 1) / (8 * L->vmax);
    int at = 0;
    for (int c = 0; c < 3; ++c) {
        const int hs = c == 0 ? L->hmax : 1, vs = c == 0 ? L->vmax : 1;
        const bool on = c < L->ncomp;
        L->bw[c] = on ? L->mcux * hs : 0;
        L->bh[c] = on ? L->mcuy * vs : 0;
        L->cw[c] = on ? (w * hs + L->hmax - 1) / L->hmax : 0;
        L->ch[c] = on ? (h * vs + L->vmax - 1) / L->vmax : 0;
        L->off[c] = at;
        at += L->bw[c] * L->bh[c];
    }
    L->blocks = at;
    return true;
}

// ---- jidctint.c, ISLOW: CONST_BITS = 13, PASS1_BITS = 2 ----------------------------------------------------------------------------
// One 1-D pass over v[0..7] in place, DESCALE by `shift` (11 for the columns, 18 for the rows).  The zero-AC shortcut of the column
// pass gives the same values ((in0 << 13) + 2^10) >> 11 = in0 << 2) and is not taken.  Multiplies wrap like libjpeg-turbo's pmaddwd on
// inputs outside the guard (unsigned arithmetic: no undefined overflow on the host).
MVLDM_HD int32_t jpeg_mul(int32_t a, int32_t k) { return (int32_t)((uint32_t)a * (uint32_t)k); }
MVLDM_HD int32_t jpeg_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
MVLDM_HD int32_t jpeg_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
MVLDM_HD int32_t jpeg_shl(int32_t a, int n) { return (int32_t)((uint32_t)a << n); }
MVLDM_HD int32_t jpeg_descale(int32_t x, int n) { return jpeg_add(x, 1 << (n - 1)) >> n; }

MVLDM_HD void jpeg_idct_1d(int32_t* v, int shift) {
    // even part
    int32_t z2 = v[2], z3 = v[6];
    int32_t z1 = jpeg_mul(jpeg_add(z2, z3), 4433);                  // FIX(0.541196100)
    int32_t tmp2 = jpeg_sub(z1, jpeg_mul(z3, 15137));               // FIX(1.847759065)
    int32_t tmp3 = jpeg_add(z1, jpeg_mul(z2, 6270));                // FIX(0.765366865)
    int32_t tmp0 = jpeg_shl(jpeg_add(v[0], v[4]), 13);
    int32_t tmp1 = jpeg_shl(jpeg_sub(v[0], v[4]), 13);
    const int32_t tmp10 = jpeg_add(tmp0, tmp3), tmp13 = jpeg_sub(tmp0, tmp3);
    const int32_t tmp11 = jpeg_add(tmp1, tmp2), tmp12 = jpeg_sub(tmp1, tmp2);
    // odd part
    tmp0 = v[7];
    tmp1 = v[5];
    tmp2 = v[3];
    tmp3 = v[1];
    z1 = jpeg_add(tmp0, tmp3);
    z2 = jpeg_add(tmp1, tmp2);
    z3 = jpeg_add(tmp0, tmp2);
    int32_t z4 = jpeg_add(tmp1, tmp3);
    const int32_t z5 = jpeg_mul(jpeg_add(z3, z4), 9633);            // FIX(1.175875602)
    tmp0 = jpeg_mul(tmp0, 2446);                                    // FIX(0.298631336)
    tmp1 = jpeg_mul(tmp1, 16819);                                   // FIX(2.053119869)
    tmp2 = jpeg_mul(tmp2, 25172);                                   // FIX(3.072711026)
    tmp3 = jpeg_mul(tmp3, 12299);                                   // FIX(1.501321110)
    z1 = jpeg_mul(z1, -7373);                                       // FIX(0.899976223)
    z2 = jpeg_mul(z2, -20995);                                      // FIX(2.562915447)
    z3 = jpeg_add(jpeg_mul(z3, -16069), z5);                        // FIX(1.961570560)
    z4 = jpeg_add(jpeg_mul(z4, -3196), z5);                         // FIX(0.390180644)
    tmp0 = jpeg_add(tmp0, jpeg_add(z1, z3));
    tmp1 = jpeg_add(tmp1, jpeg_add(z2, z4));
    tmp2 = jpeg_add(tmp2, jpeg_add(z2, z3));
    tmp3 = jpeg_add(tmp3, jpeg_add(z1, z4));
    v[0] = jpeg_descale(jpeg_add(tmp10, tmp3), shift);
    v[7] = jpeg_descale(jpeg_sub(tmp10, tmp3), shift);
    v[1] = jpeg_descale(jpeg_add(tmp11, tmp2), shift);
    v[6] = jpeg_descale(jpeg_sub(tmp11, tmp2), shift);
    v[2] = jpeg_descale(jpeg_add(tmp12, tmp1), shift);
    v[5] = jpeg_descale(jpeg_sub(tmp12, tmp1), shift);
    v[3] = jpeg_descale(jpeg_add(tmp13, tmp0), shift);
    v[4] = jpeg_descale(jpeg_sub(tmp13, tmp0), shift);
}
MVLDM_HD uint32_t jpeg_sample(int32_t x) {     // the saturating pack: clip(x + 128, 0, 255)
    x = jpeg_add(x, 128);
    return (uint32_t)(x < 0 ? 0 : x > 255 ? 255 : x);
}

// ---- jdsample.c (fancy upsampling) and jdcolor.c -----------------------------------------------------------------------------------
// One chroma sample of output pixel (y, x) from the component's plane (row stride `ld`, real size ch x cw).  libjpeg takes the
// triangle filters only for components more than two samples wide (jinit_upsampler: downsampled_width > 2) and replicates otherwise.
MVLDM_HD int jpeg_chroma(const uint8_t* plane, int ld, int ch, int cw, int hmax, int vmax, int y, int x) {
    if (hmax == 1) return plane[(size_t)y * ld + x];
    const int i = x >> 1;
    if (vmax == 1) {                            // h2v1
        const uint8_t* r = plane + (size_t)y * ld;
        if (cw <= 2) return r[i];
        if (x & 1) return i == cw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
        return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
    }
    const int cy = y >> 1;                      // h2v2
    if (cw <= 2) return plane[(size_t)cy * ld + i];
    int fy = (y & 1) ? cy + 1 : cy - 1;         // the far row; beyond the first / last real row it is that row
    fy = fy < 0 ? 0 : fy > ch - 1 ? ch - 1 : fy;
    const uint8_t* near = plane + (size_t)cy * ld;
    const uint8_t* far = plane + (size_t)fy * ld;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}
MVLDM_HD int jpeg_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// the three bytes of a pixel in bits 0-23 (R lowest): jdcolor.c's tables, SCALEBITS = 16, arithmetic shifts
MVLDM_HD uint32_t jpeg_rgb(int yy, int cb, int cr) {
    cb -= 128;
    cr -= 128;
    const int r = jpeg_clip8(yy + ((91881 * cr + 32768) >> 16));
    const int g = jpeg_clip8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const int b = jpeg_clip8(yy + ((116130 * cb + 32768) >> 16));
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}
// pixel (y, x) of a frame from its planes
MVLDM_HD uint32_t jpeg_pixel(const uint8_t* planes, const JpegLayout& L, int y, int x) {
    const int yy = planes[(size_t)y * (L.bw[0] * 8) + x];
    if (L.ncomp == 1) return (uint32_t)yy * 0x010101u;
    const int cb = jpeg_chroma(planes + (size_t)L.off[1] * 64, L.bw[1] * 8, L.ch[1], L.cw[1], L.hmax, L.vmax, y, x);
    const int cr = jpeg_chroma(planes + (size_t)L.off[2] * 64, L.bw[2] * 8, L.ch[2], L.cw[2], L.hmax, L.vmax, y, x);
    return jpeg_rgb(yy, cb, cr);
}

}  // namespace mvldm
