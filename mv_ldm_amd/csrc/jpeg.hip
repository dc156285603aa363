// The device half of the JPEG decoder (include/mvldm.h, "JPEG frames"): the quantised coefficients the host's entropy decoder wrote
// (jpeg_host.cpp) become the bytes Pillow's `Image.open(...).convert("RGB")` gives.  All arithmetic is the integer arithmetic of
// jpeg_common.h, shared with mvldm_jpeg_idct_host.
//   jpeg_idct_kernel   8 lanes per 8 x 8 block, 8 blocks per wave, 32 per workgroup; a block is block g of [n_img][blocks per frame].
//                      Lane r of a block loads ROW r of it -- 8 int16 in one 16-byte load, so a wave reads 1 KiB contiguous -- and the
//                      same row of the component's table, multiplies in int32 and leaves the row in LDS.  Lane c then reads COLUMN c
//                      (the transpose is the LDS read: blocks are 72 dwords apart, so the 32 lanes of a ds_read_b32 group hit 32
//                      banks), runs the column pass in registers, writes the column back, and lane r reads row r for the row pass.
//                      The 8 samples of the row go out as two dwords of the component's plane.  The 8 lanes of a block share a wave;
//                      the barriers between the three LDS phases are workgroup barriers all the same (every lane reaches them).
//   jpeg_color_kernel  one lane per 4 consecutive pixels of dst taken as a flat [n_img h w] list: 12 bytes = three aligned dwords
//                      whatever h and w are.  Per pixel: the luma byte, the two chroma samples through the triangle filters on the
//                      component's real size, jdcolor's fixed-point conversion.
#include "common.h"
#include "jpeg_common.h"

namespace mvldm {

constexpr int kJpegBlockLd = 72;            // dwords between the blocks of a workgroup in LDS: 64 + 8

template <bool VEC>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, uint8_t* __restrict__ planes,
                                                        JpegLayout L, unsigned total) {
    __shared__ int32_t tile[32 * kJpegBlockLd];
    const unsigned slot = threadIdx.x >> 3, r = threadIdx.x & 7;
    const unsigned g = blockIdx.x * 32u + slot;
    const bool live = g < total;
    const unsigned img = live ? g / (unsigned)L.blocks : 0u, bi = live ? g % (unsigned)L.blocks : 0u;
    const int c = bi >= (unsigned)L.off[2] && L.ncomp == 3 ? 2 : bi >= (unsigned)L.off[1] && L.ncomp == 3 ? 1 : 0;
    const unsigned off_c = c == 2 ? (unsigned)L.off[2] : c == 1 ? (unsigned)L.off[1] : 0u;     // selects, not L.off[c]: a runtime index
    const unsigned bw_c = c == 0 ? (unsigned)L.bw[0] : (unsigned)L.bw[1];                       // into the argument struct would go to scratch
    int32_t* mine = tile + slot * kJpegBlockLd;
    int32_t v[8];
    if (live) {
        const int16_t* src = coef + ((size_t)g * 64 + r * 8);
        const uint16_t* q = qt + ((size_t)img * 192 + c * 64 + r * 8);
        uint32_t cw[4], qw[4];
        if (VEC) {
            const u32x4 a = *(const u32x4*)src, b = *(const u32x4*)q;
            cw[0] = a.x, cw[1] = a.y, cw[2] = a.z, cw[3] = a.w;
            qw[0] = b.x, qw[1] = b.y, qw[2] = b.z, qw[3] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cw[j] = ((const uint32_t*)src)[j];
                qw[j] = ((const uint32_t*)q)[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = (int32_t)(int16_t)(cw[j] & 0xFFFFu) * (int32_t)(qw[j] & 0xFFFFu);
            v[2 * j + 1] = ((int32_t)cw[j] >> 16) * (int32_t)(qw[j] >> 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) mine[r * 8 + j] = v[j];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = mine[k * 8 + r];         // column r
    jpeg_idct_1d(v, 11);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[k * 8 + r] = v[k];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = mine[r * 8 + j];         // row r
    jpeg_idct_1d(v, 18);
    if (live) {
        const unsigned bc = bi - off_c;
        const unsigned by = bc / bw_c, bx = bc % bw_c;
        uint8_t* out = planes + ((size_t)img * L.blocks + off_c) * 64 + (size_t)(by * 8 + r) * (bw_c * 8) + bx * 8;
        const uint32_t lo = jpeg_sample(v[0]) | (jpeg_sample(v[1]) << 8) | (jpeg_sample(v[2]) << 16) | (jpeg_sample(v[3]) << 24);
        const uint32_t hi = jpeg_sample(v[4]) | (jpeg_sample(v[5]) << 8) | (jpeg_sample(v[6]) << 16) | (jpeg_sample(v[7]) << 24);
        if (VEC) {
            *(u32x2*)out = u32x2{lo, hi};
        } else {
            ((uint32_t*)out)[0] = lo;
            ((uint32_t*)out)[1] = hi;
        }
    }
}

// Lane t: pixels 4 t .. 4 t + 3 of the flat list; `pixels` = n_img h w.  The last lane may hold fewer than 4: it stores bytes.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst, JpegLayout L, int h, int w,
                                                         size_t pixels) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t p0 = t * 4;
    if (p0 >= pixels) return;
    const size_t per = (size_t)h * w;
    size_t img = p0 / per;
    const unsigned rem = (unsigned)(p0 % per);      // h, w <= 16384
    int y = (int)(rem / (unsigned)w), x = (int)(rem % (unsigned)w);
    uint32_t px[4] = {0, 0, 0, 0};
    int count = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p0 + j < pixels) {
            px[j] = jpeg_pixel(planes + img * (size_t)L.blocks * 64, L, y, x);
            ++count;
            if (++x == w) {
                x = 0;
                if (++y == h) {
                    y = 0;
                    ++img;
                }
            }
        }
    }
    uint8_t* out = dst + p0 * 3;
    if (count == 4) {
        uint32_t* o = (uint32_t*)out;
        o[0] = px[0] | (px[1] << 24);
        o[1] = (px[1] >> 8) | (px[2] << 16);
        o[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int j = 0; j < count; ++j) {
            out[3 * j] = (uint8_t)px[j];
            out[3 * j + 1] = (uint8_t)(px[j] >> 8);
            out[3 * j + 2] = (uint8_t)(px[j] >> 16);
        }
    }
}

size_t jpeg_workspace_bytes(int n_img, int h, int w, int sampling) {
    JpegLayout L;
    if (n_img < 1 || !jpeg_layout(h, w, sampling, &L)) return 0;
    return (size_t)n_img * L.blocks * 64;
}

int jpeg_decode(const int16_t* coef, const uint16_t* qt, uint8_t* dst, int n_img, int h, int w, int sampling, void* ws, size_t ws_bytes, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "jpeg_decode: n_img %d", n_img);
    JpegLayout L;
    MVLDM_REQUIRE(jpeg_layout(h, w, sampling, &L), "jpeg_decode: frame %d x %d, sampling %d (edges 1 .. %d, sampling 0 .. 3)", h, w, sampling, kJpegMaxDim);
    if (n_img == 0) return MVLDM_OK;
    const size_t need = (size_t)n_img * L.blocks * 64;
    MVLDM_REQUIRE(ws_bytes >= need, "jpeg_decode: workspace of %zu bytes, need %zu", ws_bytes, need);
    MVLDM_REQUIRE(aligned(coef, 4) && aligned(qt, 4) && aligned(dst, 4) && aligned(ws, 4), "jpeg_decode: null or unaligned pointer (4 bytes)");
    const size_t total = (size_t)n_img * L.blocks, pixels = (size_t)n_img * h * w;
    const size_t g1 = (total + 31) / 32, g2 = (pixels + 1023) / 1024;
    MVLDM_REQUIRE(total <= 0x7FFFFFFFu && g2 <= 0x7FFFFFFFu, "jpeg_decode: %zu blocks, %zu pixels", total, pixels);
    uint8_t* planes = (uint8_t*)ws;
    if (aligned(coef, 16) && aligned(qt, 16) && aligned(ws, 8))
        hipLaunchKernelGGL(jpeg_idct_kernel<true>, dim3((unsigned)g1), dim3(256), 0, s, coef, qt, planes, L, (unsigned)total);
    else
        hipLaunchKernelGGL(jpeg_idct_kernel<false>, dim3((unsigned)g1), dim3(256), 0, s, coef, qt, planes, L, (unsigned)total);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)g2), dim3(256), 0, s, (const uint8_t*)planes, dst, L, h, w, pixels);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" size_t mvldm_jpeg_workspace_bytes(int n_img, int h, int w, int sampling) { return jpeg_workspace_bytes(n_img, h, w, sampling); }
extern "C" int mvldm_jpeg_decode(const int16_t* coef, const uint16_t* qt, uint8_t* dst, int n_img, int h, int w, int sampling, void* workspace,
                                 size_t workspace_bytes, mvldm_stream_t stream) {
    return jpeg_decode(coef, qt, dst, n_img, h, w, sampling, workspace, workspace_bytes, (hipStream_t)stream);
}
