// PNG frames on the device: row unfiltering (None / Sub / Up / Average / Paeth) and expansion to RGB (include/mvldm.h, "PNG frames").
// One wave per frame.  Average and Paeth are serial along a row, and a row needs the one above, which leaves a skewed wavefront: in a band
// of 64 rows lane r reconstructs unit t - r at step t (a unit is one pixel, or one byte of pixels below 8 bits), and the two units of the
// row above it needs -- above and above-left -- are lane r - 1's result of step t - 1 and of step t - 2: one lane shift per step, no memory
// round trip.  A band's last row waits in LDS (one word per unit) for lane 0 of the next band.  The kernel is latency-bound by construction
// (a frame is one serial chain of about (units + 63) * bands steps) and a batch of 64 frames is 64 waves: DESIGN.md 3.8.
#include "common.h"
#include "png_common.h"

namespace mvldm {

constexpr int kPngAhead = 8;        // steps whose filtered bytes are loaded ahead of the chain: the loads of a block fly while the previous one is reconstructed

// the filtered unit u of a row, byte k in bits 8k .. 8k + 7; 0 outside the row.  Rows start at any byte: byte loads.
template <int BPP> __device__ __forceinline__ uint32_t png_load_unit(const uint8_t* __restrict__ rowp, int u, int units, bool active) {
    uint32_t x = 0;
    if (active && u >= 0 && u < units) {
        const uint8_t* p = rowp + 1 + (size_t)u * BPP;
#pragma unroll
        for (int k = 0; k < BPP; ++k) x |= (uint32_t)p[k] << (8 * k);
    }
    return x;
}

template <int BPP>
__device__ __forceinline__ int png_frame(const uint8_t* __restrict__ src, int ctype, int depth, void* __restrict__ dst, int kind, size_t img, int h, int w,
                                         const uint32_t* pal, uint32_t* prev) {
    const int lane = (int)threadIdx.x;
    const size_t stride = png_stride(w, ctype, depth);
    const int units = (int)(stride / BPP);                  // 8-bit formats: pixels; below: bytes
    int miss = 0;
    for (int band0 = 0; band0 < h; band0 += WAVE) {
        const int rows = h - band0 < WAVE ? h - band0 : WAVE;
        const int row = band0 + lane;
        const bool active = lane < rows;
        const uint8_t* rowp = src + (size_t)(active ? row : band0) * (1 + stride);
        uint32_t ft = active ? rowp[0] : 0u;
        ft = ft > 4u ? 0u : ft;
        const bool more = band0 + WAVE < h;                 // another band follows: lane 63 leaves its row in LDS
        const int steps = units + rows - 1;
        uint32_t last = 0, b = 0;                           // my previous unit (a); the row above at my unit (b) -- c is the b of the step before
        const bool from_lds = lane == 0 && band0 > 0;       // lane 0's row above is the previous band's last row.  Its words are read a block ahead
        uint32_t nxt[kPngAhead], nup[kPngAhead];            // too: word t is only overwritten at step t + 63 of this band, long after it was used
#pragma unroll
        for (int j = 0; j < kPngAhead; ++j) {
            nxt[j] = png_load_unit<BPP>(rowp, j - lane, units, active);
            nup[j] = (from_lds && j < units) ? prev[j] : 0u;
        }
        for (int t0 = 0; t0 < steps; t0 += kPngAhead) {
            uint32_t cur[kPngAhead], cup[kPngAhead];
#pragma unroll
            for (int j = 0; j < kPngAhead; ++j) {
                const int tt = t0 + kPngAhead + j;
                cur[j] = nxt[j];
                cup[j] = nup[j];
                nxt[j] = png_load_unit<BPP>(rowp, tt - lane, units, active);
                nup[j] = (from_lds && tt < units) ? prev[tt] : 0u;
            }
#pragma unroll
            for (int j = 0; j < kPngAhead; ++j) {
                const int t = t0 + j, u = t - lane;
                uint32_t up = (uint32_t)__shfl_up((int)last, 1, WAVE);
                if (lane == 0) up = cup[j];
                const uint32_t c = b;
                b = up;
                if (active && u >= 0 && u < units) {
                    last = png_recon_unit<BPP>(ft, cur[j], last, b, c);
                    miss |= png_emit_unit(dst, kind, img, h, w, row, u, last, ctype, depth, pal);
                    if (more && lane == WAVE - 1) prev[u] = last;
                }
            }
        }
        __syncthreads();                                    // one wave: orders this band's LDS row before the next band reads it
    }
    return miss;
}

__global__ __launch_bounds__(WAVE) void png_unfilter_kernel(const uint8_t* __restrict__ streams, size_t stream_bytes, const int32_t* __restrict__ desc,
                                                            const uint8_t* __restrict__ palettes, size_t palette_bytes, void* __restrict__ dst, int kind, int h, int w,
                                                            int32_t* __restrict__ status) {
    extern __shared__ uint32_t png_lds[];                   // [256] palette slots, then [w] the last row of a band
    uint32_t* pal = png_lds;
    uint32_t* prev = png_lds + 256;
    const size_t img = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int32_t* d = desc + img * kPngDescInts;
    if (!png_desc_ok(d, stream_bytes, palette_bytes, h, w)) {   // uniform in the workgroup: nothing of the frame is read, nothing written
        if (lane == 0) status[img] = MVLDM_PNG_DESC;
        return;
    }
    const int ctype = d[1], depth = d[2];
    if (ctype == 3) {
        for (int i = lane; i < 256; i += WAVE) pal[i] = png_pal_slot(palettes + d[3], d[4], i);
    }
    __syncthreads();
    const uint8_t* src = streams + (size_t)d[0];
    int miss;
    switch (png_bpp(ctype, depth)) {
        case 1: miss = png_frame<1>(src, ctype, depth, dst, kind, img, h, w, pal, prev); break;
        case 2: miss = png_frame<2>(src, ctype, depth, dst, kind, img, h, w, pal, prev); break;
        case 3: miss = png_frame<3>(src, ctype, depth, dst, kind, img, h, w, pal, prev); break;
        default: miss = png_frame<4>(src, ctype, depth, dst, kind, img, h, w, pal, prev); break;
    }
    const int any_miss = __any(miss);
    if (lane == 0) status[img] = any_miss ? MVLDM_PNG_PALETTE_INDEX : MVLDM_PNG_OK;
}

int png_unfilter(const uint8_t* streams, size_t stream_bytes, const int32_t* desc, const uint8_t* palettes, size_t palette_bytes, void* dst, int dst_kind,
                 int n_img, int h, int w, int32_t* status, hipStream_t s) {
    MVLDM_REQUIRE(n_img >= 0, "png_unfilter: n_img %d", n_img);
    MVLDM_REQUIRE(png_dims_ok(h, w), "png_unfilter: frame %d x %d (edges 1 .. %d)", h, w, kPngMaxDim);
    MVLDM_REQUIRE(dst_kind == MVLDM_PNG_DST_U8 || dst_kind == MVLDM_PNG_DST_F32, "png_unfilter: dst_kind %d", dst_kind);
    if (n_img == 0) return MVLDM_OK;
    MVLDM_REQUIRE(streams != nullptr && dst != nullptr && aligned(desc, 4) && aligned(status, 4) && (palettes != nullptr || palette_bytes == 0),
                  "png_unfilter: null or unaligned pointer (desc, status: 4 bytes)");
    MVLDM_REQUIRE(dst_kind == MVLDM_PNG_DST_U8 || aligned(dst, 4), "png_unfilter: a float dst is 4-byte aligned");
    MVLDM_REQUIRE(stream_bytes <= 0x7FFFFFFFu && palette_bytes <= 0x7FFFFFFFu, "png_unfilter: %zu bytes of streams, %zu of palettes (below 2^31)", stream_bytes,
                  palette_bytes);
    const int smem = (256 + w) * (int)sizeof(uint32_t);
    static std::atomic<uint64_t> done{0};
    if (int rc = ensure_dyn_smem((const void*)png_unfilter_kernel, smem, done)) return rc;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n_img), dim3(WAVE), smem, s, streams, stream_bytes, desc, palettes, palette_bytes, dst, dst_kind, h, w,
                       status);
    return check_launch();
}

}  // namespace mvldm

using namespace mvldm;
extern "C" int mvldm_png_unfilter(const uint8_t* streams, size_t stream_bytes, const int32_t* desc, const uint8_t* palettes, size_t palette_bytes, void* dst,
                                  int dst_kind, int n_img, int h, int w, int32_t* status, mvldm_stream_t stream) {
    return png_unfilter(streams, stream_bytes, desc, palettes, palette_bytes, dst, dst_kind, n_img, h, w, status, (hipStream_t)stream);
}
