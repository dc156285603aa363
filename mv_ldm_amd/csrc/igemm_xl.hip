// Implicit GEMM, tiles 9, 10 and 18 (256 x 256, 256 x 320, and the deep-ring 192 x 128: one workgroup fills the CU's LDS): igemm_bl_kernel
// only, 16-bit types only.
#include "igemm_bl.h"

namespace mvldm {

int igemm_launch_xl(const IgemmParams& p, int tile, int act_dtype, hipStream_t s) {
    if (tile == 18) {
        // (deep-ring forms of tiles 2 / 4 -- 128x64 with 5 slots, 64x64 with 6 -- were built and measured SLOWER than their 2-slot forms on every
        //  one-scene shape (tools/skinny_probe.py: 25.2 / 30.2 us against 22.0 / 21.8 on the 4x4-level conv): several 2-slot
        //  workgroups per CU already overlap each other's round trips; not instantiated)
        // (GEGLU pairs a value block with the gate block 32 columns on INSIDE a wave's tile: a 32-column wave tile cannot -- refused,
        //  never remapped.  The first build let it through; the epilogue then read the neighbouring wave's parked block, which is the
        //  right one whenever that wave had already parked it: correct in most runs, different between eager and graph replay.)
        if (p.epilogue == MVLDM_EPI_GEGLU) return set_error(MVLDM_ERR_UNSUPPORTED, "igemm: tile 18 does not take the GEGLU epilogue");
        if (act_dtype == MVLDM_F32 || !p.use_bl || p.upsample)
            return set_error(MVLDM_ERR_ARG, "igemm: tile 18 needs the 16-bit block-major path (no upsampling forms)");
    } else if (int rc = require_bl(p, tile, act_dtype)) {
        return rc;
    }
    return dispatch_16bit(act_dtype, [&](auto t) {
        using T = decltype(t);
        switch (tile) {
            case 9: return launch_bl_any<T, 256, 256, 4, 2>(p, s);
            case 10: return launch_bl_any<T, 256, 320, 4, 2>(p, s);
            case 18: return launch_bl_deep<T, 192, 128, 2, 4, 4>(p, s);
            default: return set_error(MVLDM_ERR_ARG, "igemm: bad tile %d", tile);
        }
    });
}

}  // namespace mvldm
