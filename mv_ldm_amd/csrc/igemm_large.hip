// Implicit GEMM, tiles 6 - 8 (256 x 64, 256 x 128, 128 x 256): igemm_bl_kernel only, 16-bit types only.
#include "igemm_bl.h"

namespace mvldm {

int igemm_launch_large(const IgemmParams& p, int tile, int act_dtype, hipStream_t s) {
    if (int rc = require_bl(p, tile, act_dtype)) return rc;
    return dispatch_16bit(act_dtype, [&](auto t) {
        using T = decltype(t);
        switch (tile) {
            case 6: return launch_bl_any<T, 256, 64, 4, 1>(p, s);
            case 7: return launch_bl_any<T, 256, 128, 4, 2>(p, s);
            case 8: return launch_bl_any<T, 128, 256, 2, 4>(p, s);
            default: return set_error(MVLDM_ERR_ARG, "igemm: bad tile %d", tile);
        }
    });
}

}  // namespace mvldm
