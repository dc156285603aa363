// Implicit GEMM, tiles 1 - 5 (workgroups of 1 - 4 waves): igemm_kernel for the three dtypes, igemm_bl_kernel for the two 16-bit ones.
#include "igemm_bl.h"

namespace mvldm {

int igemm_launch_small(const IgemmParams& p, int tile, int act_dtype, hipStream_t s) {
    return dispatch_dtype(act_dtype, [&](auto t) {
        using T = decltype(t);
        switch (tile) {
            case 1: return launch_tile<T, 128, 128, 2, 2>(p, s);
            case 2: return launch_tile<T, 128, 64, 4, 1>(p, s);
            case 3: return launch_tile<T, 64, 128, 2, 2>(p, s);
            case 4: return launch_tile<T, 64, 64, 2, 1>(p, s);
            case 5: return launch_tile<T, 32, 64, 1, 1>(p, s);
            default: return set_error(MVLDM_ERR_ARG, "igemm: bad tile %d", tile);
        }
    });
}

}  // namespace mvldm
