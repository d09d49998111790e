// VQ/SQ (tensor-core packing) fused decode + skinny GEMM for batches 17..64 (512-thread workgroups).
#include "gemv_launch.h"
#include "lut_kernels_api.h"

namespace qpal {

int launch_lut_tc_gemv_wide(const TcMultiParams &p, int bits, int vec, int nbg, int grid, hipStream_t stream) {
#define QPAL_LUT(B_, V_)                                                                                       \
    if (bits == B_ && vec == V_) {                                                                             \
        if (nbg == 4) {                                                                                        \
            return launch_gemv<LutCodec<B_, V_>, void, 4>(p, grid, stream);                                    \
        } else if constexpr (LutCodec<B_, V_>::LDS_DWORDS * 4 <= 64 * 1024) {  /* 8 groups: 64 KiB reduction buffer */ \
            return launch_gemv<LutCodec<B_, V_>, void, 8>(p, grid, stream);                                    \
        } else {                                                                                               \
            return QPAL_E_SHAPE;                                                                               \
        }                                                                                                      \
    }
#include "lut_table.inc"
#undef QPAL_LUT
    return QPAL_E_PARAM;
}

}  // namespace qpal
