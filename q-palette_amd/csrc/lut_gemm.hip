// VQ/SQ (tensor-core packing) fused decode + skinny GEMM with the step's activations shared through LDS (tc_gemm.h).
#include "tc_gemm16.h"
#include "lut_kernels_api.h"

namespace qpal {

int launch_lut_tc_gemm(const TcMultiParams &p, int bits, int vec, int nbg, int grid, hipStream_t stream) {
// nbg batch groups of 8 rows (the fragment mapping: gemm_map, tc_gemm16.h); from 4 groups on only where the codebook image leaves room
// for two x tiles
#define QPAL_GEMM(NBG_)                                                                                                    \
    hipLaunchKernelGGL((tc_gemm_kernel<C, void, gemm_map<NBG_>>), dim3(grid), dim3(64 * kGemmWaves), 0, stream, gemm_item_table(p), p);
#define QPAL_GEMM_IF_FITS(NBG_)                                                                                            \
    if constexpr (C::LDS_DWORDS * 4 + 2 * gemm_map<NBG_>::XBUF <= 160 * 1024) { QPAL_GEMM(NBG_) }                          \
    else return QPAL_E_SHAPE;
#define QPAL_LUT(B_, V_)                                                                                                   \
    if (bits == B_ && vec == V_) {                                                                                         \
        using C = LutCodec<B_, V_>;                                                                                        \
        if (nbg == 1) { QPAL_GEMM(1) }                                                                                     \
        else if (nbg == 2) { QPAL_GEMM(2) }                                                                                \
        else if (nbg == 4) { QPAL_GEMM_IF_FITS(4) }                                                                        \
        else if (nbg == 8) { QPAL_GEMM_IF_FITS(8) }                                                                        \
        else if (nbg == 10) { QPAL_GEMM_IF_FITS(10) }                                                                      \
        else { QPAL_GEMM_IF_FITS(16) }                                                                                     \
        return (int)hipGetLastError();                                                                                     \
    }
#include "lut_table.inc"
#undef QPAL_LUT
#undef QPAL_GEMM_IF_FITS
#undef QPAL_GEMM
    return QPAL_E_PARAM;
}

}  // namespace qpal
