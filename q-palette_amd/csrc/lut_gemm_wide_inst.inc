// One translation unit per (NG, vec) (parallel compile): #define QPAL_WIDE_NG and QPAL_WIDE_VEC before including.
#include "lut_gemm_wide.h"

namespace qpal {

#define QPAL_CAT3_(a, b, c, d) a##b##c##d
#define QPAL_CAT3(a, b, c, d) QPAL_CAT3_(a, b, c, d)
int QPAL_CAT3(launch_lut_gemm_wide_ng, QPAL_WIDE_NG, _v, QPAL_WIDE_VEC)(const LutWideParams &p, int bits, int grid, hipStream_t stream) {
    // (the codecs of the other vec are discarded inside a generic lambda: never instantiated here)
    auto launch = [&](auto bc, auto vc) {
        if constexpr (decltype(vc)::value == QPAL_WIDE_VEC) {
            using C = LutCodec<decltype(bc)::value, decltype(vc)::value, kLutWideCapLog2>;
            hipLaunchKernelGGL((lut_gemm_wide_kernel<C, QPAL_WIDE_NG>), dim3(grid), dim3(kWdThreads), 0, stream, p);
        }
    };
#define QPAL_LUT(B_, V_)                                                                                  \
    if (bits == B_ && V_ == QPAL_WIDE_VEC) {                                                              \
        launch(std::integral_constant<int, B_>{}, std::integral_constant<int, V_>{});                     \
        return (int)hipGetLastError();                                                                    \
    }
#include "lut_table.inc"
#undef QPAL_LUT
    return QPAL_E_PARAM;
}

}  // namespace qpal
