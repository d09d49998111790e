// One translation unit per batch-group count (parallel compile): #define QPAL_GEMM_NBG before including.
#include "tc_gemm16.h"
#include "tcq_kernels_api.h"

namespace qpal {

#define QPAL_CAT2(a, b) a##b
#define QPAL_CAT(a, b) QPAL_CAT2(a, b)
int QPAL_CAT(launch_tcq_gemm_nbg, QPAL_GEMM_NBG)(const TcMultiParams &p, int S, int KV1, int KV2, int grid, hipStream_t stream) {
// QPAL_GEMM_NBG = 1, 2: batches <= 8 / 16; 4, 8, 10, 16: batches <= 32 / 64 / 80 / 128 (the fragment mapping: gemm_map, tc_gemm16.h)
#define QPAL_TCQ(S_, A_, B_)                                                                                              \
    if (S == S_ && KV1 == A_ && KV2 == B_) {                                                                              \
        using C1 = TcqCodec<S_, A_, 0>;                                                                                   \
        using C2 = std::conditional_t<B_ == 0, void, TcqCodec<S_, B_ == 0 ? A_ : B_, 0>>;                                 \
        hipLaunchKernelGGL((tc_gemm_kernel<C1, C2, gemm_map<QPAL_GEMM_NBG>>), dim3(grid), dim3(64 * kGemmWaves), 0, stream, gemm_item_table(p), p); \
        return (int)hipGetLastError();                                                                                    \
    }
#include "tcq_table.inc"
#undef QPAL_TCQ
    return QPAL_E_PARAM;
}

}  // namespace qpal
