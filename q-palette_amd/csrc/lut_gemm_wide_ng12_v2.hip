// VQ/SQ wide dequant GEMM (lut_gemm_wide.h): the vec 2 codecs at 12 groups of 16 batch rows.
#define QPAL_WIDE_NG 12
#define QPAL_WIDE_VEC 2
#include "lut_gemm_wide_inst.inc"
