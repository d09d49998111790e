// The 8-bit KV-cache element: OCP e4m3fn (torch.float8_e4m3fn; not the MI300 fnuz encoding), one byte, no scale.
//   store: fp16 -> fp32, clamped to [-448, 448] in fp32 BEFORE the convert instruction (its overflow behaviour is never relied on),
//          round to nearest even, subnormals kept: h.float().clamp(-448, 448).to(torch.float8_e4m3fn).  NaN: unspecified.
//   load:  exact (every e4m3 value, subnormals included, is a normal fp16 value).
// gfx950 converts two elements per instruction in both directions.
#pragma once
#include "qpal_common.h"

namespace qpal {

typedef _Float16 kv8_half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 kv8_half8_t __attribute__((ext_vector_type(8)));
typedef float kv8_float2_t __attribute__((ext_vector_type(2)));

// cache element type -> is it the one-byte format
template <class CT>
inline constexpr bool kIsKv8 = sizeof(CT) == 1;

// two fp16 values -> their e4m3fn bytes in bits 0..7 (a) and 8..15 (b)
__device__ __forceinline__ uint32_t e4m3_pack2(_Float16 a, _Float16 b) {
    const float fa = __builtin_amdgcn_fmed3f((float)a, -448.f, 448.f), fb = __builtin_amdgcn_fmed3f((float)b, -448.f, 448.f);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(fa, fb, 0, false) & 0xffffu;
}
// eight fp16 values (four dwords) -> eight bytes
__device__ __forceinline__ u32x2 e4m3_pack8(u32x4 h) {
    const kv8_half8_t v = __builtin_bit_cast(kv8_half8_t, h);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] = __builtin_amdgcn_fmed3f((float)v[e], -448.f, 448.f);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false), hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    return u32x2{(uint32_t)lo, (uint32_t)hi};
}
// bytes 2 HI, 2 HI + 1 of w -> two fp16 values (one dword), exact
template <bool HI>
__device__ __forceinline__ uint32_t e4m3_half2(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, 1.0f, HI));
}
// eight bytes -> eight fp16 values
__device__ __forceinline__ u32x4 e4m3_half8(u32x2 w) {
    return u32x4{e4m3_half2<false>(w.x), e4m3_half2<true>(w.x), e4m3_half2<false>(w.y), e4m3_half2<true>(w.y)};
}
// bytes 2 HI, 2 HI + 1 of w -> fp32 (= the fp32 value of their fp16 image)
template <bool HI>
__device__ __forceinline__ kv8_float2_t e4m3_float2(uint32_t w) {
    return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
}

}  // namespace qpal
