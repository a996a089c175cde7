// OCP e4m3fn helpers shared by the fp8 KV cache (attention_decode.hip) and the fp8-weight decode GEMV (gemm_skinny.hip).
// Both quantize a vector x as amax = max|x|, inv = 448 / amax, q = e4m3(RNE(x * inv)), scale = amax / 448 (include/gar_hip.h).
#pragma once
#include "common.h"

#define FP8_MAX 448.0f

// four f32 (already times inv) -> four e4m3 bytes, byte i = element i (v_cvt_pk_fp8_f32: round to nearest even)
__device__ __forceinline__ unsigned int pk4_fp8(float a, float b, float c, float d) {
    const int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return (unsigned int)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}
// eight e4m3 bytes -> the MFMA operand of the 16-bit type (exact: e4m3 values are bf16 / fp16 values)
__device__ __forceinline__ bf16x8 fp8x8_to_h16(u32x2 w) {
#if GAR_HALF_F16
    const h16x2_hw_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w[0], 1.0f, false);
    const h16x2_hw_t b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w[0], 1.0f, true);
    const h16x2_hw_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w[1], 1.0f, false);
    const h16x2_hw_t d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w[1], 1.0f, true);
#else
    const bf16x2_hw_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[0], 1.0f, false);
    const bf16x2_hw_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[0], 1.0f, true);
    const bf16x2_hw_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[1], 1.0f, false);
    const bf16x2_hw_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[1], 1.0f, true);
#endif
    const u32x4 r = {__builtin_bit_cast(unsigned int, a), __builtin_bit_cast(unsigned int, b), __builtin_bit_cast(unsigned int, c),
                     __builtin_bit_cast(unsigned int, d)};
    return __builtin_bit_cast(bf16x8, r);
}
