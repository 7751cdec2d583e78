// The e4m3 row quantizer's device functions, shared by the weight quantizers (quantize.hip) and the quantizing KV-cache append (attention_kvfp8.hip): one row of bf16
// values -> scale = absmax / 448 (1 for an all-zero row), bytes = e4m3(x * (1 / scale)).  Both encoders give the same byte for every finite product (RNE, saturating at
// +-448): the integer one does not depend on the hardware convert's overflow mode, the hardware one costs 1.5 vector operations per element instead of ~25.
#pragma once
#include "common.h"

namespace mila {

// scale of one per-channel / per-row e4m3 group from its exact absmax (CudaFp8WeightQuantization.cu:57-121; Quantization/KvCache/QuantPolicy.ixx:56-88 names the same rule
// for one KV head of one cached token).  The division is IEEE-correct.
__device__ __forceinline__ float fp8_row_scale(float absmax) { return (absmax > 0.0f) ? (absmax / 448.0f) : 1.0f; }

// OCP E4M3FN <- f32, RNE, saturate-to-finite, NaN -> 0x7f (== __nv_fp8_e4m3(float))
__device__ __forceinline__ uint32_t f32_to_e4m3_rne_sat(float v)
{
    const uint32_t u = __float_as_uint(v);
    const uint32_t sign = (u >> 24) & 0x80u;
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7fu;
    if (a >= 0x43e80000u) return sign | 0x7eu;          // >= 464 (midpoint 448/480) or inf
    if (a < 0x3c800000u)                                 // < 2^-6: subnormal grid, step 2^-9
    {
        const float q = __builtin_rintf(__uint_as_float(a) * 512.0f);   // v_rndne_f32, 0..8
        return sign | (uint32_t)q;                                       // 8 == 0x08 == 2^-6
    }
    a += 0x7ffffu + ((a >> 20) & 1u);                    // RNE to 3 mantissa bits
    const uint32_t code = (((a >> 23) - 120u) << 3) | ((a >> 20) & 7u);
    return sign | (code > 0x7eu ? 0x7eu : code);
}

// four finite f32 -> four OCP e4m3 bytes with the hardware convert (v_cvt_pk_fp8_f32: RNE), saturating to +-448 first as
// f32_to_e4m3_rne_sat does (|v| >= 464 -> 0x7e); inputs here are products of finite values and scales, never NaN
__device__ __forceinline__ uint32_t f32x4_to_e4m3x4_hw(float a, float b, float c, float d)
{
    a = __builtin_amdgcn_fmed3f(a, -448.0f, 448.0f); b = __builtin_amdgcn_fmed3f(b, -448.0f, 448.0f);
    c = __builtin_amdgcn_fmed3f(c, -448.0f, 448.0f); d = __builtin_amdgcn_fmed3f(d, -448.0f, 448.0f);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (uint32_t)r;
}

// two packed bf16 pairs (four consecutive elements of a row) -> their four e4m3 bytes
__device__ __forceinline__ uint32_t bf16x4_to_e4m3x4(uint32_t p01, uint32_t p23, float inv)
{
    return f32x4_to_e4m3x4_hw(bf16_lo(p01) * inv, bf16_hi(p01) * inv, bf16_lo(p23) * inv, bf16_hi(p23) * inv);
}

// one e4m3 dword (four consecutive elements) -> the two packed bf16 pairs bf16_rne(float(e4m3) * scale): the value a dequantized weight / cached K or V element has
// (Fp8Prefill/CudaFp8Prefill.cu:64-84; dequant_fp8_kernel in gemm.hip computes the same expression)
__device__ __forceinline__ void e4m3x4_to_bf16x4(uint32_t w, float scale, uint32_t& p01, uint32_t& p23)
{
    const f32x2 a = fp8x2_to_f32x2(w, false), b = fp8x2_to_f32x2(w, true);
    p01 = pack_bf16x2(a[0] * scale, a[1] * scale);
    p23 = pack_bf16x2(b[0] * scale, b[1] * scale);
}

}  // namespace mila
