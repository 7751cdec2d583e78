// Which kernel a row entry launches, decided in one host function per entry: the launch switches on the plan, and mila_cdna4_row_kernel_form (csrc/internal.h)
// reports the same choice as a name without touching the device -- tests/row_kernel_classes.py holds every row of its table to the form it names, so a change of a
// threshold here cannot silently empty a test class.  Host code only; the kernels are in norm.hip, quantize.hip, rope.hip and fused.hip.
#pragma once
#include <cstdio>
#include <cstring>

namespace mila {

constexpr int kRmsBlockMaxGroups = 256;   // rows up to 131072 elements through the workgroup-per-row RMSNorm kernel (one LDS partial per 64-chunk group)
constexpr int kTailChunks = 4;            // tail_norm_kernel: 16-byte chunks per thread, dim <= 8 * 256 * kTailChunks

enum class RmsForm { Wave, Block, Strided };
// contiguous rows of whole 16-byte chunks: a wave per row up to 1024 elements (and beyond what the block kernel's LDS partials hold), a workgroup per row between
inline RmsForm plan_rmsnorm_bf16(int dim, int inner)
{
    if (inner != 1 || dim % 8 != 0) return RmsForm::Strided;
    return (dim > 1024 && dim <= kRmsBlockMaxGroups * 512) ? RmsForm::Block : RmsForm::Wave;
}

// rmsnorm_fp32_kernel<VEC>: 16-byte accesses for contiguous rows of whole float4s
inline bool plan_rmsnorm_fp32_vec(int dim, int inner) { return inner == 1 && dim % 4 == 0; }

// layernorm_bf16: NV of layernorm_wave_bf16_kernel<NV> (16-byte chunks per lane, the row in registers), 0 = the workgroup-per-row layernorm_kernel
inline int plan_layernorm_bf16(int dim)
{
    if (dim % 8 != 0 || dim > 4096) return 0;
    const int nv = (dim / 8 + 63) / 64;
    return nv <= 1 ? 1 : nv == 2 ? 2 : nv <= 4 ? 4 : 8;
}

// fused_tail_norm(_quant)_bf16: NCH of tail_norm_kernel<NCH, QUANT> = ceil(dim / 8 / 256), 1 .. kTailChunks
inline int plan_tail_norm(int dim)
{
    const int nch = (dim / 8 + 255) / 256;
    return nch <= 1 ? 1 : nch >= kTailChunks ? kTailChunks : nch;
}

// quantize_fp8_per_token: NCH of quantize_fp8_per_token_kernel<NCH> (the row kept in registers), 0 = the form that reads the row twice
inline int plan_quantize_per_token(int K)
{
    const int nch = (K / 8 + 255) / 256;
    return nch <= 2 ? 2 : nch <= 4 ? 4 : nch <= 8 ? 8 : 0;
}

// rope_forward_bf16: eight rotation pairs per thread on 16-byte loads, or one pair per thread for head sizes that are no multiple of 16
inline bool plan_rope_vec(int HS) { return HS % 16 == 0; }

// qkv_post_kernel: the hv = HS / 16 lanes of a row's lane group (64 / hv rows per wave), 0 = one row per wave (HS = 1024)
inline int plan_qkv_post_hv(int HS)
{
    const int hv = HS / 16;
    return hv <= 32 ? hv : 0;
}
inline int qkv_post_rows_per_wave(int HS)
{
    const int hv = plan_qkv_post_hv(HS);
    return hv ? 64 / hv : 1;
}

}  // namespace mila
