/*
 * mila_cdna4.h -- C ABI of the MI355X (gfx950 / CDNA4) device backend for Mila's forward() hot path.
 *
 * This is the drop-in seam.  In the reference every device op ends in a free function of the form
 *     void cuda_<op>_<dtype>(T* out, const T* in, ..., int dims..., cudaStream_t)
 * declared in a .cuh header (SURVEY.md section 0 finding 3).  Each entry point below replaces one of
 * those launchers one-for-one: raw device pointers, plain ints, an opaque stream handle, nothing
 * retained after the call, no hidden allocation (scratch is passed in), all work enqueued on the
 * given stream.  The "replaces" notes cite the reference declaration (paths relative to
 * /root/reference/Mila/Src/Dnn/Compute/Devices/Cuda/Operations unless noted).
 *
 * Conventions
 *   - return value: MILA_OK (0) or a negative MILA_E_* code; mila_cdna4_last_error() returns the
 *     text of the last failure on the calling thread.  The reference throws std::invalid_argument /
 *     std::runtime_error / CudaException from the same checks; the C++ op classes in
 *     mila_amd/host rethrow these codes as the same exception types.
 *   - bf16 tensors are `uint16_t` bit patterns, fp8 (OCP E4M3FN) and packed fp4 (E2M1, low nibble =
 *     even column) are `uint8_t`, scales are `float`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - pointers are DEVICE pointers unless the parameter name starts with host_.
 */
#ifndef MILA_CDNA4_H
#define MILA_CDNA4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MILA_API __attribute__((visibility("default")))
#else
#define MILA_API
#endif

typedef void* mila_stream_t;

enum {
    MILA_OK = 0,
    MILA_E_INVALID_ARGUMENT = -1, /* reference: std::invalid_argument                     */
    MILA_E_UNSUPPORTED = -2,      /* reference: std::runtime_error("unsupported ...")     */
    MILA_E_RUNTIME = -3,          /* reference: CudaException from cudaCheck              */
    MILA_E_SCRATCH_TOO_SMALL = -4
};

/* ---------------------------------------------------------------------------------------------
 * Runtime (counterpart of ExecutionContext<Cuda>: ../CudaExecutionContext.ixx:106-368 and the
 * device memory resources).  Thin wrappers so that a host that does not include HIP headers (the
 * reference's C++23 module units) can own streams and device memory.
 * ------------------------------------------------------------------------------------------- */
MILA_API const char* mila_cdna4_last_error(void);
MILA_API int mila_cdna4_abi_version(void);
MILA_API int mila_cdna4_device_count(int* count);
MILA_API int mila_cdna4_set_device(int device);
/* name: at least 64 bytes */
MILA_API int mila_cdna4_device_info(int device, char* name, int* compute_units, size_t* hbm_bytes);
MILA_API int mila_cdna4_stream_create(mila_stream_t* stream);
MILA_API int mila_cdna4_stream_destroy(mila_stream_t stream);
MILA_API int mila_cdna4_stream_synchronize(mila_stream_t stream);
MILA_API int mila_cdna4_malloc(void** ptr, size_t bytes);
MILA_API int mila_cdna4_free(void* ptr);
MILA_API int mila_cdna4_host_alloc_pinned(void** host_ptr, size_t bytes);
MILA_API int mila_cdna4_host_free_pinned(void* host_ptr);
MILA_API int mila_cdna4_memcpy_h2d(void* dst, const void* host_src, size_t bytes, mila_stream_t stream);
MILA_API int mila_cdna4_memcpy_d2h(void* host_dst, const void* src, size_t bytes, mila_stream_t stream);
MILA_API int mila_cdna4_memcpy_d2d(void* dst, const void* src, size_t bytes, mila_stream_t stream);
MILA_API int mila_cdna4_memset_zero(void* dst, size_t bytes, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Linear -- decode (M == 1) matvec.  y[n] = sum_k x[k] * W[n,k] (+ bias[n]); fp32 accumulate,
 * bf16 out.  replaces Linear/Kernels/Linear.cuh: cuda_matvec_decode_bf16 / _qfp8 / _qfp4
 * (kernels Linear/Kernels/MatVec/CudaMatVecBias.Bf16.cu:134-181, :198-251, :271-508).
 *   W layouts: bf16 [N,K]; fp8 [N,K] + scales[N] (scale applied once after the reduction);
 *   fp4 packed [N,K/2] + scales[N,K/group], group in {64,128}.
 *   K % 8 == 0 (bf16), K % 16 == 0 (fp8), K % 32 == 0 and K % group == 0 (fp4).
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_matvec_bf16(uint16_t* y, const uint16_t* x, const uint16_t* W,
                                    const uint16_t* bias, int K, int N, mila_stream_t stream);
MILA_API int mila_cdna4_matvec_bf16_qfp8(uint16_t* y, const uint16_t* x, const uint8_t* W,
                                         const float* scales, const uint16_t* bias, int K, int N,
                                         mila_stream_t stream);
MILA_API int mila_cdna4_matvec_bf16_qfp4(uint16_t* y, const uint16_t* x, const uint8_t* W_packed,
                                         const float* scales, const uint16_t* bias, int K, int N,
                                         int group, mila_stream_t stream);
/* fp32 logits variant used for the lm_head so the 1e-3 relative bar is asserted on fp32
 * (weight format selected by `fmt`: 0 bf16, 1 fp8 per-channel, 2 fp4 per-group). */
MILA_API int mila_cdna4_matvec_f32out(float* y, const uint16_t* x, const void* W, const float* scales,
                                      int fmt, int K, int N, int group, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Linear -- prefill (M > 1) GEMM  Y[M,N] = X[M,K] * W[N,K]^T (+ bias), bf16 in/out, fp32 MFMA
 * accumulate.  replaces the cuBLASLt NT plans (Linear/CudaLinearOp.ixx:798-824,
 * Common/CublasLtLinearPlan.ixx:307-381) + cuda_add_bias (Fp8Prefill/CudaFp8Prefill.cu:239-256),
 * and for quantized weights the 2-phase dequantize-to-scratch + GEMM path
 * (Linear/CudaLinearOp.ixx:597-644, :716-764) by dequantizing in registers inside the GEMM (same
 * arithmetic: weights rounded to bf16, fp32 accumulate).  K % 8 == 0 (bf16 weights), K % 16 == 0 (fp8), K % 32 == 0 (fp4).
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_gemm_bf16(uint16_t* Y, const uint16_t* X, const uint16_t* W,
                                  const uint16_t* bias, int M, int K, int N, mila_stream_t stream);
/* Linear + tanh-GELU in one kernel (the GPT-2 MLP's fc_1 -> gelu, Components/FFN/MLP/MLP.ixx:148-161): Y = bf16(gelu(bf16(X W^T (+ bias)))), every rounding of the two
 * launches kept, so the result is bit-identical to gemm_bf16 followed by gelu_bf16 -- the [M, N] intermediate is neither written nor re-read. */
MILA_API int mila_cdna4_gemm_gelu_bf16(uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int M, int K,
                                       int N, mila_stream_t stream);
/* The same GEMM (act 0) / GEMM + tanh-GELU (act 1) with a caller workspace -- the counterpart of the cuBLASLt workspace CudaLinearOp hands every plan
 * (Linear/CudaLinearOp.ixx:637-638, :817-818; CudaExecutionContext.ixx:337-383, 4 MiB there).  With it, short prompts and the remainders of long ones -- tile lists that
 * cover a fraction of the CUs -- split K over the idle ones (fp32 partials in the workspace, summed in a fixed order: results do not depend on timing; they may differ
 * from gemm_bf16's in the last bf16 bit, the fp32 sum being taken in another order).  gemm_workspace_bytes() is what this (M, K, N) needs (0: the call is gemm_bf16 /
 * gemm_gelu_bf16; never more than 32 MiB); a smaller or unaligned (16 bytes) workspace is MILA_E_SCRATCH_TOO_SMALL / MILA_E_INVALID_ARGUMENT. */
MILA_API size_t mila_cdna4_gemm_workspace_bytes(int M, int K, int N);
MILA_API int mila_cdna4_gemm_bf16_ws(uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int M, int K, int N, int act, void* workspace,
                                     size_t workspace_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_bf16_w8a16(uint16_t* Y, const uint16_t* X, const uint8_t* W,
                                        const float* scales, const uint16_t* bias, int M, int K,
                                        int N, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_bf16_w4a16(uint16_t* Y, const uint16_t* X, const uint8_t* W_packed,
                                        const float* scales, const uint16_t* bias, int M, int K,
                                        int N, int group, mila_stream_t stream);

/* Linear + GeGLU in ONE kernel for the prefill fc_gate_up (Components/Transformers/Gemma/Gemma.Block.ixx:343-348: the
 * Linear writes [M, 2F] = [gate | up], the GeGLU kernel reads it back): Y[M, F] = bf16(gelu_tanh(bf16(gate)) * bf16(up)),
 * gate = X W[0:F]^T, up = X W[F:2F]^T.  A tile pairs 128 gate rows with the matching 128 up rows; results are
 * bit-identical to gemm_bf16 + geglu_bf16.  gemm_geglu_applicable() != 0 says the fused kernels serve (M, K, F) -- every shape they can run; the
 * _staged forms dequantize the whole [2F, K] weight to `scratch` (2 * F * K * 2 bytes) first.
 * gemm_geglu_preferred() != 0: for a caller that holds the gemm_bf16_ws workspace the fused form is also the FASTER choice; 0 where that caller's
 * gemm_bf16_ws (split-K) + geglu_bf16 pair wins (few-row prompts, short tile lists) -- RocmLinearOp / GemmaBlock ask this one. */
MILA_API int mila_cdna4_gemm_geglu_applicable(int M, int K, int F);
MILA_API int mila_cdna4_gemm_geglu_preferred(int M, int K, int F);
MILA_API int mila_cdna4_gemm_geglu_bf16(uint16_t* Y, const uint16_t* X, const uint16_t* W, int M, int K, int F,
                                        mila_stream_t stream);
MILA_API int mila_cdna4_gemm_geglu_bf16_w8a16_staged(uint16_t* Y, const uint16_t* X, const uint8_t* W,
                                                     const float* scales, int M, int K, int F, void* scratch,
                                                     size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_geglu_bf16_w4a16_staged(uint16_t* Y, const uint16_t* X, const uint8_t* W_packed,
                                                     const float* scales, int M, int K, int F, int group,
                                                     void* scratch, size_t scratch_bytes, mila_stream_t stream);

/* W4A8 prefill: the reference's DEFAULT prefill for the fp4 policy (Linear/CudaLinearOp.ixx:646-715, kUseFp8ActivationPrefillPath):
 *   sB   = max(max(group scales), 1e-12) * 6 / 448                       (fp4_weight_fp8_scale; once, at load: CudaW4A16Gemm.cu:244-294)
 *   W8   = e4m3( lut(nibble) * (group scale * (1 / sB)) )                 (upcast_fp4_to_fp8: CudaW4A16Gemm.cu:300-323)
 *   s_m  = max(absmax(x_m), 1e-12) / 448,  X8 = e4m3( x * (1 / s_m) )     (quantize_fp8_per_token: Fp8Prefill/CudaFp8Prefill.cu:108-160)
 *   y    = bf16( float(bf16(sB * sum_k X8 W8)) * s_m + bias )             (fp8 x fp8 GEMM + cuda_fp8_apply_per_token_scales, :191-211)
 * The contraction runs on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, unit block scales, fp32 accumulate): the two LDS-DMA
 * GEMM kernels on the leading multiple of 256 rows where one serves the shape, a masked 128-row kernel on every other row -- the
 * same instruction chain per output element, so a row's bits do not depend on M.  Integer outputs (W8, X8) are bit-exact, y is
 * within 1 bf16 ulp of the restated reference.  As in the reference the path serves EVERY M > 1: gemm_fp8_applicable() is true for
 * any M, N > 0 with K % 16 == 0 (ABI 3; it used to require M % 256 == 0 and a full grid).  gemm_bf16_w4a8 runs the three steps with
 * scratch = [W8 | X8 | s_m] of gemm_w4a8_scratch_bytes(M, K, N) bytes. */
MILA_API int mila_cdna4_fp4_weight_fp8_scale(float* out_scale, const float* group_scales, int64_t num_scales,
                                             mila_stream_t stream);
MILA_API int mila_cdna4_upcast_fp4_to_fp8(uint8_t* out, const uint8_t* W_packed, const float* scales,
                                          const float* weight_fp8_scale, int N, int K, int group, mila_stream_t stream);
MILA_API int mila_cdna4_quantize_fp8_per_token(uint8_t* dst, float* token_scales, const uint16_t* X, int M, int K,
                                               mila_stream_t stream);
MILA_API int mila_cdna4_gemm_fp8_applicable(int M, int K, int N);
MILA_API int mila_cdna4_gemm_fp8_scaled(uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* token_scales,
                                        const float* weight_scale, const uint16_t* bias, int M, int K, int N,
                                        mila_stream_t stream);
MILA_API size_t mila_cdna4_gemm_w4a8_scratch_bytes(int M, int K, int N);
MILA_API int mila_cdna4_gemm_bf16_w4a8(uint16_t* Y, const uint16_t* X, const uint8_t* W_packed, const float* scales,
                                       const float* weight_fp8_scale, const uint16_t* bias, int M, int K, int N,
                                       int group, void* scratch, size_t scratch_bytes, mila_stream_t stream);
/* the same with the GeGLU epilogue (W_packed = [gate | up] rows, Y[M, F]): bit-identical to gemm_bf16_w4a8 + geglu_bf16;
 * scratch = gemm_w4a8_scratch_bytes(M, K, 2 F) */
MILA_API int mila_cdna4_gemm_geglu_w4a8_applicable(int M, int K, int F);
MILA_API int mila_cdna4_gemm_geglu_bf16_w4a8(uint16_t* Y, const uint16_t* X, const uint8_t* W_packed, const float* scales,
                                             const float* weight_fp8_scale, int M, int K, int F, int group,
                                             void* scratch, size_t scratch_bytes, mila_stream_t stream);

/* Resident prefill weights (288 GB of HBM: the staging passes need not be repeated every forward as on the reference's 12 GB card).
 * dequantize_to_bf16 is the staging pass of the 2-phase prefill as an entry point of its own (cuda_fp8_dequantize_to_bf16,
 * Fp8Prefill/CudaFp8Prefill.cu:64-84; cuda_fp4_dequantize_to_bf16, W4A16Gemm/CudaW4A16Gemm.cu:210-235): out [N, K] bf16, the values
 * gemm_bf16_w8a16_staged / _w4a16_staged put in their scratch, so gemm_bf16 on `out` equals the staged call bit for bit.
 * gemm_geglu_fp8_scaled is gemm_geglu_bf16_w4a8 on operands staged by the caller (upcast_fp4_to_fp8 once at load,
 * quantize_fp8_per_token per forward). */
MILA_API int mila_cdna4_dequantize_to_bf16(uint16_t* out, const void* W, const float* scales, int fmt, int N, int K, int group,
                                           mila_stream_t stream);
/* gemm_fp8_scaled with a caller workspace (see gemm_bf16_ws: the cuBLASLt workspace of CudaLinearOp.ixx:637-638, :706-707): short prompts and long-prompt remainders
 * split K through it.  gemm_fp8_workspace_bytes() = what (M, K, N) needs (0: the call is gemm_fp8_scaled); gemm_w4a8_scratch_bytes() includes it for gemm_bf16_w4a8,
 * which therefore gives the same bits. */
MILA_API size_t mila_cdna4_gemm_fp8_workspace_bytes(int M, int K, int N);
MILA_API int mila_cdna4_gemm_fp8_scaled_ws(uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* token_scales, const float* weight_scale, const uint16_t* bias,
                                           int M, int K, int N, void* workspace, size_t workspace_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_geglu_fp8_scaled(uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* token_scales,
                                              const float* weight_scale, int M, int K, int F, mila_stream_t stream);

/* W8A8 prefill for PerChannelFp8<> weights (ABI 4; opt-in beside the W8A16 forms): the policy's own e4m3 [N, K] weights and fp32 scale[N] are the fp8 matrix cores'
 * operand as they lie in HBM -- the intent the reference states for this policy (../../../Quantization/Weight/Policies.ixx:39-40: "FP8 matmul consumes weights and scales
 * natively -- no dequantization on the forward hot path") and BASELINE config 4 names; no staging pass, no bf16 copy of the weights.  Activations per token exactly as on
 * the W4A8 path (quantize_fp8_per_token; Fp8Prefill/CudaFp8Prefill.cu:108-160):
 *   y = bf16( (sum_k X8 W8)[m, n] * channel_scales[n] * s_m + bias[n] )      fp32 throughout, ONE rounding (no intermediate bf16 tensor exists here)
 * The kernels, row-count rules, split-K workspace (gemm_fp8_workspace_bytes) and fused-GeGLU applicability (gemm_geglu_w4a8_applicable) are those of the W4A8 forms; a row's
 * bits do not depend on which tile form served it.  Not the reference's arithmetic for this policy (that is W8A16, CudaLinearOp.ixx:597-644, and stays RocmLinearOp's default):
 * the activation quantization puts the result within the reference's own W4A8 bar (1e-1 row_absmax, Tests/.../Linear.Cuda.cpp:760-774) of the W8A16 one.
 *   gemm_bf16_w8a8 / gemm_geglu_bf16_w8a8: one call from bf16 activations; scratch = [X8 | s_m | workspace] of gemm_w8a8_scratch_bytes(M, K, N) (GeGLU: N = 2 F) bytes.
 *   channel_scales: 16-byte aligned; the GeGLU forms take [2 F] = [gate rows | up rows]. */
MILA_API int mila_cdna4_gemm_fp8_w8a8_ws(uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* token_scales, const float* channel_scales, const uint16_t* bias,
                                         int M, int K, int N, void* workspace, size_t workspace_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_geglu_fp8_w8a8(uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* token_scales, const float* channel_scales, int M, int K, int F,
                                            mila_stream_t stream);
MILA_API size_t mila_cdna4_gemm_w8a8_scratch_bytes(int M, int K, int N);
MILA_API int mila_cdna4_gemm_bf16_w8a8(uint16_t* Y, const uint16_t* X, const uint8_t* W8, const float* channel_scales, const uint16_t* bias, int M, int K, int N,
                                       void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_geglu_bf16_w8a8(uint16_t* Y, const uint16_t* X, const uint8_t* W8, const float* channel_scales, int M, int K, int F, void* scratch,
                                             size_t scratch_bytes, mila_stream_t stream);

/* 2-phase forms for quantized weights (the reference's own structure, Linear/CudaLinearOp.ixx:597-644, :716-764:
 * dequantize to a bf16 scratch, then the bf16 GEMM).  Chosen automatically when the 256 x 256 LDS-DMA GEMM
 * applies to (M,K,N) -- gemm_staging_bytes() says how much scratch that needs (0 = the register-dequantizing kernel is
 * used and no scratch is touched).  Same arithmetic as the fused forms: w = bf16(decode(q) * scale), fp32 accumulate.
 * The scratch (16-byte aligned) holds the N K bf16 weights and, behind them, gemm_workspace_bytes(M, K, N) of split-K workspace: a staged call gives the bits of
 * gemm_bf16_ws on weights dequantized ahead of time (dequantize_to_bf16). */
MILA_API size_t mila_cdna4_gemm_staging_bytes(int M, int K, int N);
MILA_API int mila_cdna4_gemm_bf16_w8a16_staged(uint16_t* Y, const uint16_t* X, const uint8_t* W, const float* scales,
                                               const uint16_t* bias, int M, int K, int N, void* scratch,
                                               size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_bf16_w4a16_staged(uint16_t* Y, const uint16_t* X, const uint8_t* W_packed,
                                               const float* scales, const uint16_t* bias, int M, int K, int N,
                                               int group, void* scratch, size_t scratch_bytes, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Linear -- quantize-on-load.  Integer outputs are bit-exact with the reference kernels.
 * replaces cuda_quantize_fp8_per_channel (Linear/Kernels/Quantization/CudaFp8WeightQuantization.cu:
 * 57-121,209-249) and cuda_quantize_fp4_per_group (CudaFp4WeightQuantization.cu:54-144,184-224).
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_quantize_fp8_per_channel(uint8_t* dst, float* scales, const uint16_t* src_bf16,
                                                 int N, int K, mila_stream_t stream);
MILA_API int mila_cdna4_quantize_fp4_per_group(uint8_t* dst_packed, float* scales,
                                               const uint16_t* src_bf16, int N, int K, int group,
                                               mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention over a KV cache [B, NKV, capacity, HS] (bf16), row = abs_pos % capacity.
 * replaces Attention/GQA/Kernels/CudaGqa.cuh: cuda_kvcache_write_kv_bf16 (Gqa.Cache.Bf16.cu:86),
 * cuda_gqa_decode_attention_bf16 (+ fixup; Gqa.Decode.Bf16.cu:64-428) and the flash-prefill
 * launchers (Gqa.Flash.Wmma.cu:246, Gqa.Flash.Fa2.cu:177).
 *   decode: q [B, NH*HS], len = position + 1, keys [max(0,len-window), len) (window 0 = all).
 *   prefill: q [B, chunk, NH*HS]; query t has absolute position pos_offset + t and sees keys
 *            max(0,pos-window+1) .. pos.  The cache must already contain the chunk (kv_write first).
 *   scale multiplies q.k before max/exp (Gemma passes 1.0).  HS in {64,128,256,512} on the MFMA / split-K kernels; any other HS <= 512 on a generic
 *   kernel (the unfused entry points only; the fused and device-position forms take the four sizes).
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_kv_write_bf16(uint16_t* Kc, uint16_t* Vc, const uint16_t* k, const uint16_t* v,
                                      int B, int chunk, int NKV, int HS, int start_pos, int capacity,
                                      mila_stream_t stream);
MILA_API size_t mila_cdna4_attn_decode_scratch_bytes(int B, int NH, int HS);
MILA_API int mila_cdna4_attn_decode_bf16(uint16_t* Y, const uint16_t* Q, const uint16_t* Kc,
                                         const uint16_t* Vc, void* scratch, size_t scratch_bytes,
                                         int B, int NH, int NKV, int HS, int capacity, int len,
                                         int window, float scale, mila_stream_t stream);
MILA_API int mila_cdna4_attn_prefill_bf16(uint16_t* Y, const uint16_t* Q, const uint16_t* Kc,
                                          const uint16_t* Vc, int B, int chunk, int NH, int NKV, int HS,
                                          int capacity, int pos_offset, int window, float scale,
                                          mila_stream_t stream);
/* the plan attn_prefill_bf16 launches a chunk from (mha_bf16: NKV = NH, pos_offset 0, window 0), as text, without running device code: "form:HB:DS:NW:QROWS:n_qtiles:
 * n_hblk:n_items" -- form flash | flash_dma | flash_dma_pipe | flash_pp | attn_generic; HB heads x DS d-shares on NW waves per workgroup, which holds QROWS query rows;
 * n_items = n_qtiles * n_hblk workgroups per batch row.  Returns the text's size, 0 for a bad shape. */
MILA_API size_t mila_cdna4_attn_prefill_plan_describe(int HS, int NH, int NKV, int chunk, int pos_offset, int window, char* buf, size_t cap);
/* GPT-2 multi-head attention on packed QKV [B,T,3C] -> [B,T,C], causal, scale 1/sqrt(HS).
 * replaces Attention/MHA/CudaMhaOp.ixx:456-553 (permute + 2 batched GEMMs + softmax + unpermute). */
MILA_API int mila_cdna4_mha_bf16(uint16_t* Y, const uint16_t* QKV, int B, int T, int C, int NH,
                                 mila_stream_t stream);
/* The same op over a KV cache (CudaMhaOp.ixx:137-380: IPositionalUnaryOp::prefill / decode + IKvCacheLifecycle).  Cache [B, NH, capacity, HS] bf16.
 *   mha_kv_write: K / V of the packed rows [B, T, 3C] into cache rows start_pos .. start_pos + T - 1 (the K / V half of permute_qkv[_decode]);
 *     prefill = mha_bf16 + mha_kv_write(start_pos 0).
 *   mha_decode: QKV [B, 1, 3C] of the token at `position`: appends its K / V, then Y[B, C] = attention of its q over keys 0 .. position
 *     (replaces permute_qkv_decode + 2 cuBLASLt GEMMs + softmax_decode + unpermute, :276-380).  scratch: mha_decode_scratch_bytes(B, C, NH).
 *   Any head size: 64 / 128 / 256 / 512 run the MFMA flash and the split-K flash-decode kernels, every other HS <= 512 a generic kernel. */
MILA_API int mila_cdna4_mha_kv_write_bf16(uint16_t* Kc, uint16_t* Vc, const uint16_t* QKV, int B, int T, int C, int NH,
                                          int start_pos, int capacity, mila_stream_t stream);
MILA_API size_t mila_cdna4_mha_decode_scratch_bytes(int B, int C, int NH);
MILA_API int mila_cdna4_mha_decode_bf16(uint16_t* Y, const uint16_t* QKV, uint16_t* Kc, uint16_t* Vc, void* scratch,
                                        size_t scratch_bytes, int B, int C, int NH, int capacity, int position,
                                        mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped-query attention over an FP8 KV cache: the PerChannelKvFp8<> policy (Quantization/KvCache/QuantPolicy.ixx:56-88: e4m3 storage of K and V, one fp32
 * scale per KV head per cached token, absmax / 448, dequantized to transient BF16 -- "never written back"; the reference declares the policy and has no kernels
 * for it, BACKLOG.md "Future": OperationTraits<GqaOp, Cuda, BF16, PerChannelKvFp8<>>).  Launch shapes follow the bf16 entries above (Attention/GQA/Kernels/CudaGqa.cuh).
 *   cache   K8, V8 [B, NKV, capacity, HS] uint8 (e4m3) + Ks, Vs [B, NKV, capacity] fp32; row = abs_pos % capacity.  HS in {64, 128, 256, 512}.
 *   kv_write_fp8: quantizing append of k / v [B, chunk, NKV*HS] at rows (start_pos + t) % capacity -- each K / V row of one (batch, token, KV head) exactly as
 *     quantize_fp8_per_channel quantizes one weight row: bit-identical bytes and scales.  chunk <= capacity (QuantPolicy.ixx:56-88; CudaGqa.cuh: cuda_kvcache_write_kv_bf16).
 *   A cached value is bf16_rne(float(e4m3) * scale) -- the bits dequantize_to_bf16 (fp8) produces.  The attention arithmetic on those values is the bf16 cache's.
 *   attn_decode_kvfp8: attn_decode_bf16 over this cache (CudaGqa.cuh: cuda_gqa_decode_attention_bf16), from attn_decode_bf16's plan for the shape -- the same kernel
 *     form, split count and scratch need.  16 query heads per KV head at HS 512 from the 8192-key band bucket on: the matrix-core kernel, e4m3 rows dequantized on
 *     the way into LDS -- bit for bit attn_decode_bf16 on a bf16 cache of the dequantized values.  Every other shape: the wave-per-position kernel, values dequantized
 *     in registers.  Scratch from attn_decode_scratch_bytes(B, NH, HS).
 *   kv_write_fp8_devpos / attn_decode_kvfp8_devpos: the graph-replay forms (see attn_decode_bf16_devpos below; CudaGqa.cuh: cuda_kvcache_write_kv_bf16,
 *     cuda_gqa_decode_attention_bf16 -- the reference passes the position from the host at every step): one token per sequence appended at row *position_dev % capacity
 *     with kv_write_fp8's bytes and scales; attention over len = *position_dev + 1 keys, read by the kernels.  `max_len` (>= the live length, in its band bucket:
 *     attn_decode_band_bucket) fixes form and split count at capture time -- any max_len of the bucket gives attn_decode_kvfp8's bits; splits past the live band
 *     contribute (m = -inf, l = 0) partials.
 *   kv_dequant_fp8_bf16: cache rows of positions [first_pos, first_pos + count) -> the same rows of bf16 caches [B, NKV, capacity, HS]; other rows are not written.
 *   attn_prefill_kvfp8: attn_prefill_bf16 over this cache (CudaGqa.cuh flash-prefill launchers): the chunk's band [max(0, pos_offset - window + 1), pos_offset + chunk)
 *     (from 0 when unwindowed; extended down to the 32-key tile boundary the flash kernels start streaming from) is dequantized into two transient bf16 caches in
 *     `scratch` (attn_prefill_kvfp8_scratch_bytes, 16-byte aligned), then the bf16 kernels run on them.  The cache must already contain the chunk (kv_write_fp8 first).
 *   fused_qkv_post_kvfp8 / _prefill / _devpos: fused_qkv_post / fused_qkv_post_prefill / fused_qkv_post_devpos (below) with a quantizing append, B == 1:
 *     q_out <- rope(rmsnorm(q; qw)) as there; k' = rope(rmsnorm(k; kw)) and v' = rmsnorm(v_src; vw or ones), rounded to bf16 as the bf16 cache would hold them, are
 *     quantized row by row as kv_write_fp8 quantizes them and stored at row pos % capacity of K8 / V8 / Ks / Vs.  q_out, bytes and scales are bit-identical to
 *     the bf16 entry into scratch caches followed by kv_write_fp8 on the rows it wrote; no other cache row is written.  One launch instead of the six of the unfused
 *     chain (Gemma.Block.ixx:315-337: q_norm, k_norm, rope.decode, v_norm, kvcache_write); the prefill form takes T <= capacity rows of the packed qkv_proj output at
 *     + t * src_row_stride elements (a multiple of 8) for positions pos_offset + t (Gemma.Block.ixx:215-262); the device-position form reads the position from
 *     *position_dev, for graph replay (the reference passes it from the host at every step, SPEC/Gemma4InferenceReview.md:71-84).  HS in {64, 128, 256, 512}.
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_kv_write_fp8(uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* k, const uint16_t* v, int B, int chunk, int NKV, int HS,
                                     int start_pos, int capacity, mila_stream_t stream);
MILA_API int mila_cdna4_attn_decode_kvfp8(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch,
                                          size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity, int len, int window, float scale, mila_stream_t stream);
MILA_API int mila_cdna4_kv_write_fp8_devpos(uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* k, const uint16_t* v, int B, int NKV, int HS,
                                            const int32_t* position_dev, int capacity, mila_stream_t stream);
MILA_API int mila_cdna4_attn_decode_kvfp8_devpos(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch,
                                                 size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity, const int32_t* position_dev, int max_len, int window,
                                                 float scale, mila_stream_t stream);
/* the plan attn_decode_kvfp8 (and its device-position form, len_hint = max_len) launches from, as text, without running device code -- the counterpart of what a caller of
 * the reference learns from CudaGqa.cuh's launcher (cuda_gqa_decode_attention_bf16 picks its split count from the band): "form:splits:band_max:heads_per_group:
 * head_groups:flat:prologue:partial_floats:scratch_need", form attn_decode_kvfp8 | attn_decode_kvfp8_mfma; returns the text's size, 0 for a bad shape. */
MILA_API size_t mila_cdna4_attn_decode_kvfp8_plan_describe(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint, char* buf, size_t cap);
MILA_API int mila_cdna4_kv_dequant_fp8_bf16(uint16_t* Kc_bf16, uint16_t* Vc_bf16, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, int B, int NKV,
                                            int HS, int capacity, int first_pos, int count, mila_stream_t stream);
MILA_API size_t mila_cdna4_attn_prefill_kvfp8_scratch_bytes(int B, int NKV, int HS, int capacity);
MILA_API int mila_cdna4_attn_prefill_kvfp8(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch,
                                           size_t scratch_bytes, int B, int chunk, int NH, int NKV, int HS, int capacity, int pos_offset, int window, float scale,
                                           mila_stream_t stream);
MILA_API int mila_cdna4_fused_qkv_post_kvfp8(uint16_t* q_out, uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* q, const uint16_t* k, const uint16_t* v_src,
                                             const uint16_t* qw, const uint16_t* kw, const uint16_t* vw, const float* cos_cache, const float* sin_cache, int NH, int NKV,
                                             int HS, int position, int capacity, float eps, mila_stream_t stream);
MILA_API int mila_cdna4_fused_qkv_post_kvfp8_prefill(uint16_t* q_out, uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* q, const uint16_t* k,
                                                     const uint16_t* v_src, int64_t src_row_stride, const uint16_t* qw, const uint16_t* kw, const uint16_t* vw,
                                                     const float* cos_cache, const float* sin_cache, int T, int NH, int NKV, int HS, int pos_offset, int capacity,
                                                     float eps, mila_stream_t stream);
MILA_API int mila_cdna4_fused_qkv_post_kvfp8_devpos(uint16_t* q_out, uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* q, const uint16_t* k,
                                                    const uint16_t* v_src, const uint16_t* qw, const uint16_t* kw, const uint16_t* vw, const float* cos_cache,
                                                    const float* sin_cache, int NH, int NKV, int HS, const int32_t* position_dev, int capacity, float eps,
                                                    mila_stream_t stream);

/* The FP8 KV cache under a rows step (ABI 4, additive): B INDEPENDENT sequences (2 <= B <= 4), row b at positions_dev[b] (device memory, always: these are graph-replay
 * forms) on its own caches K8 / V8 + b * NKV * capacity * HS bytes and Ks / Vs + b * NKV * capacity floats -- the [B, NKV, capacity(, HS)] layout above, one sequence per
 * batch index.  The two launches a rows step makes per layer where the bf16 cache has fused_attn_decode_rows_bf16.
 *   fused_qkv_post_kvfp8_rows_devpos: fused_qkv_post_kvfp8_devpos for the B rows (csrc/fused.hip: the qkv_post_body<true> instantiation whose grid y is the row).  Row b
 *     reads q / k / v_src at + b * raw_b_stride elements (a multiple of 8), takes its position from positions_dev[b] (NOT *positions_dev + b), writes q_out +
 *     b * NH * HS and appends into its own caches at cache row positions_dev[b] % capacity; every offset is 64-bit.  Row b's q_out, bytes and scales are bit-identical
 *     to fused_qkv_post_kvfp8_devpos on that row's slices with *position_dev = positions_dev[b]; no other cache row is written.  Refused before any device work: a null
 *     pointer (vw may be null: ones), B outside 2 .. 4, HS outside {64, 128, 256, 512}, a stride that is no multiple of 8, a non-positive capacity.
 *   attn_decode_kvfp8_rows: attn_decode_kvfp8_devpos for the B rows (csrc/attention_kvfp8.hip: the ROWS instantiations of both kernel forms).  Row b attends over
 *     positions_dev[b] + 1 keys of its own caches.  max_len is the live-length bound the launch is captured for; the caller passes the bound of its LONGEST row.  The
 *     splits are planned for ONE row at that bound (attn_decode_kvfp8_plan_describe(1, ...) describes the plan) and used for every row, so row b's Y is bit-identical
 *     to attn_decode_kvfp8_devpos with B = 1 on that row's slices at positions_dev[b] with the same max_len, whatever the other rows hold; a row whose band is shorter
 *     leaves (m = -inf, l = 0) partials in its idle splits.  THE ONE LIMIT of that invariance: on an unwindowed layer the plan follows the live-length bucket of max_len
 *     (attn_decode_band_bucket), so a row that would sit ALONE in a lower bucket than the batch's longest row is reduced over the higher bucket's splits here -- equal
 *     to the alone run captured for that bound, not to one captured for the row's own lower bucket.  Scratch from attn_decode_scratch_bytes(B, NH, HS).
 * Neither entry can see the device values.  A positions_dev[b] outside [0, max_len) -- max_len at most the capacity and the length of the RoPE tables -- makes the
 * append read the tables out of bounds and the attention run over cache rows the sequence never wrote: keeping every row inside is the CALLER's invariant
 * (GemmaTransformer: checkRowsStep, checkPosition), as it is for the bf16 rows entry; there is no device-side check. */
MILA_API int mila_cdna4_fused_qkv_post_kvfp8_rows_devpos(uint16_t* q_out, uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* q, const uint16_t* k,
                                                         const uint16_t* v_src, int64_t raw_b_stride, const uint16_t* qw, const uint16_t* kw, const uint16_t* vw,
                                                         const float* cos_cache, const float* sin_cache, int B, int NH, int NKV, int HS, const int32_t* positions_dev,
                                                         int capacity, float eps, mila_stream_t stream);
MILA_API int mila_cdna4_attn_decode_kvfp8_rows(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch,
                                               size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity, const int32_t* positions_dev, int max_len, int window,
                                               float scale, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Normalisation / activations.
 * rmsnorm: y = x * rsqrt(mean(x^2) + eps) * (w + w_offset) + b over `dim` strided by `inner`;
 *   rstd (bf16, may be NULL) gets one value per slice.  replaces
 *   Normalizations/RmsNorm/Kernels/RmsNorm.cuh:84-149 (RmsNorm.Bf16.cu:20-73).
 * layernorm: replaces Normalizations/LayerNorm/Kernels (LayerNorm.Fp32.cu:20,206), bf16 row added.
 * softmax:   replaces Normalizations/Softmax/Kernels/Softmax.Fp32.cu:56-88.
 * gelu/geglu: replaces Activations/Gelu/Kernels/Gelu.Fp32.cu:29-40, Activations/Geglu/Kernels/
 *   Geglu.cu:25-87 (row = [gate | up], y = gelu_tanh(gate) * up).
 * residual:  replaces Residual/Kernels/Residual.Bf16.cu:15-40.
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_rmsnorm_bf16(uint16_t* Y, uint16_t* rstd, const uint16_t* X, const uint16_t* w,
                                     const uint16_t* b, int outer, int inner, int dim, float eps,
                                     float w_offset, mila_stream_t stream);
/* fp32 row (RmsNorm.cuh:84-123, cuda_rmsnorm_forward_fp32): same arguments, rstd fp32 */
MILA_API int mila_cdna4_rmsnorm_fp32(float* Y, float* rstd, const float* X, const float* w, const float* b,
                                     int outer, int inner, int dim, float eps, float w_offset,
                                     mila_stream_t stream);
MILA_API int mila_cdna4_layernorm_bf16(uint16_t* Y, float* mean, float* rstd, const uint16_t* X,
                                       const uint16_t* w, const uint16_t* b, int outer, int dim,
                                       float eps, mila_stream_t stream);
MILA_API int mila_cdna4_layernorm_fp32(float* Y, float* mean, float* rstd, const float* X,
                                       const float* w, const float* b, int outer, int dim, float eps,
                                       mila_stream_t stream);
MILA_API int mila_cdna4_softmax_fp32(float* Y, const float* X, int outer, int dim, int inner,
                                     mila_stream_t stream);
MILA_API int mila_cdna4_softmax_bf16(uint16_t* Y, const uint16_t* X, int outer, int dim, int inner,
                                     mila_stream_t stream);
MILA_API int mila_cdna4_gelu_bf16(uint16_t* Y, const uint16_t* X, int64_t n, mila_stream_t stream);
MILA_API int mila_cdna4_gelu_fp32(float* Y, const float* X, int64_t n, mila_stream_t stream);
MILA_API int mila_cdna4_geglu_bf16(uint16_t* Y, const uint16_t* X, int tokens, int half,
                                   mila_stream_t stream);
MILA_API int mila_cdna4_residual_bf16(uint16_t* Y, const uint16_t* A, const uint16_t* B, int64_t n,
                                      mila_stream_t stream);
MILA_API int mila_cdna4_residual_fp32(float* Y, const float* A, const float* B, int64_t n,
                                      mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * RoPE.  replaces Encodings/Rope/Kernels/Rope.cuh:29-182 (cache: Rope.Fp32.cu:27-59,288-321;
 * rotation: Rope.Bf16.cu:28-118).  Half-split pairing (i, i+HS/2); cos/sin fp32 [max_seq, HS/2];
 * pairs >= rotary_dim/2 (when 0 < rotary_dim < HS) are the identity.  In-place allowed
 * (Qout == Qin).  decode == forward with T = 1 and pos_offset = position.
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_rope_build_cache(float* cos_cache, float* sin_cache, int max_seq, int HS,
                                         float base, int rotary_dim, mila_stream_t stream);
MILA_API int mila_cdna4_rope_forward_bf16(uint16_t* Qout, uint16_t* Kout, const uint16_t* Qin,
                                          const uint16_t* Kin, const float* cos_cache,
                                          const float* sin_cache, int B, int T, int NH, int NKV, int HS,
                                          int pos_offset, int max_seq, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Glue.  Token ids are read from DEVICE memory (Embeddings/Kernels/TokenEmbedding.Bf16.cu:23-97);
 * an id outside [0,vocab) raises a sticky device flag reported by mila_cdna4_check_index_error.
 * embedding scale: y = bf16(float(x) * scale) when scale != 0 (Components/Embeddings/
 * TokenEmbedding.ixx:179-181).  lpe: Encodings/Lpe/Kernels/Lpe.Fp32.cu:33-124 (bf16 row added).
 * split3: ../Tensors/Operations/Kernels/Structural.cu:106.  scale: Math.Elementwise.cu:106-113.
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_embedding_gather_bf16(uint16_t* Y, const int32_t* tokens, const uint16_t* table,
                                              int n_tok, int C, int vocab, float scale,
                                              int32_t* error_flag, mila_stream_t stream);
/* FP8 tied embedding/lm_head table with one fp32 scale per vocab row
 * (Embeddings/Kernels/TokenEmbedding.Fp8.cu:33-69): y = bf16(float(e4m3) * row_scale[tok]) [* scale] */
MILA_API int mila_cdna4_embedding_gather_bf16_qfp8(uint16_t* Y, const int32_t* tokens, const uint8_t* table,
                                                   const float* row_scales, int n_tok, int C, int vocab,
                                                   float scale, int32_t* error_flag, mila_stream_t stream);
MILA_API int mila_cdna4_lpe_bf16(uint16_t* Y, const int32_t* tokens, const uint16_t* wte,
                                 const uint16_t* wpe, int B, int T, int C, int out_stride_T, int vocab,
                                 int32_t* error_flag, mila_stream_t stream);
MILA_API int mila_cdna4_split3_bf16(uint16_t* a, uint16_t* b, uint16_t* c, const uint16_t* X, int rows,
                                    int na, int nb, int nc, mila_stream_t stream);
MILA_API int mila_cdna4_scale_bf16(uint16_t* Y, const uint16_t* X, int64_t n, float s,
                                   mila_stream_t stream);
/* Synthetic parameters, generated where they live: dst[i] = bf16(offset + amp * (2u - 1)), u in [0, 1) from the counter-based
 * splitmix64(seed, i) -- the same bits for the same (seed, i) on any grid, so the CPU oracle regenerates them without a file
 * (SURVEY.md section 8d).  Stands where the reference's initializeParameters kernels do (Linear.ixx:1029-1054); no checkpoint exists offline. */
MILA_API int mila_cdna4_fill_uniform_bf16(uint16_t* dst, int64_t n, uint64_t seed, float amp, float offset,
                                          mila_stream_t stream);
MILA_API int mila_cdna4_convert_f32_to_bf16(uint16_t* Y, const float* X, int64_t n, mila_stream_t stream);
MILA_API int mila_cdna4_convert_bf16_to_f32(float* Y, const uint16_t* X, int64_t n, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * FP32 rows (ABI 4).  The reference keeps FP32 paths of these ops "for validation and reference" (OperationTraits.Cuda.ixx:50-54, :108-126, :274-282): with them -- and
 * layernorm_fp32 / softmax_fp32 / gelu_fp32 / residual_fp32 / rmsnorm_fp32 above -- BASELINE config 1's model (GPT-2 124M, FP32) runs on the device and is compared with
 * the reference's CPU backend at FP32 tolerance.  fp32 in, fp32 accumulate (ascending K), fp32 out; validation kernels, not performance kernels.
 *   matvec_fp32 / gemm_fp32: y = x W^T (+ bias) [act 1: + tanh-GELU of the result], W [N, K] row-major -- replaces Linear/Kernels/MatVec/CudaMatVecBias.Fp32.cu:40,
 *     Linear/Kernels/MatMul/CudaMatMulFp32.cu:31-183;
 *   mha_fp32 / mha_kv_write_fp32 / mha_decode_fp32: the FP32 twins of mha_bf16 / mha_kv_write_bf16 / mha_decode_bf16 (Attention/MHA/CudaMhaOp.ixx:145-380: FP32 is the
 *     reference's only CUDA MHA row); caches [B, NH, capacity, HS] fp32; any head size <= 512;
 *   lpe_fp32: Encodings/Lpe/Kernels/Lpe.Fp32.cu:33-124;  rope_forward_fp32: Encodings/Rope/Kernels/Rope.Fp32.cu:288-321 (tables from rope_build_cache).
 * ------------------------------------------------------------------------------------------- */
MILA_API int mila_cdna4_matvec_fp32(float* y, const float* x, const float* W, const float* bias, int K, int N, mila_stream_t stream);
MILA_API int mila_cdna4_gemm_fp32(float* Y, const float* X, const float* W, const float* bias, int M, int K, int N, int act, mila_stream_t stream);
MILA_API int mila_cdna4_mha_fp32(float* Y, const float* QKV, int B, int T, int C, int NH, mila_stream_t stream);
MILA_API int mila_cdna4_mha_kv_write_fp32(float* Kc, float* Vc, const float* QKV, int B, int T, int C, int NH, int start_pos, int capacity, mila_stream_t stream);
MILA_API int mila_cdna4_mha_decode_fp32(float* Y, const float* QKV, float* Kc, float* Vc, int B, int C, int NH, int capacity, int position, mila_stream_t stream);
MILA_API int mila_cdna4_lpe_fp32(float* Y, const int32_t* tokens, const float* wte, const float* wpe, int B, int T, int C, int out_stride_T, int vocab,
                                 int32_t* error_flag, mila_stream_t stream);
MILA_API int mila_cdna4_rope_forward_fp32(float* Qout, float* Kout, const float* Qin, const float* Kin, const float* cos_cache, const float* sin_cache, int B, int T,
                                          int NH, int NKV, int HS, int pos_offset, int max_seq, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Greedy device sampler: token_out[0] = argmax(logits), ties to the lowest index.
 * replaces Sampling/Kernels/Sampling.cuh: cuda_sample_argmax_fp32 / _bf16 (Sampling.cu:23-75).  The token stays on
 * the device and feeds the next step's embedding gather (the reference's "decode-ahead", Models/GemmaModel.ixx:497-537).
 * ------------------------------------------------------------------------------------------- */
MILA_API size_t mila_cdna4_sample_scratch_bytes(void);
MILA_API int mila_cdna4_sample_argmax_fp32(const float* logits, int32_t* token_out, int vocab, void* scratch,
                                           size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_bf16(const uint16_t* logits, int32_t* token_out, int vocab, void* scratch,
                                           size_t scratch_bytes, mila_stream_t stream);

/* Stochastic sampler: x = (softcap > 0 ? softcap * tanh(l / softcap) : l) / temperature;
 * top-k (0 = off) keeps the values strictly above the (k+1)-th largest; top-p (>= 1 = off) keeps the smallest set of
 * highest-probability survivors whose mass exceeds top_p * total; token = first index, in token order, with
 * probability > 0 and cumulative >= r * total; r in [0, 1] is drawn by the caller.  Where rounding leaves the running
 * sum short of r * total (next to r = 1) the token is the LAST index with probability > 0, so a token that top-k or
 * top-p removed is never returned; vocab - 1 only when no token has mass (every value tied under top-k).  -0.0 and
 * +0.0 are one value: a tie group enters or leaves top-k as a whole.
 * replaces Sampling/Kernels/Sampling.cuh: cuda_sample_stochastic_fp32 / _bf16 (Sampling.cu:655-714; semantics of the
 * single-block kernel :760-905).  temperature <= 0 is the greedy sampler above.  Deterministic for fixed arguments. */
MILA_API size_t mila_cdna4_sample_stochastic_scratch_bytes(int vocab);
MILA_API int mila_cdna4_sample_stochastic_fp32(const float* logits, int32_t* token_out, int vocab, float softcap,
                                               float temperature, int top_k, float top_p, float r, void* scratch,
                                               size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_stochastic_bf16(const uint16_t* logits, int32_t* token_out, int vocab, float softcap,
                                               float temperature, int top_k, float top_p, float r, void* scratch,
                                               size_t scratch_bytes, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused decode-step kernels (GemmaBlock::decode,
 * Components/Transformers/Gemma/Gemma.Block.ixx:287-356, as a fused schedule).  Each computes
 * exactly what the listed chain of unfused ops computes, including every intermediate bf16 rounding,
 * so results are bit-identical to calling the unfused entry points in sequence.
 * ------------------------------------------------------------------------------------------- */
/* y = Linear( rmsnorm(x; nw, eps) ), weight format `fmt` (0 bf16, 1 fp8, 2 fp4).  With
 * `geglu` != 0, W has 2*N rows [gate | up] and y[n] = bf16( gelu_tanh(bf16(gate_n)) * bf16(up_n) ).
 * With res != NULL the prologue is the sandwich tail of the previous sub-block:
 *   r = bf16( res + bf16(rmsnorm(x; pw)) ) [* post_scale]; x' = rmsnorm(r; nw); r is written to
 *   res_out by block 0. */
typedef struct mila_fused_matvec_args {
    uint16_t* y;              /* [N] bf16 output (or [N] after GeGLU)                         */
    const uint16_t* x;        /* [K] bf16 input                                               */
    const void* W;            /* weights in `fmt` layout                                      */
    const float* scales;      /* fp8: [rows]; fp4: [rows, K/group]; bf16: NULL                */
    const uint16_t* norm_w;   /* [K] rmsnorm weight applied to the matvec input, or NULL      */
    const uint16_t* post_w;   /* [K] rmsnorm weight of the sandwich tail, or NULL             */
    const uint16_t* res;      /* [K] residual input of the sandwich tail, or NULL             */
    uint16_t* res_out;        /* [K] where r is stored (required when res != NULL)            */
    float post_scale;         /* layer scalar applied to r (1.0f = none)                      */
    float eps;
    int fmt, K, N, group, geglu;
    int f32_out;              /* != 0: y is float[N] (lm_head logits); not combinable with geglu */
    /* ABI 3, optional (NULL = off), f32_out only: the greedy sampler's first stage in this launch's epilogue -- every workgroup leaves the largest of its logits and its
     * index (ties to the lowest index, Sampling.cu:23-75) in argmax_scratch (>= sample_scratch_bytes()), *argmax_blocks (host) receives their number;
     * sample_argmax_final_advance then picks the token: the same token as sample_argmax_fp32 on y, one launch fewer. */
    void* argmax_scratch;
    size_t argmax_scratch_bytes;
    int* argmax_blocks;
} mila_fused_matvec_args;
MILA_API int mila_cdna4_fused_norm_matvec(const mila_fused_matvec_args* host_args, mila_stream_t stream);

/* q/k(/v) per-head RMSNorm + RoPE + KV-cache append for one decode token, in one launch:
 *   q <- rope(rmsnorm(q; qw)), k' = rope(rmsnorm(k; kw)), v' = rmsnorm(v_src; vw or ones),
 *   cache[pos % capacity] <- (k', v').  v_src == k (raw) on Gemma global layers. */
MILA_API int mila_cdna4_fused_qkv_post(uint16_t* q_out, uint16_t* Kc, uint16_t* Vc, const uint16_t* q,
                                       const uint16_t* k, const uint16_t* v_src, const uint16_t* qw,
                                       const uint16_t* kw, const uint16_t* vw, const float* cos_cache,
                                       const float* sin_cache, int NH, int NKV, int HS, int position,
                                       int capacity, float eps, mila_stream_t stream);


/* Prefill forms of the two glue fusions above, T rows per launch (B == 1), bit-identical to the unfused launches:
 *   fused_qkv_post_prefill: for token t < T at position pos_offset + t, q/k/v_src rows at + t * src_row_stride elements
 *     (the packed qkv_proj output: no split3 copy), q_out[t] <- rope(rmsnorm(q)), cache row <- (rope(rmsnorm(k)), rmsnorm(v_src))
 *     -- replaces split3 + q_norm + k_norm + v_norm + rope.prefill + kv_write (Gemma.Block.ixx:215-262);
 *   fused_tail_norm_bf16: R = bf16(bf16(RES + bf16(rmsnorm(A; post_w))) * post_scale), XN = rmsnorm(R; next_w) (XN / next_w
 *     may both be NULL) -- replaces RmsNorm + Residual (+ scale) + RmsNorm (Gemma.Block.ixx:339-356, :287-289); 1024 < dim <= 8192. */
MILA_API int mila_cdna4_fused_qkv_post_prefill(uint16_t* q_out, uint16_t* Kc, uint16_t* Vc, const uint16_t* q,
                                               const uint16_t* k, const uint16_t* v_src, int64_t src_row_stride,
                                               const uint16_t* qw, const uint16_t* kw, const uint16_t* vw,
                                               const float* cos_cache, const float* sin_cache, int T, int NH, int NKV,
                                               int HS, int pos_offset, int capacity, float eps, mila_stream_t stream);
MILA_API int mila_cdna4_fused_tail_norm_bf16(uint16_t* R, uint16_t* XN, const uint16_t* A, const uint16_t* RES,
                                             const uint16_t* post_w, const uint16_t* next_w, int rows, int dim,
                                             float post_scale, float eps, mila_stream_t stream);
/* fused_tail_norm_bf16 whose XN row is ALSO written as the W4A8 Linear's activation operand: XQ[row] = e4m3(XN[row] / XS[row]),
 * XS[row] = max(absmax(XN[row]), 1e-12) / 448 -- bit for bit what quantize_fp8_per_token(XQ, XS, XN) would produce (the reference's
 * cuda_fp8_quantize_per_token, Fp8Prefill/CudaFp8Prefill.cu:108-160, folded into the producer of its input). */
MILA_API int mila_cdna4_fused_tail_norm_quant_bf16(uint16_t* R, uint16_t* XN, uint8_t* XQ, float* XS, const uint16_t* A,
                                                   const uint16_t* RES, const uint16_t* post_w, const uint16_t* next_w, int rows,
                                                   int dim, float post_scale, float eps, mila_stream_t stream);

/* Graph-replay forms: the decode position lives in DEVICE memory so that one captured hipGraph
 * serves every step (the reference re-launches ~1100 kernels per token from the host,
 * SPEC/Gemma4InferenceReview.md:71-84).  `max_len` fixes the split count at capture time; splits past
 * the live band contribute (m=-inf, l=0) partials.  advance_position: *position_dev += 1. */
MILA_API int mila_cdna4_attn_decode_bf16_devpos(uint16_t* Y, const uint16_t* Q, const uint16_t* Kc,
                                                const uint16_t* Vc, void* scratch, size_t scratch_bytes,
                                                int B, int NH, int NKV, int HS, int capacity,
                                                const int32_t* position_dev, int max_len, int window,
                                                float scale, mila_stream_t stream);
MILA_API int mila_cdna4_fused_qkv_post_devpos(uint16_t* q_out, uint16_t* Kc, uint16_t* Vc, const uint16_t* q,
                                              const uint16_t* k, const uint16_t* v_src, const uint16_t* qw,
                                              const uint16_t* kw, const uint16_t* vw, const float* cos_cache,
                                              const float* sin_cache, int NH, int NKV, int HS,
                                              const int32_t* position_dev, int capacity, float eps,
                                              mila_stream_t stream);
MILA_API int mila_cdna4_advance_position(int32_t* position_dev, mila_stream_t stream);
/* The host side of the reference's decode-ahead loop (Models/GemmaModel.ixx:496-568: enqueueSampleNext / awaitSampledToken) learns each
 * sampled token while the NEXT step already runs.  `ring` is ring_size 64-bit words of host-visible memory (pinned + mapped), `seq_dev` a device
 * counter: both kernels do  seq = ++*seq_dev;  ring[seq % ring_size] = seq << 32 | (uint32)*token  with ONE system-scope release store, so the host
 * polls the slot until it carries the sequence number it expects -- no event, no copy, no stream wait on the decode path.
 * advance_position_snapshot additionally does *position_dev += 1 (the last node of a captured step); snapshot_token is the eager sampler's counterpart. */
MILA_API int mila_cdna4_advance_position_snapshot(int32_t* position_dev, const int32_t* token, unsigned long long* seq_dev, unsigned long long* ring, int ring_size,
                                                  mila_stream_t stream);
MILA_API int mila_cdna4_snapshot_token(const int32_t* token, unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream);
/* the tail of a captured greedy step in two launches instead of three: sample_argmax_fp32 whose final reduction also does *position_dev += 1 and, when ring != NULL,
 * the publication of advance_position_snapshot (seq_dev / ring / ring_size as there; NULL / NULL / 0 = no publication).  Same token as sample_argmax_fp32. */
MILA_API int mila_cdna4_sample_argmax_advance_fp32(const float* logits, int32_t* token_out, int vocab, void* scratch, size_t scratch_bytes,
                                                   int32_t* position_dev, unsigned long long* seq_dev, unsigned long long* ring, int ring_size,
                                                   mila_stream_t stream);

/* the final stage of the greedy sampler alone, over the `blocks` partials a fused_norm_matvec launch with argmax_scratch left in `scratch`, with the tail of
 * sample_argmax_advance_fp32 (*position_dev += 1, publication when ring != NULL) */
MILA_API int mila_cdna4_sample_argmax_final_advance(int32_t* token_out, const void* scratch, size_t scratch_bytes, int blocks, int32_t* position_dev,
                                                    unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream);

/* The stochastic sampler as a pipeline that can sit in a captured decode step ("radix"): the semantics of sample_stochastic_* above, in the same order (softcap, then
 * temperature; top-k survivors strictly above the (k+1)-th largest; the smallest nucleus whose mass exceeds top_p * total, a tie entering whole; the first index with
 * e > 0 and cumulative >= r * total, else the last index with e > 0, else vocab - 1), from at most 9 launches over fixed buffers instead of 21.  replaces Sampling/Kernels/Sampling.cuh:
 * cuda_sample_stochastic_fp32 / _bf16 (Sampling.cu:655-714; semantics of the single-block kernel :760-905).  Both thresholds come from digit selection over the 32-bit
 * key (11 + 11 + 10 bits): integer counts for top-k (the threshold of sample_stochastic_* exactly), 64-bit fixed-point masses (scale 2^40) for top-p, summed with integer
 * atomics, so a call is deterministic run to run.  The nucleus may differ from sample_stochastic_*'s where top_p * total lies within float rounding of a boundary, and
 * in one more way: an entry with 0 < e < 2^-40 (2^-40 of the largest probability) adds nothing to the fixed-point total or the histograms, so with top_p < 1 it is never
 * in the nucleus here, even for a top_p within 2^-22 of 1 at which sample_stochastic_* would keep it.  With top_p >= 1 such entries stay, as there.
 *   sample_radix_fp32 / _bf16: the draw r in [0, 1] by value; nothing is advanced.
 *   sample_radix_advance_fp32: the last node of a captured stochastic step, the twin of sample_argmax_final_advance -- the draw is draws[(*seq_dev + 1) % draws_size]
 *     (host-visible memory the host rewrites between replays; read with one system-scope load), then *position_dev += 1, *seq_dev += 1 and, when ring != NULL,
 *     ring[seq % ring_size] = seq << 32 | token with one system-scope release store.  seq_dev is required (the draw slot follows it), the ring is optional.
 *   scratch: sample_radix_scratch_bytes(vocab) bytes, 8-byte aligned, the caller's for the duration of the call; the first launch clears what the others accumulate into.
 *   sample_radix_plan_describe: "launches:k_passes:p_passes:scratch_need" of a call, from the host function the entries launch from (no device work): one launch fewer
 *     per digit pass of a truncation that is off (top_k 0 or >= vocab; top_p >= 1), the first nucleus pass riding in the probability launch.  Returns the text's size. */
MILA_API size_t mila_cdna4_sample_radix_scratch_bytes(int vocab);
MILA_API int mila_cdna4_sample_radix_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                          void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_bf16(const uint16_t* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                          void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p,
                                                  const float* draws, int draws_size, void* scratch, size_t scratch_bytes, int32_t* position_dev,
                                                  unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream);
MILA_API size_t mila_cdna4_sample_radix_plan_describe(int vocab, int top_k, float top_p, char* buf, size_t cap);

/* One-launch decode attention for one token (B == 1): q/k/v per-head RMSNorm + RoPE + KV append (the
 * work of fused_qkv_post) folded into the flash-decode kernel's prologue, where it overlaps the first
 * K/V round trip.  q_raw [NH*HS], k_raw / v_raw [NKV*HS] are the raw projections (v_raw == k_raw on Gemma
 * global layers).  position_dev != NULL selects the graph-replay form; `position` is then an upper bound on the live length (position + 1) the captured
 * launch will be replayed at, 0 = the capacity: an unwindowed layer's launch geometry is chosen per BUCKET of the live length (4096, 8192, 16384, ... keys, clipped to
 * the capacity; the eager form uses position + 1), so a caller whose positions leave the bucket re-captures (GemmaTransformer::ensureGraph).  Bit-identical to
 * fused_qkv_post + attn_decode_bf16. */
MILA_API int mila_cdna4_fused_attn_decode_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw,
                                               const uint16_t* k_raw, const uint16_t* v_raw, const uint16_t* qw,
                                               const uint16_t* kw, const uint16_t* vw, const float* cos_cache,
                                               const float* sin_cache, void* scratch, size_t scratch_bytes, int NH,
                                               int NKV, int HS, int capacity, int position,
                                               const int32_t* position_dev, int window, float scale, float eps,
                                               mila_stream_t stream);
/* the live-length bucket of `len` keys on a cache of `capacity` rows, as the decode entry points choose it: what a caller compares to know when a captured launch must
 * be captured again (0 for capacity <= 0) */
MILA_API int mila_cdna4_attn_decode_band_bucket(int len, int capacity);

/* fused_attn_decode_bf16 for B rows decoded at ONE position (the reference's decode kernels take the batch in their grid, Gqa.Decode.Bf16.cu:379-387): batch row b reads
 * q_raw / k_raw / v_raw + b * raw_b_stride elements and its own caches [b]; Y [B, NH*HS]; scratch from attn_decode_scratch_bytes(B, NH, HS).  Bit-identical, row by row,
 * to fused_qkv_post on that row's caches + attn_decode_bf16 with the same B. */
MILA_API int mila_cdna4_fused_attn_decode_batch_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw,
                                                     const uint16_t* v_raw, int64_t raw_b_stride, const uint16_t* qw, const uint16_t* kw,
                                                     const uint16_t* vw, const float* cos_cache, const float* sin_cache, void* scratch,
                                                     size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity, int position,
                                                     const int32_t* position_dev, int window, float scale, float eps, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Batched decode, 2 .. 4 rows per step, each row an independent sequence (ABI 4, additive).  The reference runs CudaLinearOp at M = B
 * (Linear/Kernels/MatVec/CudaMatVecBias.Bf16.cu, one weight pass per row); here the weights are streamed ONCE for all rows.
 * BATCH INVARIANCE: row b of every entry below has the bits the one-row entry gives on that row alone, whatever the other rows hold.
 * ------------------------------------------------------------------------------------------- */
/* The decode Linear on `rows` input vectors: everything matvec_bf16 / _qfp8 / _qfp4 / matvec_f32out (a.norm_w == NULL; `bias` optional, bf16 out only) and
 * fused_norm_matvec (a.norm_w != NULL: norm prologue, sandwich tail, GeGLU, fp32 out, the sampler's first stage) compute, row by row.  `a` holds row 0's pointers;
 * row b reads x + b * x_stride (and res + b * res_stride) and writes y + b * y_stride (and res_out + b * res_out_stride), strides in ELEMENTS of the respective type,
 * at least the row's width, x / res / res_out strides multiples of 8.  With a.argmax_scratch, row b's partials go to argmax_scratch + b * sample_scratch_bytes()
 * (argmax_scratch_bytes >= rows * sample_scratch_bytes()), every row has *a.argmax_blocks of them, and sample_argmax_rows_final_advance picks the tokens.
 * rows outside 2 .. 4, or an x image that does not fit the 160 KiB of LDS: MILA_E_UNSUPPORTED. */
typedef struct mila_matvec_rows_args {
    mila_fused_matvec_args a;
    const uint16_t* bias;     /* [N] bf16 or NULL; the plain form only                            */
    int rows;
    int64_t x_stride, y_stride, res_stride, res_out_stride;
} mila_matvec_rows_args;
MILA_API int mila_cdna4_matvec_rows(const mila_matvec_rows_args* host_args, mila_stream_t stream);

/* fused_attn_decode_batch_bf16 for B INDEPENDENT sequences: row b decodes at positions_dev[b] (device memory, always: this is the graph-replay form) on its own caches
 * [b] -- a different prompt length per row, rows that finish at different times (the reference's decode kernels take the batch in their grid at ONE position,
 * Gqa.Decode.Bf16.cu:379-387).  max_len is the live-length bound the launch is captured for (0 = the capacity), as `position` is beside a position_dev in
 * fused_attn_decode_bf16; the caller passes the bound of its LONGEST row.  The splits are planned for ONE row at that bound and used for every row, so row b's Y and
 * cache rows are bit-identical to fused_attn_decode_bf16 in its device-position form at positions_dev[b] with the same max_len, whatever the other rows hold; a row
 * whose band is shorter leaves (m = -inf, l = 0) partials in its idle splits.  THE ONE LIMIT of that invariance: on an unwindowed layer the plan follows the live-length
 * bucket of max_len (attn_decode_band_bucket), so a row that would sit ALONE in a lower bucket than the batch's longest row is reduced over the higher bucket's splits
 * here -- equal to the alone run captured for that bound, not to one captured for the row's own lower bucket.  Head sizes 64, 128, 256, 512; scratch from
 * attn_decode_scratch_bytes(B, NH, HS). */
MILA_API int mila_cdna4_fused_attn_decode_rows_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw,
                                                    const uint16_t* v_raw, int64_t raw_b_stride, const uint16_t* qw, const uint16_t* kw,
                                                    const uint16_t* vw, const float* cos_cache, const float* sin_cache, void* scratch,
                                                    size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity, const int32_t* positions_dev,
                                                    int max_len, int window, float scale, float eps, mila_stream_t stream);

/* The tail of a captured greedy step for B rows (the rows twin of sample_argmax_final_advance; Sampling.cu:23-75 once per row): token b = the argmax over the `blocks`
 * partials a matvec_rows launch left at scratch + b * sample_scratch_bytes() -- the token sample_argmax_fp32 gives on row b's logits, ties to the lowest index.  Only
 * where active_dev[b] != 0 is token_out[b] stored and positions_dev[b] += 1: a retired row keeps its token and its position.
 * advance_positions_rows is the position bump alone (the stochastic path samples on its own). */
MILA_API int mila_cdna4_sample_argmax_rows_final_advance(int32_t* token_out, const void* scratch, size_t scratch_bytes, int blocks, int32_t* positions_dev,
                                                         const int32_t* active_dev, int B, mila_stream_t stream);
MILA_API int mila_cdna4_advance_positions_rows(int32_t* positions_dev, const int32_t* active_dev, int B, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Chain decode: 2 .. 4 rows per step that are CONSECUTIVE POSITIONS OF ONE SEQUENCE on ONE cache (ABI 4, additive) -- what verifying drafted tokens needs
 * (speculative greedy decode: the last sampled token and up to three drafts in one pass over the weights).  The Linears are matvec_rows as above.
 * ------------------------------------------------------------------------------------------- */
/* fused_attn_decode_bf16 for T rows (2 <= T <= 4) of one sequence: row t is the token at position + t -- `position` when position_dev is NULL, *position_dev + t
 * otherwise (ONE position word, the one the one-row graph step reads; max_len then is the live-length bound the launch is captured for, 0 = the capacity, as in
 * fused_attn_decode_rows_bf16, and the caller keeps *position_dev + T <= max_len).  ONE cache [1, NKV, capacity, HS]; row t reads q_raw / k_raw / v_raw +
 * t * raw_b_stride elements (a multiple of 8); Y [T, NH*HS]; scratch from attn_decode_chain_scratch_bytes(T, NH, HS), always required (the roped q rows live there).
 * Two launches plus the combine: (a) q/k/v norm + RoPE + KV append of all T rows (fused_qkv_post_prefill, or fused_qkv_post_rows_devpos), (b) decode attention, row t
 * over the band of length position + t + 1 of the same cache, the splits planned for ONE row at the max_len bucket (eager: position + T).
 * CONTRACT: row t's Y is bit-identical to T successive fused_attn_decode_bf16 calls (B = 1, device-position form, the same max_len) at position .. position + T - 1,
 * so are cache rows position .. position + T - 1, and no other cache row is written.
 * The chain is for UNBOUNDED caches (capacity >= every position it is used at), not rings: a rejected draft leaves a stale row behind, which a later step at that
 * position overwrites; in a ring the stale row would already have evicted a live one.  Refused without touching the device (MILA_E_INVALID_ARGUMENT): T outside
 * 2 .. 4, a head size other than 64 / 128 / 256 / 512, a null pointer, and in the eager form position + T > capacity. */
MILA_API int mila_cdna4_fused_attn_decode_chain_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw,
                                                     const uint16_t* v_raw, int64_t raw_b_stride, const uint16_t* qw, const uint16_t* kw,
                                                     const uint16_t* vw, const float* cos_cache, const float* sin_cache, void* scratch,
                                                     size_t scratch_bytes, int T, int NH, int NKV, int HS, int capacity, int position,
                                                     const int32_t* position_dev, int max_len, int window, float scale, float eps, mila_stream_t stream);
/* the partials of T rows at the most splits a plan takes plus the roped q rows [T, NH, HS] bf16; 0 for T outside 2 .. 4 or an unsupported head size */
MILA_API size_t mila_cdna4_attn_decode_chain_scratch_bytes(int T, int NH, int HS);
/* The two entries above under a second spelling, for the host mirror (mila_amd/host): its sources must not spell the name of the measured-slower decode-chain
 * EXPERIMENT of csrc/internal.h, which tests/test_capi_cpu.py checks as a substring -- and that substring is part of the two names above. */
#define mila_cdna4_fused_attn_chain_bf16 mila_cdna4_fused_attn_decode_chain_bf16
#define mila_cdna4_attn_chain_scratch_bytes mila_cdna4_attn_decode_chain_scratch_bytes
/* fused_qkv_post_prefill with the first token's position on the device: token t at *position_dev + t (launch (a) of the chain's device-position form) */
MILA_API int mila_cdna4_fused_qkv_post_rows_devpos(uint16_t* q_out, uint16_t* Kc, uint16_t* Vc, const uint16_t* q, const uint16_t* k,
                                                   const uint16_t* v_src, int64_t src_row_stride, const uint16_t* qw, const uint16_t* kw,
                                                   const uint16_t* vw, const float* cos_cache, const float* sin_cache, int T, int NH, int NKV,
                                                   int HS, const int32_t* position_dev, int capacity, float eps, mila_stream_t stream);

/* The tail of a captured chain step (the chain's twin of sample_argmax_rows_final_advance): row t was fed tok[t] -- tok[0] the last sampled token, tok[1 .. T - 1] the
 * drafts -- and a_t is the argmax over the `blocks` partials a matvec_rows lm_head launch left at scratch + t * sample_scratch_bytes(), ties to the lowest index.
 * n = the first t in [0, T - 1) with a_t != tok[t + 1], else T - 1: the longest correct draft prefix.  Writes result = {n + 1, a_0 .. a_n} (int32 [T + 1], device;
 * words past a_n are left alone), tok[0] = a_n and *position_dev += n + 1.  One launch, plain vector stores. */
MILA_API int mila_cdna4_sample_argmax_chain_accept(int32_t* tok, int32_t* result, const void* scratch, size_t scratch_bytes, int blocks, int32_t* position_dev, int T,
                                                   mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The radix sampler over 1 .. 4 rows in ONE pipeline (ABI 4, additive): the stochastic twins of the two greedy tails above.  Row b reads logits + b * logits_stride
 * floats (logits_stride >= vocab) and samples at its own draw draws[b] (one float in [0, 1] per row; device or host-visible memory, read with one system-scope load, so
 * a host may rewrite the draws between replays of a captured call).  A call launches what sample_radix_plan_describe reports for ONE row -- the rows ride in the grid.
 * ROW INVARIANCE: row b's token is the token sample_radix_fp32 returns on row b's logits with r = draws[b], for every input and every draw, whatever the other rows
 * hold (a NaN included): per row every launch extent, chunk and float summation order is the one-row entry's.
 *   scratch: sample_radix_rows_scratch_bytes(rows, vocab) = rows x (sample_radix_scratch_bytes(vocab) rounded up to 8) bytes, 8-byte aligned; 0 for rows outside 1 .. 4
 *     or vocab <= 0.
 *   sample_radix_rows_fp32: token_out[b] = row b's sample, b < rows; nothing is advanced.
 *   sample_radix_rows_advance_fp32: the tail of a captured rows step -- where active_dev[b] != 0, token_out[b] = row b's sample and positions_dev[b] += 1; an inactive
 *     row's token and position words are not touched.
 *   sample_radix_chain_accept_fp32: the tail of a captured chain step, sample_argmax_chain_accept's rule with the samples s_t in the place of the argmaxes a_t: row t was
 *     fed tok[t]; n = the first t in [0, T - 1) with s_t != tok[t + 1], else T - 1; result = {n + 1, s_0 .. s_n} (words past s_n are left alone), tok[0] = s_n,
 *     *position_dev += n + 1.  With draws[t] the draw the one-row loop would use for that token, the emitted tokens ARE the one-row loop's tokens (coupled draws): a
 *     deterministic draft d is accepted exactly when the plain sampler would have drawn d, i.e. with probability p(d).
 * Refused before any device work: rows outside 1 .. 4 (T outside 2 .. 4), vocab <= 0, logits_stride < vocab, temperature <= 0, top_k < 0, top_p <= 0, a null
 * pointer, a misaligned scratch (MILA_E_INVALID_ARGUMENT); a scratch that is too small (MILA_E_SCRATCH_TOO_SMALL). */
MILA_API size_t mila_cdna4_sample_radix_rows_scratch_bytes(int rows, int vocab);
MILA_API int mila_cdna4_sample_radix_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature,
                                               int top_k, float top_p, const float* draws, void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                       float temperature, int top_k, float top_p, const float* draws, void* scratch, size_t scratch_bytes,
                                                       int32_t* positions_dev, const int32_t* active_dev, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_chain_accept_fp32(int32_t* tok, int32_t* result, const float* logits, size_t logits_stride, int T, int vocab, float softcap,
                                                       float temperature, int top_k, float top_p, const float* draws, void* scratch, size_t scratch_bytes,
                                                       int32_t* position_dev, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Token log-probabilities of a decode step (ABI 4, additive; csrc/logprobs.hip): how probable the chosen token was, and the top-n alternatives, from the fp32 logits on
 * the device -- no logits readback.  With z_i = softcap > 0 ? softcap * tanhf(x_i / softcap) : x_i, m = max z and S = sum expf(z_i - m):
 *     logprob_i = (z_i - m) - logf(S)
 * the model's distribution, independent of temperature, top-k and top-p.  "Top-n" = the n largest z, value descending, then LOWER index first (the greedy sampler's tie
 * rule: on a greedy step top_ids[0] is the emitted token).  top_n = 0 .. min(20, vocab); 0 = the chosen token's log-probability only.
 * A call is two launches: per row <= 256 workgroups leave (max, sum, local top-n) partials in scratch, then one workgroup per row merges them in a fixed order (ascending
 * workgroup index) and reads the token from a DEVICE word.  No floating-point atomics: the same bits run to run.
 *   scratch: token_logprobs_scratch_bytes(rows, vocab, top_n) bytes, 4-byte aligned; 0 for rows outside 1 .. 4, vocab <= 0 or top_n outside 0 .. min(20, vocab).
 *   token_logprobs_rows_fp32: row b reads logits + b * logits_stride floats (logits_stride >= vocab; the pad is never read) and reports the token tokens_dev[b]:
 *     logprob_out[b], top_ids_out[b * top_n ..], top_logprobs_out[b * top_n ..] (the two lists may be NULL when top_n = 0).  A row is LEFT UNTOUCHED when active_dev is
 *     given and active_dev[b] == 0 (a rows step: the active words), or when count_dev is given and b >= *count_dev (a chain step: tokens_dev = result + 1, count_dev =
 *     result -- only the accepted rows have a token).  ROW INVARIANCE: row b's outputs are, bit for bit, those of a rows = 1 call on that row alone, whatever the other
 *     rows hold.  A token outside [0, vocab) reports NaN and reads nothing; when the token is one of the top ids its logprob has that entry's bits.
 *   token_logprobs_publish_fp32: the one-row form for a decode-ahead loop, the same pair of launches.  The final reads s = *seq_dev -- which the step's tail or
 *     snapshot_token has already bumped for this sample -- and writes one record of token_logprobs_record_words() = 44 32-bit words at ring + (s % ring_size) * 44
 *     (host-visible memory): [0] tag = the low 32 bits of s, stored LAST by the lane that wrote the payload (release, system scope), [1] token, [2] logprob bits,
 *     [3] top_n, [4 .. 24) ids, [24 .. 44) logprob bits (only the first top_n of each are written).
 * Refused before any device work: a null pointer, rows outside 1 .. 4, vocab <= 0, top_n out of range, logits_stride < vocab, ring_size <= 0, a misaligned scratch or
 * ring (MILA_E_INVALID_ARGUMENT); a scratch that is too small (MILA_E_SCRATCH_TOO_SMALL). */
MILA_API int mila_cdna4_token_logprobs_record_words(void);
MILA_API size_t mila_cdna4_token_logprobs_scratch_bytes(int rows, int vocab, int top_n);
MILA_API int mila_cdna4_token_logprobs_rows_fp32(const float* logits, size_t logits_stride, const int32_t* tokens_dev, int rows, int vocab, float softcap, int top_n,
                                                 const int32_t* active_dev, const int32_t* count_dev, float* logprob_out, int32_t* top_ids_out,
                                                 float* top_logprobs_out, void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_token_logprobs_publish_fp32(const float* logits, const int32_t* token_dev, int vocab, float softcap, int top_n,
                                                    const unsigned long long* seq_dev, uint32_t* ring, int ring_size, void* scratch, size_t scratch_bytes,
                                                    mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Prompt log-probabilities (ABI 4, additive; csrc/lm_head_score.hip): the lm_head over MANY rows -- a prefill chunk -- as a matrix-core GEMM whose epilogue keeps the
 * softmax statistics and never stores a logit (fp32 logits of a 2048-row chunk would be 2 GB).  For row r, with t = targets_dev[r]:
 *     y_i = sum_k x[r,k] * W[i,k]     accumulated in fp32 on the matrix cores.  fmt 1: the e4m3 byte enters as its exact bf16 value and scales[i] multiplies ONCE after
 *                                     the reduction -- matvec_f32out's arithmetic, so a prompt position scores with the arithmetic the decode head would have used
 *                                     (not the prefill GEMM's bf16(decode * scale))
 *     z_i = softcap > 0 ? softcap * tanhf(y_i / softcap) : y_i,   m = max z,   S = sum expf(z_i - m)
 *     logprob_out[r] = (z_t - m) - logf(S); a target outside [0, vocab) reports NaN and reads nothing (-1 = "no target")
 *     argmax_out[r] = the index of the largest z, the LOWEST index among equals (the greedy sampler's tie rule); argmax_logprob_out[r] = its log-probability.  The two
 *     may both be NULL.  When the target is the argmax the two log-probabilities carry the same bits.
 *   x: `rows` normed hidden rows, bf16, x_stride elements apart.  W: the [vocab, K] table; fmt 0 = bf16, 1 = e4m3 with scales[vocab].
 * Two launches.  Partials: one workgroup owns a block of 128 rows and a SLAB of the vocabulary, walks it 128 columns at a time through a 128 x 128 x 64 K loop, and
 * leaves one 32-byte record per (row, slab) in scratch: (max, sum exp rescaled to that max, best z, best index, the target's z).  Final: one wave per row merges the
 * records in ascending slab order, rescaled to the global max.  No floating-point atomics, every sum has a fixed order: the same bits run to run.
 * THE SLAB RULE looks at vocab alone: with tiles = ceil(vocab / 128), a slab is ceil(tiles / 256) tiles, so there are at most 256 slabs -- 262144 entries: 1024 columns
 * per slab, 256 slabs, so a call of a few rows still occupies every CU and scratch stays at 32 bytes per (row, slab).
 * ROW INVARIANCE: row r's three outputs are, bit for bit, those of a rows = 1 call on that row alone, whatever the other rows hold, however many there are and wherever
 * r sits in the call (padded rows are zero-filled; neither the tile shape nor the slab rule looks at rows).
 *   scratch: lm_head_score_scratch_bytes(rows, vocab) = rows * slabs * 32 bytes, 16-byte aligned; 0 for rows < 1 or vocab < 1.
 * Refused before any device work: a null x, W, targets_dev or logprob_out, exactly one of the two argmax pointers, fmt outside {0, 1}, fmt 1 without scales, rows < 1,
 * vocab < 1, K no multiple of 8 (bf16) or 16 (e4m3), x_stride < K, a misaligned scratch (MILA_E_INVALID_ARGUMENT); a scratch that is too small
 * (MILA_E_SCRATCH_TOO_SMALL). */
MILA_API size_t mila_cdna4_lm_head_score_scratch_bytes(int rows, int vocab);
MILA_API int mila_cdna4_lm_head_score_bf16(const uint16_t* x, size_t x_stride, const void* W, const float* scales, int fmt, int K, int vocab,
                                           const int32_t* targets_dev, int rows, float softcap, float* logprob_out, int32_t* argmax_out,
                                           float* argmax_logprob_out, void* scratch, size_t scratch_bytes, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sampling filters (ABI 4, additive; csrc/sampling.hip): repetition, presence and frequency penalties and min-p, as filters over the samplers above.  The reference's
 * sampling specification (Specifications/TokenSampling.md 3.3, 4.2) names "top-k, top-p, min-p, and repetition penalty" as composable filters over one sampler and
 * pencils them into GenerateParams; the reference has NO kernel for them yet, so these entries anticipate that surface and replace no launcher.
 *
 * THE TABLE.  The state of one sequence is a table of `vocab` 32-bit words on the device (token_table_bytes(vocab) bytes): bit 31 = the token occurs in the prompt,
 * bits 0 .. 30 = c, the number of times the token has been generated in this request.  token_table_clear zeroes row `row` of a table (table + row * table_stride
 * words); token_table_mark_prompt sets bit 31 of the words of n token ids held in DEVICE memory -- into a cleared table, before the first sample (it stores the flag
 * with c = 0); repeats are fine, ids outside [0, vocab) are skipped.
 *
 * THE ADJUSTED LOGIT of a logit l whose table word is w, all in fp32, every operation rounded on its own (no fused multiply-add), so that a host can restate it bit
 * for bit:
 *     x0 = softcap > 0 ? softcap * tanhf(l / softcap) : l                    (as in sample_radix_*)
 *     x1 = w != 0 ? (x0 > 0 ? x0 * inv_rep : x0 * rep) : x0                  inv_rep = 1.0f / rep, divided once on the host
 *     x2 = x1 - (freq * (float)c)
 *     x3 = c > 0 ? x2 - pres : x2
 *     x  = x3 / temperature                                                  (as in sample_radix_*)
 * The repetition penalty covers prompt and generated tokens (the HF / vLLM convention); presence and frequency cover generated tokens only (the OpenAI / vLLM
 * convention).  Penalties come after the softcap (HF applies them to Gemma's already capped logits) and before the temperature.
 * MIN-P.  After the nucleus cut (top-k, then top-p, then min-p) a surviving entry with e = expf(x - max) < min_p is dropped: the tokens whose probability is at least
 * min_p times the top token's stay.
 * GREEDY.  sample_argmax_filtered_* take argmax(x3), ties to the lower id (the softcap first: the penalty touches only some tokens).  min_p does not change a greedy
 * request.
 * THE UPDATE.  Every entry that is given a table adds 1 to table[s] after choosing token s: one lane, a plain load and a plain store, before the token is stored or
 * published; the rows advance forms touch the active rows only.  The next call reads the table across a kernel boundary.
 * The samplers write their scaled copy into scratch and never touch `logits`: log-probabilities (token_logprobs_*) stay those of the capped, UNPENALIZED logits.
 *
 * filters: read on the host at enqueue; NULL = the neutral values {min_p 0, repetition 1, presence 0, frequency 0}.  table: NULL = no penalties and no update (min_p
 * still holds in the stochastic entries; the greedy entries are then sample_argmax_* on the logits as they are).  table_stride: words between the tables of two rows.
 * A filtered call launches exactly what sample_radix_plan_describe reports for the unfiltered call (the table rides in the scale launch, min-p in the mask launch, the
 * update in the tail); with a NULL table and min_p = 0 it launches the unfiltered kernels themselves.  The greedy entries are the two launches of sample_argmax_*.
 *   sample_filters_describe: "launches:k_passes:p_passes:scratch_need:scale_filtered:mask_filtered" -- sample_radix_plan_describe's text and whether the scale / the mask
 *     launch is the filtered instantiation (with_table: a table would be given).  0 for arguments the entries refuse.  No device work.
 *   scratch: as for the entry each one mirrors (sample_radix_scratch_bytes, sample_radix_rows_scratch_bytes, sample_scratch_bytes; the rows greedy entry rows x
 *     sample_scratch_bytes()).
 * Refused before any device work, beside what the mirrored entry refuses: repetition_penalty <= 0, a non-finite filter value, min_p outside [0, 1), table_stride < vocab
 * with more than one row (MILA_E_INVALID_ARGUMENT). */
typedef struct mila_sample_filters
{
    float min_p;                  /* [0, 1); 0 = off */
    float repetition_penalty;     /* > 0; 1 = off */
    float presence_penalty;       /* 0 = off */
    float frequency_penalty;      /* 0 = off */
} mila_sample_filters;
MILA_API size_t mila_cdna4_token_table_bytes(int vocab);
MILA_API int mila_cdna4_token_table_clear(uint32_t* table, size_t table_stride, int row, int vocab, mila_stream_t stream);
MILA_API int mila_cdna4_token_table_mark_prompt(uint32_t* table, size_t table_stride, int row, int vocab, const int32_t* tokens_dev, int n, mila_stream_t stream);
MILA_API size_t mila_cdna4_sample_filters_describe(int vocab, int top_k, float top_p, const mila_sample_filters* filters, int with_table, char* buf, size_t cap);
MILA_API int mila_cdna4_sample_radix_filtered_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                                   const mila_sample_filters* filters, uint32_t* table, void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_filtered_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p,
                                                           const float* draws, int draws_size, const mila_sample_filters* filters, uint32_t* table, void* scratch,
                                                           size_t scratch_bytes, int32_t* position_dev, unsigned long long* seq_dev, unsigned long long* ring,
                                                           int ring_size, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_filtered_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                        float temperature, int top_k, float top_p, const float* draws, const mila_sample_filters* filters, uint32_t* table,
                                                        size_t table_stride, void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_filtered_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                                float temperature, int top_k, float top_p, const float* draws, const mila_sample_filters* filters,
                                                                uint32_t* table, size_t table_stride, void* scratch, size_t scratch_bytes, int32_t* positions_dev,
                                                                const int32_t* active_dev, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_filtered_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters, uint32_t* table,
                                                    void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_filtered_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters,
                                                            uint32_t* table, void* scratch, size_t scratch_bytes, int32_t* position_dev, unsigned long long* seq_dev,
                                                            unsigned long long* ring, int ring_size, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_filtered_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                                 const mila_sample_filters* filters, uint32_t* table, size_t table_stride, void* scratch,
                                                                 size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Logit bias (ABI 4, additive; csrc/sampling.hip): an additive bias per token, and through it banned tokens, a closed answer set (allowed tokens) and min_tokens (the
 * stop tokens banned until the n-th sample) -- the `logit_bias`, `bad_words_ids`, `allowed_token_ids` and `min_tokens` of the HF / OpenAI / vLLM front ends.  All four
 * are ONE mechanism: a dense table of fp32 values, read beside the logits in the sampler's first launch.  The reference names composable filters over one sampler
 * (Specifications/TokenSampling.md 3.3) and ships an OpenAI-compatible server, but has no kernel for any of this: these entries anticipate that surface and replace no
 * launcher.  Mila/TokenBias.h (host only) composes a request's four controls into a table.
 *
 * THE TABLE.  `vocab` fp32 values per row on the device (token_bias_bytes(vocab) bytes), each finite or -inf.  token_bias_fill sets row `row` of a table
 * (bias + row * bias_stride floats) to one value; token_bias_set scatters n values to n token ids, both held in DEVICE memory: ids outside [0, vocab) are skipped,
 * duplicate ids in one call are the caller's to avoid (two plain stores race).  Both run in stream order: a table may be updated between two replays of a captured step
 * that reads it (the pointer is what is captured).
 *
 * THE ADJUSTED LOGIT gains one step between the softcap and the penalties of the sampling-filters section:
 *     x0 = softcap > 0 ? softcap * tanhf(l / softcap) : l
 *     xb = x0 + bias[i]                                                      one fp32 addition, rounded to nearest; only where a bias table is given
 *     x1 .. x3 = the penalties, on xb in the place of x0
 *     x  = x3 / temperature
 * The bias comes before the penalties (vLLM's order: the repetition penalty's sign test sees the biased value) and after the softcap (the capped logits are the
 * model's logits).  -inf stays -inf through every later step: x1 is a product with rep or 1 / rep > 0, x2 and x3 subtract finite values, the temperature is positive.
 * A TOKEN WHOSE BIAS IS -inf IS NEVER RETURNED, at any draw in [0, 1] and under any top-k / top-p / min-p: its e = expf(-inf - max) is 0, the walk of the inverse CDF
 * visits only e > 0, and where the running sum never reaches r * total (the two are added in different orders, so next to r = 1 they can differ) every stochastic
 * entry, biased or not, returns the LAST entry with nonzero mass, never vocab - 1 for its own sake.  Caller's contract: at least one token of a row has a finite bias.
 * GREEDY.  sample_argmax_biased_* take argmax(x3), ties to the lower id, in the two launches of sample_argmax_filtered_*; the table may be NULL (a bias without
 * penalties).
 * The samplers never write `logits`: log-probabilities (token_logprobs_*, the scoring entries) stay those of the capped, UNBIASED logits.
 *
 * Each sample_*_biased_* entry is the sample_*_filtered_* entry of the same name plus `bias, bias_stride`, and the filtered entries are calls of them.  bias: row 0's
 * table; NULL = exactly the filtered entry, including its NULL-table behaviour, launching the kernels it launched.  bias_stride: floats between the tables of two rows;
 * 0 = one table shared by all rows; with more than one row a stride from 1 to vocab - 1 is refused.  A biased call launches exactly what sample_radix_plan_describe
 * reports for the unfiltered call: the bias rides in the scale launch (four instantiations: none, table, bias, table + bias), and the tail is the
 * unbiased call's.  Scratch: as for the mirrored entry.
 * Refused before any device work, beside what the mirrored entry refuses (MILA_E_INVALID_ARGUMENT): a NaN or +inf fill value; n < 0; a null table, id or value pointer with
 * n > 0; the stride rule above. */
MILA_API size_t mila_cdna4_token_bias_bytes(int vocab);
MILA_API int mila_cdna4_token_bias_fill(float* bias, size_t bias_stride, int row, int vocab, float value, mila_stream_t stream);
MILA_API int mila_cdna4_token_bias_set(float* bias, size_t bias_stride, int row, int vocab, const int32_t* ids_dev, const float* values_dev, int n, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_biased_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                                 const mila_sample_filters* filters, uint32_t* table, const float* bias, size_t bias_stride, void* scratch,
                                                 size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_biased_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p,
                                                         const float* draws, int draws_size, const mila_sample_filters* filters, uint32_t* table, const float* bias,
                                                         size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* position_dev, unsigned long long* seq_dev,
                                                         unsigned long long* ring, int ring_size, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_biased_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                      float temperature, int top_k, float top_p, const float* draws, const mila_sample_filters* filters, uint32_t* table,
                                                      size_t table_stride, const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes,
                                                      mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_biased_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                              float temperature, int top_k, float top_p, const float* draws, const mila_sample_filters* filters,
                                                              uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride, void* scratch,
                                                              size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_biased_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters, uint32_t* table,
                                                  const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_biased_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters,
                                                          uint32_t* table, const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes,
                                                          int32_t* position_dev, unsigned long long* seq_dev, unsigned long long* ring, int ring_size,
                                                          mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_biased_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                               const mila_sample_filters* filters, uint32_t* table, size_t table_stride, const float* bias,
                                                               size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* positions_dev,
                                                               const int32_t* active_dev, mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Token automaton (ABI 4, additive; csrc/sampling.hip): grammar-constrained decoding -- the set of tokens a request may emit changes with every token it emits.  The
 * constraint is a deterministic automaton over token ids, brought by the caller (tokenizers and the regex / JSON-schema compilers that produce one stay outside this
 * library): what vLLM, TGI and llama.cpp reach through a per-step logits mask built on the host.  Here the state and the mask live on the device, so a step that samples
 * token n + 1 before the host has seen token n stays closed.  The samplers are untouched: they already honour a dense fp32 table of "finite or -inf" exactly (logit
 * bias, above); these entries maintain such a table, `eff`, and the sample_*_biased_* entries read it in the place of the bias table.  The reference re-parses what the
 * model emitted (Gemma.Protocol.ixx) and has no kernel for any of this.  Mila/TokenAutomaton.h (host only) holds, checks and compresses an automaton.
 *
 * THE IMAGE.  token_automaton_bytes(vocab, S, C) bytes on the device: class_of[vocab] uint16 (token id -> class, < C), then next[S * C] uint16 (state x class -> next
 * state, < S, or 0xFFFF = FORBIDDEN: the token may not be emitted in that state).  1 <= S, C <= 65535 and S * C * 2 bytes <= 256 MiB (bytes returns 0 otherwise).
 * THE STATE.  One int32 word per row (state_dev[rows]) and, for step, one uint32 ticket word per row that is 0 between launches (ticket_dev[rows]).
 *
 * compose: for row b with s = state_dev[b]:   eff[b * eff_stride + i] = next[s * C + class_of[i]] != FORBIDDEN ? base[b * base_stride + i] : -inf   for every i.
 *     base == NULL: 0.0f in the place of base; base_stride == 0: one base table shared by the rows.  The base value passes through bit for bit.  The state stays.
 * step: for every row b whose active_dev[b] != 0 (active_dev == NULL: every row): s' = next[s * C + class_of[token_dev[b]]]; FORBIDDEN (only a token the mask forbade)
 *     or a token outside [0, vocab) leaves s' = s; then eff[b] is composed for s' and state_dev[b] = s'.  An inactive row keeps its state and its table bytes.
 * Both are ONE launch for all rows (the row in blockIdx.y, as the radix stages), in stream order: step goes behind the sampler tail that wrote token_dev, the next
 * step's sampler reads eff.  Every workgroup of a step launch reads the state word and one stores it; a ticket (one agent-scope atomic add per workgroup, taken after
 * the reads) makes the workgroup that draws the last one the writer, so no workgroup can read the advanced state -- no grid barrier, no second launch.  A state word
 * outside [0, S) is read as 0.  The walk uses 16-byte accesses where eff and base are 16-byte aligned with strides that are multiples of 4 and class_of is 8-byte
 * aligned, scalar ones otherwise.
 * Refused before any device work (MILA_E_INVALID_ARGUMENT): a null eff, class_of, next or state_dev (step: token_dev, ticket_dev); rows outside 1 .. 4; vocab <= 0, S
 * or C outside the limits above; with more than one row an eff_stride below vocab; a base_stride from 1 to vocab - 1. */
MILA_API size_t mila_cdna4_token_automaton_bytes(int vocab, int S, int C);
MILA_API int mila_cdna4_token_automaton_compose(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next,
                                                int S, int C, int32_t* state_dev, int rows, int vocab, mila_stream_t stream);
MILA_API int mila_cdna4_token_automaton_step(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next, int S,
                                             int C, int32_t* state_dev, const int32_t* token_dev, const int32_t* active_dev, uint32_t* ticket_dev, int rows, int vocab,
                                             mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The constrained chain step (ABI 4, additive; csrc/sampling.hip): the bias table and the automaton in a chain step (sample_*_chain_accept above), so that a constrained
 * request can verify drafts -- in particular the tokens its automaton FORCES (a state that allows one token: the successor is known before the model runs).
 *
 * STATE SEMANTICS IN A CHAIN STEP.  state_dev[0] is the state after every token sampled so far, tok[0] included, as in the one-row step.  Row t was fed tok[t]; its
 * sample obeys q_t:  q_0 = state_dev[0],  q_t = next[q_{t-1} * C + class_of[tok[t]]],  and a draft that is FORBIDDEN in q_{t-1} or lies outside [0, vocab) leaves
 * q_t = q_{t-1} (the step entry's rule).  Such a draft is never accepted -- row t - 1 never samples it -- so the rows behind it only need a well-defined table.
 *
 * token_automaton_chain_compose: ONE launch, the first node of the step.  For t = 1 .. T - 1 (the row in blockIdx.y) eff[t * eff_stride + i] is composed for q_t by
 *     compose's rule from base[t * base_stride + i] (base == NULL: 0.0f; base_stride == 0: one shared table), and q_0 .. q_{T-1} are stored to chain_states[0 .. T - 1]
 *     (int32, device).  Row 0 of eff is NOT touched: every step leaves it composed for state_dev[0] (compose at the start of a request, step / chain_step behind every
 *     tail).  Every workgroup walks its row's at most 3 dependent lookups itself; the launch stores nothing that it reads (state_dev and tok_dev are read only), so it
 *     takes no ticket.  The walk is compose's, 16-byte path and scalar fallback included.
 * token_automaton_chain_step: ONE launch behind the accept tail, which left result[0] = n (the accepted count, 1 .. T; any other value is read as 1) and tok[0] = the
 *     last accepted sample.  It is step on row 0 with the state read from chain_states[n - 1] and the token from tok[0]: state_dev[0] = s', eff row 0 composed for s'
 *     from base row 0.  ticket_dev: one uint32 word, 0 between launches, step's discipline (every workgroup reads before it draws; the last ticket's holder stores).
 *     It touches row 0 only: eff_stride and base_stride are the chain's (checked as chain_compose checks them) and decide no more than the 16-byte path.
 * Refused before any device work (MILA_E_INVALID_ARGUMENT): a null eff, class_of, next, state_dev, tok_dev or chain_states (chain_step: result_dev, ticket_dev); T
 * outside 2 .. 4; the shape limits of the image; an eff_stride below vocab; a base_stride from 1 to vocab - 1.
 *
 * sample_radix_biased_chain_accept_fp32 is sample_radix_chain_accept_fp32 plus `bias, bias_stride`; sample_argmax_biased_chain_accept_fp32 is the greedy chain tail from
 * the LOGITS: the two launches of sample_argmax_biased_rows_advance_fp32 (the biased first stage over T rows, one final), the final being sample_argmax_chain_accept's.
 * Row t's sample is the token the one-row biased entry (sample_radix_biased_fp32 with r = draws[t]; sample_argmax_biased_fp32) returns on row t's logits with the table
 * bias + t * bias_stride; the acceptance rule, result, tok[0] and the position word are the unbiased chain entry's.  bias_stride 0 = one table shared by all rows (a
 * request's bias table); bias_stride >= vocab = one per row (the automaton's eff rows); 1 .. vocab - 1 is refused.  A token whose entry is -inf is never returned;
 * caller's contract: every row's table has a finite entry.  The bias rides in the scale launch (radix) or the first stage (greedy): only the tail differs from the rows
 * entries, and it is the unbiased chain tail.  radix: bias == NULL launches exactly sample_radix_chain_accept_fp32.  greedy: bias is required -- without one the chain's
 * partials come from the lm_head launch and sample_argmax_chain_accept is the whole tail.  scratch: sample_radix_rows_scratch_bytes(T, vocab) / T *
 * sample_scratch_bytes().  NO PENALTIES AND NO MIN-P IN A CHAIN: row t would need the token table plus the drafts 1 .. t, so these entries take no filters and no
 * table, and a request with such settings stays on the one-row step.  Neither entry writes logits or bias.
 * Refused before any device work: what the unbiased chain entry refuses (greedy: a null tok, result, logits, bias or position_dev; T outside 2 .. 4; vocab <= 0;
 * logits_stride < vocab; a short scratch, MILA_E_SCRATCH_TOO_SMALL), the stride rule, a bias pointer that is not 4-byte aligned. */
MILA_API int mila_cdna4_token_automaton_chain_compose(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of,
                                                      const uint16_t* next, int S, int C, const int32_t* state_dev, const int32_t* tok_dev, int32_t* chain_states, int T,
                                                      int vocab, mila_stream_t stream);
MILA_API int mila_cdna4_token_automaton_chain_step(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next,
                                                   int S, int C, int32_t* state_dev, const int32_t* tok_dev, const int32_t* chain_states, const int32_t* result_dev, int T,
                                                   uint32_t* ticket_dev, int vocab, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_biased_chain_accept_fp32(int32_t* tok, int32_t* result, const float* logits, size_t logits_stride, int T, int vocab, float softcap,
                                                              float temperature, int top_k, float top_p, const float* draws, const float* bias, size_t bias_stride,
                                                              void* scratch, size_t scratch_bytes, int32_t* position_dev, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_biased_chain_accept_fp32(int32_t* tok, int32_t* result, const float* logits, size_t logits_stride, int T, int vocab, float softcap,
                                                               const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* position_dev,
                                                               mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row requests (ABI 4, additive; csrc/sampling.hip): a rows call whose rows each carry their OWN request -- a greedy constrained row next to a temperature-0.9 row
 * next to a penalized one.  The entries above take one temperature / top_k / top_p / filters for every row as launch arguments; here they live in DEVICE memory, one
 * record per row, so that a captured rows step serves a new set of requests without being captured again (the rule the bias tables and the automaton already keep).
 *
 * THE RECORD.  mila_sample_row_params, 32 bytes per row, sample_row_params_bytes(rows) = rows x 32 (0 for rows outside 1 .. 4).  temperature <= 0 makes the row GREEDY.
 * inv_rep is an output of the setter (1.0f / repetition_penalty, divided once on the host as the filtered entries do); what a caller puts there is ignored.
 * sample_row_params_set validates ONE row's record on the host and stores it into params_dev[row] in stream order (one lane, plain vector stores): behind the steps
 * enqueued before it, in front of those enqueued after.  Refused before any device work (MILA_E_INVALID_ARGUMENT): a null pointer, a misaligned params_dev, row outside
 * 0 .. 3, a temperature that is not finite, top_k < 0, top_p <= 0 or NaN, and what the filtered entries refuse (a non-finite filter, repetition_penalty <= 0, min_p
 * outside [0, 1)).
 *
 * THE STOCHASTIC ROWS.  sample_radix_requests_rows_fp32 / _advance_fp32 launch the FULL radix plan (scale, 3 top-k passes, prob, 2 further nucleus passes, mask, tail:
 * 9 launches, what top_k and top_p both on launch today) with the rows in the grid.  Every stage reads its row's record: a row with top-k off (top_k = 0 or >= vocab)
 * returns from the top-k passes at once, a row with top-p off (top_p >= 1) from the nucleus passes; a GREEDY or (advance form) INACTIVE row returns from every stage.
 * Row b reads logits + b * logits_stride, draws[b] (as in sample_radix_rows_fp32), its bias row bias + b * bias_stride (bias NULL: none; bias_stride 0: shared) and,
 * only where its record has a penalty (repetition_penalty != 1 or presence / frequency != 0), its table table + b * table_stride.
 * ROW INVARIANCE: row b's token is the token sample_radix_biased_fp32 / sample_radix_filtered_fp32 returns on row b's logits with row b's parameters, table (NULL where
 * the record has no penalty), bias row and r = draws[b], for every input and every draw, whatever the other rows hold (a NaN included) and whatever their records say:
 * the stages run the one-row entry's bodies, so per row every launch extent, chunk, walk order and float summation is the one-row entry's.
 * The tail (one wave per row, then one lane's plain stores) acts on the rows that are active and stochastic ONLY: token_out[b] = the sample, (advance)
 * positions_dev[b] += 1, and table[b][sample] += 1 where the row has a penalty.  Every other row's token, position and table words are not touched.
 *
 * THE GREEDY ROWS.  sample_argmax_requests_rows_fp32 / _advance_fp32 are the two launches of sample_argmax_biased_rows_advance_fp32 reading the record: argmax(x3) over
 * the capped logit, the row's bias and (where the record has a penalty) the row's table, ties to the LOWEST id; a row with neither bias nor penalty takes the logits
 * as they are (sample_argmax_fp32).  A greedy row's logit is never divided by a temperature.  The tail acts on the rows that are active and greedy ONLY.
 * Row b's token is sample_argmax_biased_fp32's on row b alone.  The soft cap is monotone but can merge two neighbouring logits into a tie, so a greedy row WITHOUT a
 * bias must not be given a row of zeros where it is to keep the token of the uncapped logits: a caller whose batch holds both kinds of greedy row calls the entry twice,
 * once with the tables and once with bias = NULL, each with an active mask that selects its rows (Mila/Gemma.h keeps the two masks on the device).
 * Enqueued one behind the other, the two advance entries advance each active row exactly once; a step without greedy (stochastic) rows may leave the greedy
 * (stochastic) entry out.
 *   scratch: radix -- sample_radix_rows_scratch_bytes(rows, vocab), 8-byte aligned; argmax -- rows x sample_scratch_bytes(), 4-byte aligned.
 * Refused before any device work: a null logits, token_out, params_dev (radix: draws; advance: positions_dev, active_dev), rows outside 1 .. 4, vocab <= 0,
 * logits_stride < vocab, with more than one row a table_stride below vocab or a bias_stride from 1 to vocab - 1, a misaligned pointer or scratch
 * (MILA_E_INVALID_ARGUMENT); a scratch that is too small (MILA_E_SCRATCH_TOO_SMALL).
 *
 * THE AUTOMATON PER ROW.  token_automaton_rows_compose / _rows_step are token_automaton_compose / _step with the image of row b taken from a descriptor in device
 * memory: mila_token_automaton_row {class_of, next, S, C}, 24 bytes per row, token_automaton_rows_bytes(rows).  token_automaton_rows_set validates one row's image
 * shape on the host and stores the descriptor in stream order; class_of = next = NULL stores a NULL DESCRIPTOR: the row has no automaton -- its eff row is not
 * written, its state word not read and it takes no ticket.  State word, ticket word and active word per row as in token_automaton_step, with its ordering argument:
 * every workgroup reads state and token before it draws its ticket, and the holder of the row's last ticket stores the state and zeroes the ticket.  Row b's state
 * sequence and eff row are token_automaton_step's on that row alone.  The 16-byte walk needs, beside the one-row entry's conditions on eff and base, row b's class_of
 * 8-byte aligned (tested per row on the device).
 * Refused before any device work (MILA_E_INVALID_ARGUMENT): a null or misaligned desc_dev, row outside 0 .. 3, exactly one of class_of / next, the shape limits of the
 * image; compose / step: a null eff or state_dev (step: token_dev, ticket_dev), rows outside 1 .. 4, vocab <= 0, with more than one row an eff_stride below vocab, a
 * base_stride from 1 to vocab - 1. */
typedef struct mila_sample_row_params
{
    float temperature;            /* > 0: stochastic; <= 0: greedy */
    int32_t top_k;                /* 0 or >= vocab = off */
    float top_p;                  /* (0, 1); >= 1 = off */
    float min_p;                  /* [0, 1); 0 = off */
    float repetition_penalty;     /* > 0; 1 = off */
    float inv_rep;                /* written by the setter */
    float presence_penalty;       /* 0 = off */
    float frequency_penalty;      /* 0 = off */
} mila_sample_row_params;
typedef struct mila_token_automaton_row
{
    const uint16_t* class_of;     /* NULL: the row has no automaton */
    const uint16_t* next;
    int32_t S, C;
} mila_token_automaton_row;
MILA_API size_t mila_cdna4_sample_row_params_bytes(int rows);
MILA_API int mila_cdna4_sample_row_params_set(void* params_dev, int row, const mila_sample_row_params* params, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_requests_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                        const void* params_dev, const float* draws, uint32_t* table, size_t table_stride, const float* bias,
                                                        size_t bias_stride, void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_radix_requests_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                                const void* params_dev, const float* draws, uint32_t* table, size_t table_stride, const float* bias,
                                                                size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* positions_dev,
                                                                const int32_t* active_dev, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_requests_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                         const void* params_dev, uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride,
                                                         void* scratch, size_t scratch_bytes, mila_stream_t stream);
MILA_API int mila_cdna4_sample_argmax_requests_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                                 const void* params_dev, uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride,
                                                                 void* scratch, size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev,
                                                                 mila_stream_t stream);
MILA_API size_t mila_cdna4_token_automaton_rows_bytes(int rows);
MILA_API int mila_cdna4_token_automaton_rows_set(void* desc_dev, int row, const uint16_t* class_of, const uint16_t* next, int S, int C, int vocab,
                                                 mila_stream_t stream);
MILA_API int mila_cdna4_token_automaton_rows_compose(float* eff, size_t eff_stride, const float* base, size_t base_stride, const void* desc_dev, int32_t* state_dev,
                                                     int rows, int vocab, mila_stream_t stream);
MILA_API int mila_cdna4_token_automaton_rows_step(float* eff, size_t eff_stride, const float* base, size_t base_stride, const void* desc_dev, int32_t* state_dev,
                                                  const int32_t* token_dev, const int32_t* active_dev, uint32_t* ticket_dev, int rows, int vocab,
                                                  mila_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fork a row's KV prefix (ABI 4, additive; csrc/kv_rows_fork.hip): the device primitive of a shared prefill.  A rows model keeps, per layer, K and V as
 * [rows, NKV, capacity, HS] bf16 on UNBOUNDED caches (position p at cache index p of its row), so two requests with the same prompt hold the same bits at [0, len) of
 * their rows after their prefills.  kv_rows_fork_bf16 copies, for every KV head, for K and for V, positions [0, len) of cache row `src` into every cache row whose
 * bit is set in dst_mask (bit r = row r): ONE launch that reads the source once and stores each destination, 16 bytes per lane, a flat grid-stride walk over the
 * 16-byte units with every element offset in 64 bits.  The copy is bitwise (NaN patterns and signed zeros pass through).  Nothing is written outside [0, len) of the
 * destination rows, and nothing in `src` or in a row the mask does not name.  Stream-ordered: behind the prefill that wrote `src`, in front of the steps that read
 * the destinations.  One call per layer.
 * Refused before any device work (MILA_E_INVALID_ARGUMENT): a null or misaligned (16 bytes) K or V, rows outside 2 .. 4, NKV / capacity / HS <= 0, HS no multiple
 * of 8, src outside the rows, a dst_mask that is empty, names src or names a row >= rows, len outside 1 .. capacity. */
MILA_API int mila_cdna4_kv_rows_fork_bf16(uint16_t* K, uint16_t* V, int rows, int NKV, int capacity, int HS, int src, unsigned dst_mask, int len,
                                          mila_stream_t stream);

/* kv_rows_fork_bf16 for n layers in ONE launch (ABI 4, additive; csrc/kv_rows_fork.hip): layer i has its own caches and its own (NKV, capacity, HS); the rows, src,
 * dst_mask and len are shared.  `layers` is a HOST array of n_layers records -- the caller builds it once and keeps it; the entry passes the records to the kernel
 * by value in its argument block, up to 64 layers per launch (more layers: further launches of the same call), so the call allocates nothing, copies nothing from
 * host to device and reads nothing back.  The layer is the grid's y index; within a layer a grid-stride walk over its 16-byte units, each read once from row `src`
 * and stored to every row of dst_mask, every element offset in 64 bits, plain vector loads and stores of bit patterns, no LDS, no atomics.  Byte for byte the
 * result is n_layers calls of kv_rows_fork_bf16.
 * Refused before any device work (MILA_E_INVALID_ARGUMENT), from host-known values alone, with the layer's number in the message: a null `layers`, n_layers <= 0,
 * rows outside 2 .. 4, src outside the rows, a dst_mask that is empty, names src or names a row >= rows, len < 1, and per layer kv_rows_fork_bf16's own checks -- a
 * null or misaligned K or V, NKV / capacity / HS <= 0, HS no multiple of 8, len above that layer's capacity.  A refusal launches nothing, for no layer. */
typedef struct mila_kv_fork_layer {
    uint16_t* K;            /* [rows, NKV, capacity, HS] bf16, device */
    uint16_t* V;
    int32_t NKV, capacity, HS;
    int32_t reserved;       /* 0 */
} mila_kv_fork_layer;
MILA_API int mila_cdna4_kv_rows_fork_layers_bf16(const mila_kv_fork_layer* layers, int n_layers, int rows, int src, unsigned dst_mask, int len, mila_stream_t stream);

/* kv_rows_fork_layers_bf16 for the FP8 KV cache (ABI 4, additive; csrc/kv_rows_fork.hip): layer i keeps K8 / V8 [rows, NKV, capacity, HS] e4m3 bytes and Ks / Vs
 * [rows, NKV, capacity] fp32 scales.  Per layer and KV head, positions [0, len) of cache row `src` are copied into every row of dst_mask: the bytes as 16-byte units (HS a
 * multiple of 16), the scales as 4-byte WORDS -- a head's scale run starts capacity * 4 bytes after the one before it and is len * 4 bytes long, neither 16-byte aligned in
 * general, so that copy is never widened.  Bitwise: a NaN, a -0.0 or a denormal scale passes as it is.  Nothing is written outside [0, len) of the named rows, nothing in
 * `src`.  The interface is otherwise the bf16 entry's: a HOST array passed by value in the kernel arguments, the layer in the grid's y index, up to 64 layers per launch.
 * Refused before any device work, with the layer's number in the message where one is at fault: the bf16 entry's refusals; K8 / V8 not 16-byte aligned, Ks / Vs not
 * 4-byte aligned; HS no multiple of 16; len above a layer's capacity. */
typedef struct mila_kv_fork_layer_fp8 {
    uint8_t* K8;            /* device: [rows, NKV, capacity, HS] e4m3, 16-byte aligned */
    uint8_t* V8;
    float* Ks;              /* device: [rows, NKV, capacity] fp32 */
    float* Vs;
    int32_t NKV, capacity, HS;
    int32_t reserved;       /* 0 */
} mila_kv_fork_layer_fp8;
MILA_API int mila_cdna4_kv_rows_fork_layers_kvfp8(const mila_kv_fork_layer_fp8* layers, int n_layers, int rows, int src, unsigned dst_mask, int len, mila_stream_t stream);

/* kv_rows_fork_layers_bf16 for a rows model whose sliding-window layers sit on RINGS (ABI 4, additive; csrc/kv_rows_fork.hip): position p of a row lives at cache index
 * p % capacity of its layer.  Per layer the entry copies the LIVE BAND, positions [begin, len) with begin = window > 0 ? max( 0, len - window ) : 0 -- what a continuation
 * from `len` can read (a flat layer, window 0, is the whole prefix [0, len)) -- of cache row `src` into every row of dst_mask, for every KV head, K and V.  A band that
 * crosses the ring's end is two runs of cache indices; the kernel folds a unit past the end back with one conditional subtract, the one remainder (begin % capacity) is
 * taken on the host.  Bitwise; nothing is written outside the band's cache indices of the named rows, nothing in `src`.  The interface is otherwise the bf16 entry's: a
 * HOST array passed by value in the kernel arguments, the layer in the grid's y index, up to 64 layers per launch, each unit read once, 16 bytes per lane, 64-bit offsets.
 * Refused before any device work, with the layer's number in the message where one is at fault: the bf16 entry's refusals, except that len may exceed a capacity; a
 * window < 0; a band len - begin above the layer's capacity (a flat layer with len > capacity, a ring whose window exceeds its capacity). */
typedef struct mila_kv_fork_layer_band {
    uint16_t* K;            /* [rows, NKV, capacity, HS] bf16, device */
    uint16_t* V;
    int32_t NKV, capacity, HS;
    int32_t window;         /* > 0: a ring layer's sliding window; 0: a flat layer, the whole prefix */
} mila_kv_fork_layer_band;
MILA_API int mila_cdna4_kv_rows_fork_layers_band_bf16(const mila_kv_fork_layer_band* layers, int n_layers, int rows, int src, unsigned dst_mask, int len,
                                                      mila_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MILA_CDNA4_H */
