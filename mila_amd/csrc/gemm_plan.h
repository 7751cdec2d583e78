// Prefill (M > 1) Linear dispatch: which kernel forms serve a shape is decided in ONE place (gemm_plan.hip) and is data -- a GemmPlan, a short list of
// rectangles of the output, one kernel form each -- that the size / applicability queries read and the two executors (bf16 operands, e4m3 operands) launch from.
// This header also declares every leaf launcher once; the kernels, their parameter structs and their launch-time tunables stay in their own files.
#pragma once
#include "common.h"

namespace mila {

// one value per string mila_cdna4_last_form reports for the plan-driven entry points
enum GemmForm
{
    GF_GEMM128, GF_GEMM256, GF_GEMM256X128, GF_GEMM256X128_SPLITK, GF_FEWROW_BF16, GF_SKINNY_BF16, GF_SKINNY_BF16_GEGLU, GF_GEMM256_GEGLU,
    GF_FP8_GEMM256, GF_FP8_GEMM256X128, GF_FP8_GEMM256X128_SPLITK, GF_FP8_GEMM256_GEGLU, GF_FP8_GEMM256X128_GEGLU,
    GF_FP8_SKINNY, GF_FP8_SKINNY_GEGLU, GF_FP8_TAIL, GF_FP8_TAIL_GEGLU
};

// one step = one kernel-form launch over rows [row0, row0 + rows) x output columns [col0, col0 + cols); S > 0: a split-K step (S fp32 partial copies in the
// workspace, the step includes its reduce launch), S = 0: not split
struct GemmStep { GemmForm form; int row0, rows, col0, cols, S; };
// (the bound: gemm_fp8.tail_form = 2 -- a test setting -- cuts EVERY row into 64-row skinny steps, 128 of them at 8192 rows; the default rules give at most 3)
constexpr int kMaxGemmSteps = 8192 / 64 + 8;
struct GemmPlan
{
    GemmStep step[kMaxGemmSteps];
    int n = 0;                  // steps the rules asked for; 0 = the fused (GeGLU) forms do not serve the shape; > kMaxGemmSteps = too long to run
    size_t ws_bytes = 0;        // the largest S * rows * cols * 4 over the split steps
    bool colsplit = false;      // the column split: noted as "[fp8_]gemm256_colsplit" ahead of the steps
};
// M rows of K, N output columns; have_ws: the caller holds a workspace (split-K forms allowed).  GeGLU: F output columns of a [2F, K] = [gate | up] weight.
GemmPlan plan_bf16(int M, int K, int N, bool have_ws);
GemmPlan plan_bf16_geglu(int M, int K, int F);
GemmPlan plan_fp8(int M, int K, int N, bool have_ws);
GemmPlan plan_fp8_geglu(int M, int K, int F);

// the executors: walk the steps, derive every pointer from (row0, col0), note the form, call the leaf launcher.  N: the output's row pitch (GeGLU: F)
int run_gemm_bf16(const GemmPlan& pl, uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int K, int N, int act, void* ws, hipStream_t s);
int run_gemm_fp8(const GemmPlan& pl, uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* x_scales, Fp8WScale w_scale, const uint16_t* bias, int K, int N, void* ws,
                 hipStream_t s);

extern int g_gemm_pingpong;      // gemm256.hip: "gemm.schedule", a tunable of the kernels' own that also gates plan rules

// ---- leaf launchers (none of them notes a form) ----
// gemm.hip: the 128 x 128 register-staged kernel, any shape
int launch_gemm128(uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int M, int K, int N, int act, hipStream_t s);
// gemm256.hip: the LDS-DMA kernels (ldy: row pitch of Y when the call writes a column range of it, 0 = N)
int launch_gemm256(uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int M, int K, int N, hipStream_t s, int act = 0, int ldy = 0);
int launch_gemm256x128(uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int M, int K, int N, hipStream_t s, int act = 0);
int launch_gemm256_geglu(uint16_t* Y, const uint16_t* X, const uint16_t* W, int M, int K, int F, hipStream_t s);
int launch_gemm256x128_splitk(uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int M, int K, int N, hipStream_t s, int act, float* partials, int S, int ldy = 0);
int launch_splitk_reduce(uint16_t* Y, const float* partials, const uint16_t* bias, int M, int N, int S, int act, hipStream_t s, int ldy = 0);
int launch_gemm_fp8_ldsdma(GemmForm form, uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* x_scales, Fp8WScale w_scale, const uint16_t* bias, int M, int K, int N,
                           hipStream_t s, int ldy = 0);      // form: one of the four GF_FP8_GEMM256* tile forms; GeGLU: N = F
int launch_gemm256x128_fp8_splitk(uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* x_scales, Fp8WScale w_scale, const uint16_t* bias, int M, int K, int N,
                                  hipStream_t s, float* partials, int S, int ldy = 0);
// gemm_skinny_bf16.hip: weight streaming for <= 64 rows per launch (any M as 64-row pieces)
int launch_gemm_bf16_skinny(uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int M, int K, int N, int act, hipStream_t s);
int launch_gemm_bf16_skinny_geglu(uint16_t* Y, const uint16_t* X, const uint16_t* W, int M, int K, int F, hipStream_t s);
// gemm_fewrow_bf16.hip: the few-row (<= 32 rows) weight stream into [S][M][N] partials; its split count (>= 1), or 0 where it does not serve the shape
int gemm_fewrow_splits(int M, int K, int N);
int launch_gemm_bf16_fewrow(float* partials, const uint16_t* X, const uint16_t* W, int M, int K, int N, int S, hipStream_t s);
// gemm_fp8_tail.hip: the same arithmetic as the fp8 LDS-DMA kernels for any row count -- skinny: ONE weight-streaming launch (<= kFp8SkinnyRows rows), else masked 128-row tiles
constexpr int kFp8SkinnyRows = 64;
int launch_gemm_fp8_tail(uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* x_scales, Fp8WScale w_scale, const uint16_t* bias, int M, int K, int N, bool skinny,
                         bool geglu, hipStream_t s);

}  // namespace mila
