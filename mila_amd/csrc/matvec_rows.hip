// Decode Linear for 2 .. 4 rows: Y[b] = W X[b] for up to four independent sequences from ONE pass over the weights -- the matvec kernel (matvec.hip) with NB x-images
// in LDS and NB accumulators per weight row.  A decode step is bound by the weight stream, so the rows beyond the first cost LDS reads and FMAs, not HBM bytes.
//
// Stands for CudaLinearOp at M = B (Linear/Kernels/MatVec/CudaMatVecBias.Bf16.cu, one launch per row there).
//
// BATCH INVARIANCE: row b of a launch has the bits the one-row entry (matvec_* / fused_norm_matvec) gives on that row alone, whatever the other rows hold.  Every row keeps
// the one-row arithmetic: the same chunk positions per lane (U comes from matvec_launch_shape, the rule the one-row kernels launch from, with its tuning variables), the
// order inside chunk_dot, per lane over (step, u), the fp4 fmaf(scale, chunk_dot(.., 0), acc), wave_sum, the fp8 scale and the bias after the reduction, the canonical
// rstd_of order of the prologues and round_bf16 before GeGLU.  Output columns per wave step (always 1 here) and the grid do not enter a column's arithmetic.
//
// As in matvec.hip every load is unconditional with a clamped address, x and the prologue operands of all rows are requested ahead of two pipeline steps of weights, and
// the streaming loop is the same two-buffer pipeline with its last <= 3 steps peeled.
#include <cstdio>

#include "common.h"
#include "internal.h"
#include "rms_common.h"
#include "matvec_body.h"

namespace mila {

constexpr int kMaxMatvecRows = 4;
constexpr size_t kMatvecRowsLdsLimit = 160 * 1024;   // gfx950: 160 KiB of LDS per workgroup

// by-value tail of the kernel arguments (the leading plain ones are preloaded into SGPRs, matvec.hip)
struct MatvecRowsTail
{
    void* y;
    const float* scales;
    const uint16_t* bias;
    const uint16_t* post_w;
    uint16_t* res_out;
    float post_scale, eps;
    int group;
    long long x_stride, y_stride, res_stride, res_out_stride;   // elements between consecutive rows
    float* amax_v;             // row b's partials: amax_v + b * amax_stride floats (values [kArgmaxPartials], then indices [kArgmaxPartials])
    long long amax_stride;
};

// PRO / GEGLU / F32OUT / U / XC: see matvec_body.h.  NB = rows.  One output column (GEGLU: its gate and up rows) per wave step.
template <int FMT, int U, int PRO, bool GEGLU, bool F32OUT, int XC, int NB>
__global__ __launch_bounds__(1024) void matvec_rows_kernel(const uint8_t* W, const uint16_t* x, const uint16_t* norm_w, const uint16_t* res, int K, int N, int nblocks,
                                                           const MatvecRowsTail t)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ float red[NB][2][16 * XC];
    u32x4* xs0 = reinterpret_cast<u32x4*>(smem_raw);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int block = (int)blockIdx.x;
    const int nx16 = K / 8;   // 16-byte units of one x row

    constexpr int EPC = Fmt<FMT>::kElemsPerChunk;
    constexpr int XPC = EPC / 8;
    constexpr int NR = GEGLU ? 2 : 1;                  // weight rows per wave step
    const int nchunks = K / EPC;
    const size_t row_bytes = (size_t)nchunks * 16;
    const int S = (nchunks + 64 * U - 1) / (64 * U);   // pipeline steps per output column
    const int nx16_pad = S * 64 * U * XPC;             // x units of one row's LDS image
    const int ngroups = (FMT == FMT_FP4) ? K / t.group : 0;
    const int cpg_shift = (FMT == FMT_FP4) ? (t.group == 128 ? 2 : 1) : 0;
    const int total_waves = nblocks * kMatvecWaves;
    const int wave_g = block * kMatvecWaves + wib;
    const int ncol_w = wave_g < N ? (N - 1 - wave_g) / total_waves + 1 : 0;
    const int T = ncol_w * S;                          // pipeline steps of this wave

    // ---- x / prologue operands of every row first ----
    u32x4 px[NB][XC], pnw[PRO != 0 ? XC : 1], ppw[PRO == 2 ? XC : 1], pres[PRO == 2 ? NB : 1][XC];
#pragma unroll
    for (int k = 0; k < XC; ++k)
    {
        const size_t e = (size_t)min(tid + 1024 * k, nx16 - 1) * 8;
#pragma unroll
        for (int b = 0; b < NB; ++b)
        {
            px[b][k] = ld16(x + (size_t)b * t.x_stride + e);
            if constexpr (PRO == 2) pres[b][k] = ld16(res + (size_t)b * t.res_stride + e);
        }
        if constexpr (PRO != 0) pnw[k] = ld16(norm_w + e);
        if constexpr (PRO == 2) ppw[k] = ld16(t.post_w + e);
    }

    auto issue = [&](WBuf<FMT, U, NR>& wb, int col_, int s) {
        const int c0 = s * (64 * U) + lane;
        const int col = min(col_, N - 1);
#pragma unroll
        for (int j = 0; j < NR; ++j)
        {
            const int row = j ? (N + col) : col;
            const uint8_t* wrow = W + (size_t)row * row_bytes;
#pragma unroll
            for (int u = 0; u < U; ++u)
            {
                const int c = min(c0 + 64 * u, nchunks - 1);
                wb.w[u][j] = ld16_nt(wrow + (size_t)c * 16);
                if constexpr (FMT == FMT_FP4) wb.sc[u][j] = t.scales[(size_t)row * ngroups + (c >> cpg_shift)];
            }
        }
    };
    // wave-uniform cursors over (column, step): `ci` issues, two steps ahead of `cc`, which computes
    int ci_col = wave_g, ci_s = 0, cc_col = wave_g, cc_s = 0;
    auto advance = [&](int& col_, int& s_) {
        const bool wrap = (s_ + 1 == S);
        s_ = wrap ? 0 : s_ + 1;
        col_ = wrap ? col_ + total_waves : col_;
    };
    WBuf<FMT, U, NR> ba, bb;
    issue(ba, ci_col, ci_s); advance(ci_col, ci_s);
    issue(bb, ci_col, ci_s); advance(ci_col, ci_s);

    // ---- stage every row's x into its LDS image (through the fused prologue), zero-pad the tails ----
#pragma unroll
    for (int b = 0; b < NB; ++b)
        for (int i = nx16 + tid; i < nx16_pad; i += 1024) xs0[(size_t)b * nx16_pad + i] = u32x4{0u, 0u, 0u, 0u};
    if constexpr (PRO == 0)
    {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int k = 0; k < XC; ++k)
                if (tid + 1024 * k < nx16) xs0[(size_t)b * nx16_pad + tid + 1024 * k] = px[b][k];
    }
    else
    {
        // the canonical order of rms_rstd_block (rms_common.h), as in matvec_body; every reduction has an LDS array of its own
        const int G = (nx16 + 63) / 64;
        auto rstd_of = [&](const u32x4* v, float* r) {
#pragma unroll
            for (int k = 0; k < XC; ++k)
            {
                float s = (tid + 1024 * k < nx16) ? sumsq8(v[k], 0.0f) : 0.0f;
                s = wave_sum(s);
                if (lane == 0) r[wib + kMatvecWaves * k] = s;
            }
            __syncthreads();
            float tt = 0.0f;
            for (int g = 0; g < G; ++g) tt += r[g];
            return rsqrtf(tt / (float)K + t.eps);
        };
#pragma unroll
        for (int b = 0; b < NB; ++b)
        {
            u32x4* xs = xs0 + (size_t)b * nx16_pad;
            if constexpr (PRO == 1)
            {
                const float rstd = rstd_of(px[b], red[b][0]);
#pragma unroll
                for (int k = 0; k < XC; ++k)
                    if (tid + 1024 * k < nx16) xs[tid + 1024 * k] = rms_apply8(px[b][k], pnw[k], rstd, 0.0f);
            }
            else
            {
                u32x4 rk[XC];
                const float rstd_a = rstd_of(px[b], red[b][0]);
#pragma unroll
                for (int k = 0; k < XC; ++k) rk[k] = sandwich_tail8(rms_apply8(px[b][k], ppw[k], rstd_a, 0.0f), pres[b][k], t.post_scale);
                if (block == 0 && t.res_out != nullptr)
                {
#pragma unroll
                    for (int k = 0; k < XC; ++k)
                        if (tid + 1024 * k < nx16) st16(t.res_out + (size_t)b * t.res_out_stride + (size_t)(tid + 1024 * k) * 8, rk[k]);
                }
                const float rstd_r = rstd_of(rk, red[b][1]);
#pragma unroll
                for (int k = 0; k < XC; ++k)
                    if (tid + 1024 * k < nx16) xs[tid + 1024 * k] = rms_apply8(rk[k], pnw[k], rstd_r, 0.0f);
            }
        }
    }
    __syncthreads();

    float acc[NB][NR];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[b][j] = 0.0f;

    auto compute = [&](const WBuf<FMT, U, NR>& wb, int s) {
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            const int c = s * (64 * U) + lane + 64 * u;    // < S * 64 * U: inside the zero-padded x
#pragma unroll
            for (int j = 0; j < NR; ++j)
#pragma unroll
                for (int b = 0; b < NB; ++b)
                {
                    const u32x4* xs = xs0 + (size_t)b * nx16_pad;
                    if constexpr (FMT == FMT_FP4)
                        acc[b][j] = fmaf(wb.sc[u][j], chunk_dot<FMT>(wb.w[u][j], xs, c, 0.0f), acc[b][j]);
                    else
                        acc[b][j] = chunk_dot<FMT>(wb.w[u][j], xs, c, acc[b][j]);
                }
        }
    };

    float amax_bv[NB];      // lane 0 of each wave: the best (value, column) of row b among the columns this wave has stored
    int amax_bi[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { amax_bv[b] = -3.402823466e+38f; amax_bi[b] = 0x7fffffff; }

    auto finish = [&](int col) {       // col < N: a wave only walks its own columns
        float scale[NR], bias[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j)
        {
            const int row = j ? (N + col) : col;
            scale[j] = 1.0f;
            bias[j] = 0.0f;
            if constexpr (FMT == FMT_FP8) scale[j] = __builtin_bit_cast(float, sload32(t.scales + row));
            if (t.bias)
            {
                const uint32_t pair = sload32(reinterpret_cast<const uint32_t*>(t.bias) + (row >> 1));
                bias[j] = bf16_bits_to_f32((uint16_t)((row & 1) ? (pair >> 16) : (pair & 0xffffu)));
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
        {
#pragma unroll
            for (int j = 0; j < NR; ++j)
            {
                float v = wave_sum(acc[b][j]);
                if constexpr (FMT == FMT_FP8) v = scale[j] * v;
                if (t.bias) v += bias[j];
                acc[b][j] = v;
            }
            if (lane == 0)
            {
                float v = acc[b][0];
                if constexpr (GEGLU)
                {
                    const float g = round_bf16(acc[b][0]), up = round_bf16(acc[b][1]);
                    v = gelu_tanh(g) * up;
                }
                if constexpr (F32OUT)
                {
                    reinterpret_cast<float*>(t.y)[(size_t)b * t.y_stride + col] = v;
                    if (t.amax_v) argmax_better(amax_bv[b], amax_bi[b], v, col);
                }
                else reinterpret_cast<uint16_t*>(t.y)[(size_t)b * t.y_stride + col] = f32_to_bf16_bits(v);
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) acc[b][j] = 0.0f;
        }
    };

    auto consume = [&](const WBuf<FMT, U, NR>& wb) {
        compute(wb, cc_s);
        const int col_prev = cc_col;
        advance(cc_col, cc_s);
        if (cc_col != col_prev) finish(col_prev);
    };

    int ts = 0;
    for (; ts + 4 <= T; ts += 2)      // steps ts + 2 and ts + 3 exist: refill unconditionally
    {
        consume(ba);
        issue(ba, ci_col, ci_s); advance(ci_col, ci_s);
        consume(bb);
        issue(bb, ci_col, ci_s); advance(ci_col, ci_s);
    }
    const int rem = T - ts;           // 0 (idle wave), 1, 2 or 3
    if (rem >= 1)
    {
        consume(ba);
        if (rem == 3) issue(ba, ci_col, ci_s);
    }
    if (rem >= 2) consume(bb);
    if (rem == 3) consume(ba);

    if constexpr (F32OUT)
    {
        // the sampler's first stage, per row: the workgroup's 16 per-wave candidates through LDS (free since the prologue), one partial per workgroup and row
        if (t.amax_v)
        {
            __syncthreads();
            if (lane == 0)
            {
#pragma unroll
                for (int b = 0; b < NB; ++b) { red[b][0][wib] = amax_bv[b]; red[b][1][wib] = __int_as_float(amax_bi[b]); }
            }
            __syncthreads();
            if (tid < NB)
            {
                float bv = red[tid][0][0];
                int bi = __float_as_int(red[tid][1][0]);
                for (int w = 1; w < kMatvecWaves; ++w) argmax_better(bv, bi, red[tid][0][w], __float_as_int(red[tid][1][w]));
                float* pv = t.amax_v + (size_t)tid * t.amax_stride;
                pv[block] = bv;
                reinterpret_cast<int*>(pv + kArgmaxPartials)[block] = bi;
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------
struct MatvecRowsArgs
{
    const uint8_t* W;
    const uint16_t* x;
    const uint16_t* norm_w;
    const uint16_t* res;
    int K, N;
    MatvecRowsTail t;
};

// what a launch is made of: the one-row rule's U (and, for rows == 1, its R), x chunks per thread, dynamic LDS bytes and workgroups
struct MatvecRowsPlan { int R, U, xc; size_t lds, lds_static; int blocks; };      // lds: the dynamic x images; lds_static: what the kernel declares itself

static bool plan_rows(int fmt, int K, int N, bool geglu, bool argmax, int rows, MatvecRowsPlan& pl)
{
    if (fmt < 0 || fmt > 2 || K <= 0 || N <= 0 || K > 16384 || rows < 1 || rows > kMaxMatvecRows) return false;
    const int epc = fmt == FMT_BF16 ? 8 : (fmt == FMT_FP8 ? 16 : 32);
    if (K % epc != 0) return false;
    const MatvecShape shape = matvec_launch_shape(fmt, geglu, N, argmax);
    pl.R = rows == 1 ? shape.R : 1;
    pl.U = shape.U;
    pl.xc = K <= 8192 ? 1 : 2;
    const int nchunks = K / epc;
    const int S = (nchunks + 64 * pl.U - 1) / (64 * pl.U);
    pl.lds = (size_t)rows * S * 64 * pl.U * epc * 2;
    pl.lds_static = rows > 1 ? (size_t)rows * 2 * 16 * pl.xc * sizeof(float) : (size_t)2 * 16 * pl.xc * sizeof(float);      // the kernels' reduction arrays (red / red_a, red_b)
    const int n_rg = (N + pl.R - 1) / pl.R;
    int blocks = (n_rg + kMatvecWaves - 1) / kMatvecWaves;
    if (blocks > shape.max_blocks) blocks = shape.max_blocks;
    pl.blocks = blocks < 1 ? 1 : blocks;
    return true;
}

template <int FMT, int U, int PRO, bool GEGLU, bool F32OUT, int XC, int NB>
static int launch_rows_t(const MatvecRowsArgs& a, const MatvecRowsPlan& pl, hipStream_t s)
{
    auto kernel = matvec_rows_kernel<FMT, U, PRO, GEGLU, F32OUT, XC, NB>;
    // more than the 64 KiB a kernel gets by default (as attention_prefill.hip does for its LDS-DMA forms): once per instantiation and device.  The 160 KiB hold the
    // kernel's own reduction arrays as well (every form but the plain bf16 one keeps them): asking for all of it as dynamic LDS is refused with an invalid-value error
    static thread_local int raised_for = -1;
    int dev = 0;
    if (pl.lds > 65536)
    {
        int rc = check_hip(hipGetDevice(&dev), "matvec_rows");
        if (rc) return rc;
        if (raised_for != dev)
        {
            rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMatvecRowsLdsLimit - pl.lds_static)),
                           "matvec_rows");
            if (rc) return rc;
            raised_for = dev;
        }
    }
    note_form("matvec_rows");
    hipLaunchKernelGGL(kernel, dim3(pl.blocks), dim3(64 * kMatvecWaves), pl.lds, s, a.W, a.x, a.norm_w, a.res, a.K, a.N, pl.blocks, a.t);
    MILA_LAUNCH_CHECK("matvec_rows");
}

template <int FMT, int U, int PRO, bool GEGLU, bool F32OUT, int XC>
static int launch_rows_nb(const MatvecRowsArgs& a, const MatvecRowsPlan& pl, int rows, hipStream_t s)
{
    if (rows == 2) return launch_rows_t<FMT, U, PRO, GEGLU, F32OUT, XC, 2>(a, pl, s);
    if (rows == 3) return launch_rows_t<FMT, U, PRO, GEGLU, F32OUT, XC, 3>(a, pl, s);
    return launch_rows_t<FMT, U, PRO, GEGLU, F32OUT, XC, 4>(a, pl, s);
}

template <int FMT, int PRO, bool GEGLU, bool F32OUT>
static int launch_rows_u(const MatvecRowsArgs& a, const MatvecRowsPlan& pl, int rows, hipStream_t s)
{
    if (pl.xc == 1)
    {
        if (pl.U == 1) return launch_rows_nb<FMT, 1, PRO, GEGLU, F32OUT, 1>(a, pl, rows, s);
        if (pl.U == 2) return launch_rows_nb<FMT, 2, PRO, GEGLU, F32OUT, 1>(a, pl, rows, s);
        return launch_rows_nb<FMT, 4, PRO, GEGLU, F32OUT, 1>(a, pl, rows, s);
    }
    if (pl.U == 1) return launch_rows_nb<FMT, 1, PRO, GEGLU, F32OUT, 2>(a, pl, rows, s);
    if (pl.U == 2) return launch_rows_nb<FMT, 2, PRO, GEGLU, F32OUT, 2>(a, pl, rows, s);
    return launch_rows_nb<FMT, 4, PRO, GEGLU, F32OUT, 2>(a, pl, rows, s);
}

template <int PRO, bool GEGLU, bool F32OUT>
static int launch_rows_fmt(int fmt, const MatvecRowsArgs& a, const MatvecRowsPlan& pl, int rows, hipStream_t s)
{
    switch (fmt)
    {
        case FMT_BF16: return launch_rows_u<FMT_BF16, PRO, GEGLU, F32OUT>(a, pl, rows, s);
        case FMT_FP8: return launch_rows_u<FMT_FP8, PRO, GEGLU, F32OUT>(a, pl, rows, s);
        default: return launch_rows_u<FMT_FP4, PRO, GEGLU, F32OUT>(a, pl, rows, s);
    }
}

}  // namespace mila

using namespace mila;

extern "C" {

size_t mila_cdna4_matvec_rows_plan_describe(int fmt, int K, int N, int geglu, int f32_out, int rows, char* buf, size_t cap)
{
    if (buf && cap) buf[0] = 0;
    MatvecRowsPlan pl;
    // the lm_head launch (fp32 out) of the decode step carries the sampler's first stage: its grid is capped at the sampler's partials
    if ((geglu && f32_out) || !plan_rows(fmt, K, N, geglu != 0, f32_out != 0, rows, pl) || pl.lds + pl.lds_static > kMatvecRowsLdsLimit) return 0;
    return 1 + snprintf(buf, buf ? cap : 0, "%d:%d:%d:%zu:%d", pl.R, pl.U, pl.xc, pl.lds, pl.blocks);
}

int mila_cdna4_matvec_rows(const mila_matvec_rows_args* r, mila_stream_t stream)
{
    MILA_REQUIRE(r != nullptr, "matvec_rows: null args");
    const mila_fused_matvec_args* a = &r->a;
    MILA_REQUIRE(a->y && a->x && a->W, "matvec_rows: null pointer (y=%p x=%p W=%p)", (const void*)a->y, (const void*)a->x, a->W);
    MILA_REQUIRE(a->K > 0 && a->N > 0, "matvec_rows: K and N must be positive (K=%d N=%d)", a->K, a->N);
    MILA_REQUIRE(a->fmt >= 0 && a->fmt <= 2, "matvec_rows: unknown weight format %d", a->fmt);
    MILA_REQUIRE(a->K <= 16384, "matvec_rows: K=%d exceeds the register-staged x limit (16384)", a->K);
    if (a->fmt == FMT_BF16) MILA_REQUIRE(a->K % 8 == 0, "matvec_rows: K=%d must be a multiple of 8 for bf16 weights", a->K);
    if (a->fmt == FMT_FP8)
    {
        MILA_REQUIRE(a->K % 16 == 0, "matvec_rows: K=%d must be a multiple of 16 for fp8 weights", a->K);
        MILA_REQUIRE(a->scales != nullptr, "matvec_rows: fp8 weights need per-channel scales");
    }
    if (a->fmt == FMT_FP4)
    {
        MILA_REQUIRE(a->group == 64 || a->group == 128, "matvec_rows: fp4 group size must be 64 or 128 (got %d)", a->group);
        MILA_REQUIRE(a->K % 32 == 0 && a->K % a->group == 0, "matvec_rows: K=%d must be a multiple of 32 and of the group size %d", a->K, a->group);
        MILA_REQUIRE(a->scales != nullptr, "matvec_rows: fp4 weights need per-group scales");
    }
    if (r->rows < 2 || r->rows > kMaxMatvecRows)
        return set_error(MILA_E_UNSUPPORTED, "matvec_rows: rows=%d is outside 2 .. %d (one row: the matvec_* / fused_norm_matvec entries)", r->rows, kMaxMatvecRows);
    const int rows = r->rows;
    const bool geglu = a->geglu != 0, f32 = a->f32_out != 0;
    MILA_REQUIRE(!(geglu && f32), "matvec_rows: geglu and f32_out are exclusive");
    MILA_REQUIRE(a->norm_w != nullptr || (!a->res && !a->post_w && !geglu), "matvec_rows: res / post_w / geglu need norm_w (the fused forms)");
    MILA_REQUIRE(a->norm_w == nullptr || r->bias == nullptr, "matvec_rows: bias goes with the plain form (norm_w == NULL) only");
    MILA_REQUIRE(!(f32 && r->bias), "matvec_rows: bias goes with bf16 output only (matvec_f32out takes none: no one-row entry defines those bits)");
    MILA_REQUIRE((a->res == nullptr) == (a->post_w == nullptr), "matvec_rows: res and post_w go together");
    // rows must not overlap: a stride below the row's width would make one row's store another row's output
    const long long out_w = a->N;
    MILA_REQUIRE(r->x_stride >= a->K && r->y_stride >= out_w, "matvec_rows: x_stride %lld / y_stride %lld below the row widths %d / %lld", (long long)r->x_stride,
                 (long long)r->y_stride, a->K, out_w);
    if (a->res)
    {
        MILA_REQUIRE(a->res_out != nullptr, "matvec_rows: res_out is required with res");
        MILA_REQUIRE(a->res_out != a->res && a->res_out != a->x, "matvec_rows: res_out must not alias res or x");
        MILA_REQUIRE(r->res_stride >= a->K && r->res_out_stride >= a->K, "matvec_rows: res_stride %lld / res_out_stride %lld below the row width %d", (long long)r->res_stride,
                     (long long)r->res_out_stride, a->K);
    }
    MILA_REQUIRE(r->x_stride % 8 == 0 && (!a->res || (r->res_stride % 8 == 0 && r->res_out_stride % 8 == 0)), "matvec_rows: x / res / res_out row strides must be multiples of 8 elements (16-byte accesses)");

    MatvecRowsPlan pl;
    if (!plan_rows(a->fmt, a->K, a->N, geglu, a->argmax_scratch != nullptr, rows, pl)) return set_error(MILA_E_INVALID_ARGUMENT, "matvec_rows: no plan for fmt=%d K=%d N=%d", a->fmt, a->K, a->N);
    if (pl.lds + pl.lds_static > kMatvecRowsLdsLimit)
        return set_error(MILA_E_UNSUPPORTED, "matvec_rows: K=%d at %d rows needs %zu bytes of LDS for x (limit %zu)", a->K, rows, pl.lds, kMatvecRowsLdsLimit);

    MatvecRowsArgs k{reinterpret_cast<const uint8_t*>(a->W), a->x, a->norm_w, a->res, a->K, a->N,
                     MatvecRowsTail{a->y, a->scales, r->bias, a->post_w, a->res_out, a->norm_w ? a->post_scale : 1.0f, a->eps, a->group, r->x_stride, r->y_stride,
                                    r->res_stride, r->res_out_stride, nullptr, 0}};
    if (a->argmax_scratch)
    {
        // row b's partials at argmax_scratch + b * sample_scratch_bytes(), each laid out as sample_argmax_fp32 lays its own; sample_argmax_rows_final_advance reduces them
        MILA_REQUIRE(f32, "matvec_rows: argmax_scratch needs f32_out (the logits)");
        MILA_REQUIRE(a->argmax_blocks != nullptr, "matvec_rows: argmax_blocks is required with argmax_scratch");
        const size_t per_row = mila_cdna4_sample_scratch_bytes();
        if (a->argmax_scratch_bytes < per_row * rows)
            return set_error(MILA_E_SCRATCH_TOO_SMALL, "matvec_rows: argmax scratch %zu bytes < required %zu (%d rows)", a->argmax_scratch_bytes, per_row * rows, rows);
        if (pl.blocks > kArgmaxPartials) return set_error(MILA_E_RUNTIME, "matvec_rows: %d workgroups exceed the %d sampler partials", pl.blocks, kArgmaxPartials);
        k.t.amax_v = reinterpret_cast<float*>(a->argmax_scratch);
        k.t.amax_stride = (long long)(per_row / sizeof(float));
    }
    hipStream_t s = as_stream(stream);
    int rc;
    if (!a->norm_w) rc = f32 ? launch_rows_fmt<0, false, true>(a->fmt, k, pl, rows, s) : launch_rows_fmt<0, false, false>(a->fmt, k, pl, rows, s);
    else if (f32) rc = a->res ? launch_rows_fmt<2, false, true>(a->fmt, k, pl, rows, s) : launch_rows_fmt<1, false, true>(a->fmt, k, pl, rows, s);
    else if (a->res) rc = geglu ? launch_rows_fmt<2, true, false>(a->fmt, k, pl, rows, s) : launch_rows_fmt<2, false, false>(a->fmt, k, pl, rows, s);
    else rc = geglu ? launch_rows_fmt<1, true, false>(a->fmt, k, pl, rows, s) : launch_rows_fmt<1, false, false>(a->fmt, k, pl, rows, s);
    if (rc == MILA_OK && a->argmax_scratch) *a->argmax_blocks = pl.blocks;
    return rc;
}

}  // extern "C"
