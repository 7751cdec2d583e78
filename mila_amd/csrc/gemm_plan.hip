// Prefill (M > 1) Linear dispatch, host code only: shape -> GemmPlan (gemm_plan.h), the queries that read a plan, the two executors that launch one.  Every tunable that
// steers WHICH form is chosen lives here, next to its rule and its measurement; what steers how a chosen form is launched stays with its kernel (gemm.schedule -- which also
// gates rules here --, gemm.persistent, gemm.walk_min_tiles, gemm.rowwise_epilogue, gemm_fp8.skinny_whole_x; the tail kernels' tile width, the skinny kernels' row groups).
#include "gemm_plan.h"
#include "internal.h"
#include <algorithm>
#include <cstdio>

namespace mila {

static const char* gemm_form_name(GemmForm form)
{
    static const char* const names[] = {"gemm128", "gemm256", "gemm256x128", "gemm256x128_splitk", "fewrow_bf16", "skinny_bf16", "skinny_bf16_geglu", "gemm256_geglu",
                                        "fp8_gemm256", "fp8_gemm256x128", "fp8_gemm256x128_splitk", "fp8_gemm256_geglu", "fp8_gemm256x128_geglu",
                                        "fp8_skinny", "fp8_skinny_geglu", "fp8_tail", "fp8_tail_geglu"};
    return names[form];
}

static void add_step(GemmPlan& pl, GemmForm form, int row0, int rows, int col0, int cols, int S = 0)
{
    if (pl.n < kMaxGemmSteps) pl.step[pl.n] = GemmStep{form, row0, rows, col0, cols, S};
    ++pl.n;
    if (S) pl.ws_bytes = std::max(pl.ws_bytes, (size_t)S * rows * cols * sizeof(float));
}

// ================================================ the rules every plan shares, each written once ================================================
// the LDS-DMA kernels address their operands through 32-bit buffer offsets (bytes, signed int arithmetic): both tensors must stay below 2 GiB
static bool lds_dma_addressable(int M, int K, int w_rows) { return (int64_t)M * K * 2 < 0x7fffffffll && (int64_t)w_rows * K * 2 < 0x7fffffffll; }

static int rounds_of(int tiles) { return (tiles + kNumCU - 1) / kNumCU; }
// the fill rule: the tile list fills at least `percent` of its rounds of CUs (one workgroup per CU and round)
static bool fills_rounds(int tiles, int percent) { return (int64_t)tiles * 100 >= (int64_t)percent * rounds_of(tiles) * kNumCU; }
// the new-round test: one more tile-row of `per_row` tiles after `tile_rows` of them opens another round of the grid
static bool opens_new_round(int tile_rows, int per_row) { return rounds_of(tile_rows * per_row) < rounds_of((tile_rows + 1) * per_row); }

constexpr int kSkinnyTailRows = 64;      // a remainder (or a whole prompt) of up to this many rows is a weight stream: the skinny kernels (bf16 and fp8)
// the skinny-remainder split: the rows the tile kernels keep when a prompt of at least min_rows rows ends in a <= 64-row remainder past its last whole tile-row
// (M itself: no such remainder)
static int rows_ahead_of_skinny_tail(int M, int min_rows)
{
    const int tail = M % 256;
    return (M >= min_rows && tail > 0 && tail <= kSkinnyTailRows) ? M - tail : M;
}

// ---- split-K (round 3): short prompts and the remainders of long ones.  A 300-row prompt gives fc_down (N = 3840, K = 15360) 60 tiles of 240 K-tiles each: 60 CUs
// busy for a full-length K loop, 196 idle.  The split form starts S copies of the tile list, copy ks taking 1 / S of K, and a second kernel sums the S fp32 partials in
// a fixed order and applies the epilogue (bias, GELU, bf16) -- same bits whatever the timing.  The partials live in caller workspace (S M N floats, <= 32 MiB since
// tiles x S <= 256 CUs): the entry that takes one is mila_cdna4_gemm_bf16_ws, the counterpart of the cuBLASLt workspace CudaLinearOp hands its plans
// (CudaLinearOp.ixx:637-638, CudaExecutionContext.ixx:337).
static int g_gemm_splitk = 1;            // tuning "gemm.splitk": the split-K forms of gemm_bf16_ws / gemm_fp8_scaled_ws
MILA_TUNE("gemm.splitk", g_gemm_splitk);
static int g_gemm_fp8_tail_form = 0;     // tuning "gemm_fp8.tail_form": 0 = LDS-DMA kernels on the leading rows, the tail kernels by row count on the rest; 1 = EVERY row on the masked 128-row
                                         // LDS tiles (bit-identical to the LDS-DMA kernels: the test of that statement); 2 = every row as skinny pieces
MILA_TUNE("gemm_fp8.tail_form", g_gemm_fp8_tail_form);
// the split count of the 256 x 128 ring, S (>= 2), or 0: no split-K form for this shape.  bk: the ring's K-tile width (64 bf16, 128 e4m3)
static int splitk_count(int M, int K, int N, int bk)
{
    if (!g_gemm_splitk || g_gemm_pingpong != 5 || (bk == 128 && g_gemm_fp8_tail_form != 0)) return 0;
    if (M <= 0 || N % 128 != 0 || K % bk != 0 || !lds_dma_addressable(M, K, N)) return 0;
    const int tiles = ((M + 255) / 256) * (N / 128), nk = K / bk;
    if (tiles > kNumCU / 2) return 0;
    const int S = std::min(std::min(kNumCU / tiles, nk / 8), 16);      // at least 8 K-tiles per copy: the ring's fill and drain are 3
    return S >= 2 ? S : 0;
}

// one 512-thread workgroup per CU: worth it only when the tile count fills whole rounds of 256 CUs
static int g_gemm256_min_fill = 80;      // tuning "gemm.tile256_min_fill": the 256 x 256 grid applies when its tiles fill at least this many percent of their rounds of CUs
MILA_TUNE("gemm.tile256_min_fill", g_gemm256_min_fill);

// ---- column split (round 4): an output whose 256 x 256 tile list ends in a nearly empty round -- Gemma's global qkv_proj, N = 8704 at T = 2048: 272 tiles on 256 CUs (the
// 256 x 128 ring ran it as 544 tiles in three rounds for 2.1 rounds of work, 165 us = 0.83 PFLOP/s) -- is cut at the last whole round: columns [0, n_main) as whole rounds
// of 256 x 256 tiles, the few remaining column tiles through the split-K form of the ring (their S copies cover the idle CUs), both writing their column range of Y with
// the pitch of the whole row.  Needs the caller's workspace (S M (N - n_main) floats).
static int g_gemm_colsplit = 1;
MILA_TUNE("gemm.colsplit", g_gemm_colsplit);
// the geometry: the columns the whole rounds of 256 x 256 tiles take and the split count of the rest; 0 = no column split for this shape
static int colsplit_columns(int M, int K, int N, int bk, int* S_rest)
{
    *S_rest = 0;
    if (!g_gemm_colsplit || g_gemm_pingpong != 5 || N % 256 != 0 || K % bk != 0 || !lds_dma_addressable(M, K, N)) return 0;
    const int tm = (M + 255) / 256, tn = N / 256, tiles = tm * tn;
    if (tiles <= kNumCU || fills_rounds(tiles, g_gemm256_min_fill)) return 0;      // the whole list fills its rounds well enough (gemm256_applicable's rule)
    const int tn_main = ((tiles / kNumCU) * kNumCU) / tm;                          // column tiles of the whole rounds
    if (tn_main <= 0 || tn_main >= tn) return 0;
    const int n_main = tn_main * 256;
    *S_rest = splitk_count(M, K, N - n_main, bk);
    return *S_rest >= 2 ? n_main : 0;
}

// ================================================ bf16 operands ================================================
static int g_gemm_force128 = 0;      // tuning "gemm.force128": 1 = always the 128 x 128 register-staged GEMM (A/B against the LDS-DMA kernels)
MILA_TUNE("gemm.force128", g_gemm_force128);
static int g_bf16_skinny = 1;      // tuning "gemm.bf16_skinny": the bf16 skinny kernel for <= 64-row prompts and remainders
MILA_TUNE("gemm.bf16_skinny", g_bf16_skinny);
// Few rows (tools/experiments/few_row_rules.sh, profiles/r03_splitk.txt): bf16-policy prefill of 2 / 4 / 8 / 16 tokens with the skinny kernels ahead of the tile grids up
// to 16 rows 7.46 / 7.39 / 7.75 / 7.94 ms, never ahead 7.41 / 7.05 / 7.13 / 7.28 -- a one-round tile grid and the split-K form stream the weights at 3-4 TB/s from two
// rows on, the skinny kernel's 16-row groups at that rate only for one group.  The skinny kernels keep what has no such grid: a 1-row remainder, narrow outputs, calls
// without a workspace on the N = 3840 shapes.
static int g_skinny_ahead_rows = 1;         // tuning "gemm.skinny_ahead_rows": up to this many rows the skinny kernels go ahead of an applicable tile grid (plain and GeGLU)
MILA_TUNE("gemm.skinny_ahead_rows", g_skinny_ahead_rows);
static int g_fewrow = 1;                    // tuning "gemm.fewrow": the few-row weight-streaming form for <= 32 rows with a workspace
MILA_TUNE("gemm.fewrow", g_fewrow);
static int g_splitk_min_rows = 2;           // tuning "gemm.splitk_min_rows": row counts below this stay off the split-K form even with a workspace
MILA_TUNE("gemm.splitk_min_rows", g_splitk_min_rows);

static int g_ldsdma_loose_tiles = 30;     // the 256 x 128 ring applies from this many tiles on whatever the fill of its last round (tuning "gemm.ldsdma_loose_tiles"; 0 = the fill rule only).
MILA_TUNE("gemm.ldsdma_loose_tiles", g_ldsdma_loose_tiles);
                                   // Measured with tools/experiments/bf16_ragged_rules.py (profiles/r03_bf16_ragged.txt): even a 30-tile ring beats the register-staged 128-tile kernel --
                                   // bf16-policy prefill of 100 / 300 / 511 / 1000 tokens 23.6 / 25.1 / 26.4 / 31.6 -> 16.3 / 17.9 / 21.4 / 26.7 ms
// taken when the 256 x 256 grid does not apply and the 256 x 128 grid fills most of one round of CUs (or several)
static bool gemm256x128_applicable(int M, int K, int N)
{
    if (M <= 0 || N % 128 != 0 || K % 64 != 0 || !lds_dma_addressable(M, K, N)) return false;
    const int tiles = ((M + 255) / 256) * (N / 128);      // a ragged last tile-row counts (and costs) whole: rows past M re-read row M - 1, their stores are masked
    if (g_ldsdma_loose_tiles > 0 && tiles >= g_ldsdma_loose_tiles) return true;      // experiment / ragged-M rule: see g_ldsdma_loose_tiles
    return tiles >= 160 && fills_rounds(tiles, 70);      // (192 tiles -- GPT-2's 768-wide projections at B T = 8192 -- beat the 128-tile kernel's 384: 18 / 51 vs 29 / 74 us)
}
static bool gemm256_applicable(int M, int K, int N)
{
    if (M <= 0 || N % 256 != 0 || K % 64 != 0 || !lds_dma_addressable(M, K, N)) return false;
    const int tiles = ((M + 255) / 256) * (N / 256);
    return tiles >= 200 && fills_rounds(tiles, g_gemm256_min_fill);      // (80 %: nine tile-rows of fc_gate_up -- 1080 tiles, 4.2 rounds walked as 5 -- stay on the fused kernel)
}
// bf16 only: N of any size (ragged last column tile of width tile_n, any row pitch) when the grid is many rounds deep -- GPT-2's lm_head (N = 50257, K = 768, at M = 8192:
// 12 576 tiles of the ring, 6 304 of the 256 x 256 kernel on its PERSISTENT schedule; k_mult: 64 and 128).  A 256 x 256 tile there is 12 K-tiles, as long as what a one-tile
// workgroup pays around them (launch, first-load latency, the store drain): the persistent walk overlaps all three with the next tile's K loop
static bool ragged_n_applicable(int M, int K, int N, int tile_n, int k_mult)
{
    if (M <= 0 || K % k_mult != 0 || N % tile_n == 0 || !lds_dma_addressable(M, K, N)) return false;
    return (int64_t)((M + 255) / 256) * ((N + tile_n - 1) / tile_n) >= 4 * kNumCU;
}
// Y[M, F] = GeGLU(X W^T), W = [gate rows 0 .. F-1 | up rows F .. 2F-1]  (its own rule with its own measurement: the literal 80, not gemm.tile256_min_fill)
static bool gemm256_geglu_applicable(int M, int K, int F)
{
    if (M <= 0 || F % 128 != 0 || K % 64 != 0 || !lds_dma_addressable(M, K, 2 * F)) return false;
    const int tiles = ((M + 255) / 256) * (F / 128);
    return tiles >= 200 && fills_rounds(tiles, 80);
}

// which direct-to-LDS kernel serves a bf16-weight GEMM of this shape: GF_GEMM256, GF_GEMM256X128, or GF_GEMM128 = none (128 x 128 register-staged)
static GemmForm glds_kernel_for(int M, int K, int N)
{
    if (g_gemm_force128) return GF_GEMM128;
    if (g_gemm_pingpong == 2 && gemm256x128_applicable(M, K, N)) return GF_GEMM256X128;      // tuning: the 256 x 128 ring wherever it applies
    if (gemm256_applicable(M, K, N)) return GF_GEMM256;
    if (gemm256x128_applicable(M, K, N)) return GF_GEMM256X128;
    if (g_gemm_pingpong >= 3 && ragged_n_applicable(M, K, N, 256, 128)) return GF_GEMM256;
    if (ragged_n_applicable(M, K, N, 128, 64)) return GF_GEMM256X128;
    return GF_GEMM128;
}

// bf16-weight GEMM over rows [row0, row0 + M) without a workspace: LDS-DMA kernel on the leading multiple of 256 rows when one applies, 128-tile kernel on the rest
static void plan_bf16_rows(GemmPlan& pl, int row0, int M, int K, int N)
{
    if (!g_gemm_force128 && g_bf16_skinny)
    {
        // few rows: a weight stream (the 128-tile kernel pushed the bf16 model's weights past a 16-row prompt at 1 TB/s)
        // (past g_skinny_ahead_rows, and above all past one 16-row group -- the stream then re-reads X per 16 W rows and runs at 1.2-2 TB/s -- a tile grid that covers half
        // the chip or more is the faster form --
        // fc_gate_up at 64 rows 196 us against ~55 as 240 tiles of 256 x 128; on the N = 3840 shapes' 30 tiles the stream still wins)
        if (M <= kSkinnyTailRows && (M <= g_skinny_ahead_rows || (int64_t)((N + 127) / 128) < kNumCU / 2 || glds_kernel_for(M, K, N) == GF_GEMM128))
            return add_step(pl, GF_SKINNY_BF16, row0, M, 0, N);
        // a long prompt's <= 64-row remainder: the LDS-DMA kernels on the leading tile-rows, the skinny kernel on the rest (a ragged tile-row of the N = 3840 shapes
        // would open a second round of full-length tiles; the 128-tile kernel cost a 1-row remainder +18 ms per prefill)
        const int lead = rows_ahead_of_skinny_tail(M, 512);
        if (lead < M && glds_kernel_for(lead, K, N) != GF_GEMM128)
        {
            add_step(pl, glds_kernel_for(lead, K, N), row0, lead, 0, N);
            return add_step(pl, GF_SKINNY_BF16, row0 + lead, M - lead, 0, N);
        }
        // (a longer remainder, 65 .. 255 rows, rides in a ragged tile-row.  Where that row opens a new round of the grid -- the N = 3840 shapes: 240 tiles fill the chip, 270
        // need a second round of full-length tiles -- 64-row skinny passes were tried instead and are slower: the staged 64-row form streams at 1.2 TB/s, fc_down 4 x 90 us
        // against 180 for the extra round; profiles/r03_bf16_ragged.txt.  What that case wants is a split-K tail: plan_bf16 with a workspace.)
    }
    // Ragged prompt lengths (round 3): the LDS-DMA kernels take ANY M -- a ragged last tile-row stages row M - 1 for the rows past M and masks its stores (the fp8 forms'
    // mechanism) -- so a 2049- or 2000-token prompt stays on them (bf16 policy: 60.6 / 62.5 ms -> one tile-row more / the 2048 time; the register-staged 128-tile
    // kernel streamed a 1-row remainder's weights at 1 TB/s).  Where the whole M does not make an LDS-DMA grid, the leading multiple of 256 rows may still, and the
    // rest goes to the 128-tile kernel (rows are independent; no padding, nothing read past the tensors).
    GemmForm form = glds_kernel_for(M, K, N);
    int lead = form != GF_GEMM128 ? M : 0;
    if (!lead && M - M % 256 >= 512 && (form = glds_kernel_for(M - M % 256, K, N)) != GF_GEMM128) lead = M - M % 256;
    if (lead) add_step(pl, form, row0, lead, 0, N);
    if (lead < M) add_step(pl, GF_GEMM128, row0 + lead, M - lead, 0, N);
}

// the split-K step for `rows` rows after `lead` rows of other forms: up to 32 rows the few-row weight stream (gemm_fewrow_bf16.hip), else the 256 x 128 ring over S
// copies of the tile list; false: neither splits this shape
static bool add_bf16_splitk(GemmPlan& pl, int lead, int rows, int K, int N)
{
    // (a remainder takes the few-row form only where the ring form could split too -- at most half a round of tiles: a wide output's remainder stays with the call's
    // other forms, so that a long prompt's fc_gate_up keeps its fused GeGLU kernel)
    if (g_fewrow && rows <= 32 && (lead == 0 || (N + 127) / 128 <= kNumCU / 2))
    {
        const int Sf = gemm_fewrow_splits(rows, K, N);
        if (Sf) { add_step(pl, GF_FEWROW_BF16, lead, rows, 0, N, Sf); return true; }
    }
    const int S = splitk_count(rows, K, N, 64);
    if (S) add_step(pl, GF_GEMM256X128_SPLITK, lead, rows, 0, N, S);
    return S != 0;
}

GemmPlan plan_bf16(int M, int K, int N, bool have_ws)
{
    GemmPlan pl;
    if (have_ws && !g_gemm_force128 && M >= g_splitk_min_rows)      // what a caller workspace (mila_cdna4_gemm_bf16_ws) changes: the split-K forms
    {
        // a short prompt: the whole tile list covers at most half the CUs (or the few-row form serves it)
        if (add_bf16_splitk(pl, 0, M, K, N)) return pl;
        // a tile list that ends in a nearly empty round (N = 8704 at T = 2048): whole rounds of 256 x 256 tiles + the remaining columns split-K
        // (a long prompt's <= 64-row remainder stays with the skinny kernel -- the dispatch ladder showed T = 2049 turning its ONE extra row into a ninth tile-row of the split)
        const int rows = g_bf16_skinny ? rows_ahead_of_skinny_tail(M, 512) : M;
        int S_rest = 0;
        const int n_main = rows >= 256 ? colsplit_columns(rows, K, N, 64, &S_rest) : 0;
        if (n_main > 0 && gemm256_applicable(rows, K, n_main))
        {
            pl.colsplit = true;
            add_step(pl, GF_GEMM256, 0, rows, 0, n_main);
            add_step(pl, GF_GEMM256X128_SPLITK, 0, rows, n_main, N - n_main, S_rest);
            if (rows < M) plan_bf16_rows(pl, rows, M - rows, K, N);
            return pl;
        }
        // a long prompt's remainder whose ragged tile-row would open another round of the grid (T = 2303 on the N = 3840 shapes: 240 tiles fill the chip, 270 run two
        // rounds of full-length tiles -- fc_down 200 -> 400 us): the whole tile-rows as before, the remainder split-K
        const int tail = M % 256, lead = M - tail;
        const GemmForm form = (M >= 512 && tail >= g_splitk_min_rows) ? glds_kernel_for(lead, K, N) : GF_GEMM128;
        if (form != GF_GEMM128 && opens_new_round(lead / 256, form == GF_GEMM256 ? (N + 255) / 256 : (N + 127) / 128))
        {
            plan_bf16_rows(pl, 0, lead, K, N);
            if (add_bf16_splitk(pl, lead, tail, K, N)) return pl;
            pl.n = 0;
        }
    }
    plan_bf16_rows(pl, 0, M, K, N);
    return pl;
}

// Linear + GeGLU over any row count the fused forms serve: the LDS-DMA GeGLU kernel on whole / ragged tile-rows, the skinny GeGLU kernel on <= 64 rows (a short prompt,
// or the remainder of a long one).  No step: the fused kernels do not serve the shape.
GemmPlan plan_bf16_geglu(int M, int K, int F)
{
    GemmPlan pl;
    const bool whole = gemm256_geglu_applicable(M, K, F);
    const int lead = g_bf16_skinny ? rows_ahead_of_skinny_tail(M, 512) : M;
    if (g_bf16_skinny && M <= kSkinnyTailRows && (M <= g_skinny_ahead_rows || !whole)) add_step(pl, GF_SKINNY_BF16_GEGLU, 0, M, 0, F);
    else if (lead < M && (M - lead <= g_skinny_ahead_rows || !whole) && gemm256_geglu_applicable(lead, K, F))
    {
        add_step(pl, GF_GEMM256_GEGLU, 0, lead, 0, F);
        add_step(pl, GF_SKINNY_BF16_GEGLU, lead, M - lead, 0, F);
    }
    else if (whole) add_step(pl, GF_GEMM256_GEGLU, 0, M, 0, F);
    return pl;
}
// ... and where they are also the faster choice for a caller that holds the gemm_bf16_ws workspace (RocmLinearOp / GemmaBlock): not where the plain GEMM over the
// [2F, K] weight would split K (that Linear + GeGLU pair is faster, and fused and unfused prefill keep identical bits: the fused kernels sum K in one order only), and,
// past g_skinny_ahead_rows, not where the plain Linear has an LDS-DMA grid (fc_gate_up at 64 rows: 196 us skinny, ~55 as a one-round tile grid + the elementwise pass)
static bool plan_bf16_geglu_preferred(int M, int K, int F)
{
    const GemmPlan pl = plan_bf16_geglu(M, K, F);
    if (!pl.n || plan_bf16(M, K, 2 * F, true).ws_bytes) return false;
    if (pl.step[0].form == GF_SKINNY_BF16_GEGLU && M > g_skinny_ahead_rows) return glds_kernel_for(M, K, 2 * F) == GF_GEMM128;
    return true;
}

int run_gemm_bf16(const GemmPlan& pl, uint16_t* Y, const uint16_t* X, const uint16_t* W, const uint16_t* bias, int K, int N, int act, void* ws, hipStream_t s)
{
    MILA_REQUIRE(pl.n > 0 && pl.n <= kMaxGemmSteps, "bf16 GEMM: no runnable plan for this shape (%d steps)", pl.n);
    if (pl.colsplit) note_form("gemm256_colsplit");
    float* partials = static_cast<float*>(ws);
    for (int i = 0; i < pl.n; ++i)
    {
        const GemmStep& st = pl.step[i];
        uint16_t* y = Y + (size_t)st.row0 * N + st.col0;
        const uint16_t* x = X + (size_t)st.row0 * K;
        const uint16_t* w = W + (size_t)st.col0 * K;
        const uint16_t* b = bias ? bias + st.col0 : nullptr;
        const int ldy = st.cols == N ? 0 : N;      // a column range of Y keeps the pitch of the whole row
        note_form(gemm_form_name(st.form));
        int rc;
        switch (st.form)
        {
        case GF_GEMM128: rc = launch_gemm128(y, x, w, b, st.rows, K, st.cols, act, s); break;
        case GF_GEMM256: rc = launch_gemm256(y, x, w, b, st.rows, K, st.cols, s, act, ldy); break;
        case GF_GEMM256X128: rc = launch_gemm256x128(y, x, w, b, st.rows, K, st.cols, s, act); break;
        case GF_GEMM256X128_SPLITK: rc = launch_gemm256x128_splitk(y, x, w, b, st.rows, K, st.cols, s, act, partials, st.S, ldy); break;
        case GF_FEWROW_BF16:
            rc = launch_gemm_bf16_fewrow(partials, x, w, st.rows, K, st.cols, st.S, s);
            if (!rc) rc = launch_splitk_reduce(y, partials, b, st.rows, st.cols, st.S, act, s);
            break;
        case GF_SKINNY_BF16: rc = launch_gemm_bf16_skinny(y, x, w, b, st.rows, K, st.cols, act, s); break;
        case GF_SKINNY_BF16_GEGLU: rc = launch_gemm_bf16_skinny_geglu(y, x, w, st.rows, K, st.cols, s); break;
        case GF_GEMM256_GEGLU: rc = launch_gemm256_geglu(y, x, w, st.rows, K, st.cols, s); break;
        default: rc = set_error(MILA_E_RUNTIME, "bf16 GEMM: form %s in a bf16 plan", gemm_form_name(st.form));
        }
        if (rc) return rc;
    }
    return MILA_OK;
}

// ================================================ e4m3 operands (W4A8 / W8A8) ================================================
// Row counts of any kind (the fp4 policy's prefill is W4A8 for EVERY M > 1, CudaLinearOp.ixx:646-715):
//   (short prompts, measured with tools/experiments/short_prompt_rules.py, profiles/r03_short_prompts.txt: below 512 rows the LDS-DMA kernels still win wherever their grid
//    has >= 120 tiles -- qkv, fc_gate_up -- and lose on the N = 3840 shapes, whose 30-60 tiles leave the chip empty; fp4-policy prefill of 300 / 400 / 511 tokens
//    14.8 / 17.4 / 18.3 -> 11.8 / 13.0 / 13.6 ms, monotonic in T again)
//   M >= 512 and N % 128 == 0, K % 128 == 0: the LDS-DMA kernels over ceil(M / 256) tile-rows -- a ragged last tile-row stages row M - 1 for the rows past M
//     and masks its stores (a 208-row tail costs one tile-row, 1/8 of a T = 2048 chunk; on the masked 128-row tiles it cost 40 % of the chunk) -- except that a
//     tail of <= 64 rows goes to the skinny weight-streaming kernel instead (a 1-row tail: +11 % of the chunk instead of +12.5 %, and no MFMA work on padding);
//   everything else: the tail kernels of gemm_fp8_tail.hip alone.
// Rows are independent and the LDS-DMA kernels and the masked tiles run the same instruction chain per output element.
// Few rows (tools/experiments/few_row_rules_fp4.sh, profiles/r03_splitk.txt): one 16-row group stays with the skinny kernel -- a weight stream of one byte per weight
// (fp4-policy prefill of 8 / 16 tokens 4.83 / 4.92 ms, against 4.95 / 5.02 on the tile forms); from 17 rows on the tile grids (>= 120 tiles) and the split-K form are faster
// (17 / 24 / 32 tokens 5.39 / 5.50 / 5.69 ms skinny, 5.09 / 5.10 / 5.17 here; 64 tokens 7.15 -> 5.66).  A W4A8 form of the few-row kernel (gemm_fewrow_bf16.hip with
// e4m3 operands; parity-green) was slower than both on every length -- the skinny kernel's fused GeGLU saves fc_gate_up a reduce and an elementwise pass -- and is not kept.
static int g_fp8_splitk_min_rows = 17;      // tuning "gemm_fp8.splitk_min_rows": fewer rows stay with the skinny kernel
MILA_TUNE("gemm_fp8.splitk_min_rows", g_fp8_splitk_min_rows);
static int g_fp8_big_rule = 3;      // tuning "gemm_fp8.big_rule": 0 = LDS-DMA kernels from 512 rows on (round 3's first rule), 1 = from 128 rows on,
                                    // 2 = from 512 rows on or wherever ceil(M / 256) x (W rows / 128) >= 120 tiles, 3 (default) = 2 without the skinny split of a short prompt's remainder
MILA_TUNE("gemm_fp8.big_rule", g_fp8_big_rule);
static int fp8_big_rows(int M, int K, int N_mult, int w_rows)      // rows the LDS-DMA kernels take (0 = none); N_mult: the column granularity the form needs (128, or 64 for 256 x 128 GeGLU)
{
    if (!lds_dma_addressable(M, K, w_rows)) return 0;
    if (g_gemm_fp8_tail_form != 0 || K % 128 != 0 || N_mult == 0) return 0;
    // below two full tile-rows the LDS-DMA kernels pay only where their grid still covers the chip (tuning variable gemm_fp8.big_rule)
    const int tiles = ((M + 255) / 256) * (w_rows / 128);
    const bool big = g_fp8_big_rule == 1 ? M >= 128 : (g_fp8_big_rule >= 2 ? (M >= 512 || (M >= g_fp8_splitk_min_rows && tiles >= 120)) : M >= 512);
    if (!big) return 0;
    // (rule 3: a short prompt's <= 64-row remainder stays in the ragged tile-row: a skinny pass re-streams every weight, which only a long main part amortises)
    return rows_ahead_of_skinny_tail(M, g_fp8_big_rule == 3 ? 512 : 0);
}
// which LDS-DMA kernel: 256 x 256 (enough tiles for the chip, N % 256 == 0), else 256 x 128
static GemmForm fp8_pick(int rows, int N) { return (N % 256 == 0 && ((rows + 255) / 256) * (N / 256) >= 200) ? GF_FP8_GEMM256 : GF_FP8_GEMM256X128; }

// rows the LDS-DMA kernels do not take: tails up to 64 rows run as ONE skinny launch; longer ones on the 128-row LDS tiles (measured: four skinny pieces of a 208-row
// tail cost more than two LDS tile rows); gemm_fp8.tail_form = 2: 64-row skinny pieces, one step each
static void plan_fp8_tail(GemmPlan& pl, int row0, int M, int N, bool geglu)
{
    if (g_gemm_fp8_tail_form == 2 || (g_gemm_fp8_tail_form == 0 && M <= kSkinnyTailRows))
        for (int r0 = 0; r0 < M; r0 += kFp8SkinnyRows) add_step(pl, geglu ? GF_FP8_SKINNY_GEGLU : GF_FP8_SKINNY, row0 + r0, std::min(kFp8SkinnyRows, M - r0), 0, N);
    else add_step(pl, geglu ? GF_FP8_TAIL_GEGLU : GF_FP8_TAIL, row0, M, 0, N);
}
static void plan_fp8_rows(GemmPlan& pl, int M, int K, int N)
{
    const int rows = fp8_big_rows(M, K, N % 128 == 0 ? 128 : 0, N);
    if (rows) add_step(pl, fp8_pick(rows, N), 0, rows, 0, N);
    if (rows < M) plan_fp8_tail(pl, rows, M - rows, N, false);
}

// with a caller workspace (mila_cdna4_gemm_fp8_scaled_ws), as plan_bf16: a short prompt whose tile list covers at most half the CUs splits K whole; a long prompt's
// remainder whose ragged tile-row would open another round of the grid (T = 2303 on the N = 3840 shapes) splits K alone
GemmPlan plan_fp8(int M, int K, int N, bool have_ws)
{
    GemmPlan pl;
    if (have_ws && M >= g_fp8_splitk_min_rows)
    {
        int S = splitk_count(M, K, N, 128);
        if (S) { add_step(pl, GF_FP8_GEMM256X128_SPLITK, 0, M, 0, N, S); return pl; }
        // the 256 x 256 fp8 tile list of N = 8704 at T = 2048 is 272 tiles: one round and sixteen stragglers, walked as two (fp8_pick).  Whole rounds + a split-K rest instead.
        const int n_main = (g_gemm_fp8_tail_form == 0 && M >= 512) ? colsplit_columns(M, K, N, 128, &S) : 0;
        if (n_main > 0 && fp8_big_rows(M, K, 128, n_main) == M && fp8_pick(M, n_main) == GF_FP8_GEMM256)
        {
            pl.colsplit = true;
            add_step(pl, GF_FP8_GEMM256, 0, M, 0, n_main);
            add_step(pl, GF_FP8_GEMM256X128_SPLITK, 0, M, n_main, N - n_main, S);
            return pl;
        }
        const int tail = M % 256, lead = M - tail;
        if (M >= 512 && tail >= g_fp8_splitk_min_rows && fp8_big_rows(lead, K, N % 128 == 0 ? 128 : 0, N) == lead &&
            opens_new_round(lead / 256, fp8_pick(lead, N) == GF_FP8_GEMM256 ? N / 256 : N / 128) && (S = splitk_count(tail, K, N, 128)) != 0)
        {
            plan_fp8_rows(pl, lead, K, N);
            add_step(pl, GF_FP8_GEMM256X128_SPLITK, lead, tail, 0, N, S);
            return pl;
        }
    }
    plan_fp8_rows(pl, M, K, N);
    return pl;
}

// Y[M, F] = GeGLU of the W4A8 / W8A8 Linear over W8 = [gate rows | up rows] (2F x K e4m3)
GemmPlan plan_fp8_geglu(int M, int K, int F)
{
    GemmPlan pl;
    const bool form256 = F % 128 == 0 && ((M + 255) / 256) * (F / 128) >= 200;
    const int rows = fp8_big_rows(M, K, form256 ? 128 : (F % 64 == 0 ? 64 : 0), 2 * F);
    if (rows) add_step(pl, form256 ? GF_FP8_GEMM256_GEGLU : GF_FP8_GEMM256X128_GEGLU, 0, rows, 0, F);
    if (rows < M) plan_fp8_tail(pl, rows, M - rows, F, true);
    return pl;
}

int run_gemm_fp8(const GemmPlan& pl, uint16_t* Y, const uint8_t* X8, const uint8_t* W8, const float* x_scales, Fp8WScale w_scale, const uint16_t* bias, int K, int N, void* ws,
                 hipStream_t s)
{
    MILA_REQUIRE(pl.n > 0 && pl.n <= kMaxGemmSteps, "fp8 GEMM: no runnable plan for this shape (%d steps)", pl.n);
    if (pl.colsplit) note_form("fp8_gemm256_colsplit");
    float* partials = static_cast<float*>(ws);
    for (int i = 0; i < pl.n; ++i)
    {
        const GemmStep& st = pl.step[i];
        uint16_t* y = Y + (size_t)st.row0 * N + st.col0;
        const uint8_t* x = X8 + (size_t)st.row0 * K;
        const uint8_t* w = W8 + (size_t)st.col0 * K;
        const float* xs = x_scales + st.row0;
        const Fp8WScale wsc{w_scale.per_channel ? w_scale.p + st.col0 : w_scale.p, w_scale.per_channel};
        const uint16_t* b = bias ? bias + st.col0 : nullptr;
        const int ldy = st.cols == N ? 0 : N;      // a column range of Y keeps the pitch of the whole row
        note_form(gemm_form_name(st.form));
        int rc;
        switch (st.form)
        {
        case GF_FP8_GEMM256: case GF_FP8_GEMM256X128: case GF_FP8_GEMM256_GEGLU: case GF_FP8_GEMM256X128_GEGLU:
            rc = launch_gemm_fp8_ldsdma(st.form, y, x, w, xs, wsc, b, st.rows, K, st.cols, s, ldy); break;
        case GF_FP8_GEMM256X128_SPLITK: rc = launch_gemm256x128_fp8_splitk(y, x, w, xs, wsc, b, st.rows, K, st.cols, s, partials, st.S, ldy); break;
        case GF_FP8_SKINNY: case GF_FP8_TAIL: rc = launch_gemm_fp8_tail(y, x, w, xs, wsc, b, st.rows, K, st.cols, st.form == GF_FP8_SKINNY, false, s); break;
        case GF_FP8_SKINNY_GEGLU: case GF_FP8_TAIL_GEGLU: rc = launch_gemm_fp8_tail(y, x, w, xs, wsc, b, st.rows, K, st.cols, st.form == GF_FP8_SKINNY_GEGLU, true, s); break;
        default: rc = set_error(MILA_E_RUNTIME, "fp8 GEMM: form %s in an fp8 plan", gemm_form_name(st.form));
        }
        if (rc) return rc;
    }
    return MILA_OK;
}

}  // namespace mila

using namespace mila;

extern "C" {

// ---- the size / applicability queries of the ABI: readings of the plan ----
size_t mila_cdna4_gemm_workspace_bytes(int M, int K, int N) { return (M > 0 && K > 0 && N > 0 && K % 8 == 0) ? plan_bf16(M, K, N, true).ws_bytes : 0; }
size_t mila_cdna4_gemm_fp8_workspace_bytes(int M, int K, int N) { return (M > 0 && K > 0 && N > 0 && K % 16 == 0) ? plan_fp8(M, K, N, true).ws_bytes : 0; }

// the staged forms' scratch: the dequantized [N, K] bf16 weights, then (16-byte aligned: K % 8 == 0) the split-K workspace of the bf16 GEMM over them -- the staged call
// and gemm_bf16_ws on weights dequantized ahead of time (the host's resident prefill weights) then run the same kernels and give the same bits
size_t mila_cdna4_gemm_staging_bytes(int M, int K, int N)
{
    if (M <= 0 || K <= 0 || N <= 0 || K % 8 != 0) return 0;
    const GemmPlan pl = plan_bf16(M, K, N, true);
    // staged wherever a step streams bf16 weights: any form but the 128-tile kernel, which has in-register-dequantizing forms of its own (few rows: the staged forms
    // dequantize once and stream the bf16 weights through the skinny kernel -- the dequantizing 128-tile kernel pushed the fp8 policy's weights past a 16-row prompt at 1 TB/s)
    bool staged = false;
    for (int i = 0; i < pl.n && i < kMaxGemmSteps; ++i) staged |= pl.step[i].form != GF_GEMM128;
    // (one row is the decode matvecs' in the hosts; the staged call keeps the dequantizing kernel for it unless a tile grid would apply)
    if (M == 1 && !pl.ws_bytes) staged = glds_kernel_for(M, K, N) != GF_GEMM128;
    return staged ? (size_t)N * K * 2 + pl.ws_bytes : 0;
}

/* Linear + GeGLU in one kernel (prefill fc_gate_up): where the fused bf16 forms serve the shape ... */
int mila_cdna4_gemm_geglu_applicable(int M, int K, int F) { return (M > 0 && K > 0 && F > 0 && K % 8 == 0 && !g_gemm_force128 && plan_bf16_geglu(M, K, F).n > 0) ? 1 : 0; }
// ... and, for a caller that HOLDS the gemm_bf16_ws workspace, where they are also the faster choice: where the plain GEMM over the [2F, K] weight would split K (few-row
// prompts, short tile lists), its Linear (gemm_bf16_ws) + GeGLU pair is the faster one and the fused form steps aside -- a host decision (it used to hide inside
// gemm_geglu_applicable, so a caller WITHOUT a workspace lost the fused kernels on those shapes for nothing)
int mila_cdna4_gemm_geglu_preferred(int M, int K, int F) { return (mila_cdna4_gemm_geglu_applicable(M, K, F) && plan_bf16_geglu_preferred(M, K, F)) ? 1 : 0; }
// (0 also where the plain W4A8 GEMM over [2F, K] would split K given a workspace: Linear + GeGLU as two calls is the faster pair there and keeps the bits of the unfused path)
int mila_cdna4_gemm_geglu_w4a8_applicable(int M, int K, int F) { return (M > 0 && K > 0 && F > 0 && K % 16 == 0 && !plan_fp8(M, K, 2 * F, true).ws_bytes) ? 1 : 0; }

// test hook (internal.h): the plan of an entry point as text, "form:row0:rows:col0:cols:S" items joined by '+', the column-split marker (all zeros) first.  Runs no device code.
size_t mila_cdna4_gemm_plan_describe(int entry, int M, int K, int N, char* buf, size_t cap)
{
    if (buf && cap) buf[0] = 0;
    if (entry < 0 || entry > 5 || M <= 0 || K <= 0 || N <= 0) return 0;
    const GemmPlan pl = entry == 0 ? plan_bf16(M, K, N, false) : entry == 1 ? plan_bf16(M, K, N, true) : entry == 2 ? plan_bf16_geglu(M, K, N)
                      : entry == 3 ? plan_fp8(M, K, N, false) : entry == 4 ? plan_fp8(M, K, N, true) : plan_fp8_geglu(M, K, N);
    size_t len = 0;
    auto item = [&](const char* form, const GemmStep& st) {      // (an item that does not fit is left out; the return value says what the whole text needs)
        const bool fits = buf && len + 96 < cap;
        len += snprintf(fits ? buf + len : nullptr, fits ? cap - len : 0, "%s%s:%d:%d:%d:%d:%d", len ? "+" : "", form, st.row0, st.rows, st.col0, st.cols, st.S);
    };
    if (pl.colsplit) item(entry < 3 ? "gemm256_colsplit" : "fp8_gemm256_colsplit", GemmStep{GF_GEMM128, 0, 0, 0, 0, 0});
    for (int i = 0; i < pl.n && i < kMaxGemmSteps; ++i) item(gemm_form_name(pl.step[i].form), pl.step[i]);
    return len + 1;
}

}  // extern "C"
