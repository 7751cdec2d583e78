// Prompt log-probabilities: the lm_head GEMM over many rows whose epilogue keeps the softmax statistics and never stores a logit.
//   y_i = sum_k x[r,k] * W[i,k]      fp32 on the matrix cores; an e4m3 table enters as its exact bf16 values and the per-row scale multiplies ONCE after the reduction
//                                    (matvec_f32out's arithmetic -- what the decode head computes -- not gemm.hip's bf16(decode * scale))
//   z_i = softcap > 0 ? softcap * tanhf(y_i / softcap) : y_i                                            (soft_cap of common.h)
//   m = max z,  S = sum expf(z_i - m),  logprob_t = (z_t - m) - logf(S);  argmax = the largest z, the LOWEST index among equals (the greedy sampler's tie rule)
// Two launches:
//   partials: one workgroup owns a block of 128 rows and a SLAB of the vocabulary and walks the slab 128 columns at a time through the K loop of gemm.hip's gemm_kernel
//             (128 x 128 x 64 tile, 2 x 2 waves of v_mfma_f32_32x32x16_bf16, register-staged double buffer, quantized tiles converted on their way to LDS, the product
//             transposed so that a lane holds columns of ONE row, the XCD-aware order).  Each lane keeps, for each of its two rows, running (max, sum exp rescaled to that
//             max, best z, best index, z of the target if it passed by); at the end of the slab the four lanes that share a row merge in a fixed order and leave ONE record
//             of 8 words per (row, slab) in scratch.
//   final:    one wave per row merges the slabs' records -- lane l takes slabs 4l .. 4l+3 in ascending order, rescaled to the global max, then the butterfly of
//             logprobs.hip -- and writes the outputs.
// No floating-point atomics; every sum has a fixed order: the same bits run to run.  THE SLAB RULE looks at `vocab` alone (ls_tiles_per_slab below), the tile shape at
// nothing, and padded rows are zero-filled: a row's outputs are, bit for bit, those of a rows = 1 call on that row alone.
#include <cfloat>
#include <cmath>

#include "common.h"

namespace mila {

constexpr int kLsTile = 128;                // rows and vocabulary columns of one tile
constexpr int kLsBK = 64;
constexpr int kLsTileBytes = kLsTile * kLsBK * 2;
constexpr int kLsMaxSlabs = 256;            // one slab per CU at the workload's vocabulary: a call of <= 128 rows still fills the chip
constexpr int kLsRecWords = 8;              // max, sum, best z, best index, target z, 3 x pad
constexpr int kLsNone = 0x7fffffff;

// THE SLAB RULE: a slab is the least whole number of 128-column tiles that covers the vocabulary with at most 256 slabs.  262144 -> 8 tiles = 1024 columns, 256 slabs.
static int ls_tiles(int vocab) { return (int)(((int64_t)vocab + kLsTile - 1) / kLsTile); }
static int ls_tiles_per_slab(int vocab) { return (ls_tiles(vocab) + kLsMaxSlabs - 1) / kLsMaxSlabs; }
static int ls_slabs(int vocab) { return (ls_tiles(vocab) + ls_tiles_per_slab(vocab) - 1) / ls_tiles_per_slab(vocab); }

struct LsParams
{
    const uint16_t* X;
    size_t x_stride;
    const uint8_t* W;
    const float* scales;
    const int32_t* targets;
    float* scratch;                  // [rows][nslabs][kLsRecWords]
    int rows, K, vocab;
    int nrb, nslabs, tiles_per_slab, ntiles;
    float softcap;
    float* logprob_out;
    int32_t* argmax_out;
    float* argmax_logprob_out;
};

__device__ __forceinline__ int ls_swz(int row, int slot) { return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4); }
// a 16-byte load from an address that is only 2-byte aligned (x rows at any stride); st16_a2's counterpart
__device__ __forceinline__ u32x4 ls_ld16_a2(const void* p)
{
    const u32x4_a2 v = *reinterpret_cast<const u32x4_a2*>(p);
    return u32x4{v.x, v.y, v.z, v.w};
}

template <int FMT> struct LsRegs;
template <> struct LsRegs<0> { u32x4 x[4]; u32x4 w[4]; };
template <> struct LsRegs<1> { u32x4 x[4]; u32x4 w[2]; };

template <int FMT>
__device__ __forceinline__ void ls_stage_load(LsRegs<FMT>& r, const LsParams& p, int m0, int n0, int k0)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i)      // x tile: 128 rows x 8 slots of 16 bytes; rows beyond the call are ZERO
    {
        const int s = tid + 256 * i, row = s >> 3, slot = s & 7;
        const int m = m0 + row, k = k0 + slot * 8;
        r.x[i] = (m < p.rows && k < p.K) ? ls_ld16_a2(p.X + (size_t)m * p.x_stride + k) : u32x4{0u, 0u, 0u, 0u};
    }
    if constexpr (FMT == 0)
    {
        const uint16_t* W = reinterpret_cast<const uint16_t*>(p.W);
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const int s = tid + 256 * i, row = s >> 3, slot = s & 7;
            const int n = n0 + row, k = k0 + slot * 8;
            r.w[i] = (n < p.vocab && k < p.K) ? ld16(W + (size_t)n * p.K + k) : u32x4{0u, 0u, 0u, 0u};
        }
    }
    else
    {
#pragma unroll
        for (int i = 0; i < 2; ++i)  // 128 rows x 4 segments of 16 e4m3
        {
            const int s = tid + 256 * i, row = s >> 2, seg = s & 3;
            const int n = n0 + row, k = k0 + seg * 16;
            r.w[i] = (n < p.vocab && k < p.K) ? ld16(p.W + (size_t)n * p.K + k) : u32x4{0u, 0u, 0u, 0u};
        }
    }
}

template <int FMT>
__device__ __forceinline__ void ls_stage_store(const LsRegs<FMT>& r, unsigned char* ldsX, unsigned char* ldsW)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        const int s = tid + 256 * i, row = s >> 3, slot = s & 7;
        *reinterpret_cast<u32x4*>(ldsX + ls_swz(row, slot)) = r.x[i];
    }
    if constexpr (FMT == 0)
    {
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const int s = tid + 256 * i, row = s >> 3, slot = s & 7;
            *reinterpret_cast<u32x4*>(ldsW + ls_swz(row, slot)) = r.w[i];
        }
    }
    else
    {
#pragma unroll
        for (int i = 0; i < 2; ++i)  // every e4m3 value is a bf16 value: the convert is exact, the scale waits for the epilogue
        {
            const int s = tid + 256 * i, row = s >> 2, seg = s & 3;
            u32x4 lo, hi;
#pragma unroll
            for (int d = 0; d < 2; ++d)
            {
                lo[2 * d] = __builtin_bit_cast(uint32_t, fp8x2_to_bf16x2(r.w[i][d], false));
                lo[2 * d + 1] = __builtin_bit_cast(uint32_t, fp8x2_to_bf16x2(r.w[i][d], true));
                hi[2 * d] = __builtin_bit_cast(uint32_t, fp8x2_to_bf16x2(r.w[i][d + 2], false));
                hi[2 * d + 1] = __builtin_bit_cast(uint32_t, fp8x2_to_bf16x2(r.w[i][d + 2], true));
            }
            *reinterpret_cast<u32x4*>(ldsW + ls_swz(row, seg * 2)) = lo;
            *reinterpret_cast<u32x4*>(ldsW + ls_swz(row, seg * 2 + 1)) = hi;
        }
    }
}

// a lane's running values for one row
struct LsState { float m, s, bz; int bi; float tz; };

template <int FMT>
__global__ __launch_bounds__(256) void lm_head_score_partial_kernel(const LsParams p)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2 bufs][x tile | W tile]; at the end the lanes' states

    // XCD-aware order (gemm_kernel's): the workgroups of one XCD (id % 8) take consecutive items, the row blocks of ONE slab next to each other, so a slab of the
    // table is fetched into one L2
    const int nwg = gridDim.x, id = blockIdx.x;
    const int xcd = id & 7, q = nwg >> 3, rem = nwg & 7;
    const int item = ((xcd < rem) ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (id >> 3);
    const int slab = item / p.nrb, rb = item % p.nrb;
    const int m0 = rb * kLsTile;
    const int tile0 = slab * p.tiles_per_slab;
    const int ntiles = min(p.tiles_per_slab, p.ntiles - tile0);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wn = wave >> 1, wm = wave & 1;
    const int r32 = lane & 31, h = lane >> 5;

    int tgt[2];
    LsState st[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
    {
        const int m = m0 + wm * 64 + b * 32 + r32;
        tgt[b] = m < p.rows ? p.targets[m] : -1;
        st[b] = LsState{-FLT_MAX, 0.0f, -INFINITY, kLsNone, __builtin_nanf("")};
    }

    f32x16 acc[2][2];                               // [column (vocabulary) tile][row tile]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.0f;

    const int nk = (p.K + kLsBK - 1) / kLsBK;
    const int steps = ntiles * nk;
    LsRegs<FMT> regs;
    ls_stage_load<FMT>(regs, p, m0, tile0 * kLsTile, 0);
    ls_stage_store<FMT>(regs, smem, smem + kLsTileBytes);
    __syncthreads();

    int vt = 0, kt = 0;                             // the tile of the slab and the K-tile of this step
    for (int it = 0; it < steps; ++it)
    {
        unsigned char* cur = smem + (it & 1) * 2 * kLsTileBytes;
        unsigned char* nxt = smem + ((it + 1) & 1) * 2 * kLsTileBytes;
        const bool more = it + 1 < steps;
        const bool last_k = kt + 1 == nk;
        const int vt2 = last_k ? vt + 1 : vt, kt2 = last_k ? 0 : kt + 1;
        if (more) ls_stage_load<FMT>(regs, p, m0, (tile0 + vt2) * kLsTile, kt2 * kLsBK);

        const unsigned char* lx = cur;
        const unsigned char* lw = cur + kLsTileBytes;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
        {
            s16x8 fw[2], fx[2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
            {
                fw[a] = *reinterpret_cast<const s16x8*>(lw + ls_swz(wn * 64 + a * 32 + r32, ks * 2 + h));
                fx[a] = *reinterpret_cast<const s16x8*>(lx + ls_swz(wm * 64 + a * 32 + r32, ks * 2 + h));
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fw[a]), __builtin_bit_cast(bf16x8, fx[b]), acc[a][b], 0, 0, 0);
        }

        if (last_k)
        {
            // D[n][m]: lane -> row m = r32 of row tile b; registers -> columns n = (e & 3) + 8 * (e >> 2) + 4 * h of column tile a: ascending in (a, e)
            const int nb = (tile0 + vt) * kLsTile + wn * 64 + 4 * h;
#pragma unroll
            for (int b = 0; b < 2; ++b)
            {
                float z[2][16];
                float mt = -INFINITY;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                    {
                        const int n = nb + a * 32 + (e & 3) + 8 * (e >> 2);
                        const bool in = n < p.vocab;
                        float y = acc[a][b][e];
                        if constexpr (FMT == 1) y = (in ? p.scales[n] : 0.0f) * y;
                        const float v = in ? soft_cap(y, p.softcap) : -INFINITY;
                        z[a][e] = v;
                        mt = fmaxf(mt, v);
                        if (v > st[b].bz) { st[b].bz = v; st[b].bi = n; }          // ascending n: the first of equals stays
                        if (in && n == tgt[b]) st[b].tz = v;
                        acc[a][b][e] = 0.0f;
                    }
                const float m2 = fmaxf(st[b].m, mt);
                float sum = 0.0f;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int e = 0; e < 16; ++e) sum += expf(z[a][e] - m2);        // a column beyond the vocabulary is -inf: adds 0
                st[b].s = st[b].s * expf(st[b].m - m2) + sum;
                st[b].m = m2;
            }
        }

        if (more) ls_stage_store<FMT>(regs, nxt, nxt + kLsTileBytes);
        __syncthreads();
        vt = vt2;
        kt = kt2;
    }

    // the four lanes that share a row -- part = wn * 2 + h -- through LDS, merged by one thread in ascending part order
    float* parts = reinterpret_cast<float*>(smem);                                  // [128 rows][4 parts][5 words]
#pragma unroll
    for (int b = 0; b < 2; ++b)
    {
        float* d = parts + ((wm * 64 + b * 32 + r32) * 4 + wn * 2 + h) * 5;
        d[0] = st[b].m; d[1] = st[b].s; d[2] = st[b].bz; d[3] = __int_as_float(st[b].bi); d[4] = st[b].tz;
    }
    __syncthreads();
    const int row = threadIdx.x;
    if (row >= kLsTile || m0 + row >= p.rows) return;
    const float* s = parts + row * 20;
    float mx = s[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) mx = fmaxf(mx, s[5 * i]);
    float sum = 0.0f, bz = -INFINITY, tz = __builtin_nanf("");
    int bi = kLsNone;
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        sum += s[5 * i + 1] * expf(s[5 * i] - mx);
        const float v = s[5 * i + 2];
        const int vi = __float_as_int(s[5 * i + 3]);
        if (v > bz || (v == bz && vi < bi)) { bz = v; bi = vi; }
        const float t = s[5 * i + 4];
        if (t == t) tz = t;                                                         // at most one part saw the target
    }
    float* rec = p.scratch + ((size_t)(m0 + row) * p.nslabs + slab) * kLsRecWords;
    st16(rec, u32x4{__float_as_uint(mx), __float_as_uint(sum), __float_as_uint(bz), (uint32_t)bi});
    st16(rec + 4, u32x4{__float_as_uint(tz), 0u, 0u, 0u});
}

// one wave per row
__global__ __launch_bounds__(64) void lm_head_score_final_kernel(const LsParams p)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, row = blockIdx.x;
    const float* recs = p.scratch + (size_t)row * p.nslabs * kLsRecWords;
    float m4[4], s4[4];
    float mx = -FLT_MAX, bz = -INFINITY;
    int bi = kLsNone;
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        const int sl = 4 * lane + i;
        m4[i] = -FLT_MAX;
        s4[i] = 0.0f;
        if (sl < p.nslabs)
        {
            const u32x4 r = ld16(recs + (size_t)sl * kLsRecWords);
            m4[i] = __uint_as_float(r[0]);
            s4[i] = __uint_as_float(r[1]);
            const float v = __uint_as_float(r[2]);
            if (v > bz) { bz = v; bi = (int)r[3]; }                     // ascending slabs hold ascending indices
        }
        mx = fmaxf(mx, m4[i]);
    }
    mx = wave_max(mx);
    float f = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) f += s4[i] * expf(m4[i] - mx);
    f = wave_sum(f);
    const float lse = logf(f);
    const float best = wave_max(bz);
    bi = wave_min_i32(bz == best ? bi : kLsNone);
    if (lane != 0) return;
    const int t = p.targets[row];
    float lp = __builtin_nanf("");                                      // a target outside the vocabulary has no log-probability, and nothing is read for it
    if (t >= 0 && t < p.vocab) lp = (recs[(size_t)(t / (p.tiles_per_slab * kLsTile)) * kLsRecWords + 4] - mx) - lse;
    p.logprob_out[row] = lp;
    if (p.argmax_out != nullptr)
    {
        p.argmax_out[row] = bi;
        p.argmax_logprob_out[row] = (best - mx) - lse;
    }
}

static bool ls_shape_ok(int rows, int vocab) { return rows >= 1 && vocab >= 1; }
static size_t ls_scratch_bytes(int rows, int vocab) { return (size_t)rows * (size_t)ls_slabs(vocab) * kLsRecWords * 4; }

}  // namespace mila

using namespace mila;

extern "C" {

size_t mila_cdna4_lm_head_score_scratch_bytes(int rows, int vocab) { return ls_shape_ok(rows, vocab) ? ls_scratch_bytes(rows, vocab) : 0; }

int mila_cdna4_lm_head_score_bf16(const uint16_t* x, size_t x_stride, const void* W, const float* scales, int fmt, int K, int vocab, const int32_t* targets_dev, int rows,
                                  float softcap, float* logprob_out, int32_t* argmax_out, float* argmax_logprob_out, void* scratch, size_t scratch_bytes,
                                  mila_stream_t stream)
{
    const char* who = "lm_head_score_bf16";
    MILA_REQUIRE(x && W && targets_dev && logprob_out, "%s: null pointer", who);
    MILA_REQUIRE((argmax_out == nullptr) == (argmax_logprob_out == nullptr), "%s: argmax_out and argmax_logprob_out go together (both or neither)", who);
    MILA_REQUIRE(fmt == 0 || fmt == 1, "%s: fmt must be 0 (bf16) or 1 (e4m3 per channel), got %d", who, fmt);
    MILA_REQUIRE(fmt == 0 || scales != nullptr, "%s: per-channel scales are required with fmt 1", who);
    MILA_REQUIRE(rows >= 1, "%s: rows=%d must be positive", who, rows);
    MILA_REQUIRE(vocab >= 1, "%s: vocab=%d must be positive", who, vocab);
    MILA_REQUIRE(K > 0 && K % (fmt == 0 ? 8 : 16) == 0, "%s: K=%d must be a positive multiple of %d", who, K, fmt == 0 ? 8 : 16);
    MILA_REQUIRE(x_stride >= (size_t)K, "%s: x_stride %zu < K %d", who, x_stride, K);
    const size_t need = ls_scratch_bytes(rows, vocab);
    if (!scratch || scratch_bytes < need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, need);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15u) == 0, "%s: scratch must be 16-byte aligned", who);
    LsParams p{};
    p.X = x; p.x_stride = x_stride; p.W = static_cast<const uint8_t*>(W); p.scales = scales; p.targets = targets_dev;
    p.scratch = reinterpret_cast<float*>(scratch);
    p.rows = rows; p.K = K; p.vocab = vocab;
    p.nrb = (int)(((int64_t)rows + kLsTile - 1) / kLsTile);
    p.ntiles = ls_tiles(vocab); p.tiles_per_slab = ls_tiles_per_slab(vocab); p.nslabs = ls_slabs(vocab);
    p.softcap = softcap;
    p.logprob_out = logprob_out; p.argmax_out = argmax_out; p.argmax_logprob_out = argmax_logprob_out;
    MILA_REQUIRE((int64_t)p.nrb * p.nslabs <= 0x7fffffff, "%s: rows=%d is beyond one launch", who, rows);
    const dim3 grid((unsigned)(p.nrb * p.nslabs));
    if (fmt == 0) hipLaunchKernelGGL(lm_head_score_partial_kernel<0>, grid, dim3(256), 4 * kLsTileBytes, as_stream(stream), p);
    else hipLaunchKernelGGL(lm_head_score_partial_kernel<1>, grid, dim3(256), 4 * kLsTileBytes, as_stream(stream), p);
    int rc = check_hip(hipGetLastError(), who);
    if (rc) return rc;
    hipLaunchKernelGGL(lm_head_score_final_kernel, dim3(rows), dim3(64), 0, as_stream(stream), p);
    MILA_LAUNCH_CHECK(who);
}

}  // extern "C"
