// Attention over a (ring) KV cache: append and split-K flash-decode (+ combine).  The MFMA
// flash-prefill / MHA kernels live in attention_prefill.hip.
//
// Semantics restated from the reference:
//   * cache [B, NKV, capacity, HS] bf16, row = abs_pos % capacity   (Gqa.Cache.Bf16.cu:86-130)
//   * Q head h reads KV head h / (NH/NKV)                            (Gqa.Decode.Bf16.cu:93-98)
//   * a query at absolute position t sees keys max(0, t-window+1)..t when window > 0, else 0..t
//     (Gqa.Prefill.Bf16.cu:76-81; decode band Gqa.Decode.Bf16.cu:100-105 -- the same set)
//   * score = dot(q,k) * scale BEFORE max/exp                        (Gqa.Decode.Bf16.cu:212)
//   * fp32 scores / probabilities / accumulators, bf16 only at the final store.
//
// CDNA4 design of the decode (HBM/latency bound: 4-8 MB of K/V per layer): grid (splits, NKV * head groups, B), 512 threads = 8 waves.  A wave owns every 8th
// position of its split and one wave-instruction fetches one whole K (or V) row; online-softmax state (m, l, O) lives in registers per wave and is merged across the
// waves through LDS; split partials (m, l, O) go to caller-provided scratch and are merged by a second tiny kernel (a kernel boundary is cheaper than an in-kernel
// agent-scope acquire on this chip, MI355X_MICROARCH "boundary" vs "barrier-xcd").  From the scores on -- softmax step, both merges, finaliser, the two stores --
// the kernel is attention_decode_scalar.h, shared with the fp8 cache's kernel (attention_kvfp8.hip).
//
// What this file owns: the bf16 append; attn_decode_kernel = its own row loop (bf16 rows used as loaded) around those shared phases, plus the parts only this cache
// has (fused norm + RoPE + append prologue, warm blocks, one-pass ticket tail, XCD-local grid); the combine kernels; the matrix-core decode's bf16 kernel; plan_decode -- the one place that
// chooses form, heads per workgroup and split count for BOTH caches -- and the bf16 entry points that launch from it.
#include "common.h"
#include "rms_common.h"
#include "rope_common.h"
#include "internal.h"
#include "attention_generic.h"
#include "attention_tiles.h"
#include "attention_decode_mfma.h"
#include "attention_decode_plan.h"
#include "attention_decode_scalar.h"
#include "split_div.h"

namespace mila {

// ---- KV append ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_write_bf16_kernel(uint16_t* __restrict__ Kc, uint16_t* __restrict__ Vc,
                                                            const uint16_t* __restrict__ k,
                                                            const uint16_t* __restrict__ v, int64_t total_vec,
                                                            int chunk, int NKV, int HS, int start_pos, int capacity)
{
    const int hv = HS / 8;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_vec; i += stride)
    {
        // source order [b, t, nkv, hs]
        const int e = (int)(i % hv);
        int64_t r = i / hv;
        const int n = (int)(r % NKV);
        r /= NKV;
        const int t = (int)(r % chunk);
        const int b = (int)(r / chunk);
        const int row = (start_pos + t) % capacity;
        const size_t dst = ((((size_t)b * NKV + n) * capacity + row) * hv + e) * 8;
        st16(Kc + dst, ld16(k + i * 8));
        st16(Vc + dst, ld16(v + i * 8));
    }
}

// ---- decode attention ---------------------------------------------------------------------------------
struct AttnParams
{
    uint16_t* Y;              // [B, NH*HS]
    const uint16_t* Q;        // [B, NH*HS] post-norm/rope queries (unfused form), or NULL in the fused form
    int64_t q_b_stride;       // elements between two batches' query rows (0 = NH*HS; a packed [B, 1, 3C] MHA row: 3C)
    uint16_t* K;              // cache [B, NKV, capacity, HS]
    uint16_t* V;
    float* scratch;           // [B, NH, splits, HS+4] partials when splits > 1: O (HS) | m | l | pad (rows stay 16-byte aligned)
    int no_combine;           // leave the partials for the consumer (matvec_attn_combine) instead of launching the combine
    // warm ranges: extra workgroups of the attention launch (warm_a) and of the combine launch (warm_b) touch one dword per 128-byte
    // line of weights a LATER kernel streams, so the Infinity Cache fills while these latency-bound launches leave HBM idle
    const uint8_t* warm_a; int64_t warm_a_lines; int warm_a_blocks;   // blocks per grid row (blockIdx.x >= splits)
    const uint8_t* warm_b; int64_t warm_b_lines; int warm_b_blocks; int64_t warm_b_pair;
    uint32_t* tickets;        // one-pass form: arrival counters [B, NKV * head-groups], zero between launches; the workgroup whose
                              // partials arrive last combines its head-group's splits itself, so there is no combine launch
    int NH, NKV, capacity, position, window, splits;
    float scale;
    const int32_t* pos_dev;   // when set: the position is read from device memory (graph replay)
    int flat;                 // XCD-local grid (attn.xcd_local): blockIdx.x = group + ngroups * split, so that every split of a head group -- and the combine
                              // workgroups of its heads -- carry the same blockIdx.x % 8 and land on one XCD (workgroups are dealt round-robin over the 8 XCDs)
    // fused prologue (GemmaBlock::decode lines 315-337 folded in): raw projections + norm weights + RoPE cache
    int64_t raw_b_stride;     // elements between two batch rows of q_raw / k_raw / v_raw (a packed [B, 1, q | k | v] projection row; unused at B == 1)
    const uint16_t* q_raw;    // [NH*HS] per batch row
    const uint16_t* k_raw;    // [NKV*HS]
    const uint16_t* v_raw;    // [NKV*HS] (== k_raw on Gemma global layers)
    const uint16_t* qw;
    const uint16_t* kw;
    const uint16_t* vw;       // may be NULL (unit weight)
    const float* cos_cache;
    const float* sin_cache;
    float eps;
    int pos_stride;           // elements between two batch rows' position words at pos_dev: 0 = every row at *pos_dev (every entry but fused_attn_decode_rows_bf16), 1 = row b
                              // at pos_dev[b].  It reaches the kernels as bit 1 of the leading `flat` argument, not through this tail copy (attn_params below)
    uint32_t split_mul, split_shift;      // split_div_make(splits), set by launch_decode: the kernel's ceil(band / splits) without a divide (split_div.h)
};

// Combine of one head's split partials for output dim d by the lane that owns it: the arithmetic of attn_combine_kernel, shared by
// the standalone kernel (plain loads behind a kernel boundary) and the one-pass tail of attn_decode_kernel (SC1 = agent-coherent
// loads of partials other workgroups wrote through inside the same launch).  Lane s of the wave holds split s's (m, l).
template <bool SC1>
__device__ __forceinline__ float partial_ld(const float* p)
{
    if constexpr (SC1)
        return __hip_atomic_load((const __attribute__((address_space(1))) float*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        return *p;
}
template <bool SC1>
__device__ __forceinline__ uint16_t combine_dim(const float* __restrict__ base, int HS, int splits, int d)
{
    const int STR = HS + 4;
    const int s = threadIdx.x & 63;
    // every load of the first 16 splits is requested before anything is reduced: ONE memory round trip for splits <= 16
    float vals[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) vals[u] = (u < splits) ? partial_ld<SC1>(base + (size_t)u * STR + d) : 0.0f;
    const float ms = (s < splits) ? partial_ld<SC1>(base + (size_t)s * STR + HS) : -INFINITY;
    const float ls = (s < splits) ? partial_ld<SC1>(base + (size_t)s * STR + HS + 1) : 0.0f;
    float acc = 0.0f;
    const float M = wave_max(ms);
    const float fs = (ms == -INFINITY) ? 0.0f : __expf(ms - M);
    const float L = wave_sum(ls * fs);
    const int n8 = (splits + 7) & ~7;                      // the fma chain runs over whole batches of 8 (zeros past the last split)
    for (int i0 = 0; i0 < n8; i0 += 16)
    {
        if (i0 > 0)
        {
#pragma unroll
            for (int u = 0; u < 16; ++u) vals[u] = (i0 + u < splits) ? partial_ld<SC1>(base + (size_t)(i0 + u) * STR + d) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
        {
            const float f = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(fs), min(i0 + u, 63)));
            if (i0 + u < n8) acc = fmaf(vals[u], f, acc);
        }
    }
    return f32_to_bf16_bits(L > 0.0f ? acc / L : 0.0f);
}

// one dword per 128-byte line of [base, base + 128 nlines), lines strided over `nthreads` threads; nothing is written
// pair != 0: the range is the head of TWO streams `pair` bytes apart (the gate and up halves the fused gate_up kernel reads in
// lockstep): line i is line i / 2 of stream i % 2
__device__ __forceinline__ void warm_lines(const uint8_t* __restrict__ base, int64_t nlines, int64_t tid, int64_t nthreads, float* never,
                                           int64_t pair = 0)
{
    uint32_t acc = 0;
    int64_t i = tid;
    auto at = [&](int64_t l) { return pair ? base + (l & 1) * pair + (l >> 1) * 128 : base + l * 128; };
    for (; i + 7 * nthreads < nlines; i += 8 * nthreads)
    {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const uint32_t*>(at(i + u * nthreads));
#pragma unroll
        for (int u = 0; u < 8; ++u) acc ^= v[u];
    }
    for (; i < nlines; i += nthreads) acc ^= *reinterpret_cast<const uint32_t*>(at(i));
    if (acc == 0x12345679u && never != nullptr) never[0] = 1.0f;   // keeps the loads alive; never true in practice
}

// Diagnostic build only (-DMILA_ATTN_STAMPS, never the product library; tools/experiments/attn_stamps.sh): lane 0 of workgroup (0, 0, 0) of attn_decode_kernel adds the
// shader cycles from its first instruction to the issue of its first K/V row requests to g_attn_stamps[0], those to the first score of its first group to [2], and
// counts the launch in [1]; a buffer of its own, no output is touched.  Read back with mila_dbg_attn_stamps().
#ifdef MILA_ATTN_STAMPS
__device__ unsigned long long g_attn_stamps[3];
#endif

// HS = 64 * EPL (EPL in {2,4,8}) or HS = 64 handled as EPL = 2 on 32 active lanes.
// GH = query heads per workgroup; grid = (splits, NKV * GS/GH, B); 8 waves, wave w owns positions
// begin + w + 8 j of the split.  FUSED: the q/k/v post-processing of the token is done in the prologue; the new K/V row is appended to the cache by the split that
// owns it.  Canonical helpers (rms_rstd_wave, rms_apply8, rope_rotate8_regs) => bit-identical to the standalone rmsnorm / rope kernels and to qkv_post_kernel.
//
// Order of issue (EXPERIMENTS.md section 19): the position word (a vector load) -> the by-value tail -> the prologue's rows and norm weights, their sums of squares, rstd
// and weights, V parked in LDS: none of it needs the position -> position -> cos/sin row -> the K/V rows of the first group (both groups at HS 512), every request
// unconditional so that the waits behind them are counts -> rotation, LDS, barrier, q read-back under the K/V round trip -> append.  No integer division stands between
// the position word and a K/V request unless the band wraps a ring whose length is no power of two (one remainder per wave then).
//
// Arguments: the head of the kernel's latency chain is kernel arguments -> *pos_dev -> band and row addresses -> the first K/V round trip.  What that chain reads comes
// as leading plain parameters (14 dwords), which the dispatcher preloads into SGPRs before the first instruction (kernarg preload, build.py), so the load of *pos_dev is
// the first thing a wave does; the parameter block follows as a by-value tail that is fetched from the kernarg segment under that load.  The tail is the launcher's
// whole AttnParams: its copies of the leading fields are never read, the leading parameters replace them below.  The per-row position stride (0 or 1) is on that chain
// too -- it is part of the address of the position word -- so it travels in the leading block, as bit 1 of `flat`: read from the tail, the first load of every decode
// launch would wait for the kernarg fetch again.
// NEVER read the leading `flat` argument raw: it carries two flags (bit 0: the XCD-local grid, bit 1: per-row position words).  Kernels go through attn_params(),
// which splits it into AttnParams::flat (0 / 1) and AttnParams::pos_stride (0 / 1); a kernel that tested the raw value would see 2 and 3 under the rows entry.
#define MILA_ATTN_LEAD_PARAMS const int32_t* pos_dev, uint16_t* K, uint16_t* V, const uint16_t* q_raw, int NH, int NKV, int capacity, int window, int splits, int flat
#define MILA_ATTN_LEAD_ARGS(p) (p).pos_dev, (p).K, (p).V, (p).q_raw, (p).NH, (p).NKV, (p).capacity, (p).window, (p).splits, ((p).flat | ((p).pos_stride ? 2 : 0))
__device__ __forceinline__ AttnParams attn_params(MILA_ATTN_LEAD_PARAMS, const AttnParams& tail)
{
    AttnParams p = tail;
    p.pos_dev = pos_dev; p.K = K; p.V = V; p.q_raw = q_raw;
    p.NH = NH; p.NKV = NKV; p.capacity = capacity; p.window = window; p.splits = splits; p.flat = flat & 1; p.pos_stride = (flat >> 1) & 1;
    return p;
}

// CHAIN (unfused only; fused_attn_decode_chain_bf16): the batch rows are consecutive positions of ONE sequence -- row b is the query at position + b (the one position word
// + b) over cache 0, whose rows position .. position + B - 1 the prologue launch has appended already; a row's band ends at its own position, so it never sees the
// later rows.  From the band on, a row runs the code it runs alone.
template <int HS, int GH, bool FUSED, bool CHAIN = false>
__global__ __launch_bounds__(kDecodeWaves * 64) void attn_decode_kernel(MILA_ATTN_LEAD_PARAMS, const AttnParams tail)
{
#ifdef MILA_ATTN_STAMPS
    const unsigned long long entry_ = __builtin_amdgcn_s_memtime();
#endif
    using Row = DecodeGeomBf16<HS>;
    constexpr int NW = kDecodeWaves, EPL = Row::EPL, NPAIR = Row::NPAIR, ACTIVE = Row::ACTIVE, PG = Row::PG, STR = HS + 2;
    constexpr int GH_LOG2 = GH == 4 ? 2 : (GH == 2 ? 1 : 0);
    constexpr bool PRE2 = PG < 8;                          // HS 512: both register groups are requested before the prologue
    static_assert(GH == 1 || GH == 2 || GH == 4, "heads per workgroup: 1, 2 or 4");
    static_assert(GH + 2 <= NW, "one prologue row per wave");
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (scalar: the row walk and the prologue's roles are wave-uniform)
    const bool owner = lane < ACTIVE;
    const int b = blockIdx.z;
    static_assert(!(CHAIN && FUSED), "the chain form takes its q rows from the prologue launch");
    const int cb = CHAIN ? 0 : b;                          // the batch row whose cache this row reads

    // ---- the position word: the first request of the kernel, from the preloaded pointer.  A VECTOR load (every lane the same word, read back with readfirstlane):
    // scalar loads return out of order, so a wait for the by-value tail would wait for a scalar load of the position beside it, and everything below that needs the
    // tail but not the position -- the prologue's rows -- would stand behind the position.  Without a device position the word is read from the head of K and dropped.
    int lane_zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lane_zero));      // a zero the compiler cannot see through: keeps the address per-lane, hence the load a vector one
    const int32_t* pos_at = pos_dev ? pos_dev + b * ((flat >> 1) & 1) : reinterpret_cast<const int32_t*>(K);
    const int pos_word = pos_at[lane_zero];

    const AttnParams p = attn_params(pos_dev, K, V, q_raw, NH, NKV, capacity, window, splits, flat, tail);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* sm = reinterpret_cast<float*>(smem_raw);        // [NW][GH][HS + 2]
    uint16_t* qs = reinterpret_cast<uint16_t*>(smem_raw + (size_t)NW * GH * STR * sizeof(float));   // [GH][HS], then k_new, v_new

    if (!p.flat && (int)blockIdx.x >= p.splits)             // a warm block (block-uniform): no barrier is shared with the others
    {
        const int64_t wb = ((int64_t)(blockIdx.x - p.splits) * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z;
        warm_lines(p.warm_a, p.warm_a_lines, wb * (NW * 64) + threadIdx.x, (int64_t)p.warm_a_blocks * gridDim.y * gridDim.z * (NW * 64),
                   p.scratch);
        return;
    }
    // Head geometry without a division: NH = NKV * GS with GS a power of two (decode_group_size_ok, which every launcher checks) and GH a power of two that divides GS
    // (heads_per_group), so GS is a shift, a KV head's workgroups are a mask, and kvh * GS + hg * GH is grp * GH
    const int gs_log2 = __builtin_clz((unsigned)p.NKV) - __builtin_clz((unsigned)p.NH), hg_log2 = gs_log2 - GH_LOG2;
    int split = (int)blockIdx.x, grp = (int)blockIdx.y;
    if (p.flat)
    {
        const int ngrp = p.NKV << hg_log2;
        split = (int)blockIdx.x / ngrp;
        grp = (int)blockIdx.x % ngrp;
    }
    const int kvh = grp >> hg_log2, hg = grp & ((1 << hg_log2) - 1);
    const int h0 = grp * GH;                               // first query head of this workgroup
    uint16_t* kbase = p.K + ((size_t)cb * p.NKV + kvh) * p.capacity * HS;
    uint16_t* vbase = p.V + ((size_t)cb * p.NKV + kvh) * p.capacity * HS;

    // ---- what does not need the position: q (unfused), or the prologue's rows up to the rotation (fused) ----
    // Fused: wave r < GH takes query head h0 + r, wave GH the token's K row, wave GH + 1 its V row, in EVERY workgroup (whether this split owns the new row is known
    // only with the position; the LDS slots exist anyway).  Loads, sum of squares, rstd and the weights are done here; V is finished and parked in LDS.
    constexpr int hv = HS / 16;
    const bool act = lane < hv;                            // a lane holds chunks lane and lane + hv of the row (fused.hip's qkv_post_kernel assigns them the same way)
    const int l2 = act ? lane : 0;
    const bool has_row = FUSED && wave < GH + 2, rotates = FUSED && wave <= GH;
    uint32_t q[GH][NPAIR];
    u32x4 lo = u32x4{0u, 0u, 0u, 0u}, hi = lo;
    if constexpr (FUSED)
    {
        if (has_row)
        {
            const uint16_t* src = (wave < GH ? p.q_raw + (size_t)(h0 + wave) * HS : (wave == GH ? p.k_raw : p.v_raw) + (size_t)kvh * HS) + (size_t)b * p.raw_b_stride;
            const uint16_t* w = wave < GH ? p.qw : (wave == GH ? p.kw : p.vw);
            const u32x4 xlo = ld16(src + (size_t)l2 * 8), xhi = ld16(src + (size_t)(l2 + hv) * 8);
            u32x4 wlo = u32x4{0u, 0u, 0u, 0u}, whi = wlo;
            if (w) { wlo = ld16(w + (size_t)l2 * 8); whi = ld16(w + (size_t)(l2 + hv) * 8); }
            const float rstd = rms_rstd_wave(src, HS, p.eps);
            if (w) { lo = rms_apply8(xlo, wlo, rstd, 0.0f); hi = rms_apply8(xhi, whi, rstd, 0.0f); }
            else { lo = rms_apply8_now(xlo, rstd); hi = rms_apply8_now(xhi, rstd); }
            if (wave == GH + 1 && act)
            {
                st16(qs + (size_t)(GH + 1) * HS + (size_t)lane * 8, lo);
                st16(qs + (size_t)(GH + 1) * HS + (size_t)(lane + hv) * 8, hi);
            }
        }
    }
    else
    {
#pragma unroll
        for (int g = 0; g < GH; ++g)
        {
            const uint16_t* qp = p.Q + (size_t)b * (p.q_b_stride ? (size_t)p.q_b_stride : (size_t)p.NH * HS) + (size_t)(h0 + g) * HS + lane * EPL;
            if (owner) load_row<EPL>(q[g], qp);
            else
            {
#pragma unroll
                for (int e = 0; e < NPAIR; ++e) q[g][e] = 0u;
            }
        }
    }

    // the cache row of a wave's next position is the last one stepped by NW and wrapped once; a ring shorter than the step (NW % capacity: the one division, and it
    // does not wait for the position) wraps once too
    const uint32_t cap = (uint32_t)p.capacity;
    const uint32_t row_step = cap >= (uint32_t)NW ? (uint32_t)NW : (uint32_t)NW % cap;

    // ---- behind the position: no division up to the K/V requests on a cache the band does not wrap in, one remainder per wave on a ring ----
    const int pos_read = __builtin_amdgcn_readfirstlane(pos_word);     // (unconditional: a request left pending on one path would make every later wait a full drain)
    const int pos = (p.pos_dev ? pos_read : p.position) + (CHAIN ? b : 0);
    const int len = pos + 1;
    const int band_begin = (p.window > 0) ? max(0, len - p.window) : 0;
    const int band = len - band_begin;
    const int chunk = (int)split_div((uint32_t)(band + p.splits - 1), SplitDiv{p.split_mul, p.split_shift});      // (band + splits - 1) / splits
    const int begin = band_begin + split * chunk;
    const int end = min(begin + chunk, len);
    const bool owns_new = FUSED && pos >= begin && pos < end;   // this split appends (and consumes) the new K/V row

    // the cache row of a position: the position itself while nothing has wrapped (len <= capacity: every flat cache), else its remainder
    const bool wrapped = (uint32_t)len > cap;
    auto ring_row = [&](int pp) -> uint32_t {
        if (!wrapped) return (uint32_t)pp;
        return (cap & (cap - 1u)) == 0u ? (uint32_t)pp & (cap - 1u) : (uint32_t)pp % cap;
    };
    // the first cos/sin request goes out before the K/V rows: vector memory returns in order, and the rotation is what the barrier below waits for
    f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = c0, s0 = c0, s1 = c0;
    if constexpr (FUSED)
    {
        if (rotates)
        {
            const float* cos_row = p.cos_cache + (size_t)pos * (HS / 2) + l2 * 8;
            const float* sin_row = p.sin_cache + (size_t)pos * (HS / 2) + l2 * 8;
            c0 = *reinterpret_cast<const f32x4*>(cos_row); c1 = *reinterpret_cast<const f32x4*>(cos_row + 4);
            s0 = *reinterpret_cast<const f32x4*>(sin_row); s1 = *reinterpret_cast<const f32x4*>(sin_row + 4);
        }
    }

    // A group's row requests are unconditional, so that the waits behind them are counted, not drained: a slot past the split's end (or row `pos` of the fused form,
    // which is not in the cache yet and is patched in from LDS below) reads row 0 of its KV head and is zeroed on arrival.  `row` walks with the positions
    struct KVG { uint32_t k[PG][NPAIR], v[PG][NPAIR]; };
    int base = begin + wave;
    uint32_t row = ring_row(base);
    const uint32_t lane_el = owner ? (uint32_t)lane * EPL : 0u;      // (a row's address is a scalar base plus this: nothing per-lane is computed per row)
    auto load_group = [&](KVG& gbuf, int base_) {
#pragma unroll
        for (int j = 0; j < PG; ++j)
        {
            const int pp = base_ + NW * j;
            const bool valid = pp < end && !(FUSED && pp == pos);
            const size_t r = (size_t)(valid ? row : 0u) * HS;
            const uint32_t keep = (valid && owner) ? ~0u : 0u;      // (a mask, not a select: a select becomes a branch with a full drain on its zero side)
            uint32_t kk[NPAIR], vv[NPAIR];
            load_row<EPL>(kk, (kbase + r) + lane_el);
            load_row<EPL>(vv, (vbase + r) + lane_el);
            __builtin_amdgcn_sched_barrier(0);              // a row is requested as soon as its address exists, not behind the addresses of the whole group
#pragma unroll
            for (int e = 0; e < NPAIR; ++e) { gbuf.k[j][e] = kk[e] & keep; gbuf.v[j][e] = vv[e] & keep; }
            row += row_step;
            if (row >= cap) row -= cap;
        }
    };
    KVG ga, gb;
    load_group(ga, base);                                  // in flight while the prologue finishes
#ifdef MILA_ATTN_STAMPS
    const bool stamps_ = blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0;
    bool stamp_score_ = true;
    if (stamps_)
    {
        g_attn_stamps[0] += __builtin_amdgcn_s_memtime() - entry_;
        g_attn_stamps[1] += 1;
    }
#endif
    if constexpr (PRE2) load_group(gb, base + NW * PG);

    // ---- the rest of the prologue, under the K/V round trip: rotation, LDS, barrier, q read-back; then the append by the owner ----
    if constexpr (FUSED)
    {
        if (rotates && act)
        {
            rope_rotate8_regs(lo, hi, c0, c1, s0, s1);
            st16(qs + (size_t)wave * HS + (size_t)lane * 8, lo);
            st16(qs + (size_t)wave * HS + (size_t)(lane + hv) * 8, hi);
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < GH; ++g)
        {
            if (owner) load_row<EPL>(q[g], qs + (size_t)g * HS + lane * EPL);
            else
            {
#pragma unroll
                for (int e = 0; e < NPAIR; ++e) q[g][e] = 0u;
            }
        }
        if (has_row && wave >= GH && owns_new && hg == 0 && act)
        {
            uint16_t* dst = (wave == GH ? kbase : vbase) + (size_t)ring_row(pos) * HS;
            st16(dst + (size_t)lane * 8, lo);
            st16(dst + (size_t)(lane + hv) * 8, hi);
        }
    }

    float m[GH], l[GH], o[GH][EPL];
#pragma unroll
    for (int g = 0; g < GH; ++g)
    {
        m[g] = -INFINITY;
        l[g] = 0.0f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[g][e] = 0.0f;
    }

    auto patch_new = [&](KVG& gbuf, int base_) {           // put the LDS copy of row `pos` into its slot
        if constexpr (FUSED)
        {
            if (owns_new)
            {
#pragma unroll
                for (int j = 0; j < PG; ++j)
                    if (base_ + NW * j == pos && owner)
                    {
                        load_row<EPL>(gbuf.k[j], qs + (size_t)GH * HS + lane * EPL);
                        load_row<EPL>(gbuf.v[j], qs + (size_t)(GH + 1) * HS + lane * EPL);
                    }
            }
        }
    };
    auto compute_group = [&](const KVG& gbuf, int base_) {
        float sc[PG][GH];
#pragma unroll
        for (int j = 0; j < PG; ++j)
#pragma unroll
            for (int g = 0; g < GH; ++g)
            {
                float a = 0.0f;
#pragma unroll
                for (int e = 0; e < NPAIR; ++e) a = dot2_bf16(as_bf16x2(q[g][e]), as_bf16x2(gbuf.k[j][e]), a);
                sc[j][g] = a;
            }
#ifdef MILA_ATTN_STAMPS
        if (stamp_score_)
        {
            asm volatile("" :: "v"(sc[0][0]));             // the stamp stands behind the first score
            if (stamps_) g_attn_stamps[2] += __builtin_amdgcn_s_memtime() - entry_;
            stamp_score_ = false;
        }
#endif
        decode_softmax_step<GH, Row>(sc, gbuf.v, m, l, o, base_, end, p.scale);
    };
    // one step: request the group after `cur` into `nxt` (unless it is in flight already), then score `cur`
    auto step = [&](KVG& cur, KVG& nxt, bool nxt_in_flight) -> bool {
        if (base >= end) return false;
        const int nb = base + NW * PG;
        if (!nxt_in_flight && nb < end) load_group(nxt, nb);
        patch_new(cur, base);
        compute_group(cur, base);
        base = nb;
        return true;
    };
    if (step(ga, gb, PRE2))
        while (step(gb, ga, false) && step(ga, gb, false)) {}

    const DecodeFinishArgs a{p.Y, p.scratch, p.NH, p.splits, split, b, h0, p.tickets != nullptr};
    decode_finish<HS, GH, Row>(a, m, l, o, sm);
    if (p.splits > 1 && p.tickets != nullptr)
    {
        // Arrival ticket per (batch row, head-group): MI355X_MICROARCH.md hand-off table, row 1 (sc1 payload stores drained by
        // every storing wave, a workgroup barrier, ONE lane's agent-scope atomic add; the workgroup whose add came last reads
        // with sc1 loads, its other waves behind a barrier the adding wave joins).  The last arriver re-arms the counter.
        __shared__ int s_last;
        __syncthreads();
        uint32_t* tk = p.tickets + (size_t)b * gridDim.y + blockIdx.y;
        if (threadIdx.x == 0)
        {
            // acquire-release at agent scope on top of the drained write-through stores and the sc1 loads: the hand-off then
            // holds by the memory model too, not only by the measured behaviour of the sc1 forms (this path is not the fast one)
            const uint32_t t = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            const int last = (t == (uint32_t)(p.splits - 1));
            if (last) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = last;
        }
        __syncthreads();
        if (s_last)
        {
            for (int idx = threadIdx.x; idx < GH * HS; idx += NW * 64)
            {
                const int g = idx / HS, d = idx % HS;       // a wave's 64 dims lie in one head (HS % 64 == 0)
                const int h = h0 + g;
                const float* base = p.scratch + ((size_t)b * p.NH + h) * p.splits * (HS + 4);
                p.Y[((size_t)b * p.NH + h) * HS + d] = combine_dim<true>(base, HS, p.splits, d);
            }
        }
    }
}

// combine split partials: grid (NH, B, HS/64), 64 threads -> 64 dims each; splits <= 64.
// Every thread reads all (m, l) pairs itself (broadcast loads) and all partial values of its dim in
// unrolled batches, so the kernel is two dependent memory round trips long.
// flat_gh > 0 (attn.xcd_local): grid (NH * HS / 64, B): blockIdx.x = group + ngroups * (head in group + flat_gh * dim chunk), groups of flat_gh heads -- the
// workgroups of a head group share blockIdx.x % 8 with the decode workgroups that wrote its partials
__global__ __launch_bounds__(64) void attn_combine_kernel(uint16_t* __restrict__ Y, const float* __restrict__ scratch, int NH,
                                                          int HS, int splits, const uint8_t* __restrict__ warm, int64_t warm_lines_n, int64_t warm_pair, int flat_gh)
{
    int h = blockIdx.x, zc = blockIdx.z;
    const int b = blockIdx.y;
    if (flat_gh > 0)
    {
        const int ngroups = NH / flat_gh, grp = (int)blockIdx.x % ngroups, r = (int)blockIdx.x / ngroups;
        h = grp * flat_gh + r % flat_gh;
        zc = r / flat_gh;
    }
    else if ((int)blockIdx.z >= HS / 64)                    // warm blocks (see AttnParams::warm_b)
    {
        const int64_t wb = ((int64_t)(blockIdx.z - HS / 64) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        warm_lines(warm, warm_lines_n, wb * 64 + threadIdx.x, (int64_t)(gridDim.z - HS / 64) * gridDim.y * gridDim.x * 64, nullptr, warm_pair);
        return;
    }
    const int d = zc * 64 + threadIdx.x;
    const float* base = scratch + ((size_t)b * NH + h) * splits * (HS + 4);
    Y[((size_t)b * NH + h) * HS + d] = combine_dim<false>(base, HS, splits, d);
}


// ---- long-context decode on the matrix cores (round 3) ------------------------------------------------------------------------------------------
// Gemma's global layers put 16 query heads on ONE KV head: at one decode position those 16 heads ARE a 16-row MFMA tile, and K / V rows are shared by all of them.
// The wave-per-position kernel above costs a 64-lane reduction per (head, key): at 32 768 keys it is vector-ALU-bound, 63.7 us for 67 MB of K / V (1.05 TB/s,
// profiles/r03_long_context.txt) -- and its 8 head-groups of 2 read every row 8 times from L2.  Here a workgroup takes one split of the keys for all 16 heads: the
// tile body of attention_decode_mfma.h (shared with the fp8 KV cache's kernel, attention_kvfp8.hip) under the bf16 staging policy.  Partials in the layout of the
// scalar kernel: O (unnormalised, relative to M) | M | L per (head, split); up to 256 splits, merged by attn_combine_many_kernel.  fp32 scores and statistics, P
// rounded to bf16 for the PV product (as the flash kernels do): within 1 bf16 ulp of the double-precision oracle like them, NOT bit-identical to the scalar kernel --
// the choice depends on (window, capacity) only, so every path of a model (reference order, fused, graph replay) takes the same kernel.
// CHAIN: as in attn_decode_kernel -- batch row b is the query at position + b over cache 0
template <int HS, bool CHAIN = false>
__global__ __launch_bounds__(256) void attn_decode_mfma_kernel(MILA_ATTN_LEAD_PARAMS, const AttnParams tail)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_mfma[];
    const AttnParams p = attn_params(pos_dev, K, V, q_raw, NH, NKV, capacity, window, splits, flat, tail);
    const int pos = (p.pos_dev ? p.pos_dev[(int)blockIdx.z * p.pos_stride] : p.position) + (CHAIN ? (int)blockIdx.z : 0);      // blockIdx.z: the batch row (attention_decode_mfma.h)
    const MfmaDecodeArgs a{p.Q, p.q_b_stride, p.scratch, p.NH, p.NKV, p.capacity, pos + 1, p.window, p.splits, p.scale};
    attn_decode_mfma_body<HS, MfmaStageBf16<HS>, CHAIN>(a, MfmaStageBf16<HS>{p.K, p.V}, smem_mfma);
}

// merge of up to kMaxSplitsMfma partials per head: grid (NH, B, HS / 64), 4 waves; wave w merges splits 64 w .. 64 w + 63 as attn_combine_kernel does (lane s holds
// split s's (M, L); every load of a batch of 16 splits requested before anything is reduced), the four (acc, M, L) triples meet in LDS.  Fixed order: a replay
// reproduces an eager launch.  (A first form -- 64 threads walking all 256 splits with broadcast loads -- took 51 us for 8.4 MB of partials.)
__global__ __launch_bounds__(256) void attn_combine_many_kernel(uint16_t* __restrict__ Y, const float* __restrict__ scratch, int NH, int HS, int splits)
{
    __shared__ float s_acc[4][64], s_m[4], s_l[4];
    const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = blockIdx.z * 64 + lane;
    const int STR = HS + 4;
    const int s0 = wave * 64, n = min(64, splits - s0);          // this wave's splits (n <= 0: none)
    const float* base = scratch + (((size_t)b * NH + h) * splits + s0) * STR;
    float acc = 0.0f, M = -INFINITY, L = 0.0f;
    if (n > 0)
    {
        float vals[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) vals[u] = (u < n) ? base[(size_t)u * STR + d] : 0.0f;
        const float ms = (lane < n) ? base[(size_t)lane * STR + HS] : -INFINITY;
        const float ls = (lane < n) ? base[(size_t)lane * STR + HS + 1] : 0.0f;
        M = wave_max(ms);
        const float fs = (ms == -INFINITY) ? 0.0f : __expf(ms - M);
        L = wave_sum(ls * fs);
        const int n16 = (n + 15) & ~15;
        for (int i0 = 0; i0 < n16; i0 += 16)
        {
            if (i0 > 0)
            {
#pragma unroll
                for (int u = 0; u < 16; ++u) vals[u] = (i0 + u < n) ? base[(size_t)(i0 + u) * STR + d] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u)
            {
                const float f = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(fs), min(i0 + u, 63)));
                acc = fmaf(vals[u], f, acc);
            }
        }
    }
    s_acc[wave][lane] = acc;
    if (lane == 0) { s_m[wave] = M; s_l[wave] = L; }
    __syncthreads();
    if (wave == 0)
    {
        float Mt = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
        float Lt = 0.0f, out = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
        {
            const float f = (s_m[w] == -INFINITY) ? 0.0f : __expf(s_m[w] - Mt);
            Lt = fmaf(s_l[w], f, Lt);
            out = fmaf(s_acc[w][lane], f, out);
        }
        Y[((size_t)b * NH + h) * HS + d] = f32_to_bf16_bits(Lt > 0.0f ? out / Lt : 0.0f);
    }
}

// ---- the decode plan ------------------------------------------------------------------------------------------------------------------------------------
// Everything one decode call decides before it launches -- kernel form, split count, the band the splits are sized for, grid shape, scratch -- is a DecodePlan, made in
// ONE place (plan_decode) from the shape alone; run_decode launches from it, the size / split-count queries and mila_cdna4_attn_decode_plan_describe read it.  Each
// rule stands here once, its tunable beside it.
enum DecodeForm { DF_SCALAR, DF_MFMA, DF_GENERIC };      // attn_decode_kernel | attn_decode_mfma_kernel | attention_generic.hip (any other head size)
struct DecodePlan
{
    DecodeForm form;
    int splits, band_max;         // band_max: the most keys a launch of this shape sees (the window, or the live-length bucket)
    int gh, hgroups;              // query heads per workgroup, workgroups per KV head (scalar form)
    int flat;                     // AttnParams::flat
    bool prologue;                // MFMA form of a fused entry: q/k/v norm + RoPE + KV append as a launch of its own, the roped q rows parked behind the partials
    size_t partial_floats;        // B * NH * splits * (HS + 4)
    size_t scratch_need;          // bytes; 0 = the launch touches no scratch
};

constexpr int kMaxSplits = 64;
constexpr int kMaxSplitsMfma = 256;      // the long-context MFMA decode (attn_decode_mfma_kernel): one workgroup per CU
static int g_tune_positions_per_split = 64;     // tuning "attn.positions_per_split": positions one split covers
MILA_TUNE("attn.positions_per_split", g_tune_positions_per_split);
static int g_attn_max_wgs = 256;                // decode_splits: the split count is capped so that a launch has about this many workgroups
MILA_TUNE("attn.max_workgroups", g_attn_max_wgs);
static int g_attn_gh512 = 2;      // query heads per workgroup at HS 512 (experiment: 4 = half the head groups re-reading each K / V row, twice the accumulators per wave)
MILA_TUNE("attn.heads_per_group_512", g_attn_gh512);
static int g_tune_decode_mfma = 1;      // tuning "attn.mfma_decode": 0 = never take the MFMA decode
MILA_TUNE("attn.mfma_decode", g_tune_decode_mfma);
static int g_tune_kvfp8_mfma = 1;       // tuning "attn.kvfp8_mfma_decode": 0 = the fp8 KV cache (attention_kvfp8.hip) never takes its matrix-core decode: the scalar plan
MILA_TUNE("attn.kvfp8_mfma_decode", g_tune_kvfp8_mfma);
static int g_mfma_min_band = 8192;      // tuning "attn.mfma_min_band": band bucket (keys) from which a 16-head group on one KV head takes the MFMA decode (profiles/r04_attn_band.txt)
MILA_TUNE("attn.mfma_min_band", g_mfma_min_band);
// Experiment (round 4): every split of a head group and the combine workgroups of its heads on ONE XCD (blockIdx.x % 8 equal), so that the merge
// reads the partials from that XCD's L2 instead of across the fabric.  Same arithmetic per workgroup: bit-identical.  Result: profiles/r04_attn_pair_experiments.txt
static int g_attn_xcd_local = 0;
MILA_TUNE("attn.xcd_local", g_attn_xcd_local);

// The launch geometry of an unwindowed layer (split count, and whether the matrix-core decode serves it) is chosen from a BUCKET of the live length, not from the cache
// capacity: 4096, 8192, 16384, ... keys (doubling), clipped to the capacity.  (chosen from the capacity alone, a 32K-capacity cache decoding at position 2K
// ran the matrix-core kernel with 256 splits of 8 keys each -- 28.5 us against the scalar kernel's 23.9; the crossover is at ~8K keys, profiles/r04_attn_band.txt.)  A
// bucket is a function of the position only, so eager launches and a captured graph agree as long as the graph is re-captured when the position leaves its bucket
// (GemmaTransformer::ensureGraph asks mila_cdna4_attn_decode_band_bucket); inside a bucket the geometry is static, which is what a graph needs.  Caches of <= 4096 rows
// (the benchmark's) have one bucket.
static int band_bucket(int len, int capacity)
{
    int b = 4096;
    while (b < len && b < capacity) b <<= 1;
    return min(b, capacity);
}
static int heads_per_group(int GS, int HS) { return HS >= 512 ? (GS >= g_attn_gh512 && g_attn_gh512 == 4 ? 4 : (GS >= 2 ? 2 : 1)) : (GS >= 4 ? 4 : GS); }
static int decode_splits(int B, int NKV, int hgroups, int band)
{
    // ~256 workgroups of 8 waves, 64 positions (8 per wave) per split
    const int cap = max(1, g_attn_max_wgs / (NKV * hgroups * B));
    const int pps = g_tune_positions_per_split >= 8 ? g_tune_positions_per_split : 64;      // (a tuning value below 8 means the default)
    return max(1, min(min((band + pps - 1) / pps, cap), kMaxSplits));
}
static bool mfma_decode_applies(int NH, int NKV, int HS, int band_max)
{
    return g_tune_decode_mfma && HS == 512 && NKV > 0 && (NH / NKV) % 16 == 0 && band_max >= g_mfma_min_band;
}
static int mfma_decode_splits(int B, int NH, int NKV, int band_max)
{
    const int groups = NKV * ((NH / NKV) / 16) * B;
    const int s = (band_max + 127) / 128;                      // at least four key tiles per split at the full band
    return max(1, min(min(s, max(1, kNumCU / groups)), kMaxSplitsMfma));
}
// partials [B, NH, splits, HS + 4] floats, + the roped q rows [B, NH, HS] bf16 of a prologue launch
static size_t decode_scratch_bytes(int B, int NH, int HS, int splits, bool q_rows)
{
    return (size_t)B * NH * splits * (HS + 4) * sizeof(float) + (q_rows ? (size_t)B * NH * HS * 2 : 0);
}

// len_hint: an upper bound on the live length the launch is for -- position + 1 in the eager forms; in the device-position forms what the caller captured the graph for;
// 0 = the capacity.  The split count depends only on (window, band bucket), never on the current length inside a bucket, so that eager launches and a graph captured
// once reduce in the same order: bit-identical.  hooks: the entry uses tickets, no_combine or warm ranges, which address the 3-D grid of the scalar kernel.
// kvfp8: the plan is for the fp8 KV cache's entries (attention_kvfp8.hip), whose two kernels take the same forms by the same rules; under attn.kvfp8_mfma_decode 0 they
// keep to the scalar form's plan for the shape.
static DecodePlan plan_decode(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint, bool fused, bool hooks, bool kvfp8 = false)
{
    const bool scalar_only = kvfp8 && !g_tune_kvfp8_mfma;
    DecodePlan d{};
    const int GS = NH / NKV;
    const bool split_kernel = decode_scalar_head_size(HS);
    d.band_max = (window > 0 && window < capacity) ? window : (len_hint > 0 ? band_bucket(len_hint, capacity) : capacity);
    d.gh = heads_per_group(GS, HS);
    d.hgroups = GS / d.gh;
    if (mfma_decode_applies(NH, NKV, HS, d.band_max) && !hooks && !scalar_only)
    {
        // 16 heads on one KV head over a long band: the matrix-core decode.  The fused form is the CHAIN here: the 4 us its prologue launch costs are nothing against a
        // band of thousands of keys
        d.form = DF_MFMA;
        d.splits = mfma_decode_splits(B, NH, NKV, d.band_max);
        d.prologue = fused;
    }
    else
    {
        d.form = split_kernel ? DF_SCALAR : DF_GENERIC;
        d.splits = decode_splits(B, NKV, d.hgroups, d.band_max);
        // the XCD-local grid needs the head groups to tile the 8 XCDs (8 groups, or a multiple)
        d.flat = (g_attn_xcd_local && split_kernel && (NKV * d.hgroups) % 8 == 0 && !hooks) ? 1 : 0;
    }
    d.partial_floats = (size_t)B * NH * d.splits * (HS + 4);
    d.scratch_need = (d.form == DF_MFMA || (d.form == DF_SCALAR && d.splits > 1)) ? decode_scratch_bytes(B, NH, HS, d.splits, d.prologue) : 0;
    return d;
}
int launch_attn_combine_many(uint16_t* Y, const float* partials, int B, int NH, int HS, int splits, hipStream_t s)
{
    hipLaunchKernelGGL(attn_combine_many_kernel, dim3(NH, B, HS / 64), dim3(256), 0, s, Y, partials, NH, HS, splits);
    return check_hip(hipGetLastError(), "attn_combine_many");
}
template <bool CHAIN>
static int launch_decode_mfma(const AttnParams& p, int B, hipStream_t s)
{
    constexpr int HS = 512;
    note_form("attn_decode_mfma");
    static bool attr_set = false;      // (one per instantiation: the attribute belongs to the kernel)
    const size_t lds = mfma_decode_lds_bytes<HS>();
    if (!attr_set)
    {
        int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_decode_mfma_kernel<HS, CHAIN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute(attn_decode_mfma)");
        if (rc) return rc;
        attr_set = true;
    }
    const int n16 = (p.NH / p.NKV) / 16;
    hipLaunchKernelGGL((attn_decode_mfma_kernel<HS, CHAIN>), dim3(p.splits, p.NKV * n16, B), dim3(256), lds, s, MILA_ATTN_LEAD_ARGS(p), p);
    int rc = check_hip(hipGetLastError(), "attn_decode_mfma");
    if (rc) return rc;
    return launch_attn_combine_many(p.Y, p.scratch, B, p.NH, HS, p.splits, s);
}

template <int HS, int GH, bool FUSED, bool CHAIN = false>
static int launch_decode(const AttnParams& params, int B, hipStream_t s)
{
    AttnParams p = params;
    const SplitDiv sd = split_div_make((uint32_t)p.splits);
    p.split_mul = sd.mul;
    p.split_shift = sd.shift;
    const int hgroups = (p.NH / p.NKV) / GH;
    note_form("attn_decode");
    const size_t lds = (size_t)kDecodeWaves * GH * (HS + 2) * sizeof(float) + (size_t)(GH + 2) * HS * 2;
    const int wa = (p.warm_a && p.warm_a_lines > 0) ? p.warm_a_blocks : 0;
    if (p.flat)
    {
        // (only taken without warm blocks, tickets or a caller-side combine: plan_decode)
        hipLaunchKernelGGL((attn_decode_kernel<HS, GH, FUSED, CHAIN>), dim3(p.NKV * hgroups * p.splits, 1, B), dim3(kDecodeWaves * 64), lds, s, MILA_ATTN_LEAD_ARGS(p), p);
        int rc = check_hip(hipGetLastError(), "attn_decode (xcd-local)");
        if (rc || p.splits <= 1) return rc;
        hipLaunchKernelGGL(attn_combine_kernel, dim3(p.NH * (HS / 64), B, 1), dim3(64), 0, s, p.Y, p.scratch, p.NH, HS, p.splits, nullptr, 0, 0, GH);
        return check_hip(hipGetLastError(), "attn_combine (xcd-local)");
    }
    hipLaunchKernelGGL((attn_decode_kernel<HS, GH, FUSED, CHAIN>), dim3(p.splits + wa, p.NKV * hgroups, B), dim3(kDecodeWaves * 64), lds, s, MILA_ATTN_LEAD_ARGS(p), p);
    int rc = check_hip(hipGetLastError(), "attn_decode");
    if (rc) return rc;
    if (p.splits > 1 && !p.no_combine && !p.tickets)
    {
        const int wbk = (p.warm_b && p.warm_b_lines > 0) ? p.warm_b_blocks : 0;
        hipLaunchKernelGGL(attn_combine_kernel, dim3(p.NH, B, HS / 64 + wbk), dim3(64), 0, s, p.Y, p.scratch, p.NH, HS, p.splits, p.warm_b,
                           p.warm_b_lines, p.warm_b_pair, 0);
        rc = check_hip(hipGetLastError(), "attn_combine");
    }
    return rc;
}

// the scalar form of a plan: the plan's heads per workgroup at one of the four head sizes (attention_decode_plan.h), the generic kernel at any other
template <bool FUSED, bool CHAIN = false>
static int dispatch_hs(int HS, int gh, const AttnParams& p, int B, hipStream_t s)
{
    if (decode_scalar_head_size(HS))
    {
        const int GS = p.NH / p.NKV;
        if (!decode_group_size_ok(GS)) return set_error(MILA_E_UNSUPPORTED, "attention: group size %d (NH/NKV) must be 1,2,4,8,16 or 32", GS);
        const int rc = dispatch_decode_scalar<true>(HS, gh, [&](auto hs, auto g) { return launch_decode<decltype(hs)::value, decltype(g)::value, FUSED, CHAIN>(p, B, s); });
        if (rc == kNoDecodeKernel) return set_error(MILA_E_UNSUPPORTED, "attention: no kernel for %d heads per workgroup at HS=%d", gh, HS);
        return rc;
    }
    if constexpr (!FUSED && !CHAIN)
    {
        // any other head size: one wave per (batch, head) row on the generic kernel (attention_generic.hip); the position may live on the device only in the
        // captured forms, which the benchmarked head sizes alone use
        if (p.pos_dev) return set_error(MILA_E_UNSUPPORTED, "attention: the device-position form needs a head size of 64, 128, 256 or 512 (got %d)", HS);
        const int64_t qbs = p.q_b_stride ? p.q_b_stride : (int64_t)p.NH * HS;
        GenericAttnParams g{p.Y, p.Q, p.K, p.V, qbs, qbs, (int64_t)p.NKV * p.capacity * HS, (int64_t)p.capacity * HS, HS,
                            B, 1, p.NH, p.NKV, HS, p.capacity, p.position, p.window, p.scale};
        return launch_attn_generic(g, s);
    }
    return set_error(MILA_E_UNSUPPORTED, "attention: head size %d must be 64, 128, 256 or 512", HS);
}

// The one executor: scratch check against the plan, the prologue launch where the plan has one, the leaf launcher of the plan's form.  A fused call has p.q_raw set.
static int run_decode(const DecodePlan& d, AttnParams p, int B, int HS, size_t scratch_bytes, const char* who, hipStream_t stream)
{
    const bool fused = p.q_raw != nullptr;
    p.splits = d.splits;
    p.flat = d.flat;
    if (d.scratch_need && (!p.scratch || scratch_bytes < d.scratch_need))
        return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, d.scratch_need);
    if (d.form != DF_MFMA) return fused ? dispatch_hs<true>(HS, d.gh, p, B, stream) : dispatch_hs<false>(HS, d.gh, p, B, stream);
    if (d.prologue)
    {
        uint16_t* q_tmp = reinterpret_cast<uint16_t*>(p.scratch + d.partial_floats);
        for (int b = 0; b < B; ++b)
        {
            uint16_t* kc = p.K + (size_t)b * p.NKV * p.capacity * HS;
            uint16_t* vc = p.V + (size_t)b * p.NKV * p.capacity * HS;
            const size_t ro = (size_t)b * p.raw_b_stride;
            const int rc = p.pos_dev ? mila_cdna4_fused_qkv_post_devpos(q_tmp + (size_t)b * p.NH * HS, kc, vc, p.q_raw + ro, p.k_raw + ro, p.v_raw + ro, p.qw, p.kw, p.vw, p.cos_cache,
                                                                        p.sin_cache, p.NH, p.NKV, HS, p.pos_dev + (size_t)b * p.pos_stride, p.capacity, p.eps,
                                                                        reinterpret_cast<mila_stream_t>(stream))
                                     : mila_cdna4_fused_qkv_post(q_tmp + (size_t)b * p.NH * HS, kc, vc, p.q_raw + ro, p.k_raw + ro, p.v_raw + ro, p.qw, p.kw, p.vw, p.cos_cache,
                                                                 p.sin_cache, p.NH, p.NKV, HS, p.position, p.capacity, p.eps, reinterpret_cast<mila_stream_t>(stream));
            if (rc) return rc;
        }
        p.Q = q_tmp;
        p.q_b_stride = 0;
    }
    return launch_decode_mfma<false>(p, B, stream);
}

// The unfused entries (attn_decode_bf16, its device-position form, mha_decode_bf16): plan and launch.  q_b_stride as in AttnParams; len_hint as in plan_decode.
static int unfused_decode(const char* who, uint16_t* Y, const uint16_t* Q, int64_t q_b_stride, const uint16_t* Kc, const uint16_t* Vc, void* scratch, size_t scratch_bytes, int B,
                          int NH, int NKV, int HS, int capacity, int position, const int32_t* pos_dev, int len_hint, int window, float scale, hipStream_t stream)
{
    AttnParams p{};
    p.Y = Y; p.Q = Q; p.q_b_stride = q_b_stride; p.K = const_cast<uint16_t*>(Kc); p.V = const_cast<uint16_t*>(Vc); p.scratch = reinterpret_cast<float*>(scratch);
    p.NH = NH; p.NKV = NKV; p.capacity = capacity; p.position = position; p.pos_dev = pos_dev; p.window = window; p.scale = scale;
    return run_decode(plan_decode(B, NH, NKV, HS, capacity, window, len_hint, false, false), p, B, HS, scratch_bytes, who, stream);
}

// What the fused entry points share: the checks (`who` names the entry in the messages), the prologue fields of AttnParams, the plan and its launch.  The argument
// block is fused_attn_decode_ex's; the other entries fill it from their parameter lists.
// the batch entry's B / raw_b_stride checks | tickets are required | no Y: the partials stay in scratch | row b at position_dev[b], planned as ONE row
enum { FD_BATCH = 1, FD_TICKETS = 2, FD_PARTIALS = 4, FD_ROWS = 8 };
static int fused_decode(const char* who, const mila_fused_attn_args& a, int B, int64_t raw_b_stride, int flags, hipStream_t stream)
{
    MILA_REQUIRE((a.Y || (flags & FD_PARTIALS)) && a.Kc && a.Vc && a.q_raw && a.k_raw && a.v_raw && a.qw && a.kw && a.cos_cache && a.sin_cache &&
                 (a.tickets || !(flags & FD_TICKETS)), "%s: null pointer", who);
    if (flags & FD_BATCH)
    {
        MILA_REQUIRE(B > 0 && a.NH > 0 && a.NKV > 0 && a.NH % a.NKV == 0, "%s: bad sizes (B=%d NH=%d NKV=%d)", who, B, a.NH, a.NKV);
        MILA_REQUIRE(B == 1 || raw_b_stride >= (int64_t)a.NKV * a.HS, "%s: raw_b_stride %lld is shorter than a K row", who, (long long)raw_b_stride);
    }
    else
        MILA_REQUIRE(a.NH > 0 && a.NKV > 0 && a.NH % a.NKV == 0, "%s: bad head counts (NH=%d NKV=%d)", who, a.NH, a.NKV);
    MILA_REQUIRE(a.capacity > 0 && a.window >= 0 && (a.position_dev || a.position >= 0), "%s: bad sizes", who);
    MILA_REQUIRE(a.HS % 16 == 0, "%s: HS=%d must be a multiple of 16", who, a.HS);
    MILA_REQUIRE(a.warm_a_blocks >= 0 && a.warm_a_blocks <= 64 && a.warm_b_blocks >= 0 && a.warm_b_blocks <= 64, "%s: warm block counts must be in [0, 64]", who);
    if (a.tickets)
        MILA_REQUIRE(a.ticket_count >= mila_cdna4_attn_decode_ticket_count(1, a.NH), "%s: %zu tickets < required %zu", who, a.ticket_count,
                     mila_cdna4_attn_decode_ticket_count(1, a.NH));
    AttnParams p{};
    p.Y = a.Y; p.K = a.Kc; p.V = a.Vc; p.scratch = reinterpret_cast<float*>(a.scratch);
    p.NH = a.NH; p.NKV = a.NKV; p.capacity = a.capacity; p.position = a.position; p.pos_dev = a.position_dev; p.window = a.window; p.scale = a.scale;
    p.q_raw = a.q_raw; p.k_raw = a.k_raw; p.v_raw = a.v_raw; p.raw_b_stride = raw_b_stride; p.qw = a.qw; p.kw = a.kw; p.vw = a.vw;
    p.cos_cache = a.cos_cache; p.sin_cache = a.sin_cache; p.eps = a.eps;
    p.tickets = a.tickets;
    p.no_combine = (flags & FD_PARTIALS) ? 1 : 0;
    p.pos_stride = (flags & FD_ROWS) ? 1 : 0;
    if (a.warm_a && a.warm_a_bytes >= 128 && a.warm_a_blocks > 0) { p.warm_a = (const uint8_t*)a.warm_a; p.warm_a_lines = (int64_t)(a.warm_a_bytes / 128); p.warm_a_blocks = a.warm_a_blocks; }
    if (a.warm_b && a.warm_b_bytes >= 128 && a.warm_b_blocks > 0) { p.warm_b = (const uint8_t*)a.warm_b; p.warm_b_lines = (int64_t)(a.warm_b_bytes / 128); p.warm_b_blocks = a.warm_b_blocks; p.warm_b_pair = (int64_t)a.warm_b_pair_offset; }
    // under position_dev, `position` carries the live-length bound the launch is captured for (0 = the capacity)
    // FD_ROWS: rows are independent sequences, and a row must have the bits it has decoded alone -- the splits are planned for ONE row and used for every row (a B-row
    // plan would share the chip between the rows and reduce each row over fewer, longer splits); only the scratch is sized for all of them
    DecodePlan d = plan_decode((flags & FD_ROWS) ? 1 : B, a.NH, a.NKV, a.HS, a.capacity, a.window, a.position_dev ? a.position : a.position + 1, true,
                               p.tickets || p.no_combine || p.warm_a || p.warm_b);
    if ((flags & FD_ROWS) && B > 1)
    {
        d.partial_floats *= (size_t)B;
        if (d.scratch_need) d.scratch_need = decode_scratch_bytes(B, a.NH, a.HS, d.splits, d.prologue);
    }
    if (flags & FD_PARTIALS) MILA_REQUIRE(d.splits > 1, "%s: this (window, capacity) runs unsplit; use fused_attn_decode_bf16", who);
    if (!a.position_dev)
    {
        const int band = live_band(a.position + 1, a.window);
        MILA_REQUIRE(band <= a.capacity, "%s: live band %d exceeds the cache capacity %d", who, band, a.capacity);
    }
    return run_decode(d, p, B, a.HS, a.scratch_bytes, who, stream);
}
static mila_fused_attn_args fused_args(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw, const uint16_t* v_raw, const uint16_t* qw,
                                       const uint16_t* kw, const uint16_t* vw, const float* cos_cache, const float* sin_cache, void* scratch, size_t scratch_bytes,
                                       uint32_t* tickets, size_t ticket_count, int NH, int NKV, int HS, int capacity, int position, const int32_t* position_dev, int window,
                                       float scale, float eps)
{
    return mila_fused_attn_args{Y, Kc, Vc, q_raw, k_raw, v_raw, qw, kw, vw, cos_cache, sin_cache, scratch, scratch_bytes, tickets, ticket_count, nullptr, 0, 0, nullptr, 0, 0, 0,
                                NH, NKV, HS, capacity, position, position_dev, window, scale, eps};
}

// ---- the chain: T consecutive positions of ONE sequence in one call (speculative verification) ----
// Launch (a): qkv_post_kernel over T tokens -- norm, RoPE, the roped q rows into scratch behind the partials, K / V rows position .. position + T - 1 into the cache.
// Launch (b): the unfused kernel of the plan's form in its CHAIN instantiation (row t = the query at position + t over that one cache), then the form's combine.
// The plan is ONE row's at the max_len bucket (as FD_ROWS): row t reduces over the splits it has alone, and the prologue's rows are the bits the fused kernel's own
// prologue makes (the canonical helpers), so row t is fused_attn_decode_bf16 at position + t bit for bit.
static size_t chain_partial_floats(const DecodePlan& d, int T, int NH, int HS)
{
    return (d.form == DF_MFMA || d.splits > 1) ? (size_t)T * NH * d.splits * (HS + 4) : 0;
}
static int chain_decode(const char* who, const mila_fused_attn_args& a, int T, int64_t raw_b_stride, hipStream_t stream)
{
    MILA_REQUIRE(a.Y && a.Kc && a.Vc && a.q_raw && a.k_raw && a.v_raw && a.qw && a.kw && a.cos_cache && a.sin_cache && a.scratch, "%s: null pointer", who);
    MILA_REQUIRE(T >= 2 && T <= 4, "%s: T=%d rows outside 2 .. 4", who, T);
    MILA_REQUIRE(decode_scalar_head_size(a.HS), "%s: head size %d must be 64, 128, 256 or 512", who, a.HS);
    MILA_REQUIRE(a.NH > 0 && a.NKV > 0 && a.NH % a.NKV == 0 && decode_group_size_ok(a.NH / a.NKV), "%s: bad head counts (NH=%d NKV=%d)", who, a.NH, a.NKV);
    MILA_REQUIRE(a.capacity > 0 && a.window >= 0, "%s: bad sizes", who);
    MILA_REQUIRE(raw_b_stride % 8 == 0 && raw_b_stride >= (int64_t)a.HS, "%s: raw_b_stride %lld must be a multiple of 8 and no shorter than a head row", who, (long long)raw_b_stride);
    // a.position: the first row's position (eager), or max_len = the live-length bound of the LAST row (device position)
    if (a.position_dev)
        MILA_REQUIRE(a.position >= 0 && a.position <= a.capacity, "%s: max_len %d outside 0 .. the capacity %d", who, a.position, a.capacity);
    else
        MILA_REQUIRE(a.position >= 0 && (int64_t)a.position + T <= (int64_t)a.capacity,
                     "%s: positions %d .. %d do not fit the cache capacity %d (the chain is for unbounded caches, not rings)", who, a.position, a.position + T - 1, a.capacity);
    const int len_hint = a.position_dev ? a.position : a.position + T;
    DecodePlan d = plan_decode(1, a.NH, a.NKV, a.HS, a.capacity, a.window, len_hint, true, false);
    d.partial_floats = chain_partial_floats(d, T, a.NH, a.HS);
    d.scratch_need = d.partial_floats * sizeof(float) + (size_t)T * a.NH * a.HS * 2;
    if (a.scratch_bytes < d.scratch_need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, a.scratch_bytes, d.scratch_need);
    uint16_t* q_tmp = reinterpret_cast<uint16_t*>(reinterpret_cast<float*>(a.scratch) + d.partial_floats);
    const mila_stream_t ms = reinterpret_cast<mila_stream_t>(stream);
    int rc = a.position_dev ? mila_cdna4_fused_qkv_post_rows_devpos(q_tmp, a.Kc, a.Vc, a.q_raw, a.k_raw, a.v_raw, raw_b_stride, a.qw, a.kw, a.vw, a.cos_cache, a.sin_cache, T, a.NH,
                                                                    a.NKV, a.HS, a.position_dev, a.capacity, a.eps, ms)
                            : mila_cdna4_fused_qkv_post_prefill(q_tmp, a.Kc, a.Vc, a.q_raw, a.k_raw, a.v_raw, raw_b_stride, a.qw, a.kw, a.vw, a.cos_cache, a.sin_cache, T, a.NH,
                                                                a.NKV, a.HS, a.position, a.capacity, a.eps, ms);
    if (rc) return rc;
    AttnParams p{};
    p.Y = a.Y; p.Q = q_tmp; p.K = a.Kc; p.V = a.Vc; p.scratch = reinterpret_cast<float*>(a.scratch);
    p.NH = a.NH; p.NKV = a.NKV; p.capacity = a.capacity; p.position = a.position; p.pos_dev = a.position_dev; p.window = a.window; p.scale = a.scale;
    p.splits = d.splits;
    p.flat = d.flat;
    if (d.form == DF_MFMA) return launch_decode_mfma<true>(p, T, stream);
    return dispatch_hs<false, true>(a.HS, d.gh, p, T, stream);
}

// ---- what attention_kvfp8.hip takes from this file (attention_decode_plan.h) ----
KvFp8DecodeShape plan_decode_kvfp8(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint)
{
    const DecodePlan d = plan_decode(B, NH, NKV, HS, capacity, window, len_hint, false, false, true);
    return KvFp8DecodeShape{d.form == DF_MFMA, d.splits, d.gh, d.hgroups, d.scratch_need};
}
int launch_attn_combine(uint16_t* Y, const float* partials, int B, int NH, int HS, int splits, hipStream_t s)
{
    hipLaunchKernelGGL(attn_combine_kernel, dim3(NH, B, HS / 64), dim3(64), 0, s, Y, partials, NH, HS, splits, nullptr, 0, 0, 0);
    return check_hip(hipGetLastError(), "attn_combine");
}

// packed [B, T, 3C] rows -> K / V rows of a [B, NH, capacity, HS] cache at positions start_pos .. start_pos + T - 1 (the K / V part of the reference's
// permute_qkv / permute_qkv_decode, CudaMhaOp.ixx:166-170, :276-280)
__global__ __launch_bounds__(256) void mha_kv_write_kernel(uint16_t* __restrict__ Kc, uint16_t* __restrict__ Vc, const uint16_t* __restrict__ QKV,
                                                           int64_t total, int T, int C, int HS, int start_pos, int capacity)
{
    const int NH = C / HS;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride)
    {
        const int c = (int)(i % C);
        const int64_t bt = i / C;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const int h = c / HS, d = c - h * HS;
        const size_t dst = (((size_t)b * NH + h) * capacity + (start_pos + t)) * HS + d;
        const uint16_t* row = QKV + bt * 3 * (int64_t)C;
        Kc[dst] = row[C + c];
        Vc[dst] = row[2 * C + c];
    }
}
// the same with 16-byte accesses (HS % 8 == 0: a head row is whole 8-element vectors; C % 8 == 0 follows)
__global__ __launch_bounds__(256) void mha_kv_write_vec_kernel(uint16_t* __restrict__ Kc, uint16_t* __restrict__ Vc, const uint16_t* __restrict__ QKV,
                                                               int64_t total_vec, int T, int C, int HS, int start_pos, int capacity)
{
    const int NH = C / HS, cv = C / 8;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_vec; i += stride)
    {
        const int c = (int)(i % cv) * 8;
        const int64_t bt = i / cv;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const int h = c / HS, d = c - h * HS;
        const size_t dst = (((size_t)b * NH + h) * capacity + (start_pos + t)) * HS + d;
        const uint16_t* row = QKV + bt * 3 * (int64_t)C;
        st16(Kc + dst, ld16(row + C + c));
        st16(Vc + dst, ld16(row + 2 * C + c));
    }
}

}  // namespace mila

using namespace mila;

extern "C" {

#ifdef MILA_ATTN_STAMPS
MILA_API int mila_dbg_attn_stamps(unsigned long long* out3)
{
    return (int)hipMemcpyFromSymbol(out3, HIP_SYMBOL(mila::g_attn_stamps), 3 * sizeof(unsigned long long));
}
#endif

int mila_cdna4_kv_write_bf16(uint16_t* Kc, uint16_t* Vc, const uint16_t* k, const uint16_t* v, int B, int chunk, int NKV,
                             int HS, int start_pos, int capacity, mila_stream_t stream)
{
    MILA_REQUIRE(Kc && Vc && k && v, "kv_write_bf16: null pointer");
    MILA_REQUIRE(B > 0 && chunk > 0 && NKV > 0 && HS > 0 && capacity > 0, "kv_write_bf16: bad sizes");
    MILA_REQUIRE(HS % 8 == 0, "kv_write_bf16: HS=%d must be a multiple of 8", HS);
    MILA_REQUIRE(start_pos >= 0, "kv_write_bf16: negative start position");
    MILA_REQUIRE(chunk <= capacity, "kv_write_bf16: chunk %d exceeds the cache capacity %d", chunk, capacity);
    const int64_t total_vec = (int64_t)B * chunk * NKV * (HS / 8);
    int blocks = ceil_div(total_vec, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(kv_write_bf16_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), Kc, Vc, k, v, total_vec, chunk,
                       NKV, HS, start_pos, capacity);
    MILA_LAUNCH_CHECK("kv_write_bf16");
}

// the largest scratch_need of the plans a (B, NH, HS) can take: kMaxSplits partials per head, or (HS 512) the MFMA decode's kMaxSplitsMfma + the roped q rows of its fused form
size_t mila_cdna4_attn_decode_scratch_bytes(int B, int NH, int HS)
{
    if (B <= 0 || NH <= 0 || HS <= 0) return 0;
    return std::max(decode_scratch_bytes(B, NH, HS, kMaxSplits, false), HS == 512 ? decode_scratch_bytes(B, NH, HS, kMaxSplitsMfma, true) : 0);
}

int mila_cdna4_attn_decode_band_bucket(int len, int capacity) { return capacity > 0 ? band_bucket(len, capacity) : 0; }

int mila_cdna4_attn_decode_bf16(uint16_t* Y, const uint16_t* Q, const uint16_t* Kc, const uint16_t* Vc, void* scratch,
                                size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity, int len, int window,
                                float scale, mila_stream_t stream)
{
    MILA_REQUIRE(Y && Q && Kc && Vc, "attn_decode_bf16: null pointer");
    MILA_REQUIRE(B > 0 && NH > 0 && NKV > 0 && NH % NKV == 0, "attn_decode_bf16: bad head counts (NH=%d NKV=%d)", NH, NKV);
    MILA_REQUIRE(len > 0 && capacity > 0, "attn_decode_bf16: len and capacity must be positive (len=%d capacity=%d)", len, capacity);
    MILA_REQUIRE(window >= 0, "attn_decode_bf16: negative window");
    const int band = live_band(len, window);
    MILA_REQUIRE(band <= capacity, "attn_decode_bf16: live band %d exceeds the cache capacity %d", band, capacity);
    return unfused_decode("attn_decode_bf16", Y, Q, 0, Kc, Vc, scratch, scratch_bytes, B, NH, NKV, HS, capacity, len - 1, nullptr, len, window, scale, as_stream(stream));
}

int mila_cdna4_attn_decode_bf16_devpos(uint16_t* Y, const uint16_t* Q, const uint16_t* Kc, const uint16_t* Vc, void* scratch,
                                       size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity,
                                       const int32_t* position_dev, int max_len, int window, float scale,
                                       mila_stream_t stream)
{
    MILA_REQUIRE(Y && Q && Kc && Vc && position_dev, "attn_decode_bf16_devpos: null pointer");
    MILA_REQUIRE(B > 0 && NH > 0 && NKV > 0 && NH % NKV == 0, "attn_decode_bf16_devpos: bad head counts (NH=%d NKV=%d)", NH, NKV);
    MILA_REQUIRE(max_len > 0 && capacity > 0 && window >= 0, "attn_decode_bf16_devpos: bad sizes");
    const int band = live_band(max_len, window);
    MILA_REQUIRE(band <= capacity, "attn_decode_bf16_devpos: live band %d exceeds the cache capacity %d", band, capacity);
    return unfused_decode("attn_decode_bf16_devpos", Y, Q, 0, Kc, Vc, scratch, scratch_bytes, B, NH, NKV, HS, capacity, 0, position_dev, max_len, window, scale, as_stream(stream));
}

// Fused decode attention for one token (B == 1): per-head q/k/v RMSNorm + RoPE + KV append + flash-decode.
// position_dev != NULL selects the graph-replay form (position read from device memory).
int mila_cdna4_fused_attn_decode_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw,
                                      const uint16_t* v_raw, const uint16_t* qw, const uint16_t* kw, const uint16_t* vw,
                                      const float* cos_cache, const float* sin_cache, void* scratch, size_t scratch_bytes,
                                      int NH, int NKV, int HS, int capacity, int position, const int32_t* position_dev,
                                      int window, float scale, float eps, mila_stream_t stream)
{
    return fused_decode("fused_attn_decode_bf16", fused_args(Y, Kc, Vc, q_raw, k_raw, v_raw, qw, kw, vw, cos_cache, sin_cache, scratch, scratch_bytes, nullptr, 0, NH, NKV, HS,
                                                             capacity, position, position_dev, window, scale, eps), 1, 0, 0, as_stream(stream));
}

// The same launch for B rows decoded at one position (Gqa.Decode.Bf16.cu:379-387 takes the batch in its grid): batch row b reads its raw projections at
// q_raw / k_raw / v_raw + b * raw_b_stride (the three pointers into one packed [B, 1, q | k | v] row, or separate dense tensors) and its own caches; Y [B, NH*HS].
int mila_cdna4_fused_attn_decode_batch_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw,
                                            const uint16_t* v_raw, int64_t raw_b_stride, const uint16_t* qw, const uint16_t* kw, const uint16_t* vw,
                                            const float* cos_cache, const float* sin_cache, void* scratch, size_t scratch_bytes, int B,
                                            int NH, int NKV, int HS, int capacity, int position, const int32_t* position_dev,
                                            int window, float scale, float eps, mila_stream_t stream)
{
    return fused_decode("fused_attn_decode_batch_bf16", fused_args(Y, Kc, Vc, q_raw, k_raw, v_raw, qw, kw, vw, cos_cache, sin_cache, scratch, scratch_bytes, nullptr, 0, NH, NKV,
                                                                   HS, capacity, position, position_dev, window, scale, eps), B, raw_b_stride, FD_BATCH, as_stream(stream));
}
// B independent sequences, row b at positions_dev[b]: see mila_cdna4.h for the invariance this entry keeps
int mila_cdna4_fused_attn_decode_rows_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw, const uint16_t* v_raw, int64_t raw_b_stride,
                                           const uint16_t* qw, const uint16_t* kw, const uint16_t* vw, const float* cos_cache, const float* sin_cache, void* scratch,
                                           size_t scratch_bytes, int B, int NH, int NKV, int HS, int capacity, const int32_t* positions_dev, int max_len, int window, float scale,
                                           float eps, mila_stream_t stream)
{
    MILA_REQUIRE(positions_dev != nullptr, "fused_attn_decode_rows_bf16: positions_dev is required (the rows' positions live on the device)");
    MILA_REQUIRE(max_len >= 0 && max_len <= capacity, "fused_attn_decode_rows_bf16: max_len %d outside 0 .. the capacity %d", max_len, capacity);
    MILA_REQUIRE(decode_scalar_head_size(HS), "fused_attn_decode_rows_bf16: head size %d must be 64, 128, 256 or 512", HS);
    return fused_decode("fused_attn_decode_rows_bf16", fused_args(Y, Kc, Vc, q_raw, k_raw, v_raw, qw, kw, vw, cos_cache, sin_cache, scratch, scratch_bytes, nullptr, 0, NH, NKV,
                                                                  HS, capacity, max_len, positions_dev, window, scale, eps),
                        B, raw_b_stride, FD_BATCH | FD_ROWS, as_stream(stream));
}

// T consecutive positions of ONE sequence on ONE cache: see mila_cdna4.h for the contract (row t == fused_attn_decode_bf16 at position + t)
int mila_cdna4_fused_attn_decode_chain_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw, const uint16_t* v_raw, int64_t raw_b_stride,
                                            const uint16_t* qw, const uint16_t* kw, const uint16_t* vw, const float* cos_cache, const float* sin_cache, void* scratch,
                                            size_t scratch_bytes, int T, int NH, int NKV, int HS, int capacity, int position, const int32_t* position_dev, int max_len, int window,
                                            float scale, float eps, mila_stream_t stream)
{
    return chain_decode("fused_attn_decode_chain_bf16", fused_args(Y, Kc, Vc, q_raw, k_raw, v_raw, qw, kw, vw, cos_cache, sin_cache, scratch, scratch_bytes, nullptr, 0, NH, NKV, HS,
                                                                   capacity, position_dev ? max_len : position, position_dev, window, scale, eps),
                        T, raw_b_stride, as_stream(stream));
}
// the largest scratch a chain call of (T, NH, HS) can need: the partials of T rows at the most splits a plan takes, plus the roped q rows [T, NH, HS] bf16
size_t mila_cdna4_attn_decode_chain_scratch_bytes(int T, int NH, int HS)
{
    if (T < 2 || T > 4 || NH <= 0 || !decode_scalar_head_size(HS)) return 0;
    return decode_scratch_bytes(T, NH, HS, HS == 512 ? kMaxSplitsMfma : kMaxSplits, true);
}

// ---- GPT-2 multi-head attention over a KV cache (CudaMhaOp.ixx:137-380: prefill / decode of IPositionalUnaryOp + IKvCacheLifecycle) ----
// The cache is [B, NH, capacity, HS] like the GQA one (NKV = NH); K / V come from the packed [B, T, 3C] projection.
int mila_cdna4_mha_kv_write_bf16(uint16_t* Kc, uint16_t* Vc, const uint16_t* QKV, int B, int T, int C, int NH, int start_pos, int capacity,
                                 mila_stream_t stream)
{
    MILA_REQUIRE(Kc && Vc && QKV, "mha_kv_write_bf16: null pointer");
    MILA_REQUIRE(B > 0 && T > 0 && C > 0 && NH > 0 && C % NH == 0 && capacity > 0, "mha_kv_write_bf16: bad sizes (B=%d T=%d C=%d NH=%d capacity=%d)", B, T, C, NH, capacity);
    MILA_REQUIRE(start_pos >= 0 && start_pos + T <= capacity, "mha_kv_write_bf16: positions [%d, %d) do not fit the cache capacity %d", start_pos, start_pos + T, capacity);
    const int HS = C / NH;
    const bool vec = HS % 8 == 0 && ((uintptr_t)QKV % 16 == 0) && ((uintptr_t)Kc % 16 == 0) && ((uintptr_t)Vc % 16 == 0);
    const int64_t total = vec ? (int64_t)B * T * (C / 8) : (int64_t)B * T * C;
    int blocks = ceil_div(total, 256);
    if (blocks > 4096) blocks = 4096;
    if (vec) hipLaunchKernelGGL(mha_kv_write_vec_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), Kc, Vc, QKV, total, T, C, HS, start_pos, capacity);
    else hipLaunchKernelGGL(mha_kv_write_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), Kc, Vc, QKV, total, T, C, HS, start_pos, capacity);
    MILA_LAUNCH_CHECK("mha_kv_write_bf16");
}

size_t mila_cdna4_mha_decode_scratch_bytes(int B, int C, int NH)
{
    if (B <= 0 || C <= 0 || NH <= 0 || C % NH != 0) return 0;
    return mila_cdna4_attn_decode_scratch_bytes(B, NH, C / NH);
}

int mila_cdna4_mha_decode_bf16(uint16_t* Y, const uint16_t* QKV, uint16_t* Kc, uint16_t* Vc, void* scratch, size_t scratch_bytes, int B, int C,
                               int NH, int capacity, int position, mila_stream_t stream)
{
    MILA_REQUIRE(Y && QKV && Kc && Vc, "mha_decode_bf16: null pointer");
    MILA_REQUIRE(B > 0 && C > 0 && NH > 0 && C % NH == 0 && capacity > 0, "mha_decode_bf16: bad sizes (B=%d C=%d NH=%d capacity=%d)", B, C, NH, capacity);
    MILA_REQUIRE(position >= 0 && position < capacity, "mha_decode_bf16: position %d out of range [0, %d)", position, capacity);     // CudaMhaOp.ixx:262-265
    const int HS = C / NH;
    int rc = mila_cdna4_mha_kv_write_bf16(Kc, Vc, QKV, B, 1, C, NH, position, capacity, stream);
    if (rc) return rc;
    // the query rows of a packed [B, 1, 3C] projection are 3C elements apart; the geometry is the capacity's (len_hint 0)
    return unfused_decode("mha_decode_bf16", Y, QKV, 3 * (int64_t)C, Kc, Vc, scratch, scratch_bytes, B, NH, NH, HS, capacity, position, nullptr, 0, 0, 1.0f / sqrtf((float)HS),
                          as_stream(stream));
}

// the `splits` of the plan fused_attn_decode_partials_bf16 runs for this shape and len_hint (as in plan_decode: position + 1 of an eager call, 0 = the capacity)
int mila_cdna4_attn_decode_split_count(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint)
{
    if (B <= 0 || NH <= 0 || NKV <= 0 || NH % NKV != 0 || capacity <= 0 || window < 0) return 0;
    return plan_decode(B, NH, NKV, HS, capacity, window, len_hint, true, true).splits;
}

int mila_cdna4_fused_attn_decode_partials_bf16(uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw,
                                               const uint16_t* v_raw, const uint16_t* qw, const uint16_t* kw, const uint16_t* vw,
                                               const float* cos_cache, const float* sin_cache, void* scratch, size_t scratch_bytes,
                                               int NH, int NKV, int HS, int capacity, int position, const int32_t* position_dev,
                                               int window, float scale, float eps, mila_stream_t stream)
{
    return fused_decode("fused_attn_decode_partials_bf16", fused_args(nullptr, Kc, Vc, q_raw, k_raw, v_raw, qw, kw, vw, cos_cache, sin_cache, scratch, scratch_bytes, nullptr, 0,
                                                                      NH, NKV, HS, capacity, position, position_dev, window, scale, eps), 1, 0, FD_PARTIALS, as_stream(stream));
}

size_t mila_cdna4_attn_decode_ticket_count(int B, int NH)
{
    if (B <= 0 || NH <= 0) return 0;
    return (size_t)B * NH;     // one counter per (batch row, head-group); head-groups <= NH
}

// fused_attn_decode_bf16 without the combine launch: the workgroup whose split partials arrive last (an arrival ticket per
// head-group in `tickets`: uint32 [ticket_count], zero before the first call, re-armed by every call) merges its head-group's
// splits in the same launch, with the combine kernel's arithmetic => bit-identical to fused_attn_decode_bf16.
int mila_cdna4_fused_attn_decode_onepass_bf16(uint16_t* Y, uint16_t* Kc, uint16_t* Vc, const uint16_t* q_raw, const uint16_t* k_raw,
                                              const uint16_t* v_raw, const uint16_t* qw, const uint16_t* kw, const uint16_t* vw,
                                              const float* cos_cache, const float* sin_cache, void* scratch, size_t scratch_bytes,
                                              uint32_t* tickets, size_t ticket_count, int NH, int NKV, int HS, int capacity, int position,
                                              const int32_t* position_dev, int window, float scale, float eps, mila_stream_t stream)
{
    return fused_decode("fused_attn_decode_onepass_bf16", fused_args(Y, Kc, Vc, q_raw, k_raw, v_raw, qw, kw, vw, cos_cache, sin_cache, scratch, scratch_bytes, tickets, ticket_count,
                                                                     NH, NKV, HS, capacity, position, position_dev, window, scale, eps), 1, 0, FD_TICKETS, as_stream(stream));
}

// fused_attn_decode_bf16 (or, with tickets, fused_attn_decode_onepass_bf16) from an argument block, with optional warm ranges
int mila_cdna4_fused_attn_decode_ex(const mila_fused_attn_args* a, mila_stream_t stream)
{
    MILA_REQUIRE(a != nullptr, "fused_attn_decode_ex: null arguments");
    return fused_decode("fused_attn_decode_ex", *a, 1, 0, 0, as_stream(stream));
}

static size_t describe_plan(const DecodePlan& d, const char* const* names, char* buf, size_t cap)
{
    return 1 + snprintf(buf, buf ? cap : 0, "%s:%d:%d:%d:%d:%d:%d:%zu:%zu", names[d.form], d.splits, d.band_max, d.gh, d.hgroups, d.flat, (int)d.prologue, d.partial_floats,
                        d.scratch_need);
}
size_t mila_cdna4_attn_decode_plan_describe(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint, int fused, int hooks, char* buf, size_t cap)
{
    if (buf && cap) buf[0] = 0;
    if (B <= 0 || NH <= 0 || NKV <= 0 || NH % NKV != 0 || HS <= 0 || capacity <= 0 || window < 0) return 0;
    static const char* const names[] = {"attn_decode", "attn_decode_mfma", "attn_generic"};
    return describe_plan(plan_decode(B, NH, NKV, HS, capacity, window, len_hint, fused != 0, hooks != 0), names, buf, cap);
}
// the plan attn_decode_kvfp8 and its device-position form launch from; the fp8 KV cache has kernels for the four split-kernel head sizes only
size_t mila_cdna4_attn_decode_kvfp8_plan_describe(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint, char* buf, size_t cap)
{
    if (buf && cap) buf[0] = 0;
    if (B <= 0 || NH <= 0 || NKV <= 0 || NH % NKV != 0 || (HS != 64 && HS != 128 && HS != 256 && HS != 512) || capacity <= 0 || window < 0) return 0;
    static const char* const names[] = {"attn_decode_kvfp8", "attn_decode_kvfp8_mfma", ""};
    return describe_plan(plan_decode(B, NH, NKV, HS, capacity, window, len_hint, false, false, true), names, buf, cap);
}

}  // extern "C"
