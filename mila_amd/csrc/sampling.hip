// Greedy device sampler: argmax over fp32 / bf16 logits, ties to the LOWEST index -- the reference's semantics
// (OPS/Sampling/Kernels/Sampling.cu:23-75: strict '>' while scanning in index order, lower index wins the reduction).
// Integer output => bit-exact.  Two stages so that 1 MB of logits is read by the whole chip, not by one CU.
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "common.h"

namespace mila {

constexpr int kArgmaxBlocks = kArgmaxPartials;      // (common.h) 512: the lm_head matvec runs two workgroups per CU

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<uint16_t>(uint16_t v) { return bf16_bits_to_f32(v); }

// (the (value, index) order is argmax_better of common.h)
__device__ __forceinline__ void wave_argmax(float& bv, int& bi)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        argmax_better(bv, bi, ov, oi);
    }
}

// the reduction of a 256-thread workgroup: each wave's butterfly, four LDS slots, and thread 0 folds the other three waves into its pair.  Only thread 0 holds the
// result.  One barrier: every thread of the workgroup calls it.
__device__ __forceinline__ void block_argmax(float& bv, int& bi)
{
    __shared__ float sv[4];
    __shared__ int si[4];
    wave_argmax(bv, bi);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int w = 1; w < 4; ++w) argmax_better(bv, bi, sv[w], si[w]);
    }
}

// the token of a finished reduction that started from (-FLT_MAX, 0x7fffffff).  All -FLT_MAX / NaN: the reference leaves index 0
__device__ __forceinline__ int argmax_token(int bi) { return (bi == 0x7fffffff) ? 0 : bi; }

// ---- sampling filters (TokenSampling.md 3.3: repetition penalty, presence / frequency penalty, min-p).  The per-sequence state is a table of `vocab` 32-bit words:
// bit 31 = the token occurs in the prompt, bits 0..30 = c, the times it has been generated.  The sampler that is given a table reads table[i] beside logits[i] and its
// tail adds 1 to the word of the token it chose.
struct SampleFilter
{
    uint32_t* table;              // row 0's table (nullptr: no penalties, no update)
    size_t table_stride;          // words between the tables of two rows
    float rep, inv_rep;           // repetition penalty and 1.0f / rep (divided once, on the host)
    float pres, freq, min_p;
};

// the adjusted logit x3 of a soft-capped logit x0 whose table word is w: every operation rounded on its own (no contraction into a fused multiply-add), so that a host
// can restate it bit for bit
__device__ __forceinline__ float penalized_logit(float x0, uint32_t w, const SampleFilter& f)
{
    const float x1 = w != 0u ? (x0 > 0.0f ? __fmul_rn(x0, f.inv_rep) : __fmul_rn(x0, f.rep)) : x0;
    const uint32_t c = w & 0x7fffffffu;
    const float x2 = __fsub_rn(x1, __fmul_rn(f.freq, (float)c));
    return c > 0u ? __fsub_rn(x2, f.pres) : x2;
}

// one lane, after choosing token s and before publishing it: a plain load and a plain store (the next step's first launch reads the table across a kernel boundary)
__device__ __forceinline__ void table_count(uint32_t* table, int s) { table[s] = table[s] + 1u; }

template <typename T>
__global__ __launch_bounds__(256) void argmax_partial_kernel(const T* __restrict__ logits, float* __restrict__ pv, int* __restrict__ pi,
                                                             int vocab)
{
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) argmax_better(bv, bi, to_f32(logits[i]), i);
    block_argmax(bv, bi);
    if (threadIdx.x == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// Row b's bias table from the trailing kernel arguments of a BIAS instantiation (bias0, bias_stride).  The arguments are a parameter pack, empty in the instantiations
// without a bias: those keep the parent's kernel signature, and with it the offsets of their hidden arguments -- their instruction streams do not move.
__device__ __forceinline__ const float* bias_row(int) { return nullptr; }
__device__ __forceinline__ const float* bias_row(int b, const float* bias0, size_t bias_stride) { return bias0 + (size_t)b * bias_stride; }

// the greedy sampler's first stage over the ADJUSTED logits x3 (softcap first: the penalty touches only some tokens, so the capped values decide); blockIdx.y = row b:
// logits + b * logits_stride, table + b * table_stride, partials at pv0 + b * row_floats (values, then kArgmaxBlocks floats on the indices)
// TABLE: the penalties from the token table.  BIAS: xb = x0 + bias[i] (row b's bias table at bias0 + b * bias_stride, the two trailing arguments B of the BIAS
// instantiations) between the softcap and the penalties.  A -inf entry never beats the start value -FLT_MAX.
template <bool TABLE, bool BIAS, typename... B>
__global__ __launch_bounds__(256) void argmax_partial_filtered_kernel(const float* __restrict__ logits0, size_t logits_stride, float softcap, const SampleFilter f,
                                                                      float* __restrict__ pv0, int row_floats, int vocab, B... bias_args)
{
    static_assert(TABLE || BIAS, "the unfiltered first stage is argmax_partial_kernel");
    static_assert(sizeof...(B) == (BIAS ? 2 : 0), "bias0 and bias_stride go with BIAS");
    const float* logits = logits0 + (size_t)blockIdx.y * logits_stride;
    const uint32_t* table = f.table + (size_t)blockIdx.y * f.table_stride;
    const float* __restrict__ bias = bias_row(blockIdx.y, bias_args...);
    float* pv = pv0 + (size_t)blockIdx.y * row_floats;
    int* pi = reinterpret_cast<int*>(pv + kArgmaxBlocks);
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256)
    {
        float x = soft_cap(logits[i], softcap);
        if (BIAS) x = __fadd_rn(x, bias[i]);
        if (TABLE) x = penalized_logit(x, table[i], f);
        argmax_better(bv, bi, x, i);
    }
    block_argmax(bv, bi);
    if (threadIdx.x == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// the second stage: one workgroup reduces the n partials.  TABLE: thread 0 counts the token in the table before it stores it (`table` is not read otherwise)
template <bool TABLE>
__global__ __launch_bounds__(256) void argmax_final_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int n, int32_t* __restrict__ token_out, uint32_t* table)
{
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) argmax_better(bv, bi, pv[i], pi[i]);
    block_argmax(bv, bi);
    if (threadIdx.x == 0)
    {
        const int tok = argmax_token(bi);
        if (TABLE) table_count(table, tok);
        token_out[0] = tok;
    }
}

// what one lane does behind the token of a one-row advance step: the position bump of the next step, the sequence number `seq` of this token (seq_dev != NULL) and
// (ring != NULL) the publication of seq << 32 | token to the host
__device__ __forceinline__ void publish_token(int tok, unsigned long long seq, int32_t* pos, unsigned long long* seq_dev, unsigned long long* ring, int ring_size)
{
    *pos += 1;
    if (seq_dev != nullptr) *seq_dev = seq;
    if (ring != nullptr)
        __hip_atomic_store(ring + (seq % (unsigned long long)ring_size), (seq << 32) | (unsigned long long)(uint32_t)tok, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the last node of a captured decode step: the final reduction of the greedy sampler, the position bump of the next step and (ring != NULL; seq_dev goes with it) the
// publication of the sampled token to the host -- what argmax_final + advance_position[_snapshot] did in two launches (round 3: one launch fewer per token).  The
// leading parameters are plain pointers / integers (kernarg preload), the table comes last.
template <bool TABLE>
__global__ __launch_bounds__(256) void argmax_final_advance_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int n, int32_t* __restrict__ token_out,
                                                                   int32_t* __restrict__ pos, unsigned long long* seq_dev, unsigned long long* ring, int ring_size,
                                                                   uint32_t* table)
{
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) argmax_better(bv, bi, pv[i], pi[i]);
    block_argmax(bv, bi);
    if (threadIdx.x == 0)
    {
        const int tok = argmax_token(bi);
        if (TABLE) table_count(table, tok);
        token_out[0] = tok;
        publish_token(tok, seq_dev != nullptr ? *seq_dev + 1ull : 0ull, pos, seq_dev, ring, ring_size);
    }
}

// argmax_final_advance_kernel for B independent rows, one workgroup per row: row b reduces the n partials at pv + b * row_floats (values, then kArgmaxBlocks floats on
// the indices); a row whose active word is 0 keeps its token, its position and (TABLE) its table
template <bool TABLE>
__global__ __launch_bounds__(256) void argmax_rows_final_advance_kernel(const float* __restrict__ pv0, int32_t* __restrict__ token_out, int32_t* __restrict__ pos,
                                                                        const int32_t* __restrict__ active, int n, int row_floats, uint32_t* table0, size_t table_stride)
{
    const int b = blockIdx.x;
    const float* pv = pv0 + (size_t)b * row_floats;
    const int* pi = reinterpret_cast<const int*>(pv + kArgmaxBlocks);
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) argmax_better(bv, bi, pv[i], pi[i]);
    block_argmax(bv, bi);
    if (threadIdx.x == 0 && active[b] != 0)
    {
        const int tok = argmax_token(bi);
        if (TABLE) table_count(table0 + (size_t)b * table_stride, tok);
        token_out[b] = tok;
        pos[b] += 1;
    }
}

// table maintenance: bit 31 of the words of n token ids in device memory.  Every writer stores the SAME value into a cleared table (counts are zero before the first
// sample), so plain vector stores are enough: repeats race on equal bits.  An id outside [0, vocab) is skipped.
__global__ __launch_bounds__(256) void token_table_mark_prompt_kernel(uint32_t* __restrict__ table, int vocab, const int32_t* __restrict__ tokens, int n)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    {
        const int id = tokens[i];
        if (id >= 0 && id < vocab) table[id] = 0x80000000u;
    }
}

// ---- the bias table (mila_cdna4.h: logit bias): `vocab` fp32 values per row, finite or -inf, added to the capped logit by the BIAS instantiations.  Maintenance in
// plain vector stores: a whole row to one value, and n values scattered to n ids held in device memory (an id outside [0, vocab) is skipped; two writers of one id
// race, so duplicates are the caller's to avoid).
__global__ __launch_bounds__(256) void token_bias_fill_kernel(float* __restrict__ bias, int vocab, float value)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) bias[i] = value;
}
__global__ __launch_bounds__(256) void token_bias_set_kernel(float* __restrict__ bias, int vocab, const int32_t* __restrict__ ids, const float* __restrict__ values, int n)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    {
        const int id = ids[i];
        if (id >= 0 && id < vocab) bias[id] = values[i];
    }
}

// ---- the token automaton (mila_cdna4.h: token automaton): the effective table of a row is its base table with -inf wherever the row's state forbids the token,
// eff[i] = next[s * C + class_of[i]] != FORBIDDEN ? base[i] : -inf.  One kernel, two forms.  COMPOSE writes the table of the state the word holds.  STEP first advances
// the state by the token the sampler tail just wrote, s' = next[s * C + class_of[token]] (FORBIDDEN: s stays), then writes the table of s' and leaves s' in the word.
// THE STATE WORD is read by every workgroup of the launch and stored by one of them, and a workgroup that starts late must not read the advanced value.  So lane 0 of
// every workgroup reads the word and the token, and only then takes a ticket with an agent-scope atomic add whose release ordering keeps the two loads (and the two
// dependent loads of s') in front of it: the ticket that completes the row's count, gridDim.x - 1, is drawn after every workgroup of the row has read, and its holder
// stores s' and zeroes the ticket for the next launch, which the kernel boundary orders behind both stores.  Every workgroup computes the same s' from the same words.
// The walk: four tokens per lane where the pointers allow (VEC: one 8-byte load of class_of, one 16-byte load of base, one 16-byte store), a scalar loop for the
// vocab % 4 tail or for everything when a pointer or stride is not aligned; the state's row of `next` (at most 128 KB) is gathered through the cache.
constexpr uint16_t kAutomatonForbidden = 0xFFFFu;

// the state behind token t in state s: next[s * C + class_of[t]], and s itself where that is FORBIDDEN or t lies outside [0, vocab)
__device__ __forceinline__ int automaton_advance(int s, int t, const uint16_t* __restrict__ class_of, const uint16_t* __restrict__ next, int S, int C, int vocab)
{
    int s2 = s;
    if (t >= 0 && t < vocab)
    {
        const unsigned c = class_of[t];
        const uint16_t n = c < (unsigned)C ? next[(size_t)s * C + c] : kAutomatonForbidden;
        if (n != kAutomatonForbidden && n < S) s2 = n;
    }
    return s2;
}

// the walk of row b by the workgroups blockIdx.x of gridDim.x: e[i] = x[i] (0 without a base table) where row `state` of `next` allows token i, else -inf
__device__ __forceinline__ void automaton_walk(float* __restrict__ eff, size_t eff_stride, const float* __restrict__ base, size_t base_stride, int b,
                                               const uint16_t* __restrict__ class_of, const uint16_t* __restrict__ next, int state, int C, int vocab, int vec)
{
    const uint16_t* __restrict__ row = next + (size_t)state * C;
    float* __restrict__ e = eff + (size_t)b * eff_stride;
    const float* __restrict__ x = base ? base + (size_t)b * base_stride : nullptr;
    // (a class outside [0, C) -- never from a validated image -- reads entry 0 and is forbidden: no branch in front of the gathers, so the four of a lane fly together)
    auto entry = [&](unsigned c) { return row[c < (unsigned)C ? c : 0u]; };
    auto keep = [&](unsigned c, uint16_t n) { return c < (unsigned)C && n != kAutomatonForbidden; };
    const int nvec = vec ? (vocab >> 2) : 0;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < nvec; v += gridDim.x * 256)
    {
        const uint2 cw = reinterpret_cast<const uint2*>(class_of)[v];
        float4 o = x ? reinterpret_cast<const float4*>(x)[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const unsigned c0 = cw.x & 0xFFFFu, c1 = cw.x >> 16, c2 = cw.y & 0xFFFFu, c3 = cw.y >> 16;
        const uint16_t n0 = entry(c0), n1 = entry(c1), n2 = entry(c2), n3 = entry(c3);
        o.x = keep(c0, n0) ? o.x : -INFINITY;
        o.y = keep(c1, n1) ? o.y : -INFINITY;
        o.z = keep(c2, n2) ? o.z : -INFINITY;
        o.w = keep(c3, n3) ? o.w : -INFINITY;
        reinterpret_cast<float4*>(e)[v] = o;
    }
    for (int i = nvec * 4 + blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256)
    {
        const unsigned c = class_of[i];
        const float xi = x ? x[i] : 0.0f;
        e[i] = keep(c, entry(c)) ? xi : -INFINITY;
    }
}

template <bool STEP>
__global__ __launch_bounds__(256) void token_automaton_kernel(float* __restrict__ eff, size_t eff_stride, const float* __restrict__ base, size_t base_stride,
                                                              const uint16_t* __restrict__ class_of, const uint16_t* __restrict__ next, int S, int C, int32_t* state_dev,
                                                              const int32_t* __restrict__ token_dev, const int32_t* __restrict__ active_dev, uint32_t* ticket_dev, int vocab,
                                                              int vec)
{
    const int b = blockIdx.y;
    if (STEP && active_dev && active_dev[b] == 0) return;      // (uniform over the row's workgroups: none of them takes a ticket)
    __shared__ int s_state;
    if (threadIdx.x == 0)
    {
        int s = __hip_atomic_load(state_dev + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)s >= (unsigned)S) s = 0;      // (never with a state the host set: keeps every read of `next` inside the image)
        if (STEP)
        {
            const int t = token_dev[b];
            const int s2 = automaton_advance(s, t, class_of, next, S, C, vocab);
            const unsigned ticket = __hip_atomic_fetch_add(ticket_dev + b, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            if (ticket == gridDim.x - 1)
            {
                __hip_atomic_store(state_dev + b, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ticket_dev + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            s = s2;
        }
        s_state = s;
    }
    __syncthreads();
    automaton_walk(eff, eff_stride, base, base_stride, b, class_of, next, s_state, C, vocab, vec);
}

// ---- the automaton in a chain step (mila_cdna4.h: token automaton, chain forms).  Row t of a chain was fed tok[t], so its sample obeys q_t: q_0 the state word,
// q_t = automaton_advance(q_{t-1}, tok[t]).  CHAIN COMPOSE, the first node of the step: blockIdx.y + 1 = t in 1 .. T - 1; lane 0 of every workgroup walks the t
// dependent lookups from the state word itself (the launch stores no word another workgroup reads: no ticket), workgroup 0 of row t stores q_t into chain_states[t]
// (that of row 1 also q_0 into chain_states[0]), and the row's workgroups write eff row t for q_t.  Row 0 holds the table of q_0 from the launch before.
__global__ __launch_bounds__(256) void token_automaton_chain_compose_kernel(float* __restrict__ eff, size_t eff_stride, const float* __restrict__ base, size_t base_stride,
                                                                            const uint16_t* __restrict__ class_of, const uint16_t* __restrict__ next, int S, int C,
                                                                            const int32_t* __restrict__ state_dev, const int32_t* __restrict__ tok,
                                                                            int32_t* __restrict__ chain_states, int vocab, int vec)
{
    const int t = blockIdx.y + 1;
    __shared__ int s_state;
    if (threadIdx.x == 0)
    {
        int s = state_dev[0];
        if ((unsigned)s >= (unsigned)S) s = 0;
        if (blockIdx.x == 0 && t == 1) chain_states[0] = s;
        for (int j = 1; j <= t; ++j) s = automaton_advance(s, tok[j], class_of, next, S, C, vocab);
        if (blockIdx.x == 0) chain_states[t] = s;
        s_state = s;
    }
    __syncthreads();
    automaton_walk(eff, eff_stride, base, base_stride, t, class_of, next, s_state, C, vocab, vec);
}

// CHAIN STEP, behind the accept tail: token_automaton_kernel<true> on row 0 with the state q_{n - 1} = chain_states[n - 1] of the last accepted row (n = result[0], the
// accepted count; outside 1 .. T it reads as 1) and the token tok[0] the accept tail left.  The ticket as in the step kernel: every workgroup reads its words before it
// draws, the holder of the last ticket stores the state word and zeroes the ticket.
__global__ __launch_bounds__(256) void token_automaton_chain_step_kernel(float* __restrict__ eff, const float* __restrict__ base, const uint16_t* __restrict__ class_of,
                                                                         const uint16_t* __restrict__ next, int S, int C, int32_t* state_dev,
                                                                         const int32_t* __restrict__ tok, const int32_t* __restrict__ chain_states,
                                                                         const int32_t* __restrict__ result, int T, uint32_t* ticket_dev, int vocab, int vec)
{
    __shared__ int s_state;
    if (threadIdx.x == 0)
    {
        int n = result[0];
        if (n < 1 || n > T) n = 1;
        int s = chain_states[n - 1];
        if ((unsigned)s >= (unsigned)S) s = 0;
        const int s2 = automaton_advance(s, tok[0], class_of, next, S, C, vocab);
        const unsigned ticket = __hip_atomic_fetch_add(ticket_dev, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == gridDim.x - 1)
        {
            __hip_atomic_store(state_dev, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket_dev, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_state = s2;
    }
    __syncthreads();
    automaton_walk(eff, 0, base, 0, 0, class_of, next, s_state, C, vocab, vec);
}

// The acceptance rule of a chain (speculative verification), by one lane: rows 0 .. T - 1 are consecutive positions of ONE sequence, row t fed with tok[t] (tok[0] the
// last sampled token, tok[1 ..] the drafts), and s[t] is row t's sample.  The longest correct draft prefix is accepted: n_acc = the first t in [0, T - 1) with
// s[t] != tok[t + 1], else T - 1.  result = {n_acc + 1, s[0] .. s[n_acc]} (the other words are left alone), tok[0] = s[n_acc] (the next step's input), *pos += n_acc + 1.
__device__ __forceinline__ void chain_accept(const int* s, int T, int32_t* __restrict__ tok, int32_t* __restrict__ result, int32_t* __restrict__ pos)
{
    int n_acc = T - 1;
    for (int i = T - 2; i >= 0; --i)
        if (s[i] != tok[i + 1]) n_acc = i;
    result[0] = n_acc + 1;
    for (int i = 0; i <= n_acc; ++i) result[1 + i] = s[i];
    tok[0] = s[n_acc];
    *pos += n_acc + 1;
}

// The greedy chain's tail.  One workgroup, wave t reduces row t's n partials to a_t (argmax is exact in any order: the greedy sampler's token); then chain_accept.
__global__ __launch_bounds__(256) void argmax_chain_accept_kernel(const float* __restrict__ pv0, int32_t* __restrict__ tok, int32_t* __restrict__ result, int32_t* __restrict__ pos,
                                                                  int n, int row_floats, int T)
{
    __shared__ int sa[4];
    const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
    if (t < T)
    {
        const float* pv = pv0 + (size_t)t * row_floats;
        const int* pi = reinterpret_cast<const int*>(pv + kArgmaxBlocks);
        float bv = -FLT_MAX;
        int bi = 0x7fffffff;
        for (int i = lane; i < n; i += 64) argmax_better(bv, bi, pv[i], pi[i]);
        wave_argmax(bv, bi);
        if (lane == 0) sa[t] = argmax_token(bi);
    }
    __syncthreads();
    if (threadIdx.x == 0) chain_accept(sa, T, tok, result, pos);
}

__global__ __launch_bounds__(64) void advance_positions_rows_kernel(int32_t* __restrict__ pos, const int32_t* __restrict__ active, int B)
{
    const int b = threadIdx.x;
    if (b < B && active[b] != 0) pos[b] += 1;
}

// The first stage of the two-launch greedy entries, written once: the scratch check, the split of a row's partials into values and indices, the workgroup count and
// the partial launch.  f == nullptr: the logits as they are, one row; else x3 of `rows` rows (softcap first), row b's partials at pv + b * row_floats: the penalties
// where f->table is set, the bias where `bias` is set (at least one of the two).
struct ArgmaxPartials { float* pv; int* pi; int blocks, row_floats; };
constexpr size_t kArgmaxRowBytes = (size_t)kArgmaxBlocks * 8;
template <typename T>
static int launch_argmax_partials(const T* logits, size_t logits_stride, int rows, int vocab, float softcap, const SampleFilter* f, void* scratch, size_t scratch_bytes,
                                  hipStream_t s, const char* who, ArgmaxPartials& a, const float* bias = nullptr, size_t bias_stride = 0)
{
    const size_t need = kArgmaxRowBytes * (size_t)rows;
    if (!scratch || scratch_bytes < need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, need);
    a.pv = reinterpret_cast<float*>(scratch);
    a.pi = reinterpret_cast<int*>(a.pv + kArgmaxBlocks);
    a.blocks = (vocab + 255) / 256;
    if (a.blocks > kArgmaxBlocks) a.blocks = kArgmaxBlocks;
    a.row_floats = (int)(kArgmaxRowBytes / sizeof(float));
    if constexpr (std::is_same<T, float>::value)
    {
        auto biased = [&](auto k) { hipLaunchKernelGGL(k, dim3(a.blocks, (unsigned)rows), dim3(256), 0, s, logits, logits_stride, softcap, *f, a.pv, a.row_floats, vocab, bias, bias_stride); };
        if (f && f->table && bias) biased(argmax_partial_filtered_kernel<true, true, const float*, size_t>);
        else if (f && bias) biased(argmax_partial_filtered_kernel<false, true, const float*, size_t>);
        else if (f) hipLaunchKernelGGL((argmax_partial_filtered_kernel<true, false>), dim3(a.blocks, (unsigned)rows), dim3(256), 0, s, logits, logits_stride, softcap, *f, a.pv, a.row_floats, vocab);
        else hipLaunchKernelGGL(argmax_partial_kernel<T>, dim3(a.blocks), dim3(256), 0, s, logits, a.pv, a.pi, vocab);
    }
    else hipLaunchKernelGGL(argmax_partial_kernel<T>, dim3(a.blocks), dim3(256), 0, s, logits, a.pv, a.pi, vocab);
    return check_hip(hipGetLastError(), who);
}

template <typename T>
static int run_argmax(const T* logits, int32_t* token_out, int vocab, void* scratch, size_t scratch_bytes, hipStream_t s, const char* who)
{
    MILA_REQUIRE(logits && token_out, "%s: null pointer", who);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    ArgmaxPartials a;
    const int rc = launch_argmax_partials(logits, 0, 1, vocab, 0.0f, nullptr, scratch, scratch_bytes, s, who, a);
    if (rc) return rc;
    hipLaunchKernelGGL(argmax_final_kernel<false>, dim3(1), dim3(256), 0, s, a.pv, a.pi, a.blocks, token_out, (uint32_t*)nullptr);
    return check_hip(hipGetLastError(), who);
}

// ================================================================================================
// Stochastic sampler: softcap + temperature, top-k, top-p (nucleus), inverse CDF in token-index order.
// Semantics of the reference's multinomial kernel (OPS/Sampling/Kernels/Sampling.cu:760-905), whose two 40-step value
// bisections converge to:  top-k survivors = values strictly above the (k+1)-th largest scaled logit;  nucleus = the
// smallest set of highest-probability survivors whose mass exceeds top_p * total (a tie enters as a whole);  token = the
// first index with e > 0 and cumulative >= r * total (vocab - 1 otherwise).
//
// CDNA4 design (not the reference's histogram pipeline): both thresholds are found EXACTLY by a 16-ary search over
// the 32-bit order-preserving key of the value -- 8 launches of one kernel, each evaluating 15 candidate thresholds in
// one pass over the (L2-resident, 1 MB) vector with 256 workgroups; counts are integers, masses are summed in a fixed
// order (per-thread sequential, DPP butterfly, ascending workgroup index), so a launch sequence is deterministic.
// Every kernel derives the current search state itself from the previous launch's partial sums: no host round trip.
constexpr int kSampBlocks = 256;
constexpr int kSampCand = 15;          // candidate thresholds per search step (16-ary)
constexpr int kSampSteps = 8;          // 16^8 = 2^32

struct SampParams
{
    float* w;                 // [vocab] scaled logits, then probabilities, then the masked probabilities
    uint32_t* part;           // [2][kSampCand][kSampBlocks] partial counts / masses (bit patterns)
    float* red;               // [kSampBlocks] per-workgroup max / sum partials
    uint32_t* lo_hist;        // [kSampSteps] search state after each step
    float* state;             // [0] max  [1] total  [2] k threshold key (bits)  [3] p threshold key (bits)
    int32_t* token_out;
    int vocab, top_k, nblocks;      // nblocks: workgroups of the scale / search / prob launches (<= kSampBlocks)
    float softcap, temperature, top_p, r;
};

// the order of the keys is the order of the floats with ONE exception: key(-0.0f) = 0x7FFFFFFF < key(+0.0f) = 0x80000000 while -0.0f == +0.0f.  For every other pair of
// non-NaN values x < y <=> key(x) < key(y) and x == y <=> key(x) == key(y).  The samplers compare keys where the stated semantics compare floats, so the scale launches
// never store -0.0f (canonical_zero below): over what they store the two orders are one.
__device__ __forceinline__ uint32_t ordered_key(float x)
{
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// x with -0.0f replaced by +0.0f and every other value (NaN, infinities, denormals) as it is: one IEEE addition, which the compiler may not fold (-0 + +0 = +0)
__device__ __forceinline__ float canonical_zero(float x) { return __fadd_rn(x, 0.0f); }

// the LAST index whose masked probability w[i] is nonzero, -1 when there is none: one wave scans the whole vector (`lane` its lane), every lane returns the index.
// The inverse-CDF walks take it when their running sum never reached r * total.
__device__ __forceinline__ int last_with_mass(const float* w, int vocab, int lane)
{
    int last = -1;
    for (int i = lane; i < vocab; i += 64)
        if (w[i] > 0.0f) last = i;      // ascending: the lane's largest
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
    return last;
}

// fixed-order sum of n <= 256 per-workgroup partials by one wave: lane l adds entries 4l .. 4l+3, then the butterfly
template <bool AS_FLOAT>
__device__ __forceinline__ float wave_sum_partials(const uint32_t* p, int n, int lane)
{
    float f = 0.0f;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        const int b = 4 * lane + i;
        const uint32_t v = b < n ? p[b] : 0u;
        if (AS_FLOAT) f += __uint_as_float(v); else c += v;
    }
    if (AS_FLOAT) return wave_sum(f);
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum_u32(c)));
}

// the search state at the start of step `step`: previous state advanced by the previous step's partials.
// COND: top-k  -> count(key >= t) >= k + 1 ;  top-p -> mass(key >= t) > target
template <bool MASS>
__device__ uint32_t advance_search(const SampParams& p, int step, float target, uint32_t* sh)
{
    if (step == 0) return 0u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lo_prev = p.lo_hist[step - 1];
    const uint32_t* prev = p.part + (size_t)((step - 1) & 1) * kSampCand * kSampBlocks;
    // wave w evaluates candidates w, w + 4, ...; sh[j] = 1 when candidate j + 1 still satisfies the condition
    for (int j = wave; j < kSampCand; j += 4)
    {
        const float v = wave_sum_partials<MASS>(prev + (size_t)j * kSampBlocks, p.nblocks, lane);
        bool ok;
        if (MASS) ok = v > target;
        else ok = __float_as_uint(v) >= (uint32_t)(p.top_k + 1);
        if (lane == 0) sh[j] = ok ? 1u : 0u;
    }
    __syncthreads();
    int jstar = 0;
    for (int j = 0; j < kSampCand; ++j) if (sh[j]) jstar = j + 1;      // monotone: the last satisfied candidate
    __syncthreads();
    const int shift = 28 - 4 * (step - 1);
    return lo_prev + ((uint32_t)jstar << shift);
}

template <typename T>
__global__ __launch_bounds__(256) void samp_scale_kernel(const T* __restrict__ logits, const SampParams p)
{
    __shared__ float sv[4];
    float mx = -FLT_MAX;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.vocab; i += gridDim.x * 256)
    {
        float x = soft_cap(to_f32(logits[i]), p.softcap);
        x = canonical_zero(x / p.temperature);
        p.w[i] = x;
        mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) p.red[blockIdx.x] = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
}

// one search step: evaluate the 15 candidates lo + j * 16^(7 - step) (j = 1..15) over this workgroup's elements
template <bool MASS>
__global__ __launch_bounds__(256) void samp_search_kernel(const SampParams p, int step)
{
    __shared__ uint32_t sh[16];
    __shared__ float sf[4][kSampCand];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float target = 0.0f;
    if (MASS) target = p.top_p * p.state[1];
    const uint32_t lo = advance_search<MASS>(p, step, target, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.lo_hist[step] = lo;
    const int shift = 28 - 4 * step;
    float accf[kSampCand];
    uint32_t accc[kSampCand];
#pragma unroll
    for (int j = 0; j < kSampCand; ++j) { accf[j] = 0.0f; accc[j] = 0u; }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.vocab; i += gridDim.x * 256)
    {
        const float v = p.w[i];
        const uint32_t key = MASS ? __float_as_uint(v) : ordered_key(v);      // probabilities are >= 0: bits are ordered
#pragma unroll
        for (int j = 0; j < kSampCand; ++j)
        {
            const uint32_t t = lo + ((uint32_t)(j + 1) << shift);
            const bool ge = (t > lo) && key >= t;            // t <= lo: the candidate wrapped past 2^32 (nothing is >= it)
            if (MASS) accf[j] += ge ? v : 0.0f; else accc[j] += ge ? 1u : 0u;
        }
    }
#pragma unroll
    for (int j = 0; j < kSampCand; ++j)
    {
        const float r = MASS ? wave_sum(accf[j]) : __uint_as_float(wave_sum_u32(accc[j]));
        if (lane == 0) sf[wave][j] = r;
    }
    __syncthreads();
    if (threadIdx.x < kSampCand)
    {
        const int j = threadIdx.x;
        uint32_t out;
        if (MASS) out = __float_as_uint(((sf[0][j] + sf[1][j]) + sf[2][j]) + sf[3][j]);
        else out = __float_as_uint(sf[0][j]) + __float_as_uint(sf[1][j]) + __float_as_uint(sf[2][j]) + __float_as_uint(sf[3][j]);
        p.part[(size_t)(step & 1) * kSampCand * kSampBlocks + (size_t)j * kSampBlocks + blockIdx.x] = out;
    }
}

// probabilities of the top-k survivors: e = x above the k threshold ? expf(x - max) : 0; per-workgroup sums
__global__ __launch_bounds__(256) void samp_prob_kernel(const SampParams p, int use_k, int nblocks_scale)
{
    __shared__ uint32_t sh[16];
    __shared__ float sv[4];
    const int lane = threadIdx.x & 63;
    // max over the scale kernel's partials (every workgroup computes it the same way)
    float mx = -FLT_MAX;
    for (int b = threadIdx.x; b < nblocks_scale; b += 256) mx = fmaxf(mx, p.red[b]);
    mx = wave_max(mx);
    if (lane == 0) sv[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
    __syncthreads();
    uint32_t kthr = 0u;
    if (use_k) kthr = advance_search<false>(p, kSampSteps, 0.0f, sh);    // key of the (k+1)-th largest value
    float sum = 0.0f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.vocab; i += gridDim.x * 256)
    {
        const float x = p.w[i];
        const float e = (!use_k || ordered_key(x) > kthr) ? expf(x - mx) : 0.0f;
        p.w[i] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) sv[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        // red[] is still being read by late workgroups as the max partials: the sums go to the second half
        p.red[kSampBlocks + blockIdx.x] = ((sv[0] + sv[1]) + sv[2]) + sv[3];
        if (blockIdx.x == 0) { p.state[0] = mx; p.state[2] = __uint_as_float(kthr); }
    }
}

// total = fixed-order sum of the per-workgroup sums (one wave)
__global__ __launch_bounds__(64) void samp_total_kernel(const SampParams p, int nblocks)
{
    const float t = wave_sum_partials<true>(reinterpret_cast<const uint32_t*>(p.red + kSampBlocks), nblocks, threadIdx.x);
    if (threadIdx.x == 0) p.state[1] = t;
}

// nucleus mask + contiguous-chunk sums for the index-order CDF: workgroup b owns tokens [b * chunk, (b + 1) * chunk)
__global__ __launch_bounds__(256) void samp_mask_kernel(const SampParams p, int use_p, int chunk)
{
    __shared__ uint32_t sh[16];
    __shared__ float sv[4];
    uint32_t pthr = 0u;
    if (use_p) pthr = advance_search<true>(p, kSampSteps, p.top_p * p.state[1], sh);     // bits of the nucleus boundary probability
    const int i0 = blockIdx.x * chunk, i1 = min(p.vocab, i0 + chunk);
    float sum = 0.0f;
    for (int i = i0 + threadIdx.x; i < i1; i += 256)
    {
        float e = p.w[i];
        if (use_p && __float_as_uint(e) < pthr) { e = 0.0f; p.w[i] = 0.0f; }
        sum += e;
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        p.red[blockIdx.x] = ((sv[0] + sv[1]) + sv[2]) + sv[3];
        if (blockIdx.x == 0) p.state[3] = __uint_as_float(pthr);
    }
}

// inverse CDF in token-index order: chunk sums locate the chunk, one lane walks it (and, if rounding left the target just
// beyond it, the following ones) with the reference's guard e > 0 && cumulative >= target.  Where the running sum never reaches the target -- the total is the chunk
// sums added in chunk order, the walk adds entry by entry, so next to r = 1 the two can differ in the last bits -- the wave scans for the LAST entry with mass, which
// is where an exact walk ends at r = 1; vocab - 1 only when nothing has mass (what the reference's walk leaves then)
__global__ __launch_bounds__(64) void samp_cdf_kernel(const SampParams p, int nchunks, int chunk)
{
    int result = p.vocab - 1;
    bool found = false;
    if (threadIdx.x == 0)
    {
        float total = 0.0f;
        for (int b = 0; b < nchunks; ++b) total += p.red[b];
        const float target = p.r * total;
        float before = 0.0f;
        int b = 0;
        while (b < nchunks - 1 && before + p.red[b] < target) { before += p.red[b]; ++b; }
        float cum = before;
        for (; b < nchunks && !found; ++b)
        {
            const int i1 = min(p.vocab, (b + 1) * chunk);
            for (int i = b * chunk; i < i1; ++i)
            {
                const float e = p.w[i];
                cum += e;
                if (e > 0.0f && cum >= target) { result = i; found = true; break; }
            }
        }
    }
    if (!__shfl((int)found, 0, 64))
    {
        const int last = last_with_mass(p.w, p.vocab, threadIdx.x);
        if (last >= 0) result = last;
    }
    if (threadIdx.x == 0) p.token_out[0] = result;
}

constexpr size_t kSampHeaderFloats = 64;
static size_t samp_scratch_floats(int vocab)
{
    return kSampHeaderFloats + (size_t)2 * kSampBlocks /* red */ + (size_t)2 * kSampCand * kSampBlocks /* part */ + (size_t)vocab;
}

template <typename T>
static int run_stochastic(const T* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                          void* scratch, size_t scratch_bytes, hipStream_t s, const char* who)
{
    MILA_REQUIRE(logits && token_out, "%s: null pointer", who);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE(temperature > 0.0f, "%s: temperature must be > 0 (temperature <= 0 is the greedy sampler: sample_argmax)", who);
    MILA_REQUIRE(top_k >= 0 && top_p > 0.0f && r >= 0.0f && r <= 1.0f, "%s: need top_k >= 0, top_p > 0, 0 <= r <= 1", who);
    const size_t need = samp_scratch_floats(vocab) * 4;
    if (!scratch || scratch_bytes < need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, need);
    float* f = reinterpret_cast<float*>(scratch);
    SampParams p{};
    p.state = f;
    p.lo_hist = reinterpret_cast<uint32_t*>(f + 16);
    p.red = f + kSampHeaderFloats;
    p.part = reinterpret_cast<uint32_t*>(p.red + 2 * kSampBlocks);
    p.w = reinterpret_cast<float*>(p.part + (size_t)2 * kSampCand * kSampBlocks);
    p.token_out = token_out; p.vocab = vocab; p.top_k = top_k; p.softcap = softcap; p.temperature = temperature; p.top_p = top_p; p.r = r;
    const int use_k = (top_k > 0 && top_k < vocab) ? 1 : 0;
    const int use_p = top_p < 1.0f ? 1 : 0;
    int blocks = (vocab + 255) / 256;
    if (blocks > kSampBlocks) blocks = kSampBlocks;
    p.nblocks = blocks;
    hipLaunchKernelGGL(samp_scale_kernel<T>, dim3(blocks), dim3(256), 0, s, logits, p);
    if (use_k)
        for (int step = 0; step < kSampSteps; ++step) hipLaunchKernelGGL(samp_search_kernel<false>, dim3(blocks), dim3(256), 0, s, p, step);
    hipLaunchKernelGGL(samp_prob_kernel, dim3(blocks), dim3(256), 0, s, p, use_k, blocks);
    hipLaunchKernelGGL(samp_total_kernel, dim3(1), dim3(64), 0, s, p, blocks);
    if (use_p)
        for (int step = 0; step < kSampSteps; ++step) hipLaunchKernelGGL(samp_search_kernel<true>, dim3(blocks), dim3(256), 0, s, p, step);
    const int chunk = (vocab + kSampBlocks - 1) / kSampBlocks;
    const int nchunks = (vocab + chunk - 1) / chunk;
    hipLaunchKernelGGL(samp_mask_kernel, dim3(nchunks), dim3(256), 0, s, p, use_p, chunk);
    hipLaunchKernelGGL(samp_cdf_kernel, dim3(1), dim3(64), 0, s, p, nchunks, chunk);
    return check_hip(hipGetLastError(), who);
}

// ================================================================================================
// The radix pipeline: the same sampler (softcap + temperature, top-k, top-p, inverse CDF in token-index order -- the semantics stated above) in at most 9 launches
// instead of 21, every buffer fixed, so that it can sit in a captured decode step.  Both thresholds are found by DIGIT SELECTION over the 32-bit key (11 + 11 + 10 bits):
// a launch builds the histogram of the next digit over the elements that share the digits found so far -- per workgroup in LDS, flushed with integer atomics into a
// global histogram the first launch cleared -- and the NEXT launch's prologue picks the digit by a suffix scan of that histogram, every workgroup the same way (what
// advance_search does for the 16-ary search).  Every dependency is a kernel boundary.
//   top-k: the histogram counts keys; the threshold is the largest t with count(key >= t) >= k + 1 -- integers, the 16-ary search's threshold exactly.
//   top-p: the histogram sums e = expf(x - max) as unsigned 64-bit fixed point (scale 2^40: e <= 1, 2^18 entries sum below 2^59; the truncation is below 2^-22 of the
//          total, which is >= 2^40 because the maximum contributes e = 1).  Integer sums do not depend on the order of the atomics: run to run the same bits.
// The per-element e, the survivor tests (ordered_key(x) > kthr, bits(e) >= pthr) and the final walk in index order are the first pipeline's.
constexpr int kRadixPasses = 3;
constexpr int kRadixBins = 2048;                    // bins of a pass (the last one uses 1024 of them)
constexpr int kRadixBlocks = 128;                   // workgroups of the pass / prob launches: each flushes its histogram, and adds to one word serialize
constexpr double kRadixFixedScale = 1099511627776.0;      // 2^40
__host__ __device__ constexpr int radix_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ constexpr int radix_bins(int pass) { return pass == 2 ? 1024 : 2048; }

struct RadixState                   // what i digit passes of a search have fixed
{
    unsigned long long above;       // count / fixed-point mass of the keys above the prefix's range
    uint32_t prefix;                // the digits found so far (lower bits zero)
    uint32_t pad;
};
struct RadixHeader                  // 256 bytes, cleared with the histograms by the first launch
{
    unsigned long long total;       // fixed-point sum of e over the top-k survivors
    RadixState k[kRadixPasses + 1], p[kRadixPasses + 1];      // [i]: the state after i passes ([0] stays zero); [3].prefix is the threshold
    unsigned long long pad[32 - 1 - 4 * (kRadixPasses + 1)];
};
static_assert(sizeof(RadixHeader) == 256, "RadixHeader");

struct RadixParams
{
    RadixHeader* hdr;
    uint32_t* khist;                // [kRadixPasses][kRadixBins] key counts
    unsigned long long* phist;      // [kRadixPasses][kRadixBins] fixed-point masses
    float* red;                     // [kSampBlocks] per-workgroup max, then [kSampBlocks] chunk sums of the masked probabilities
    float* w;                       // [vocab] scaled logits, then probabilities, then the masked probabilities
    int32_t* token_out;
    int vocab, top_k;
    float softcap, temperature, top_p, r;
    // the one-row advance tail (radix_cdf_kernel<true, *>)
    const float* draws;
    int draws_size, ring_size;
    int32_t* pos;
    unsigned long long* seq_dev;
    unsigned long long* ring;
};

__device__ __forceinline__ unsigned long long radix_fixed(float e) { return (unsigned long long)((double)e * kRadixFixedScale); }

// the digit of a finished histogram pass: the largest d with above + sum(hist[d ..]) >= need (STRICT: > need); `above_out` = above + sum(hist[d + 1 ..]).
// All 256 threads of the workgroup call it; thread t owns bins [t * per, (t + 1) * per).  No bin satisfies the condition (NaN input): digit 0.
template <typename T, bool STRICT>
__device__ void radix_pick(const T* __restrict__ hist, int bins, unsigned long long above, unsigned long long need, uint32_t& digit, unsigned long long& above_out,
                           unsigned long long* sh /* [8] */)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = bins >> 8;      // 8 or 4
    unsigned long long v[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = j < per ? (unsigned long long)hist[t * per + j] : 0ull; mine += v[j]; }
    unsigned long long inc = mine;      // sum over this wave's lanes >= lane
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
    {
        const unsigned long long o = __shfl_down(inc, off, 64);
        if (lane + off < 64) inc += o;
    }
    if (lane == 0) sh[wave] = inc;
    if (t == 0) { sh[4] = 0ull; sh[5] = 0ull; }
    __syncthreads();
    unsigned long long run = above + inc - mine;      // everything above this thread's bins
    for (int w = wave + 1; w < 4; ++w) run += sh[w];
    auto ok = [&](unsigned long long x) { return STRICT ? x > need : x >= need; };
    if (!ok(run) && ok(run + mine))                   // the sums are monotone: at most one thread
    {
#pragma unroll
        for (int j = 7; j >= 0; --j)
        {
            if (j >= per) continue;
            if (ok(run + v[j])) { sh[4] = (unsigned long long)(t * per + j); sh[5] = run; break; }
            run += v[j];
        }
    }
    __syncthreads();
    digit = (uint32_t)sh[4];
    above_out = sh[5];
    __syncthreads();
}

// A thread's strided walk over the vector, its first kRadixPre elements requested BEFORE the prologue that picks the previous pass's digit (a chain of dependent
// loads, a scan and three barriers): the prologue's latency hides theirs.  At 2^18 entries and kRadixBlocks workgroups that is the whole walk.
constexpr int kRadixPre = 8;
__device__ __forceinline__ void radix_preload(const float* w, int first, int stride, int end, float (&pre)[kRadixPre])
{
#pragma unroll
    for (int j = 0; j < kRadixPre; ++j)
    {
        const int i = first + j * stride;
        pre[j] = i < end ? w[i] : 0.0f;
    }
}
template <typename F>
__device__ __forceinline__ void radix_walk(const float* w, int first, int stride, int end, const float (&pre)[kRadixPre], F&& body)
{
#pragma unroll
    for (int j = 0; j < kRadixPre; ++j)
    {
        const int i = first + j * stride;
        if (i < end) body(i, pre[j]);
    }
    for (int i = first + kRadixPre * stride; i < end; i += stride) body(i, w[i]);
}

// launch 1: x = softcap / temperature, per-workgroup max; clears the header and both histograms for the launches behind it
// FILT: the adjusted logit (penalized_logit on the capped value, then the temperature) with the table word read beside the logit in the same coalesced walk; the
// copy goes to p.w as ever -- the logits are never written (the log-probabilities stay those of the unpenalized logits)
// BIAS: xb = x0 + bias[i], one more value read beside the logit, between the softcap and the penalties.  A -inf bias stays -inf through penalized_logit (a product with
// rep > 0, differences with finite values) and the division by a positive temperature; the maximum is over the finite entries (one exists: the caller's contract).
template <typename T, bool FILT = false, bool BIAS = false>
__device__ __forceinline__ void radix_scale_body(const T* __restrict__ logits, const RadixParams& p, int clear_words, const SampleFilter* f = nullptr,
                                                 const uint32_t* __restrict__ table = nullptr, const float* __restrict__ bias = nullptr)
{
    __shared__ float sv[4];
    uint32_t* z = reinterpret_cast<uint32_t*>(p.hdr);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < clear_words; i += gridDim.x * 256) z[i] = 0u;
    float mx = -FLT_MAX;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.vocab; i += gridDim.x * 256)
    {
        float x = soft_cap(to_f32(logits[i]), p.softcap);
        if (BIAS) x = __fadd_rn(x, bias[i]);
        if (FILT) x = penalized_logit(x, table[i], *f);
        x = canonical_zero(x / p.temperature);
        p.w[i] = x;
        mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) p.red[blockIdx.x] = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
}

// top-k digit pass: pick the previous pass's digit, then count this pass's digit over the keys that share the prefix
__device__ __forceinline__ void radix_kpass_body(const RadixParams& p, int pass)
{
    __shared__ uint32_t lh[kRadixBins];
    __shared__ unsigned long long sh[8];
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    float pre[kRadixPre];
    radix_preload(p.w, first, stride, p.vocab, pre);
    RadixState st{0ull, 0u, 0u};
    if (pass > 0)
    {
        const RadixState prev = p.hdr->k[pass - 1];
        uint32_t digit;
        radix_pick<uint32_t, false>(p.khist + (size_t)(pass - 1) * kRadixBins, radix_bins(pass - 1), prev.above, (unsigned long long)p.top_k + 1ull, digit, st.above, sh);
        st.prefix = prev.prefix | (digit << radix_shift(pass - 1));
        if (blockIdx.x == 0 && threadIdx.x == 0) p.hdr->k[pass] = st;
    }
    const int bins = radix_bins(pass), shift = radix_shift(pass);
    const int hshift = pass > 0 ? radix_shift(pass - 1) : 0;      // the bits above it are the prefix
    for (int b = threadIdx.x; b < bins; b += 256) lh[b] = 0u;
    __syncthreads();
    radix_walk(p.w, first, stride, p.vocab, pre, [&](int, float x)
    {
        const uint32_t key = ordered_key(x);
        if (pass == 0 || (key >> hshift) == (st.prefix >> hshift)) atomicAdd(&lh[(key >> shift) & (uint32_t)(bins - 1)], 1u);
    });
    __syncthreads();
    uint32_t* gh = p.khist + (size_t)pass * kRadixBins;
    for (int b = threadIdx.x; b < bins; b += 256)
        if (lh[b]) atomicAdd(&gh[b], lh[b]);
}

// probabilities of the top-k survivors (samp_prob_kernel's expression), their fixed-point total, and the first digit pass of the nucleus search over bits(e)
__device__ __forceinline__ void radix_prob_body(const RadixParams& p, int use_k, int use_p, int nblocks_scale)
{
    __shared__ unsigned long long lh[kRadixBins];
    __shared__ unsigned long long sh[8];
    __shared__ float sv[4];
    const int lane = threadIdx.x & 63;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    float pre[kRadixPre];
    radix_preload(p.w, first, stride, p.vocab, pre);
    float mx = -FLT_MAX;
    for (int b = threadIdx.x; b < nblocks_scale; b += 256) mx = fmaxf(mx, p.red[b]);
    mx = wave_max(mx);
    if (lane == 0) sv[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
    uint32_t kthr = 0u;
    if (use_k)
    {
        const RadixState prev = p.hdr->k[kRadixPasses - 1];
        RadixState st{0ull, 0u, 0u};
        uint32_t digit;
        radix_pick<uint32_t, false>(p.khist + (size_t)(kRadixPasses - 1) * kRadixBins, radix_bins(kRadixPasses - 1), prev.above, (unsigned long long)p.top_k + 1ull, digit,
                                    st.above, sh);
        kthr = prev.prefix | digit;       // key of the (k+1)-th largest value
        st.prefix = kthr;
        if (blockIdx.x == 0 && threadIdx.x == 0) p.hdr->k[kRadixPasses] = st;
    }
    if (use_p)
        for (int b = threadIdx.x; b < kRadixBins; b += 256) lh[b] = 0ull;
    __syncthreads();
    unsigned long long sum = 0ull;
    radix_walk(p.w, first, stride, p.vocab, pre, [&](int i, float x)
    {
        const float e = (!use_k || ordered_key(x) > kthr) ? expf(x - mx) : 0.0f;
        p.w[i] = e;
        const unsigned long long f = (use_p && e > 0.0f) ? radix_fixed(e) : 0ull;
        sum += f;
        if (f) atomicAdd(&lh[(__float_as_uint(e) >> radix_shift(0)) & (uint32_t)(kRadixBins - 1)], f);
    });
    if (!use_p) return;      // only the nucleus search reads the total and the histogram
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&p.hdr->total, (sh[0] + sh[1]) + (sh[2] + sh[3]));      // one add per workgroup
    for (int b = threadIdx.x; b < kRadixBins; b += 256)
        if (lh[b]) atomicAdd(&p.phist[b], lh[b]);
}

__device__ __forceinline__ unsigned long long radix_mass_target(float top_p, unsigned long long total)
{
    return (unsigned long long)((double)top_p * (double)total);      // the nucleus holds the keys whose mass EXCEEDS it
}

// nucleus digit pass 1 / 2: pick the previous pass's digit, then sum this pass's digit over the probabilities that share the prefix
__device__ __forceinline__ void radix_ppass_body(const RadixParams& p, int pass)
{
    __shared__ unsigned long long lh[kRadixBins];
    __shared__ unsigned long long sh[8];
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    float pre[kRadixPre];
    radix_preload(p.w, first, stride, p.vocab, pre);
    const RadixState prev = p.hdr->p[pass - 1];
    RadixState st{0ull, 0u, 0u};
    uint32_t digit;
    radix_pick<unsigned long long, true>(p.phist + (size_t)(pass - 1) * kRadixBins, radix_bins(pass - 1), prev.above, radix_mass_target(p.top_p, p.hdr->total), digit, st.above, sh);
    st.prefix = prev.prefix | (digit << radix_shift(pass - 1));
    if (blockIdx.x == 0 && threadIdx.x == 0) p.hdr->p[pass] = st;
    const int bins = radix_bins(pass), shift = radix_shift(pass), hshift = radix_shift(pass - 1);
    for (int b = threadIdx.x; b < bins; b += 256) lh[b] = 0ull;
    __syncthreads();
    radix_walk(p.w, first, stride, p.vocab, pre, [&](int, float e)
    {
        const uint32_t key = __float_as_uint(e);       // e >= 0: the bits are ordered
        if (e > 0.0f && (key >> hshift) == (st.prefix >> hshift))
        {
            const unsigned long long f = radix_fixed(e);
            if (f) atomicAdd(&lh[(key >> shift) & (uint32_t)(bins - 1)], f);
        }
    });
    __syncthreads();
    unsigned long long* gh = p.phist + (size_t)pass * kRadixBins;
    for (int b = threadIdx.x; b < bins; b += 256)
        if (lh[b]) atomicAdd(&gh[b], lh[b]);
}

// nucleus mask + contiguous-chunk sums for the index-order CDF (samp_mask_kernel with the radix search's threshold)
// MINP: after the nucleus cut a surviving entry with e = expf(x - max) < min_p is dropped (the largest entry has e = 1: the tokens whose probability is at least
// min_p times the top token's stay)
template <bool MINP = false>
__device__ __forceinline__ void radix_mask_body(const RadixParams& p, int use_p, int chunk, float min_p = 0.0f)
{
    __shared__ unsigned long long sh[8];
    __shared__ float sv[4];
    const int i0 = blockIdx.x * chunk, i1 = min(p.vocab, i0 + chunk);
    float pre[kRadixPre];
    radix_preload(p.w, i0 + threadIdx.x, 256, i1, pre);
    uint32_t pthr = 0u;
    if (use_p)
    {
        const RadixState prev = p.hdr->p[kRadixPasses - 1];
        RadixState st{0ull, 0u, 0u};
        uint32_t digit;
        radix_pick<unsigned long long, true>(p.phist + (size_t)(kRadixPasses - 1) * kRadixBins, radix_bins(kRadixPasses - 1), prev.above,
                                             radix_mass_target(p.top_p, p.hdr->total), digit, st.above, sh);
        pthr = prev.prefix | digit;       // bits of the nucleus boundary probability
        st.prefix = pthr;
        if (blockIdx.x == 0 && threadIdx.x == 0) p.hdr->p[kRadixPasses] = st;
    }
    float sum = 0.0f;
    radix_walk(p.w, i0 + threadIdx.x, 256, i1, pre, [&](int i, float e)
    {
        if (use_p && __float_as_uint(e) < pthr) { e = 0.0f; p.w[i] = 0.0f; }
        if (MINP && e > 0.0f && e < min_p) { e = 0.0f; p.w[i] = 0.0f; }
        sum += e;
    });
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) p.red[kSampBlocks + blockIdx.x] = ((sv[0] + sv[1]) + sv[2]) + sv[3];
}

__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// inverse CDF in token-index order: samp_cdf_kernel's sums and walk, value for value (the same additions in the same order), by one wave that holds the chunk sums in
// registers and steps over the zeros of the walk: adding 0 leaves the cumulative sum as it is, and after the truncations nearly every entry is 0.
// radix_cdf_walk is the walk itself, by ONE wave (`lane` its lane) at the draw r; every lane returns the token.
// When the running sum never reaches r * total -- the two are added in different orders, so next to r = 1 they can differ -- the token is the LAST entry with nonzero
// mass, found by a scan of the whole vector (taken only then): where an exact walk ends at r = 1, and never a token that top-k / top-p / min-p or a -inf bias removed.
// vocab - 1 only when nothing has mass.
__device__ __forceinline__ int radix_cdf_walk(const RadixParams& p, float r, int nchunks, int chunk, int lane)
{
    const float* cs = p.red + kSampBlocks;
    float c[4];      // chunk sums: lane l holds chunks l, 64 + l, 128 + l, 192 + l
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = (q * 64 + lane) < nchunks ? cs[q * 64 + lane] : 0.0f;
    float total = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 64; ++l)
            if (q * 64 + l < nchunks) total += lane_value(c[q], l);
    const float target = r * total;
    float before = 0.0f;
    int b = 0;
    bool located = false;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 64; ++l)
        {
            if (located || q * 64 + l >= nchunks - 1) continue;
            const float v = lane_value(c[q], l);
            if (before + v < target) { before += v; b = q * 64 + l + 1; }
            else located = true;
        }
    int result = p.vocab - 1;
    float cum = before;
    bool found = false;
    // kCdfBatch x 64 entries are requested together (a chunk of a 2^18-entry vocabulary in one round trip), then walked in index order
    constexpr int kCdfBatch = 16;
    for (int base = b * chunk; base < p.vocab && !found; base += kCdfBatch * 64)
    {
        float e[kCdfBatch];
#pragma unroll
        for (int q = 0; q < kCdfBatch; ++q) e[q] = (base + q * 64 + lane) < p.vocab ? p.w[base + q * 64 + lane] : 0.0f;
#pragma unroll
        for (int q = 0; q < kCdfBatch; ++q)
        {
            unsigned long long m = found ? 0ull : __ballot(e[q] > 0.0f);
            while (m)
            {
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                m &= m - 1ull;
                cum += lane_value(e[q], l);
                if (cum >= target) { result = base + q * 64 + l; found = true; break; }
            }
        }
    }
    if (!found)
    {
        const int last = last_with_mass(p.w, p.vocab, lane);
        if (last >= 0) result = last;
    }
    return result;
}

// The rows of a call: the stage kernels take a row dimension in the grid.  blockIdx.y = b picks row b's logits (logits + b * logits_stride), row b's table
// (f.table + b * f.table_stride) and row b's scratch region (header, histograms, red, w at scratch + b * row_stride bytes); blockIdx.x / gridDim.x are what a one-row
// launch has, so every walk, every chunk and every float sum of row b is the one-row call's on that row: row b's token is sample_radix_fp32's on row b's logits with row
// b's draw, whatever the other rows hold.  A one-row call is rows = 1, gridDim.y = 1 (row_stride is never multiplied by anything but 0).
struct RadixRows
{
    RadixParams p;                  // row 0's pointers; in a rows call p.draws = one draw per row, p.pos = the position word(s) of the tail
    size_t row_stride;              // bytes between the scratch regions of two rows (a multiple of 8)
    size_t logits_stride;           // floats between the logits of two rows
    SampleFilter f;                 // read by the FILT / TABLE instantiations only (min_p is an argument of the mask launch)
};
__device__ __forceinline__ RadixParams radix_row(const RadixRows& r, int b)
{
    RadixParams p = r.p;
    const size_t off = (size_t)b * r.row_stride;
    p.hdr = reinterpret_cast<RadixHeader*>(reinterpret_cast<char*>(r.p.hdr) + off);
    p.khist = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(r.p.khist) + off);
    p.phist = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(r.p.phist) + off);
    p.red = reinterpret_cast<float*>(reinterpret_cast<char*>(r.p.red) + off);
    p.w = reinterpret_cast<float*>(reinterpret_cast<char*>(r.p.w) + off);
    return p;
}

// the stage launches (`logits` leads: it is preloaded)
// (BIAS: bias0 and bias_stride trail the arguments -- the pack B, empty otherwise: row b's bias table is bias0 + b * bias_stride)
template <typename T, bool FILT, bool BIAS, typename... B>
__global__ __launch_bounds__(256) void radix_scale_kernel(const T* __restrict__ logits, const RadixRows r, int clear_words, B... bias_args)
{
    static_assert(sizeof...(B) == (BIAS ? 2 : 0), "bias0 and bias_stride go with BIAS");
    const RadixParams p = radix_row(r, blockIdx.y);
    radix_scale_body<T, FILT, BIAS>(logits + (size_t)blockIdx.y * r.logits_stride, p, clear_words, &r.f, FILT ? r.f.table + (size_t)blockIdx.y * r.f.table_stride : nullptr,
                                    bias_row(blockIdx.y, bias_args...));
}
__global__ __launch_bounds__(256) void radix_kpass_kernel(const RadixRows r, int pass)
{
    const RadixParams p = radix_row(r, blockIdx.y);
    radix_kpass_body(p, pass);
}
__global__ __launch_bounds__(256) void radix_prob_kernel(const RadixRows r, int use_k, int use_p, int nblocks_scale)
{
    const RadixParams p = radix_row(r, blockIdx.y);
    radix_prob_body(p, use_k, use_p, nblocks_scale);
}
__global__ __launch_bounds__(256) void radix_ppass_kernel(const RadixRows r, int pass)
{
    const RadixParams p = radix_row(r, blockIdx.y);
    radix_ppass_body(p, pass);
}
template <bool MINP>
__global__ __launch_bounds__(256) void radix_mask_kernel(const RadixRows r, int use_p, int chunk, float min_p)
{
    const RadixParams p = radix_row(r, blockIdx.y);
    radix_mask_body<MINP>(p, use_p, chunk, min_p);
}

// The one-row tail, one wave over row 0.  ADVANCE: the stochastic twin of argmax_final_advance_kernel -- the draw is slot (*seq_dev + 1) % draws_size of a host-written
// ring (system-scope load: the host rewrites the slots between replays), and the tail bumps the position, stores the sequence number and (ring != NULL) publishes
// seq << 32 | token; else the draw is p.r.  TABLE: lane 0 counts the sample in the table before it stores / publishes the token.
template <bool ADVANCE, bool TABLE>
__global__ __launch_bounds__(64) void radix_cdf_kernel(const RadixRows rr, int nchunks, int chunk)
{
    const RadixParams& p = rr.p;
    const int lane = threadIdx.x;
    float r = p.r;
    unsigned long long seq = 0ull;
    if (ADVANCE)
    {
        seq = *p.seq_dev + 1ull;
        const uint32_t* slot = reinterpret_cast<const uint32_t*>(p.draws) + (seq % (unsigned long long)p.draws_size);
        r = __uint_as_float(__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
    }
    const int result = radix_cdf_walk(p, r, nchunks, chunk, lane);
    if (lane == 0)
    {
        if (TABLE) table_count(rr.f.table, result);
        p.token_out[0] = result;
        if (ADVANCE) publish_token(result, seq, p.pos, p.seq_dev, p.ring, p.ring_size);
    }
}

// The rows tail, one workgroup: wave t walks row t's CDF (radix_cdf_walk: radix_cdf_kernel's additions in its order) at the draw draws[t] -- a system-scope load, the
// host rewrites the draws between replays -- and the samples s_t meet in LDS; then one lane does the bookkeeping in plain stores.
//   kRowsTokens:  token_out[b] = s_b, nothing advanced.
//   kRowsAdvance: where active[b] != 0, token_out[b] = s_b and pos[b] += 1; an inactive row's words are not touched.
//   kRowsChain:   chain_accept with the samples (token_out is tok[], pos the ONE position word).
// TABLE (kRowsTokens / kRowsAdvance): the lane counts row b's sample in row b's table before it stores the token -- in kRowsAdvance for the active rows only.  The chain
// tail takes no table: row t would need the table plus the drafts 1 .. t.
enum { kRowsTokens = 0, kRowsAdvance = 1, kRowsChain = 2 };
template <int MODE, bool TABLE>
__global__ __launch_bounds__(256) void radix_rows_tail_kernel(const RadixRows r, int rows, int nchunks, int chunk, const int32_t* __restrict__ active, int32_t* __restrict__ result)
{
    static_assert(!TABLE || MODE == kRowsTokens || MODE == kRowsAdvance, "the chain tail takes no table");
    __shared__ int ss[4];
    const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
    if (t < rows)
    {
        const RadixParams p = radix_row(r, t);
        const float draw = __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t*>(r.p.draws) + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
        const int s = radix_cdf_walk(p, draw, nchunks, chunk, lane);
        if (lane == 0) ss[t] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int32_t* tok = r.p.token_out;
    int32_t* pos = r.p.pos;
    if (MODE == kRowsChain) chain_accept(ss, rows, tok, result, pos);
    else
        for (int b = 0; b < rows; ++b)
        {
            if (MODE == kRowsAdvance && active[b] == 0) continue;
            if (TABLE) table_count(r.f.table + (size_t)b * r.f.table_stride, ss[b]);
            tok[b] = ss[b];
            if (MODE == kRowsAdvance) pos[b] += 1;
        }
}

// the one place that decides what a radix call launches: the entries below and sample_radix_plan_describe read it
struct RadixPlan
{
    int launches;            // kernel nodes of one call: scale + k_passes + prob + (p_passes - 1: the first nucleus pass rides in prob) + mask + cdf
    int k_passes, p_passes;  // digit passes of the two searches (0 = that truncation is off)
    int scale_blocks;        // workgroups of the scale launch (a plain stream: as many as the partial-maximum array holds)
    int blocks;              // workgroups of the pass / prob launches
    int chunk, nchunks;      // the mask launch's contiguous chunks
    size_t scratch_need;
    int scale_filtered;      // the scale launch is the instantiation that reads the token table (a table was given)
    int mask_filtered;       // the mask launch is the instantiation with the min-p test (min_p > 0)
    int scale_biased;        // the scale launch is the instantiation that reads a bias table
};
constexpr size_t kRadixHistBytes = (size_t)kRadixPasses * kRadixBins * (sizeof(uint32_t) + sizeof(unsigned long long));
// with_table / min_p / with_bias choose INSTANTIATIONS of launches the plan already has: a filtered or biased call launches what the unfiltered call launches
static RadixPlan plan_radix(int vocab, int top_k, float top_p, bool with_table = false, float min_p = 0.0f, bool with_bias = false)
{
    RadixPlan d{};
    d.scale_biased = with_bias ? 1 : 0;
    d.scale_filtered = with_table ? 1 : 0;
    d.mask_filtered = min_p > 0.0f ? 1 : 0;
    d.k_passes = (top_k > 0 && top_k < vocab) ? kRadixPasses : 0;
    d.p_passes = top_p < 1.0f ? kRadixPasses : 0;
    d.launches = 1 + d.k_passes + 1 + (d.p_passes ? d.p_passes - 1 : 0) + 2;
    d.blocks = d.scale_blocks = (vocab + 255) / 256;
    if (d.blocks > kRadixBlocks) d.blocks = kRadixBlocks;
    if (d.scale_blocks > kSampBlocks) d.scale_blocks = kSampBlocks;
    d.chunk = (vocab + kSampBlocks - 1) / kSampBlocks;
    d.nchunks = (vocab + d.chunk - 1) / d.chunk;
    d.scratch_need = sizeof(RadixHeader) + kRadixHistBytes + (size_t)2 * kSampBlocks * 4 + (size_t)vocab * 4;
    return d;
}

// the filters of a call as the kernels take them.  flt == nullptr: neutral.  table == nullptr: no penalties and no update (min_p still holds).
static int make_filter(const mila_sample_filters* flt, uint32_t* table, size_t table_stride, int rows, int vocab, SampleFilter& f, const char* who)
{
    const mila_sample_filters n = flt ? *flt : mila_sample_filters{0.0f, 1.0f, 0.0f, 0.0f};
    MILA_REQUIRE(std::isfinite(n.min_p) && std::isfinite(n.repetition_penalty) && std::isfinite(n.presence_penalty) && std::isfinite(n.frequency_penalty),
                 "%s: a sampling filter is not finite", who);
    MILA_REQUIRE(n.repetition_penalty > 0.0f, "%s: repetition_penalty must be > 0", who);
    MILA_REQUIRE(n.min_p >= 0.0f && n.min_p < 1.0f, "%s: min_p outside [0, 1)", who);
    MILA_REQUIRE(!table || rows == 1 || table_stride >= (size_t)vocab, "%s: table_stride %zu < vocab %d", who, table_stride, vocab);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3u) == 0, "%s: table must be 4-byte aligned", who);
    f.table = table; f.table_stride = table_stride;
    f.rep = n.repetition_penalty; f.inv_rep = 1.0f / n.repetition_penalty;
    f.pres = n.presence_penalty; f.freq = n.frequency_penalty; f.min_p = n.min_p;
    return MILA_OK;
}

struct RadixAdvance { const float* draws; int draws_size; int32_t* pos; unsigned long long* seq_dev; unsigned long long* ring; int ring_size; };

// row stride of the rows scratch: the one-row need, rounded up so that every row's RadixHeader (and its 64-bit histogram) stays 8-byte aligned
static size_t radix_row_stride(int vocab) { return (plan_radix(vocab, 0, 1.0f).scratch_need + 7) & ~(size_t)7; }

// What an entry asks of the pipeline.  kOneRow is the one-row call (radix_cdf_kernel behind the stages): the draw is `r`, or with `adv` the draw ring at the sequence
// number, and the scratch need is plan_radix's for one row, not rounded up to the row stride.  The kRows* modes end in radix_rows_tail_kernel<mode> with one draw per
// row in `draws`: kRowsTokens leaves pos / active / result unused; kRowsAdvance takes pos[rows], active[rows]; kRowsChain takes token_out = tok[rows], pos = the one
// position word, result.
constexpr int kOneRow = -1;
template <typename T>
struct RadixCall
{
    int mode;
    const T* logits;
    size_t logits_stride;
    int32_t* token_out;
    int rows, vocab;
    float softcap, temperature;
    int top_k;
    float top_p, r;
    const RadixAdvance* adv;
    const float* draws;
    int32_t* pos;
    const int32_t* active;
    int32_t* result;
    const SampleFilter* flt;
    const float* bias;              // row 0's bias table (nullptr: none)
    size_t bias_stride;             // floats between the bias tables of two rows; 0 = one table for every row
};

// the bias table of a call: any stride with one row; with more, 0 (shared) or at least vocab
static int check_bias(const float* bias, size_t bias_stride, int rows, int vocab, const char* who)
{
    MILA_REQUIRE(!bias || rows <= 1 || bias_stride == 0 || bias_stride >= (size_t)vocab, "%s: bias_stride %zu is neither 0 nor >= vocab %d", who, bias_stride, vocab);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(bias) & 3u) == 0, "%s: bias must be 4-byte aligned", who);
    return MILA_OK;
}

// The radix pipeline of every entry: plan_radix's launches for one row, each with the rows in grid.y, and the mode's tail.
template <typename T>
static int run_radix(const RadixCall<T>& c, void* scratch, size_t scratch_bytes, hipStream_t s, const char* who)
{
    const bool one = c.mode == kOneRow;
    const RadixAdvance* adv = c.adv;
    const SampleFilter* flt = c.flt;
    MILA_REQUIRE(c.logits && c.token_out && (one || c.draws), "%s: null pointer", who);
    MILA_REQUIRE(!adv || (adv->draws && adv->pos && adv->seq_dev), "%s: null pointer", who);
    MILA_REQUIRE(one || c.mode == kRowsTokens || c.pos, "%s: null pointer", who);
    MILA_REQUIRE(c.mode != kRowsAdvance || c.active, "%s: null pointer", who);
    MILA_REQUIRE(c.mode != kRowsChain || c.result, "%s: null pointer", who);
    if (c.mode == kRowsChain) MILA_REQUIRE(c.rows >= 2 && c.rows <= 4, "%s: T=%d rows outside 2 .. 4", who, c.rows);
    else MILA_REQUIRE(c.rows >= 1 && c.rows <= 4, "%s: rows=%d outside 1 .. 4", who, c.rows);
    MILA_REQUIRE(c.vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE(one || c.logits_stride >= (size_t)c.vocab, "%s: logits_stride %zu < vocab %d", who, c.logits_stride, c.vocab);
    MILA_REQUIRE(c.temperature > 0.0f, "%s: temperature must be > 0 (temperature <= 0 is the greedy sampler: sample_argmax)", who);
    if (one) MILA_REQUIRE(c.top_k >= 0 && c.top_p > 0.0f && c.r >= 0.0f && c.r <= 1.0f, "%s: need top_k >= 0, top_p > 0, 0 <= r <= 1", who);
    else MILA_REQUIRE(c.top_k >= 0 && c.top_p > 0.0f, "%s: need top_k >= 0, top_p > 0", who);
    MILA_REQUIRE(!adv || adv->draws_size > 0, "%s: draws_size must be positive", who);
    MILA_REQUIRE(!adv || (adv->ring ? adv->ring_size > 0 : adv->ring_size == 0), "%s: ring and ring_size go together", who);
    MILA_REQUIRE(c.mode != kRowsChain || !flt, "%s: the chain tail takes no filters", who);
    if (const int rc = check_bias(c.bias, c.bias_stride, c.rows, c.vocab, who)) return rc;
    const RadixPlan d = plan_radix(c.vocab, c.top_k, c.top_p, flt && flt->table, flt ? flt->min_p : 0.0f, c.bias != nullptr);
    const size_t row_stride = radix_row_stride(c.vocab), need = one ? d.scratch_need : row_stride * (size_t)c.rows;
    if (!scratch || scratch_bytes < need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, need);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "%s: scratch must be 8-byte aligned", who);
    RadixRows r{};
    RadixParams& p = r.p;
    char* base = reinterpret_cast<char*>(scratch);
    p.hdr = reinterpret_cast<RadixHeader*>(base);
    p.khist = reinterpret_cast<uint32_t*>(base + sizeof(RadixHeader));
    p.phist = reinterpret_cast<unsigned long long*>(p.khist + (size_t)kRadixPasses * kRadixBins);
    p.red = reinterpret_cast<float*>(base + sizeof(RadixHeader) + kRadixHistBytes);
    p.w = p.red + 2 * kSampBlocks;
    p.token_out = c.token_out; p.vocab = c.vocab; p.top_k = c.top_k;
    p.softcap = c.softcap; p.temperature = c.temperature; p.top_p = c.top_p; p.r = c.r;
    p.draws = c.draws; p.pos = c.pos;
    if (adv) { p.draws = adv->draws; p.draws_size = adv->draws_size; p.pos = adv->pos; p.seq_dev = adv->seq_dev; p.ring = adv->ring; p.ring_size = adv->ring_size; }
    r.row_stride = row_stride; r.logits_stride = c.logits_stride;
    if (flt) r.f = *flt;
    const int clear_words = (int)((sizeof(RadixHeader) + kRadixHistBytes) / 4);
    const int use_k = d.k_passes ? 1 : 0, use_p = d.p_passes ? 1 : 0;
    const unsigned R = (unsigned)c.rows;
    const dim3 wg(256);
    if constexpr (std::is_same<T, float>::value)
    {
        auto biased = [&](auto k) { hipLaunchKernelGGL(k, dim3(d.scale_blocks, R), wg, 0, s, c.logits, r, clear_words, c.bias, c.bias_stride); };
        if (d.scale_filtered && d.scale_biased) biased(radix_scale_kernel<float, true, true, const float*, size_t>);
        else if (d.scale_biased) biased(radix_scale_kernel<float, false, true, const float*, size_t>);
        else if (d.scale_filtered) hipLaunchKernelGGL((radix_scale_kernel<float, true, false>), dim3(d.scale_blocks, R), wg, 0, s, c.logits, r, clear_words);
        else hipLaunchKernelGGL((radix_scale_kernel<float, false, false>), dim3(d.scale_blocks, R), wg, 0, s, c.logits, r, clear_words);
    }
    else
    {
        MILA_REQUIRE(!c.bias, "%s: the bias table goes with fp32 logits", who);
        hipLaunchKernelGGL((radix_scale_kernel<T, false, false>), dim3(d.scale_blocks, R), wg, 0, s, c.logits, r, clear_words);
    }
    for (int pass = 0; pass < d.k_passes; ++pass) hipLaunchKernelGGL(radix_kpass_kernel, dim3(d.blocks, R), wg, 0, s, r, pass);
    hipLaunchKernelGGL(radix_prob_kernel, dim3(d.blocks, R), wg, 0, s, r, use_k, use_p, d.scale_blocks);
    for (int pass = 1; pass < d.p_passes; ++pass) hipLaunchKernelGGL(radix_ppass_kernel, dim3(d.blocks, R), wg, 0, s, r, pass);
    if (d.mask_filtered) hipLaunchKernelGGL(radix_mask_kernel<true>, dim3(d.nchunks, R), wg, 0, s, r, use_p, d.chunk, flt->min_p);
    else hipLaunchKernelGGL(radix_mask_kernel<false>, dim3(d.nchunks, R), wg, 0, s, r, use_p, d.chunk, 0.0f);
    // the tail: <mode, table> picks the instantiation
    const bool tab = d.scale_filtered != 0;
    auto cdf = [&](auto k) { hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, s, r, d.nchunks, d.chunk); };
    auto tail = [&](auto k) { hipLaunchKernelGGL(k, dim3(1), wg, 0, s, r, c.rows, d.nchunks, d.chunk, c.active, c.result); };
    if (one && adv) { if (tab) cdf(radix_cdf_kernel<true, true>); else cdf(radix_cdf_kernel<true, false>); }
    else if (one) { if (tab) cdf(radix_cdf_kernel<false, true>); else cdf(radix_cdf_kernel<false, false>); }
    else if (c.mode == kRowsTokens) { if (tab) tail(radix_rows_tail_kernel<kRowsTokens, true>); else tail(radix_rows_tail_kernel<kRowsTokens, false>); }
    else if (c.mode == kRowsAdvance) { if (tab) tail(radix_rows_tail_kernel<kRowsAdvance, true>); else tail(radix_rows_tail_kernel<kRowsAdvance, false>); }
    else tail(radix_rows_tail_kernel<kRowsChain, false>);
    return check_hip(hipGetLastError(), who);
}

// the one-row entries: the draw `r`, or with `adv` the draw ring
template <typename T>
static int call_radix_one(const T* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r, const RadixAdvance* adv,
                         void* scratch, size_t scratch_bytes, hipStream_t s, const char* who, const SampleFilter* flt = nullptr, const float* bias = nullptr,
                         size_t bias_stride = 0)
{
    const RadixCall<T> c{kOneRow, logits, 0, token_out, 1, vocab, softcap, temperature, top_k, top_p, r, adv, nullptr, nullptr, nullptr, nullptr, flt, bias, bias_stride};
    return run_radix(c, scratch, scratch_bytes, s, who);
}
// the rows entries: one draw per row in `draws`
static int call_radix_rows(int mode, const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature, int top_k, float top_p,
                          const float* draws, void* scratch, size_t scratch_bytes, int32_t* pos, const int32_t* active, int32_t* result, hipStream_t s, const char* who,
                          const SampleFilter* flt = nullptr, const float* bias = nullptr, size_t bias_stride = 0)
{
    const RadixCall<float> c{mode, logits, logits_stride, token_out, rows, vocab, softcap, temperature, top_k, top_p, 0.0f, nullptr, draws, pos, active, result, flt, bias,
                             bias_stride};
    return run_radix(c, scratch, scratch_bytes, s, who);
}

// The penalized greedy sampler over `rows` rows: argmax(x3), ties to the lower id, in the two launches of sample_argmax_*: the partial stage computes x3 from logits,
// table and softcap, the final stage counts the token in the table.  adv: the one-row advance tail; pos + active: the rows advance tail; neither: token only.
// With a bias table the first stage adds it; f.table may then be null (a bias without penalties: the final stage is the one that counts nothing).
static int run_argmax_filtered(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, const SampleFilter& f, void* scratch,
                               size_t scratch_bytes, const RadixAdvance* adv, int32_t* positions, const int32_t* active, hipStream_t s, const char* who,
                               const float* bias = nullptr, size_t bias_stride = 0)
{
    if (const int rc = check_bias(bias, bias_stride, rows, vocab, who)) return rc;
    ArgmaxPartials a;
    const int rc = launch_argmax_partials(logits, logits_stride, rows, vocab, softcap, &f, scratch, scratch_bytes, s, who, a, bias, bias_stride);
    if (rc) return rc;
    const bool tab = f.table != nullptr;
    if (positions)
    {
        auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(rows), dim3(256), 0, s, a.pv, token_out, positions, active, a.blocks, a.row_floats, f.table, f.table_stride); };
        if (tab) go(argmax_rows_final_advance_kernel<true>); else go(argmax_rows_final_advance_kernel<false>);
    }
    else if (adv)
    {
        auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, s, a.pv, a.pi, a.blocks, token_out, adv->pos, adv->seq_dev, adv->ring, adv->ring_size, f.table); };
        if (tab) go(argmax_final_advance_kernel<true>); else go(argmax_final_advance_kernel<false>);
    }
    else
    {
        auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, s, a.pv, a.pi, a.blocks, token_out, f.table); };
        if (tab) go(argmax_final_kernel<true>); else go(argmax_final_kernel<false>);
    }
    return check_hip(hipGetLastError(), who);
}

// ================================================================================================
// Row requests (mila_cdna4.h: row requests): every row of a rows call samples under its OWN parameters, read from a record in device memory, so that a new set of
// requests changes words, not launch arguments -- a captured rows step is not captured again.  The stage kernels are the rows kernels above with the row's record in
// the place of the launch arguments: each builds row b's RadixParams / SampleFilter from the record and runs the SAME stage body (radix_scale_body, radix_kpass_body,
// radix_prob_body, radix_ppass_body, radix_mask_body, radix_cdf_walk), so per row every launch extent, chunk, walk order and float summation is the one-row entry's.
// A call launches the full plan (scale, 3 k-passes, prob, 2 p-passes, mask, tail); a row whose truncation is off returns from that search's launches at once, a greedy
// or inactive row from every stage.  Every branch on the record is uniform over the row's workgroups.
struct RowParams                    // = mila_sample_row_params
{
    float temperature;              // <= 0: the row is greedy
    int32_t top_k;
    float top_p, min_p, rep, inv_rep, pres, freq;
};
static_assert(sizeof(RowParams) == sizeof(mila_sample_row_params) && sizeof(RowParams) == 32, "RowParams");

__device__ __forceinline__ bool row_stochastic(const RowParams& q) { return q.temperature > 0.0f; }
__device__ __forceinline__ bool row_penalized(const RowParams& q) { return q.rep != 1.0f || q.pres != 0.0f || q.freq != 0.0f; }
__device__ __forceinline__ bool row_use_k(const RowParams& q, int vocab) { return q.top_k > 0 && q.top_k < vocab; }
__device__ __forceinline__ bool row_use_p(const RowParams& q) { return q.top_p < 1.0f; }
__device__ __forceinline__ bool row_active(const int32_t* active, int b) { return active == nullptr || active[b] != 0; }

// what the request kernels share beside RadixRows (r.f holds table and table_stride only; r.p no temperature, top_k, top_p)
struct RowRequests
{
    const RowParams* params;        // [rows] on the device
    const int32_t* active;          // [rows] or nullptr (every row)
    const float* bias;              // row 0's bias table or nullptr; row b's at bias + b * bias_stride
    size_t bias_stride;
};

// row b's stage parameters; false: the row takes no part in the radix stages
__device__ __forceinline__ bool request_row(const RadixRows& r, const RowRequests& q, int b, RadixParams& p, RowParams& rp)
{
    rp = q.params[b];
    if (!row_stochastic(rp) || !row_active(q.active, b)) return false;
    p = radix_row(r, b);
    p.temperature = rp.temperature; p.top_k = rp.top_k; p.top_p = rp.top_p;
    return true;
}
__device__ __forceinline__ SampleFilter request_filter(const RadixRows& r, const RowParams& rp)
{
    return SampleFilter{r.f.table, r.f.table_stride, rp.rep, rp.inv_rep, rp.pres, rp.freq, rp.min_p};
}

__global__ __launch_bounds__(256) void radix_requests_scale_kernel(const float* __restrict__ logits0, const RadixRows r, const RowRequests q, int clear_words)
{
    const int b = blockIdx.y;
    RadixParams p;
    RowParams rp;
    if (!request_row(r, q, b, p, rp)) return;
    const SampleFilter f = request_filter(r, rp);
    const float* logits = logits0 + (size_t)b * r.logits_stride;
    const uint32_t* table = (f.table && row_penalized(rp)) ? f.table + (size_t)b * f.table_stride : nullptr;
    const float* bias = q.bias ? q.bias + (size_t)b * q.bias_stride : nullptr;
    if (table && bias) radix_scale_body<float, true, true>(logits, p, clear_words, &f, table, bias);
    else if (bias) radix_scale_body<float, false, true>(logits, p, clear_words, &f, nullptr, bias);
    else if (table) radix_scale_body<float, true, false>(logits, p, clear_words, &f, table, nullptr);
    else radix_scale_body<float, false, false>(logits, p, clear_words);
}
__global__ __launch_bounds__(256) void radix_requests_kpass_kernel(const RadixRows r, const RowRequests q, int pass)
{
    RadixParams p;
    RowParams rp;
    if (!request_row(r, q, blockIdx.y, p, rp) || !row_use_k(rp, p.vocab)) return;
    radix_kpass_body(p, pass);
}
__global__ __launch_bounds__(256) void radix_requests_prob_kernel(const RadixRows r, const RowRequests q, int nblocks_scale)
{
    RadixParams p;
    RowParams rp;
    if (!request_row(r, q, blockIdx.y, p, rp)) return;
    radix_prob_body(p, row_use_k(rp, p.vocab) ? 1 : 0, row_use_p(rp) ? 1 : 0, nblocks_scale);
}
__global__ __launch_bounds__(256) void radix_requests_ppass_kernel(const RadixRows r, const RowRequests q, int pass)
{
    RadixParams p;
    RowParams rp;
    if (!request_row(r, q, blockIdx.y, p, rp) || !row_use_p(rp)) return;
    radix_ppass_body(p, pass);
}
// (the min-p test with min_p = 0 drops nothing: e > 0 && e < 0 never holds -- one instantiation serves every row)
__global__ __launch_bounds__(256) void radix_requests_mask_kernel(const RadixRows r, const RowRequests q, int chunk)
{
    RadixParams p;
    RowParams rp;
    if (!request_row(r, q, blockIdx.y, p, rp)) return;
    radix_mask_body<true>(p, row_use_p(rp) ? 1 : 0, chunk, rp.min_p);
}

// The requests tail: radix_rows_tail_kernel's shape (wave t walks row t's CDF at draws[t], then one lane's plain stores) over the rows that are active and stochastic.
// The lane counts the sample in row b's table only where row b has penalties.  ADVANCE: pos[b] += 1 behind the token.
template <bool ADVANCE>
__global__ __launch_bounds__(256) void radix_requests_tail_kernel(const RadixRows r, const RowRequests q, int rows, int nchunks, int chunk)
{
    __shared__ int ss[4];
    __shared__ int take[4];
    const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
    if (t < rows)
    {
        RadixParams p;
        RowParams rp;
        const bool mine = request_row(r, q, t, p, rp);
        int s = 0;
        if (mine)
        {
            const float draw = __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t*>(r.p.draws) + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
            s = radix_cdf_walk(p, draw, nchunks, chunk, lane);
        }
        if (lane == 0) { ss[t] = s; take[t] = mine ? (r.f.table && row_penalized(rp) ? 2 : 1) : 0; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int b = 0; b < rows; ++b)
    {
        if (take[b] == 0) continue;
        if (take[b] == 2) table_count(r.f.table + (size_t)b * r.f.table_stride, ss[b]);
        r.p.token_out[b] = ss[b];
        if (ADVANCE) r.p.pos[b] += 1;
    }
}

// The greedy rows of the same step.  First stage: argmax_partial_filtered_kernel with the row's record -- x3 over the capped logit, the row's bias and (where the row
// has penalties) the row's table; a row with neither bias nor penalties takes the logits AS THEY ARE, as sample_argmax_fp32 does (the cap is monotone but can merge
// neighbours into a tie).  A greedy row's logit is never divided by a temperature.  A stochastic or inactive row returns at once and leaves its partials alone.
template <bool TABLE, bool BIAS>
__device__ __forceinline__ void argmax_request_walk(const float* __restrict__ logits, const uint32_t* __restrict__ table, const float* __restrict__ bias, float softcap,
                                                    const SampleFilter& f, int vocab, float& bv, int& bi)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256)
    {
        float x = logits[i];
        if (TABLE || BIAS) x = soft_cap(x, softcap);
        if (BIAS) x = __fadd_rn(x, bias[i]);
        if (TABLE) x = penalized_logit(x, table[i], f);
        argmax_better(bv, bi, x, i);
    }
}
__global__ __launch_bounds__(256) void argmax_requests_partial_kernel(const float* __restrict__ logits0, size_t logits_stride, float softcap, const RowRequests q,
                                                                      const uint32_t* table0, size_t table_stride, float* __restrict__ pv0, int row_floats, int vocab)
{
    const int b = blockIdx.y;
    const RowParams rp = q.params[b];
    if (row_stochastic(rp) || !row_active(q.active, b)) return;
    const float* logits = logits0 + (size_t)b * logits_stride;
    const uint32_t* table = (table0 && row_penalized(rp)) ? table0 + (size_t)b * table_stride : nullptr;
    const float* bias = q.bias ? q.bias + (size_t)b * q.bias_stride : nullptr;
    const SampleFilter f{nullptr, 0, rp.rep, rp.inv_rep, rp.pres, rp.freq, rp.min_p};
    float* pv = pv0 + (size_t)b * row_floats;
    int* pi = reinterpret_cast<int*>(pv + kArgmaxBlocks);
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    if (table && bias) argmax_request_walk<true, true>(logits, table, bias, softcap, f, vocab, bv, bi);
    else if (bias) argmax_request_walk<false, true>(logits, table, bias, softcap, f, vocab, bv, bi);
    else if (table) argmax_request_walk<true, false>(logits, table, bias, softcap, f, vocab, bv, bi);
    else argmax_request_walk<false, false>(logits, table, bias, softcap, f, vocab, bv, bi);
    block_argmax(bv, bi);
    if (threadIdx.x == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// second stage: argmax_rows_final_advance_kernel over the rows that are active and greedy, the count in the row's table only where the row has penalties
template <bool ADVANCE>
__global__ __launch_bounds__(256) void argmax_requests_final_kernel(const float* __restrict__ pv0, int32_t* __restrict__ token_out, int32_t* __restrict__ pos,
                                                                    const RowRequests q, int n, int row_floats, uint32_t* table0, size_t table_stride)
{
    const int b = blockIdx.x;
    const RowParams rp = q.params[b];
    if (row_stochastic(rp) || !row_active(q.active, b)) return;
    const float* pv = pv0 + (size_t)b * row_floats;
    const int* pi = reinterpret_cast<const int*>(pv + kArgmaxBlocks);
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256) argmax_better(bv, bi, pv[i], pi[i]);
    block_argmax(bv, bi);
    if (threadIdx.x == 0)
    {
        const int tok = argmax_token(bi);
        if (table0 && row_penalized(rp)) table_count(table0 + (size_t)b * table_stride, tok);
        token_out[b] = tok;
        if (ADVANCE) pos[b] += 1;
    }
}

// the record of one row, stored by one lane in plain vector stores (stream order: behind the steps that read the old record, in front of those that read the new)
__global__ __launch_bounds__(64) void sample_row_params_set_kernel(RowParams* __restrict__ dst, const RowParams v)
{
    if (threadIdx.x == 0) *dst = v;
}

// what the requests entries check before any launch
static int check_requests(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, const void* params_dev, uint32_t* table, size_t table_stride,
                          const float* bias, size_t bias_stride, bool advance, int32_t* positions_dev, const int32_t* active_dev, const char* who)
{
    MILA_REQUIRE(logits && token_out && params_dev, "%s: null pointer", who);
    MILA_REQUIRE(!advance || (positions_dev && active_dev), "%s: null pointer", who);
    MILA_REQUIRE(rows >= 1 && rows <= 4, "%s: rows=%d outside 1 .. 4", who, rows);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE(logits_stride >= (size_t)vocab, "%s: logits_stride %zu < vocab %d", who, logits_stride, vocab);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(params_dev) & 3u) == 0, "%s: params_dev must be 4-byte aligned", who);
    MILA_REQUIRE(!table || rows == 1 || table_stride >= (size_t)vocab, "%s: table_stride %zu < vocab %d", who, table_stride, vocab);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3u) == 0, "%s: table must be 4-byte aligned", who);
    return check_bias(bias, bias_stride, rows, vocab, who);
}

static int run_radix_requests(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, const void* params_dev, const float* draws,
                              uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, bool advance,
                              int32_t* positions_dev, const int32_t* active_dev, hipStream_t s, const char* who)
{
    if (const int rc = check_requests(logits, logits_stride, token_out, rows, vocab, params_dev, table, table_stride, bias, bias_stride, advance, positions_dev, active_dev, who))
        return rc;
    MILA_REQUIRE(draws, "%s: null pointer", who);
    const RadixPlan d = plan_radix(vocab, 1, 0.5f);      // the extents of a row; every pass is launched, the rows decide on the device which they run
    const size_t row_stride = radix_row_stride(vocab), need = row_stride * (size_t)rows;
    if (!scratch || scratch_bytes < need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, need);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "%s: scratch must be 8-byte aligned", who);
    RadixRows r{};
    RadixParams& p = r.p;
    char* base = reinterpret_cast<char*>(scratch);
    p.hdr = reinterpret_cast<RadixHeader*>(base);
    p.khist = reinterpret_cast<uint32_t*>(base + sizeof(RadixHeader));
    p.phist = reinterpret_cast<unsigned long long*>(p.khist + (size_t)kRadixPasses * kRadixBins);
    p.red = reinterpret_cast<float*>(base + sizeof(RadixHeader) + kRadixHistBytes);
    p.w = p.red + 2 * kSampBlocks;
    p.token_out = token_out; p.vocab = vocab; p.softcap = softcap;
    p.draws = draws; p.pos = positions_dev;
    r.row_stride = row_stride; r.logits_stride = logits_stride;
    r.f.table = table; r.f.table_stride = table_stride;
    const RowRequests q{reinterpret_cast<const RowParams*>(params_dev), advance ? active_dev : nullptr, bias, bias_stride};
    const int clear_words = (int)((sizeof(RadixHeader) + kRadixHistBytes) / 4);
    const unsigned R = (unsigned)rows;
    const dim3 wg(256);
    hipLaunchKernelGGL(radix_requests_scale_kernel, dim3(d.scale_blocks, R), wg, 0, s, logits, r, q, clear_words);
    for (int pass = 0; pass < kRadixPasses; ++pass) hipLaunchKernelGGL(radix_requests_kpass_kernel, dim3(d.blocks, R), wg, 0, s, r, q, pass);
    hipLaunchKernelGGL(radix_requests_prob_kernel, dim3(d.blocks, R), wg, 0, s, r, q, d.scale_blocks);
    for (int pass = 1; pass < kRadixPasses; ++pass) hipLaunchKernelGGL(radix_requests_ppass_kernel, dim3(d.blocks, R), wg, 0, s, r, q, pass);
    hipLaunchKernelGGL(radix_requests_mask_kernel, dim3(d.nchunks, R), wg, 0, s, r, q, d.chunk);
    if (advance) hipLaunchKernelGGL(radix_requests_tail_kernel<true>, dim3(1), wg, 0, s, r, q, rows, d.nchunks, d.chunk);
    else hipLaunchKernelGGL(radix_requests_tail_kernel<false>, dim3(1), wg, 0, s, r, q, rows, d.nchunks, d.chunk);
    return check_hip(hipGetLastError(), who);
}

static int run_argmax_requests(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, const void* params_dev, uint32_t* table,
                               size_t table_stride, const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, bool advance, int32_t* positions_dev,
                               const int32_t* active_dev, hipStream_t s, const char* who)
{
    if (const int rc = check_requests(logits, logits_stride, token_out, rows, vocab, params_dev, table, table_stride, bias, bias_stride, advance, positions_dev, active_dev, who))
        return rc;
    const size_t need = kArgmaxRowBytes * (size_t)rows;
    if (!scratch || scratch_bytes < need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, need);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 3u) == 0, "%s: scratch must be 4-byte aligned", who);
    float* pv = reinterpret_cast<float*>(scratch);
    int blocks = (vocab + 255) / 256;
    if (blocks > kArgmaxBlocks) blocks = kArgmaxBlocks;
    const int row_floats = (int)(kArgmaxRowBytes / sizeof(float));
    const RowRequests q{reinterpret_cast<const RowParams*>(params_dev), advance ? active_dev : nullptr, bias, bias_stride};
    hipLaunchKernelGGL(argmax_requests_partial_kernel, dim3(blocks, (unsigned)rows), dim3(256), 0, s, logits, logits_stride, softcap, q, table, table_stride, pv, row_floats, vocab);
    if (advance) hipLaunchKernelGGL(argmax_requests_final_kernel<true>, dim3(rows), dim3(256), 0, s, pv, token_out, positions_dev, q, blocks, row_floats, table, table_stride);
    else hipLaunchKernelGGL(argmax_requests_final_kernel<false>, dim3(rows), dim3(256), 0, s, pv, token_out, positions_dev, q, blocks, row_floats, table, table_stride);
    return check_hip(hipGetLastError(), who);
}

// ---- the automaton per row (mila_cdna4.h: row requests): token_automaton_kernel with the image of row b taken from a descriptor in device memory.  A null descriptor
// (class_of == nullptr): the row has no automaton -- its workgroups return before they read a word, write nothing and take no ticket.  The state word, the ticket and the
// ordering argument are token_automaton_kernel's: lane 0 of every workgroup reads state and token before it draws, the holder of the row's last ticket stores.
struct AutomatonRow                 // = mila_token_automaton_row
{
    const uint16_t* class_of;
    const uint16_t* next;
    int32_t S, C;
};
static_assert(sizeof(AutomatonRow) == sizeof(mila_token_automaton_row) && sizeof(AutomatonRow) == 24, "AutomatonRow");

template <bool STEP>
__global__ __launch_bounds__(256) void token_automaton_rows_kernel(float* __restrict__ eff, size_t eff_stride, const float* __restrict__ base, size_t base_stride,
                                                                   const AutomatonRow* __restrict__ desc, int32_t* state_dev, const int32_t* __restrict__ token_dev,
                                                                   const int32_t* __restrict__ active_dev, uint32_t* ticket_dev, int vocab, int vec)
{
    const int b = blockIdx.y;
    const AutomatonRow a = desc[b];
    if (a.class_of == nullptr) return;
    if (STEP && active_dev && active_dev[b] == 0) return;      // (both uniform over the row's workgroups: none of them takes a ticket)
    const uint16_t* __restrict__ class_of = a.class_of;
    const uint16_t* __restrict__ next = a.next;
    const int S = a.S, C = a.C;
    __shared__ int s_state;
    if (threadIdx.x == 0)
    {
        int s = __hip_atomic_load(state_dev + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)s >= (unsigned)S) s = 0;
        if (STEP)
        {
            const int t = token_dev[b];
            const int s2 = automaton_advance(s, t, class_of, next, S, C, vocab);
            const unsigned ticket = __hip_atomic_fetch_add(ticket_dev + b, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            if (ticket == gridDim.x - 1)
            {
                __hip_atomic_store(state_dev + b, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ticket_dev + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            s = s2;
        }
        s_state = s;
    }
    __syncthreads();
    automaton_walk(eff, eff_stride, base, base_stride, b, class_of, next, s_state, C, vocab, vec && (reinterpret_cast<uintptr_t>(class_of) & 7u) == 0);
}

__global__ __launch_bounds__(64) void token_automaton_row_set_kernel(AutomatonRow* __restrict__ dst, const AutomatonRow v)
{
    if (threadIdx.x == 0) *dst = v;
}

}  // namespace mila

using namespace mila;

extern "C" {

size_t mila_cdna4_sample_scratch_bytes(void) { return (size_t)kArgmaxBlocks * 8; }

int mila_cdna4_sample_argmax_fp32(const float* logits, int32_t* token_out, int vocab, void* scratch, size_t scratch_bytes,
                                  mila_stream_t stream)
{
    return run_argmax<float>(logits, token_out, vocab, scratch, scratch_bytes, as_stream(stream), "sample_argmax_fp32");
}

int mila_cdna4_sample_argmax_advance_fp32(const float* logits, int32_t* token_out, int vocab, void* scratch, size_t scratch_bytes, int32_t* position_dev,
                                          unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream)
{
    MILA_REQUIRE(logits && token_out && position_dev, "sample_argmax_advance_fp32: null pointer");
    MILA_REQUIRE(vocab > 0, "sample_argmax_advance_fp32: vocab must be positive");
    MILA_REQUIRE((ring == nullptr) == (seq_dev == nullptr) && (ring == nullptr || ring_size > 0), "sample_argmax_advance_fp32: ring, seq_dev and ring_size go together");
    ArgmaxPartials a;
    const int rc = launch_argmax_partials(logits, 0, 1, vocab, 0.0f, nullptr, scratch, scratch_bytes, as_stream(stream), "sample_argmax_advance_fp32", a);
    if (rc) return rc;
    hipLaunchKernelGGL(argmax_final_advance_kernel<false>, dim3(1), dim3(256), 0, as_stream(stream), a.pv, a.pi, a.blocks, token_out, position_dev, seq_dev, ring, ring_size,
                       (uint32_t*)nullptr);
    MILA_LAUNCH_CHECK("sample_argmax_advance_fp32");
}

// only the final stage, over `blocks` partials a lm_head launch left in `scratch` (fused_norm_matvec with argmax_scratch): the captured greedy step's tail in ONE launch
int mila_cdna4_sample_argmax_final_advance(int32_t* token_out, const void* scratch, size_t scratch_bytes, int blocks, int32_t* position_dev,
                                           unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream)
{
    MILA_REQUIRE(token_out && scratch && position_dev, "sample_argmax_final_advance: null pointer");
    MILA_REQUIRE(blocks > 0 && blocks <= kArgmaxBlocks, "sample_argmax_final_advance: blocks %d out of range (1 .. %d)", blocks, kArgmaxBlocks);
    MILA_REQUIRE((ring == nullptr) == (seq_dev == nullptr) && (ring == nullptr || ring_size > 0), "sample_argmax_final_advance: seq_dev, ring and ring_size go together");
    if (scratch_bytes < (size_t)kArgmaxBlocks * 8) return set_error(MILA_E_SCRATCH_TOO_SMALL, "sample_argmax_final_advance: scratch %zu bytes < required %zu", scratch_bytes, (size_t)kArgmaxBlocks * 8);
    const float* pv = reinterpret_cast<const float*>(scratch);
    const int* pi = reinterpret_cast<const int*>(pv + kArgmaxBlocks);
    hipLaunchKernelGGL(argmax_final_advance_kernel<false>, dim3(1), dim3(256), 0, as_stream(stream), pv, pi, blocks, token_out, position_dev, seq_dev, ring, ring_size,
                       (uint32_t*)nullptr);
    MILA_LAUNCH_CHECK("sample_argmax_final_advance");
}

// the rows twin: row b's partials at scratch + b * sample_scratch_bytes() (a matvec_rows lm_head launch with argmax_scratch), tokens and positions of the active rows only
int mila_cdna4_sample_argmax_rows_final_advance(int32_t* token_out, const void* scratch, size_t scratch_bytes, int blocks, int32_t* positions_dev,
                                                const int32_t* active_dev, int B, mila_stream_t stream)
{
    MILA_REQUIRE(token_out && scratch && positions_dev && active_dev, "sample_argmax_rows_final_advance: null pointer");
    MILA_REQUIRE(B >= 1 && B <= 64, "sample_argmax_rows_final_advance: B=%d out of range (1 .. 64)", B);
    MILA_REQUIRE(blocks > 0 && blocks <= kArgmaxBlocks, "sample_argmax_rows_final_advance: blocks %d out of range (1 .. %d)", blocks, kArgmaxBlocks);
    const size_t per_row = (size_t)kArgmaxBlocks * 8;
    if (scratch_bytes < per_row * B) return set_error(MILA_E_SCRATCH_TOO_SMALL, "sample_argmax_rows_final_advance: scratch %zu bytes < required %zu", scratch_bytes, per_row * B);
    hipLaunchKernelGGL(argmax_rows_final_advance_kernel<false>, dim3(B), dim3(256), 0, as_stream(stream), reinterpret_cast<const float*>(scratch), token_out, positions_dev,
                       active_dev, blocks, (int)(per_row / sizeof(float)), (uint32_t*)nullptr, (size_t)0);
    MILA_LAUNCH_CHECK("sample_argmax_rows_final_advance");
}

// the chain twin: rows are consecutive positions of one sequence; see mila_cdna4.h for the acceptance rule
int mila_cdna4_sample_argmax_chain_accept(int32_t* tok, int32_t* result, const void* scratch, size_t scratch_bytes, int blocks, int32_t* position_dev, int T,
                                          mila_stream_t stream)
{
    MILA_REQUIRE(tok && result && scratch && position_dev, "sample_argmax_chain_accept: null pointer");
    MILA_REQUIRE(T >= 2 && T <= 4, "sample_argmax_chain_accept: T=%d rows outside 2 .. 4", T);
    MILA_REQUIRE(blocks > 0 && blocks <= kArgmaxBlocks, "sample_argmax_chain_accept: blocks %d out of range (1 .. %d)", blocks, kArgmaxBlocks);
    const size_t per_row = (size_t)kArgmaxBlocks * 8;
    if (scratch_bytes < per_row * T) return set_error(MILA_E_SCRATCH_TOO_SMALL, "sample_argmax_chain_accept: scratch %zu bytes < required %zu", scratch_bytes, per_row * T);
    hipLaunchKernelGGL(argmax_chain_accept_kernel, dim3(1), dim3(256), 0, as_stream(stream), reinterpret_cast<const float*>(scratch), tok, result, position_dev, blocks,
                       (int)(per_row / sizeof(float)), T);
    MILA_LAUNCH_CHECK("sample_argmax_chain_accept");
}

int mila_cdna4_advance_positions_rows(int32_t* positions_dev, const int32_t* active_dev, int B, mila_stream_t stream)
{
    MILA_REQUIRE(positions_dev && active_dev, "advance_positions_rows: null pointer");
    MILA_REQUIRE(B >= 1 && B <= 64, "advance_positions_rows: B=%d out of range (1 .. 64)", B);
    hipLaunchKernelGGL(advance_positions_rows_kernel, dim3(1), dim3(64), 0, as_stream(stream), positions_dev, active_dev, B);
    MILA_LAUNCH_CHECK("advance_positions_rows");
}

int mila_cdna4_sample_argmax_bf16(const uint16_t* logits, int32_t* token_out, int vocab, void* scratch, size_t scratch_bytes,
                                  mila_stream_t stream)
{
    return run_argmax<uint16_t>(logits, token_out, vocab, scratch, scratch_bytes, as_stream(stream), "sample_argmax_bf16");
}

size_t mila_cdna4_sample_stochastic_scratch_bytes(int vocab) { return vocab > 0 ? samp_scratch_floats(vocab) * 4 : 0; }

int mila_cdna4_sample_stochastic_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k,
                                      float top_p, float r, void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    return run_stochastic<float>(logits, token_out, vocab, softcap, temperature, top_k, top_p, r, scratch, scratch_bytes, as_stream(stream),
                                 "sample_stochastic_fp32");
}

int mila_cdna4_sample_stochastic_bf16(const uint16_t* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k,
                                      float top_p, float r, void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    return run_stochastic<uint16_t>(logits, token_out, vocab, softcap, temperature, top_k, top_p, r, scratch, scratch_bytes,
                                    as_stream(stream), "sample_stochastic_bf16");
}

size_t mila_cdna4_sample_radix_scratch_bytes(int vocab) { return vocab > 0 ? plan_radix(vocab, 0, 1.0f).scratch_need : 0; }

int mila_cdna4_sample_radix_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                 void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    return call_radix_one<float>(logits, token_out, vocab, softcap, temperature, top_k, top_p, r, nullptr, scratch, scratch_bytes, as_stream(stream), "sample_radix_fp32");
}

int mila_cdna4_sample_radix_bf16(const uint16_t* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                 void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    return call_radix_one<uint16_t>(logits, token_out, vocab, softcap, temperature, top_k, top_p, r, nullptr, scratch, scratch_bytes, as_stream(stream), "sample_radix_bf16");
}

int mila_cdna4_sample_radix_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p,
                                         const float* draws, int draws_size, void* scratch, size_t scratch_bytes, int32_t* position_dev,
                                         unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream)
{
    const RadixAdvance adv{draws, draws_size, position_dev, seq_dev, ring, ring_size};
    return call_radix_one<float>(logits, token_out, vocab, softcap, temperature, top_k, top_p, 0.0f, &adv, scratch, scratch_bytes, as_stream(stream),
                            "sample_radix_advance_fp32");
}

size_t mila_cdna4_sample_radix_rows_scratch_bytes(int rows, int vocab) { return (rows >= 1 && rows <= 4 && vocab > 0) ? radix_row_stride(vocab) * (size_t)rows : 0; }

int mila_cdna4_sample_radix_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature, int top_k,
                                      float top_p, const float* draws, void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    return call_radix_rows(kRowsTokens, logits, logits_stride, token_out, rows, vocab, softcap, temperature, top_k, top_p, draws, scratch, scratch_bytes, nullptr, nullptr, nullptr,
                          as_stream(stream), "sample_radix_rows_fp32");
}

int mila_cdna4_sample_radix_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature, int top_k,
                                              float top_p, const float* draws, void* scratch, size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev,
                                              mila_stream_t stream)
{
    return call_radix_rows(kRowsAdvance, logits, logits_stride, token_out, rows, vocab, softcap, temperature, top_k, top_p, draws, scratch, scratch_bytes, positions_dev, active_dev,
                          nullptr, as_stream(stream), "sample_radix_rows_advance_fp32");
}

int mila_cdna4_sample_radix_chain_accept_fp32(int32_t* tok, int32_t* result, const float* logits, size_t logits_stride, int T, int vocab, float softcap, float temperature,
                                              int top_k, float top_p, const float* draws, void* scratch, size_t scratch_bytes, int32_t* position_dev, mila_stream_t stream)
{
    return call_radix_rows(kRowsChain, logits, logits_stride, tok, T, vocab, softcap, temperature, top_k, top_p, draws, scratch, scratch_bytes, position_dev, nullptr, result,
                          as_stream(stream), "sample_radix_chain_accept_fp32");
}

// ---- the filtered entries (mila_cdna4.h: sampling filters)
size_t mila_cdna4_token_table_bytes(int vocab) { return vocab > 0 ? (size_t)vocab * sizeof(uint32_t) : 0; }

int mila_cdna4_token_table_clear(uint32_t* table, size_t table_stride, int row, int vocab, mila_stream_t stream)
{
    MILA_REQUIRE(table, "token_table_clear: null pointer");
    MILA_REQUIRE(vocab > 0 && row >= 0 && (row == 0 || table_stride >= (size_t)vocab), "token_table_clear: need vocab > 0, row >= 0, table_stride >= vocab");
    return check_hip(hipMemsetAsync(table + (size_t)row * table_stride, 0, (size_t)vocab * sizeof(uint32_t), as_stream(stream)), "token_table_clear");
}

int mila_cdna4_token_table_mark_prompt(uint32_t* table, size_t table_stride, int row, int vocab, const int32_t* tokens_dev, int n, mila_stream_t stream)
{
    MILA_REQUIRE(table && (tokens_dev || n == 0), "token_table_mark_prompt: null pointer");
    MILA_REQUIRE(vocab > 0 && row >= 0 && n >= 0 && (row == 0 || table_stride >= (size_t)vocab), "token_table_mark_prompt: need vocab > 0, row >= 0, n >= 0, table_stride >= vocab");
    if (n == 0) return MILA_OK;
    int blocks = (n + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(token_table_mark_prompt_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), table + (size_t)row * table_stride, vocab, tokens_dev, n);
    MILA_LAUNCH_CHECK("token_table_mark_prompt");
}

// ---- the bias table and the biased entries (mila_cdna4.h: logit bias).  Each biased entry is the filtered entry plus `bias, bias_stride`; bias == NULL is the filtered
// entry itself, which is now a call of its biased sibling.
size_t mila_cdna4_token_bias_bytes(int vocab) { return vocab > 0 ? (size_t)vocab * sizeof(float) : 0; }

int mila_cdna4_token_bias_fill(float* bias, size_t bias_stride, int row, int vocab, float value, mila_stream_t stream)
{
    MILA_REQUIRE(bias, "token_bias_fill: null pointer");
    MILA_REQUIRE(vocab > 0 && row >= 0 && (row == 0 || bias_stride >= (size_t)vocab), "token_bias_fill: need vocab > 0, row >= 0, bias_stride >= vocab");
    MILA_REQUIRE(!std::isnan(value) && !(std::isinf(value) && value > 0.0f), "token_bias_fill: the value must be finite or -inf");
    int blocks = (vocab + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(token_bias_fill_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), bias + (size_t)row * bias_stride, vocab, value);
    MILA_LAUNCH_CHECK("token_bias_fill");
}

int mila_cdna4_token_bias_set(float* bias, size_t bias_stride, int row, int vocab, const int32_t* ids_dev, const float* values_dev, int n, mila_stream_t stream)
{
    MILA_REQUIRE(n >= 0, "token_bias_set: n must not be negative");
    MILA_REQUIRE(n == 0 || (bias && ids_dev && values_dev), "token_bias_set: null pointer");
    MILA_REQUIRE(vocab > 0 && row >= 0 && (row == 0 || bias_stride >= (size_t)vocab), "token_bias_set: need vocab > 0, row >= 0, bias_stride >= vocab");
    if (n == 0) return MILA_OK;
    int blocks = (n + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(token_bias_set_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), bias + (size_t)row * bias_stride, vocab, ids_dev, values_dev, n);
    MILA_LAUNCH_CHECK("token_bias_set");
}

// ---- the token automaton (mila_cdna4.h: token automaton).  One launch each, the row in blockIdx.y; at most 256 workgroups per row walk the table.
static bool automaton_shape_ok(int vocab, int S, int C)
{
    return vocab > 0 && S >= 1 && S <= 65535 && C >= 1 && C <= 65535 && (size_t)S * (size_t)C * sizeof(uint16_t) <= ((size_t)256 << 20);
}

size_t mila_cdna4_token_automaton_bytes(int vocab, int S, int C)
{
    return automaton_shape_ok(vocab, S, C) ? ((size_t)vocab + (size_t)S * (size_t)C) * sizeof(uint16_t) : 0;
}

static int launch_token_automaton(bool step, float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next, int S,
                                  int C, int32_t* state_dev, const int32_t* token_dev, const int32_t* active_dev, uint32_t* ticket_dev, int rows, int vocab,
                                  mila_stream_t stream, const char* who)
{
    MILA_REQUIRE(eff && class_of && next && state_dev && (!step || (token_dev && ticket_dev)), "token_automaton: null pointer");
    MILA_REQUIRE(rows >= 1 && rows <= 4, "token_automaton: rows must be 1 .. 4");
    MILA_REQUIRE(automaton_shape_ok(vocab, S, C), "token_automaton: need vocab > 0, 1 <= S, C <= 65535 and S * C * 2 bytes <= 256 MiB");
    MILA_REQUIRE(rows == 1 || eff_stride >= (size_t)vocab, "token_automaton: eff_stride must be at least vocab");
    MILA_REQUIRE(!base || base_stride == 0 || base_stride >= (size_t)vocab, "token_automaton: base_stride must be 0 (shared) or at least vocab");
    auto aligned = [](const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    const int vec = aligned(eff, 16) && eff_stride % 4 == 0 && aligned(class_of, 8) && (!base || (aligned(base, 16) && base_stride % 4 == 0));
    int blocks = (vocab + 1023) / 1024;
    if (blocks > 256) blocks = 256;
    if (step)
        hipLaunchKernelGGL(token_automaton_kernel<true>, dim3(blocks, rows), dim3(256), 0, as_stream(stream), eff, eff_stride, base, base_stride, class_of, next, S, C, state_dev,
                           token_dev, active_dev, ticket_dev, vocab, vec);
    else
        hipLaunchKernelGGL(token_automaton_kernel<false>, dim3(blocks, rows), dim3(256), 0, as_stream(stream), eff, eff_stride, base, base_stride, class_of, next, S, C, state_dev,
                           nullptr, nullptr, nullptr, vocab, vec);
    MILA_LAUNCH_CHECK(who);
}

int mila_cdna4_token_automaton_compose(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next, int S, int C,
                                       int32_t* state_dev, int rows, int vocab, mila_stream_t stream)
{
    return launch_token_automaton(false, eff, eff_stride, base, base_stride, class_of, next, S, C, state_dev, nullptr, nullptr, nullptr, rows, vocab, stream,
                                  "token_automaton_compose");
}

int mila_cdna4_token_automaton_step(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next, int S, int C,
                                    int32_t* state_dev, const int32_t* token_dev, const int32_t* active_dev, uint32_t* ticket_dev, int rows, int vocab, mila_stream_t stream)
{
    return launch_token_automaton(true, eff, eff_stride, base, base_stride, class_of, next, S, C, state_dev, token_dev, active_dev, ticket_dev, rows, vocab, stream,
                                  "token_automaton_step");
}

// the chain forms: what both check, the 16-byte path's condition (launch_token_automaton's) and the workgroups of a row
static int chain_automaton_args(const float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next, int S, int C,
                                int T, int vocab, const char* who, int& vec, int& blocks)
{
    MILA_REQUIRE(eff && class_of && next, "%s: null pointer", who);
    MILA_REQUIRE(T >= 2 && T <= 4, "%s: T=%d rows outside 2 .. 4", who, T);
    MILA_REQUIRE(automaton_shape_ok(vocab, S, C), "%s: need vocab > 0, 1 <= S, C <= 65535 and S * C * 2 bytes <= 256 MiB", who);
    MILA_REQUIRE(eff_stride >= (size_t)vocab, "%s: eff_stride must be at least vocab", who);
    MILA_REQUIRE(!base || base_stride == 0 || base_stride >= (size_t)vocab, "%s: base_stride must be 0 (shared) or at least vocab", who);
    auto aligned = [](const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    vec = aligned(eff, 16) && eff_stride % 4 == 0 && aligned(class_of, 8) && (!base || (aligned(base, 16) && base_stride % 4 == 0));
    blocks = (vocab + 1023) / 1024;
    if (blocks > 256) blocks = 256;
    return MILA_OK;
}

int mila_cdna4_token_automaton_chain_compose(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next, int S,
                                             int C, const int32_t* state_dev, const int32_t* tok_dev, int32_t* chain_states, int T, int vocab, mila_stream_t stream)
{
    const char* who = "token_automaton_chain_compose";
    int vec = 0, blocks = 0;
    if (const int rc = chain_automaton_args(eff, eff_stride, base, base_stride, class_of, next, S, C, T, vocab, who, vec, blocks)) return rc;
    MILA_REQUIRE(state_dev && tok_dev && chain_states, "%s: null pointer", who);
    hipLaunchKernelGGL(token_automaton_chain_compose_kernel, dim3(blocks, T - 1), dim3(256), 0, as_stream(stream), eff, eff_stride, base, base_stride, class_of, next, S, C,
                       state_dev, tok_dev, chain_states, vocab, vec);
    MILA_LAUNCH_CHECK(who);
}

int mila_cdna4_token_automaton_chain_step(float* eff, size_t eff_stride, const float* base, size_t base_stride, const uint16_t* class_of, const uint16_t* next, int S, int C,
                                          int32_t* state_dev, const int32_t* tok_dev, const int32_t* chain_states, const int32_t* result_dev, int T,
                                          uint32_t* ticket_dev, int vocab, mila_stream_t stream)
{
    const char* who = "token_automaton_chain_step";
    int vec = 0, blocks = 0;
    if (const int rc = chain_automaton_args(eff, eff_stride, base, base_stride, class_of, next, S, C, T, vocab, who, vec, blocks)) return rc;
    MILA_REQUIRE(state_dev && tok_dev && chain_states && result_dev && ticket_dev, "%s: null pointer", who);
    hipLaunchKernelGGL(token_automaton_chain_step_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), eff, base, class_of, next, S, C, state_dev, tok_dev, chain_states,
                       result_dev, T, ticket_dev, vocab, vec);
    MILA_LAUNCH_CHECK(who);
}

// the chain tails with a bias (mila_cdna4.h: logit bias, chain forms): row t's table is bias + t * bias_stride
int mila_cdna4_sample_radix_biased_chain_accept_fp32(int32_t* tok, int32_t* result, const float* logits, size_t logits_stride, int T, int vocab, float softcap,
                                                     float temperature, int top_k, float top_p, const float* draws, const float* bias, size_t bias_stride, void* scratch,
                                                     size_t scratch_bytes, int32_t* position_dev, mila_stream_t stream)
{
    return call_radix_rows(kRowsChain, logits, logits_stride, tok, T, vocab, softcap, temperature, top_k, top_p, draws, scratch, scratch_bytes, position_dev, nullptr, result,
                          as_stream(stream), bias ? "sample_radix_biased_chain_accept_fp32" : "sample_radix_chain_accept_fp32", nullptr, bias, bias_stride);
}

// the greedy chain from the logits: the biased first stage over T rows, then the chain's final.  Without a bias the greedy chain has no first stage of its own (the
// lm_head launch leaves the partials: sample_argmax_chain_accept), so a bias table is required here, as a table or a bias is in the rows entry.
int mila_cdna4_sample_argmax_biased_chain_accept_fp32(int32_t* tok, int32_t* result, const float* logits, size_t logits_stride, int T, int vocab, float softcap,
                                                      const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* position_dev, mila_stream_t stream)
{
    const char* who = "sample_argmax_biased_chain_accept_fp32";
    MILA_REQUIRE(tok && result && logits && bias && position_dev, "%s: null pointer", who);
    MILA_REQUIRE(T >= 2 && T <= 4, "%s: T=%d rows outside 2 .. 4", who, T);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE(logits_stride >= (size_t)vocab, "%s: logits_stride %zu < vocab %d", who, logits_stride, vocab);
    if (const int rc = check_bias(bias, bias_stride, T, vocab, who)) return rc;
    SampleFilter f{};
    if (const int rc = make_filter(nullptr, nullptr, 0, T, vocab, f, who)) return rc;
    ArgmaxPartials a;
    if (const int rc = launch_argmax_partials(logits, logits_stride, T, vocab, softcap, &f, scratch, scratch_bytes, as_stream(stream), who, a, bias, bias_stride)) return rc;
    hipLaunchKernelGGL(argmax_chain_accept_kernel, dim3(1), dim3(256), 0, as_stream(stream), a.pv, tok, result, position_dev, a.blocks, a.row_floats, T);
    MILA_LAUNCH_CHECK(who);
}

int mila_cdna4_sample_radix_biased_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                        const mila_sample_filters* filters, uint32_t* table, const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes,
                                        mila_stream_t stream)
{
    const char* who = bias ? "sample_radix_biased_fp32" : "sample_radix_filtered_fp32";
    SampleFilter f{};
    const int rc = make_filter(filters, table, 0, 1, vocab, f, who);
    if (rc) return rc;
    return call_radix_one<float>(logits, token_out, vocab, softcap, temperature, top_k, top_p, r, nullptr, scratch, scratch_bytes, as_stream(stream), who, &f, bias, bias_stride);
}

int mila_cdna4_sample_radix_biased_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p,
                                                const float* draws, int draws_size, const mila_sample_filters* filters, uint32_t* table, const float* bias, size_t bias_stride,
                                                void* scratch, size_t scratch_bytes, int32_t* position_dev, unsigned long long* seq_dev, unsigned long long* ring, int ring_size,
                                                mila_stream_t stream)
{
    const char* who = bias ? "sample_radix_biased_advance_fp32" : "sample_radix_filtered_advance_fp32";
    SampleFilter f{};
    const int rc = make_filter(filters, table, 0, 1, vocab, f, who);
    if (rc) return rc;
    const RadixAdvance adv{draws, draws_size, position_dev, seq_dev, ring, ring_size};
    return call_radix_one<float>(logits, token_out, vocab, softcap, temperature, top_k, top_p, 0.0f, &adv, scratch, scratch_bytes, as_stream(stream), who, &f, bias, bias_stride);
}

int mila_cdna4_sample_radix_biased_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature, int top_k,
                                             float top_p, const float* draws, const mila_sample_filters* filters, uint32_t* table, size_t table_stride, const float* bias,
                                             size_t bias_stride, void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    const char* who = bias ? "sample_radix_biased_rows_fp32" : "sample_radix_filtered_rows_fp32";
    SampleFilter f{};
    const int rc = make_filter(filters, table, table_stride, rows, vocab, f, who);
    if (rc) return rc;
    return call_radix_rows(kRowsTokens, logits, logits_stride, token_out, rows, vocab, softcap, temperature, top_k, top_p, draws, scratch, scratch_bytes, nullptr, nullptr, nullptr,
                          as_stream(stream), who, &f, bias, bias_stride);
}

int mila_cdna4_sample_radix_biased_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature,
                                                     int top_k, float top_p, const float* draws, const mila_sample_filters* filters, uint32_t* table, size_t table_stride,
                                                     const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* positions_dev,
                                                     const int32_t* active_dev, mila_stream_t stream)
{
    const char* who = bias ? "sample_radix_biased_rows_advance_fp32" : "sample_radix_filtered_rows_advance_fp32";
    SampleFilter f{};
    const int rc = make_filter(filters, table, table_stride, rows, vocab, f, who);
    if (rc) return rc;
    return call_radix_rows(kRowsAdvance, logits, logits_stride, token_out, rows, vocab, softcap, temperature, top_k, top_p, draws, scratch, scratch_bytes, positions_dev, active_dev,
                          nullptr, as_stream(stream), who, &f, bias, bias_stride);
}

// table == NULL and bias == NULL: no penalties, and min_p does not change a greedy request -- today's greedy sampler on the logits as they are
int mila_cdna4_sample_argmax_biased_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters, uint32_t* table,
                                         const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    const char* who = bias ? "sample_argmax_biased_fp32" : "sample_argmax_filtered_fp32";
    SampleFilter f{};
    const int rc = make_filter(filters, table, 0, 1, vocab, f, who);
    if (rc) return rc;
    if (!table && !bias) return run_argmax<float>(logits, token_out, vocab, scratch, scratch_bytes, as_stream(stream), who);
    MILA_REQUIRE(logits && token_out, "%s: null pointer", who);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    return run_argmax_filtered(logits, 0, token_out, 1, vocab, softcap, f, scratch, scratch_bytes, nullptr, nullptr, nullptr, as_stream(stream), who, bias, bias_stride);
}

int mila_cdna4_sample_argmax_biased_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters, uint32_t* table,
                                                 const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* position_dev,
                                                 unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream)
{
    const char* who = bias ? "sample_argmax_biased_advance_fp32" : "sample_argmax_filtered_advance_fp32";
    SampleFilter f{};
    const int rc = make_filter(filters, table, 0, 1, vocab, f, who);
    if (rc) return rc;
    if (!table && !bias) return mila_cdna4_sample_argmax_advance_fp32(logits, token_out, vocab, scratch, scratch_bytes, position_dev, seq_dev, ring, ring_size, stream);
    MILA_REQUIRE(logits && token_out && position_dev, "%s: null pointer", who);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE((ring == nullptr) == (seq_dev == nullptr) && (ring == nullptr || ring_size > 0), "%s: ring, seq_dev and ring_size go together", who);
    const RadixAdvance adv{nullptr, 0, position_dev, seq_dev, ring, ring_size};
    return run_argmax_filtered(logits, 0, token_out, 1, vocab, softcap, f, scratch, scratch_bytes, &adv, nullptr, nullptr, as_stream(stream), who, bias, bias_stride);
}

// the rows greedy tail with penalties and / or a bias: both launches (the lm_head epilogue cannot compute x3), tokens, positions and tables of the active rows only.
// Without a bias the table is required, as it always was; with one it may be NULL.
int mila_cdna4_sample_argmax_biased_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                      const mila_sample_filters* filters, uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride,
                                                      void* scratch, size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev, mila_stream_t stream)
{
    const char* who = bias ? "sample_argmax_biased_rows_advance_fp32" : "sample_argmax_filtered_rows_advance_fp32";
    MILA_REQUIRE(logits && token_out && positions_dev && active_dev && (table || bias), "%s: null pointer", who);
    MILA_REQUIRE(rows >= 1 && rows <= 4, "%s: rows=%d outside 1 .. 4", who, rows);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE(logits_stride >= (size_t)vocab, "%s: logits_stride %zu < vocab %d", who, logits_stride, vocab);
    SampleFilter f{};
    const int rc = make_filter(filters, table, table_stride, rows, vocab, f, who);
    if (rc) return rc;
    return run_argmax_filtered(logits, logits_stride, token_out, rows, vocab, softcap, f, scratch, scratch_bytes, nullptr, positions_dev, active_dev, as_stream(stream), who, bias,
                               bias_stride);
}

// the filtered entries: their biased siblings without a bias table
int mila_cdna4_sample_radix_filtered_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p, float r,
                                          const mila_sample_filters* filters, uint32_t* table, void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    return mila_cdna4_sample_radix_biased_fp32(logits, token_out, vocab, softcap, temperature, top_k, top_p, r, filters, table, nullptr, 0, scratch, scratch_bytes, stream);
}

int mila_cdna4_sample_radix_filtered_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, float temperature, int top_k, float top_p,
                                                  const float* draws, int draws_size, const mila_sample_filters* filters, uint32_t* table, void* scratch, size_t scratch_bytes,
                                                  int32_t* position_dev, unsigned long long* seq_dev, unsigned long long* ring, int ring_size, mila_stream_t stream)
{
    return mila_cdna4_sample_radix_biased_advance_fp32(logits, token_out, vocab, softcap, temperature, top_k, top_p, draws, draws_size, filters, table, nullptr, 0, scratch,
                                                       scratch_bytes, position_dev, seq_dev, ring, ring_size, stream);
}

int mila_cdna4_sample_radix_filtered_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature, int top_k,
                                               float top_p, const float* draws, const mila_sample_filters* filters, uint32_t* table, size_t table_stride, void* scratch,
                                               size_t scratch_bytes, mila_stream_t stream)
{
    return mila_cdna4_sample_radix_biased_rows_fp32(logits, logits_stride, token_out, rows, vocab, softcap, temperature, top_k, top_p, draws, filters, table, table_stride, nullptr,
                                                    0, scratch, scratch_bytes, stream);
}

int mila_cdna4_sample_radix_filtered_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, float temperature,
                                                       int top_k, float top_p, const float* draws, const mila_sample_filters* filters, uint32_t* table, size_t table_stride,
                                                       void* scratch, size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev, mila_stream_t stream)
{
    return mila_cdna4_sample_radix_biased_rows_advance_fp32(logits, logits_stride, token_out, rows, vocab, softcap, temperature, top_k, top_p, draws, filters, table, table_stride,
                                                            nullptr, 0, scratch, scratch_bytes, positions_dev, active_dev, stream);
}

int mila_cdna4_sample_argmax_filtered_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters, uint32_t* table,
                                           void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    return mila_cdna4_sample_argmax_biased_fp32(logits, token_out, vocab, softcap, filters, table, nullptr, 0, scratch, scratch_bytes, stream);
}

int mila_cdna4_sample_argmax_filtered_advance_fp32(const float* logits, int32_t* token_out, int vocab, float softcap, const mila_sample_filters* filters, uint32_t* table,
                                                   void* scratch, size_t scratch_bytes, int32_t* position_dev, unsigned long long* seq_dev, unsigned long long* ring,
                                                   int ring_size, mila_stream_t stream)
{
    return mila_cdna4_sample_argmax_biased_advance_fp32(logits, token_out, vocab, softcap, filters, table, nullptr, 0, scratch, scratch_bytes, position_dev, seq_dev, ring,
                                                        ring_size, stream);
}

int mila_cdna4_sample_argmax_filtered_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                        const mila_sample_filters* filters, uint32_t* table, size_t table_stride, void* scratch, size_t scratch_bytes,
                                                        int32_t* positions_dev, const int32_t* active_dev, mila_stream_t stream)
{
    return mila_cdna4_sample_argmax_biased_rows_advance_fp32(logits, logits_stride, token_out, rows, vocab, softcap, filters, table, table_stride, nullptr, 0, scratch,
                                                             scratch_bytes, positions_dev, active_dev, stream);
}

// "launches:k_passes:p_passes:scratch_need:scale_filtered:mask_filtered" of a filtered call (plan_radix, the function the entries launch from); 0 for arguments the
// entries refuse
size_t mila_cdna4_sample_filters_describe(int vocab, int top_k, float top_p, const mila_sample_filters* filters, int with_table, char* buf, size_t cap)
{
    if (buf && cap) buf[0] = 0;
    if (vocab <= 0 || top_k < 0 || !(top_p > 0.0f)) return 0;
    SampleFilter f{};
    if (make_filter(filters, nullptr, 0, 1, vocab, f, "sample_filters_describe")) return 0;
    const RadixPlan d = plan_radix(vocab, top_k, top_p, with_table != 0, f.min_p);
    return 1 + snprintf(buf, buf ? cap : 0, "%d:%d:%d:%zu:%d:%d", d.launches, d.k_passes, d.p_passes, d.scratch_need, d.scale_filtered, d.mask_filtered);
}

size_t mila_cdna4_sample_radix_plan_describe(int vocab, int top_k, float top_p, char* buf, size_t cap)
{
    if (buf && cap) buf[0] = 0;
    if (vocab <= 0 || top_k < 0 || !(top_p > 0.0f)) return 0;
    const RadixPlan d = plan_radix(vocab, top_k, top_p);
    return 1 + snprintf(buf, buf ? cap : 0, "%d:%d:%d:%zu", d.launches, d.k_passes, d.p_passes, d.scratch_need);
}

// ---- row requests (mila_cdna4.h: row requests)
size_t mila_cdna4_sample_row_params_bytes(int rows) { return (rows >= 1 && rows <= 4) ? (size_t)rows * sizeof(RowParams) : 0; }

int mila_cdna4_sample_row_params_set(void* params_dev, int row, const mila_sample_row_params* params, mila_stream_t stream)
{
    const char* who = "sample_row_params_set";
    MILA_REQUIRE(params_dev && params, "%s: null pointer", who);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(params_dev) & 3u) == 0, "%s: params_dev must be 4-byte aligned", who);
    MILA_REQUIRE(row >= 0 && row < 4, "%s: row=%d outside 0 .. 3", who, row);
    MILA_REQUIRE(std::isfinite(params->temperature), "%s: temperature is not finite", who);
    MILA_REQUIRE(params->top_k >= 0 && params->top_p > 0.0f, "%s: need top_k >= 0, top_p > 0", who);
    const mila_sample_filters flt{params->min_p, params->repetition_penalty, params->presence_penalty, params->frequency_penalty};
    SampleFilter f{};
    if (const int rc = make_filter(&flt, nullptr, 0, 1, 1, f, who)) return rc;
    const RowParams v{params->temperature, params->top_k, params->top_p, f.min_p, f.rep, f.inv_rep, f.pres, f.freq};      // (inv_rep: divided here, as make_filter does)
    hipLaunchKernelGGL(sample_row_params_set_kernel, dim3(1), dim3(64), 0, as_stream(stream), reinterpret_cast<RowParams*>(params_dev) + row, v);
    MILA_LAUNCH_CHECK(who);
}

int mila_cdna4_sample_radix_requests_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, const void* params_dev,
                                               const float* draws, uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride, void* scratch,
                                               size_t scratch_bytes, mila_stream_t stream)
{
    return run_radix_requests(logits, logits_stride, token_out, rows, vocab, softcap, params_dev, draws, table, table_stride, bias, bias_stride, scratch, scratch_bytes, false,
                              nullptr, nullptr, as_stream(stream), "sample_radix_requests_rows_fp32");
}

int mila_cdna4_sample_radix_requests_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                       const void* params_dev, const float* draws, uint32_t* table, size_t table_stride, const float* bias,
                                                       size_t bias_stride, void* scratch, size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev,
                                                       mila_stream_t stream)
{
    return run_radix_requests(logits, logits_stride, token_out, rows, vocab, softcap, params_dev, draws, table, table_stride, bias, bias_stride, scratch, scratch_bytes, true,
                              positions_dev, active_dev, as_stream(stream), "sample_radix_requests_rows_advance_fp32");
}

int mila_cdna4_sample_argmax_requests_rows_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap, const void* params_dev,
                                                uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride, void* scratch, size_t scratch_bytes,
                                                mila_stream_t stream)
{
    return run_argmax_requests(logits, logits_stride, token_out, rows, vocab, softcap, params_dev, table, table_stride, bias, bias_stride, scratch, scratch_bytes, false, nullptr,
                               nullptr, as_stream(stream), "sample_argmax_requests_rows_fp32");
}

int mila_cdna4_sample_argmax_requests_rows_advance_fp32(const float* logits, size_t logits_stride, int32_t* token_out, int rows, int vocab, float softcap,
                                                        const void* params_dev, uint32_t* table, size_t table_stride, const float* bias, size_t bias_stride, void* scratch,
                                                        size_t scratch_bytes, int32_t* positions_dev, const int32_t* active_dev, mila_stream_t stream)
{
    return run_argmax_requests(logits, logits_stride, token_out, rows, vocab, softcap, params_dev, table, table_stride, bias, bias_stride, scratch, scratch_bytes, true,
                               positions_dev, active_dev, as_stream(stream), "sample_argmax_requests_rows_advance_fp32");
}

size_t mila_cdna4_token_automaton_rows_bytes(int rows) { return (rows >= 1 && rows <= 4) ? (size_t)rows * sizeof(AutomatonRow) : 0; }

int mila_cdna4_token_automaton_rows_set(void* desc_dev, int row, const uint16_t* class_of, const uint16_t* next, int S, int C, int vocab, mila_stream_t stream)
{
    const char* who = "token_automaton_rows_set";
    MILA_REQUIRE(desc_dev, "%s: null pointer", who);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(desc_dev) & 7u) == 0, "%s: desc_dev must be 8-byte aligned", who);
    MILA_REQUIRE(row >= 0 && row < 4, "%s: row=%d outside 0 .. 3", who, row);
    AutomatonRow v{nullptr, nullptr, 0, 0};
    if (class_of || next)
    {
        MILA_REQUIRE(class_of && next, "%s: class_of and next go together", who);
        MILA_REQUIRE(automaton_shape_ok(vocab, S, C), "%s: need vocab > 0, 1 <= S, C <= 65535 and S * C * 2 bytes <= 256 MiB", who);
        MILA_REQUIRE(((reinterpret_cast<uintptr_t>(class_of) | reinterpret_cast<uintptr_t>(next)) & 1u) == 0, "%s: class_of and next must be 2-byte aligned", who);
        v = AutomatonRow{class_of, next, S, C};
    }
    hipLaunchKernelGGL(token_automaton_row_set_kernel, dim3(1), dim3(64), 0, as_stream(stream), reinterpret_cast<AutomatonRow*>(desc_dev) + row, v);
    MILA_LAUNCH_CHECK(who);
}

static int launch_token_automaton_rows(bool step, float* eff, size_t eff_stride, const float* base, size_t base_stride, const void* desc_dev, int32_t* state_dev,
                                       const int32_t* token_dev, const int32_t* active_dev, uint32_t* ticket_dev, int rows, int vocab, mila_stream_t stream, const char* who)
{
    MILA_REQUIRE(eff && desc_dev && state_dev && (!step || (token_dev && ticket_dev)), "%s: null pointer", who);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(desc_dev) & 7u) == 0, "%s: desc_dev must be 8-byte aligned", who);
    MILA_REQUIRE(rows >= 1 && rows <= 4, "%s: rows must be 1 .. 4", who);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE(rows == 1 || eff_stride >= (size_t)vocab, "%s: eff_stride must be at least vocab", who);
    MILA_REQUIRE(!base || base_stride == 0 || base_stride >= (size_t)vocab, "%s: base_stride must be 0 (shared) or at least vocab", who);
    auto aligned = [](const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    MILA_REQUIRE(aligned(eff, 4) && aligned(base, 4), "%s: eff and base must be 4-byte aligned", who);
    const int vec = aligned(eff, 16) && eff_stride % 4 == 0 && (!base || (aligned(base, 16) && base_stride % 4 == 0));      // (class_of: per row, on the device)
    int blocks = (vocab + 1023) / 1024;
    if (blocks > 256) blocks = 256;
    const AutomatonRow* desc = reinterpret_cast<const AutomatonRow*>(desc_dev);
    if (step)
        hipLaunchKernelGGL(token_automaton_rows_kernel<true>, dim3(blocks, rows), dim3(256), 0, as_stream(stream), eff, eff_stride, base, base_stride, desc, state_dev, token_dev,
                           active_dev, ticket_dev, vocab, vec);
    else
        hipLaunchKernelGGL(token_automaton_rows_kernel<false>, dim3(blocks, rows), dim3(256), 0, as_stream(stream), eff, eff_stride, base, base_stride, desc, state_dev, nullptr,
                           nullptr, nullptr, vocab, vec);
    MILA_LAUNCH_CHECK(who);
}

int mila_cdna4_token_automaton_rows_compose(float* eff, size_t eff_stride, const float* base, size_t base_stride, const void* desc_dev, int32_t* state_dev, int rows,
                                            int vocab, mila_stream_t stream)
{
    return launch_token_automaton_rows(false, eff, eff_stride, base, base_stride, desc_dev, state_dev, nullptr, nullptr, nullptr, rows, vocab, stream,
                                       "token_automaton_rows_compose");
}

int mila_cdna4_token_automaton_rows_step(float* eff, size_t eff_stride, const float* base, size_t base_stride, const void* desc_dev, int32_t* state_dev,
                                         const int32_t* token_dev, const int32_t* active_dev, uint32_t* ticket_dev, int rows, int vocab, mila_stream_t stream)
{
    return launch_token_automaton_rows(true, eff, eff_stride, base, base_stride, desc_dev, state_dev, token_dev, active_dev, ticket_dev, rows, vocab, stream,
                                       "token_automaton_rows_step");
}

}  // extern "C"
