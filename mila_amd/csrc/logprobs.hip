// Token log-probabilities of a decode step: the chosen token's and the top-n alternatives', from the fp32 logits the lm_head left on the device.
//   z_i = softcap > 0 ? softcap * tanhf(x_i / softcap) : x_i      (soft_cap of common.h: the samplers' expression, without the temperature)
//   m = max z,  S = sum expf(z_i - m),  logprob_i = (z_i - m) - logf(S)
// the model's distribution: no temperature, no top-k / top-p.  "Top-n" = the n largest z, value descending, then LOWER index first -- the greedy sampler's tie rule, so
// on a greedy step top_ids[0] is the emitted token.
// Two launches, the rows in the grid (each row its own scratch region, so a row's outputs do not depend on the other rows):
//   partials: <= 256 workgroups per row walk the row once; each leaves (max, sum exp(z - max)) and, when n > 0, its local top-n as (z, index) pairs.  Needs only the logits.
//   final:    one workgroup per row merges the (max, sum) pairs -- lane l of one wave adds workgroups 4l .. 4l+3 in ascending order, rescaled to the global max, then
//             the butterfly (wave_sum_partials' order in sampling.hip) -- and the candidates, reads the token from a DEVICE word and writes the outputs.
// No floating-point atomics; every sum has a fixed order: the same bits run to run.
#include <cfloat>
#include <cmath>

#include "common.h"

namespace mila {

constexpr int kLpBlocks = 256;                       // workgroups of the partials launch per row, at most
constexpr int kLpMaxTop = 20;
constexpr int kLpPre = 8;                            // elements of a thread's strided walk kept in registers (all of it up to 2^19 entries)
constexpr int kLpRecordWords = 4 + 2 * kLpMaxTop;    // tag, token, logprob, top_n, ids[20], logprobs[20]
constexpr int kLpNone = 0x7fffffff;                  // the index of an empty candidate slot: (-inf, kLpNone) loses against every element

struct LpParams
{
    const float* logits;
    size_t logits_stride;            // floats between two rows
    float* scratch;                  // row b: max[kLpBlocks], sum[kLpBlocks], cand z[kLpBlocks * top_n], cand index[kLpBlocks * top_n]
    size_t row_floats;               // floats between the scratch regions of two rows
    int vocab, top_n, nblocks;
    float softcap;
    // the final launch
    const int32_t* tokens;
    const int32_t* active;           // nullable
    const int32_t* count;            // nullable
    float* logprob_out;
    int32_t* top_ids_out;
    float* top_logprobs_out;
    const unsigned long long* seq_dev;      // the publish form
    uint32_t* ring;
    int ring_size;
};

static size_t lp_row_floats(int top_n) { return (size_t)2 * kLpBlocks + (size_t)2 * kLpBlocks * top_n; }

// (v, i) comes strictly behind (pv, pi) in the top-n order
__device__ __forceinline__ bool lp_behind(float v, int i, float pv, int pi) { return v < pv || (v == pv && i > pi); }

// the best (z, index) pair of a wave, on every lane: the largest value, then the lowest index among the lanes that hold it -- two register-only butterflies
// (wave_max's DPP / permlane steps) instead of twelve LDS-crossbar shuffles.  All 64 lanes must be active.
__device__ __forceinline__ void lp_wave_argmax(float& bv, int& bi)
{
    const float m = wave_max(bv);
    bi = wave_min_i32(bv == m ? bi : kLpNone);
    bv = m;
}

// Merge of up to 64 lists that are each in top-n order, one per lane (`len` entries at lv / li; 0 = this lane has none): the first n of the union, in order, into
// ov / oi (lane 0 stores).  Round r compares the lanes' current heads; the lane whose head won moves on to its next entry.  Every index is held once.
__device__ __forceinline__ void lp_wave_merge(const float* lv, const int* li, int len, int n, float* ov, int* oi, int lane)
{
    int k = 0;
    for (int r = 0; r < n; ++r)
    {
        const int mine = k < len ? li[k] : kLpNone;
        float bv = k < len ? lv[k] : -INFINITY;
        int bi = mine;
        lp_wave_argmax(bv, bi);
        if (lane == 0) { ov[r] = bv; oi[r] = bi; }
        if (bi != kLpNone && mine == bi) ++k;
    }
}

__global__ __launch_bounds__(256) void logprobs_partial_kernel(const LpParams p)
{
    __shared__ float red[4];
    __shared__ float wv[4 * kLpMaxTop];
    __shared__ int wi[4 * kLpMaxTop];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.y;
    const float* x = p.logits + (size_t)row * p.logits_stride;
    float* pm = p.scratch + (size_t)row * p.row_floats;
    float* ps = pm + kLpBlocks;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256, tail0 = first + kLpPre * stride;
    float z[kLpPre];
    int ix[kLpPre];
#pragma unroll
    for (int j = 0; j < kLpPre; ++j)
    {
        const int i = first + j * stride;
        z[j] = i < p.vocab ? x[i] : -INFINITY;
        ix[j] = i < p.vocab ? i : kLpNone;
    }
    float mx = -FLT_MAX;
#pragma unroll
    for (int j = 0; j < kLpPre; ++j)
    {
        if (ix[j] != kLpNone) z[j] = soft_cap(z[j], p.softcap);
        mx = fmaxf(mx, z[j]);
    }
    for (int i = tail0; i < p.vocab; i += stride) mx = fmaxf(mx, soft_cap(x[i], p.softcap));      // beyond 2^19 entries: recomputed in every walk
    mx = block_max<4>(mx, red);
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < kLpPre; ++j) sum += expf(z[j] - mx);                                   // an empty slot is -inf: adds 0
    for (int i = tail0; i < p.vocab; i += stride) sum += expf(soft_cap(x[i], p.softcap) - mx);
    sum = block_sum<4>(sum, red);
    if (threadIdx.x == 0) { pm[blockIdx.x] = mx; ps[blockIdx.x] = sum; }
    const int n = p.top_n;
    if (n == 0) return;
    // this wave's top n, then the workgroup's
    {
        float pv = INFINITY;
        int pi = -1;
        for (int r = 0; r < n; ++r)
        {
            float bv = -INFINITY;
            int bi = kLpNone;
#pragma unroll
            for (int j = 0; j < kLpPre; ++j)
                if (lp_behind(z[j], ix[j], pv, pi)) argmax_better(bv, bi, z[j], ix[j]);
            for (int i = tail0; i < p.vocab; i += stride)
            {
                const float v = soft_cap(x[i], p.softcap);
                if (lp_behind(v, i, pv, pi)) argmax_better(bv, bi, v, i);
            }
            lp_wave_argmax(bv, bi);
            if (lane == 0) { wv[wave * kLpMaxTop + r] = bv; wi[wave * kLpMaxTop + r] = bi; }
            pv = bv;
            pi = bi;
        }
    }
    __syncthreads();
    if (wave == 0)      // the four waves' lists, one per lane 0 .. 3, into this workgroup's slots of the row's candidates
    {
        float* cv = ps + kLpBlocks + (size_t)blockIdx.x * n;
        int* ci = reinterpret_cast<int*>(ps + kLpBlocks + (size_t)kLpBlocks * n) + (size_t)blockIdx.x * n;
        const int l = lane < 4 ? lane : 0;
        lp_wave_merge(wv + l * kLpMaxTop, wi + l * kLpMaxTop, lane < 4 ? n : 0, n, cv, ci, lane);
    }
}

// PUBLISH: the one-row form of the decode-ahead loop -- the outputs go into one record of a host-visible ring, slot *seq_dev % ring_size (the tail or snapshot_token
// has already bumped the sequence number for this sample): the payload by plain stores, then the tag by a release store at system scope, all by ONE lane.
template <bool PUBLISH>
__global__ __launch_bounds__(256) void logprobs_final_kernel(const LpParams p)
{
    __shared__ float wv[4 * kLpMaxTop];
    __shared__ int wi[4 * kLpMaxTop];
    __shared__ float tv[kLpMaxTop];
    __shared__ int ti[kLpMaxTop];
    __shared__ float ms[2];
    __shared__ float cvs[kLpBlocks * kLpMaxTop];      // the row's candidates (40 KB with their indices)
    __shared__ int cis[kLpBlocks * kLpMaxTop];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.x;
    if (p.active != nullptr && p.active[row] == 0) return;          // the whole workgroup: the row is left untouched
    if (p.count != nullptr && row >= p.count[0]) return;
    const float* pm = p.scratch + (size_t)row * p.row_floats;
    const float* ps = pm + kLpBlocks;
    const int n = p.top_n, nb = p.nblocks;
    if (wave == 0)
    {
        float m4[4], s4[4];
        float mx = -FLT_MAX;
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const int b = 4 * lane + i;
            m4[i] = b < nb ? pm[b] : -FLT_MAX;
            s4[i] = b < nb ? ps[b] : 0.0f;
            mx = fmaxf(mx, m4[i]);
        }
        mx = wave_max(mx);
        float f = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) f += s4[i] * expf(m4[i] - mx);
        f = wave_sum(f);
        if (lane == 0) { ms[0] = mx; ms[1] = logf(f); }
    }
    if (n > 0)
    {
        const float* cv = ps + kLpBlocks;
        const int* ci = reinterpret_cast<const int*>(cv + (size_t)kLpBlocks * n);
        const int ncand = nb * n;                                    // workgroup b's list at [b * n, (b + 1) * n), each in top-n order
        for (int c = threadIdx.x; c < ncand; c += 256) { cvs[c] = cv[c]; cis[c] = ci[c]; }
        __syncthreads();
        // thread t owns workgroup t's list: each wave merges its 64 lists, then wave 0 the four results
        const int own = (int)threadIdx.x < nb ? (int)threadIdx.x : 0;
        lp_wave_merge(cvs + own * n, cis + own * n, (int)threadIdx.x < nb ? n : 0, n, wv + wave * kLpMaxTop, wi + wave * kLpMaxTop, lane);
        __syncthreads();
        const int l = lane < 4 ? lane : 0;
        if (wave == 0) lp_wave_merge(wv + l * kLpMaxTop, wi + l * kLpMaxTop, lane < 4 ? n : 0, n, tv, ti, lane);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float mx = ms[0], lse = ms[1];
    const int tok = p.tokens[row];
    float lp = __builtin_nanf("");                                   // a token outside the vocabulary has no log-probability (and nothing is read for it)
    bool listed = false;
    for (int r = 0; r < n; ++r)
        if (ti[r] == tok) { lp = (tv[r] - mx) - lse; listed = true; }
    if (!listed && tok >= 0 && tok < p.vocab) lp = (soft_cap(p.logits[(size_t)row * p.logits_stride + tok], p.softcap) - mx) - lse;
    if (PUBLISH)
    {
        const unsigned long long s = p.seq_dev[0];
        uint32_t* rec = p.ring + (size_t)(s % (unsigned long long)p.ring_size) * kLpRecordWords;
        rec[1] = (uint32_t)tok;
        rec[2] = __float_as_uint(lp);
        rec[3] = (uint32_t)n;
        for (int r = 0; r < n; ++r)
        {
            rec[4 + r] = (uint32_t)(ti[r] == kLpNone ? -1 : ti[r]);
            rec[4 + kLpMaxTop + r] = __float_as_uint((tv[r] - mx) - lse);
        }
        __hip_atomic_store(rec, (uint32_t)s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    else
    {
        p.logprob_out[row] = lp;
        for (int r = 0; r < n; ++r)
        {
            p.top_ids_out[(size_t)row * n + r] = ti[r] == kLpNone ? -1 : ti[r];
            p.top_logprobs_out[(size_t)row * n + r] = (tv[r] - mx) - lse;
        }
    }
}

static bool lp_shape_ok(int rows, int vocab, int top_n) { return rows >= 1 && rows <= 4 && vocab > 0 && top_n >= 0 && top_n <= kLpMaxTop && top_n <= vocab; }

// the checks both entries share, then the partials launch; `p` leaves ready for the final launch
static int lp_partials(LpParams& p, const float* logits, size_t logits_stride, int rows, int vocab, float softcap, int top_n, void* scratch, size_t scratch_bytes,
                       hipStream_t s, const char* who)
{
    MILA_REQUIRE(rows >= 1 && rows <= 4, "%s: rows=%d outside 1 .. 4", who, rows);
    MILA_REQUIRE(vocab > 0, "%s: vocab must be positive", who);
    MILA_REQUIRE(top_n >= 0 && top_n <= kLpMaxTop && top_n <= vocab, "%s: top_n=%d outside 0 .. min(%d, vocab)", who, top_n, kLpMaxTop);
    MILA_REQUIRE(logits_stride >= (size_t)vocab, "%s: logits_stride %zu < vocab %d", who, logits_stride, vocab);
    const size_t need = lp_row_floats(top_n) * 4 * (size_t)rows;
    if (!scratch || scratch_bytes < need) return set_error(MILA_E_SCRATCH_TOO_SMALL, "%s: scratch %zu bytes < required %zu", who, scratch_bytes, need);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 3u) == 0, "%s: scratch must be 4-byte aligned", who);
    p.logits = logits; p.logits_stride = logits_stride;
    p.scratch = reinterpret_cast<float*>(scratch); p.row_floats = lp_row_floats(top_n);
    p.vocab = vocab; p.top_n = top_n; p.softcap = softcap;
    p.nblocks = (vocab + 255) / 256;
    if (p.nblocks > kLpBlocks) p.nblocks = kLpBlocks;
    hipLaunchKernelGGL(logprobs_partial_kernel, dim3(p.nblocks, rows), dim3(256), 0, s, p);
    return check_hip(hipGetLastError(), who);
}

}  // namespace mila

using namespace mila;

extern "C" {

int mila_cdna4_token_logprobs_record_words(void) { return kLpRecordWords; }

size_t mila_cdna4_token_logprobs_scratch_bytes(int rows, int vocab, int top_n) { return lp_shape_ok(rows, vocab, top_n) ? lp_row_floats(top_n) * 4 * (size_t)rows : 0; }

int mila_cdna4_token_logprobs_rows_fp32(const float* logits, size_t logits_stride, const int32_t* tokens_dev, int rows, int vocab, float softcap, int top_n,
                                        const int32_t* active_dev, const int32_t* count_dev, float* logprob_out, int32_t* top_ids_out, float* top_logprobs_out,
                                        void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    const char* who = "token_logprobs_rows_fp32";
    MILA_REQUIRE(logits && tokens_dev && logprob_out, "%s: null pointer", who);
    MILA_REQUIRE(top_n <= 0 || (top_ids_out && top_logprobs_out), "%s: null pointer", who);
    LpParams p{};
    int rc = lp_partials(p, logits, logits_stride, rows, vocab, softcap, top_n, scratch, scratch_bytes, as_stream(stream), who);
    if (rc) return rc;
    p.tokens = tokens_dev; p.active = active_dev; p.count = count_dev;
    p.logprob_out = logprob_out; p.top_ids_out = top_ids_out; p.top_logprobs_out = top_logprobs_out;
    hipLaunchKernelGGL(logprobs_final_kernel<false>, dim3(rows), dim3(256), 0, as_stream(stream), p);
    MILA_LAUNCH_CHECK(who);
}

int mila_cdna4_token_logprobs_publish_fp32(const float* logits, const int32_t* token_dev, int vocab, float softcap, int top_n, const unsigned long long* seq_dev,
                                           uint32_t* ring, int ring_size, void* scratch, size_t scratch_bytes, mila_stream_t stream)
{
    const char* who = "token_logprobs_publish_fp32";
    MILA_REQUIRE(logits && token_dev && seq_dev && ring, "%s: null pointer", who);
    MILA_REQUIRE(ring_size > 0, "%s: ring_size must be positive", who);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(ring) & 3u) == 0, "%s: ring must be 4-byte aligned", who);
    LpParams p{};
    int rc = lp_partials(p, logits, (size_t)(vocab > 0 ? vocab : 0), 1, vocab, softcap, top_n, scratch, scratch_bytes, as_stream(stream), who);
    if (rc) return rc;
    p.tokens = token_dev; p.seq_dev = seq_dev; p.ring = ring; p.ring_size = ring_size;
    hipLaunchKernelGGL(logprobs_final_kernel<true>, dim3(1), dim3(256), 0, as_stream(stream), p);
    MILA_LAUNCH_CHECK(who);
}

}  // extern "C"
