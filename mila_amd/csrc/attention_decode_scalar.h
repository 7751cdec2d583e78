// What the two split-K "wave per position" decode kernels share: attn_decode_kernel (attention.hip, bf16 cache) and attn_decode_kvfp8_kernel (attention_kvfp8.hip,
// e4m3 cache + one fp32 scale per row).  8 waves per workgroup, GH query heads on one KV head; a workgroup takes one of the `splits` chunks of the live band; every
// wave-instruction fetches RPW whole rows, so a lane owns EPL elements of the rows of ONE lane segment and keeps that segment's online-softmax state (m, l, O) in
// registers.  Each kernel keeps its own row loop -- loads, zero fill, the conversion of a row to packed bf16 pairs, the dot products; the bf16 one also its fused
// prologue -- because one loop for both did not keep every instantiation's registers (EXPERIMENTS.md, "One wave-per-position body").  Everything from the scores on
// exists once, here, taking its geometry from the cache's constants: the score reduction and online-softmax step, the merge of a wave's lane segments, the merge of
// the 8 waves through LDS, the finaliser, and the stores (Y unsplit, or the split's partial O | M | L).  So both caches reduce the same values in the same order.
#pragma once
#include "common.h"

namespace mila {

constexpr int kDecodeWaves = 8;     // 512 threads per workgroup

template <int EPL>
__device__ __forceinline__ void load_row(uint32_t (&dst)[EPL / 2], const uint16_t* p)
{
    if constexpr (EPL == 8) { const u32x4 v = ld16(p); dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
    else if constexpr (EPL == 4) { const u32x2 v = *reinterpret_cast<const u32x2*>(p); dst[0] = v[0]; dst[1] = v[1]; }
    else dst[0] = *reinterpret_cast<const uint32_t*>(p);
}

// sum over the LPR-lane segment a lane belongs to (segments are aligned): the leading steps of wave_sum
template <int LPR>
__device__ __forceinline__ float segment_sum(float v)
{
    if constexpr (LPR == 64) return wave_sum(v);
    v += dpp_f32<0xB1>(v);
    v += dpp_f32<0x4E>(v);
    v += dpp_f32<0x141>(v);
    v += dpp_f32<0x140>(v);
    if constexpr (LPR == 32)
    {
        const uint32_t u = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    return v;
}

// a store of a partial: plain, or (SC1) write-through to agent scope for a reader inside the same launch (the one-pass tail of attn_decode_kernel)
template <bool SC1>
__device__ __forceinline__ void partial_st(float* p, float v)
{
    if constexpr (SC1) __hip_atomic_store((__attribute__((address_space(1))) float*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// ---- lane geometry of a cached row, per cache ----------------------------------------------------------------------------------------------------------------------
// EPL     elements of a row per lane                         NPAIR  = EPL / 2 packed bf16 pairs
// LPR     lanes a row spans (the width of the score sum)     ACTIVE lanes of those that own data
// RPW     rows per wave-instruction = 64 / LPR               PG     row slots a lane keeps in flight per buffer
// FE      output elements per lane in the finaliser (HS / FE lanes take part)
// bf16 cache: a row is the whole wave, HS / 64 elements per lane (16-byte loads at HS 512, 4 slots in flight there against 8 below); HS 64 as 2 elements on 32 lanes
template <int HS>
struct DecodeGeomBf16
{
    static constexpr int EPL = (HS >= 128) ? HS / 64 : 2, NPAIR = EPL / 2;
    static constexpr int LPR = 64, ACTIVE = HS / EPL, RPW = 1;
    static constexpr int PG = (HS >= 512) ? 4 : 8, FE = EPL;
};
// e4m3 cache: a lane loads 4 bytes of a row (8 at HS 512), so a row is HS / 4 lanes wide: one row per wave-instruction at HS 256 / 512, two at HS 128, four at HS 64;
// a workgroup's group is 64 positions at every head size (8 slots in flight at HS 512, where the bf16 cache keeps 4)
template <int HS>
struct DecodeGeomKvFp8
{
    static constexpr int EPL = HS >= 512 ? 8 : 4, NPAIR = EPL / 2, ND = EPL / 4;
    static constexpr int LPR = HS / EPL, ACTIVE = LPR, RPW = 64 / LPR;
    static constexpr int PG = 8 / RPW, FE = HS / 64;
};

// what decode_finish reads of a kernel's parameter block, and the workgroup's place in the launch
struct DecodeFinishArgs
{
    uint16_t* Y;              // [B, NH*HS]
    float* scratch;           // [B, NH, splits, HS+4] partials when splits > 1: O (HS) | M | L | pad
    int NH, splits, split, b, h0;      // ... | the split of the band, the batch row, the first of the GH query heads
    bool write_through;       // the partial is stored write-through and drained (a reader inside the same launch follows)
};

// The online-softmax step of every head over one group of rows.  sc: this lane's share of the PG x GH scores (summed here over the row's lanes), vp: the rows' V values
// as packed bf16 pairs; slot j holds position first + 8 RPW j, masked where that is not below `end`.
template <int GH, class Row>
__device__ __forceinline__ void decode_softmax_step(float (&sc)[Row::PG][GH], const uint32_t (&vp)[Row::PG][Row::NPAIR], float (&m)[GH], float (&l)[GH],
                                                    float (&o)[GH][Row::EPL], int first, int end, float scale)
{
    constexpr int PG = Row::PG, NPAIR = Row::NPAIR;
#pragma unroll
    for (int j = 0; j < PG; ++j)
#pragma unroll
        for (int g = 0; g < GH; ++g) sc[j][g] = segment_sum<Row::LPR>(sc[j][g]);
#pragma unroll
    for (int g = 0; g < GH; ++g)
    {
        float a[PG], mt = -INFINITY;
#pragma unroll
        for (int j = 0; j < PG; ++j)
        {
            a[j] = (first + kDecodeWaves * Row::RPW * j < end) ? sc[j][g] * scale : -INFINITY;
            mt = fmaxf(mt, a[j]);
        }
        const float mn = fmaxf(m[g], mt);
        const float msafe = (mn == -INFINITY) ? 0.0f : mn;
        const float alpha = __expf(m[g] - msafe);        // m = -inf first time: exp(-inf) = 0
        float ex[PG], rs = 0.0f;
#pragma unroll
        for (int j = 0; j < PG; ++j) { ex[j] = __expf(a[j] - msafe); rs += ex[j]; }
        l[g] = l[g] * alpha + rs;
        m[g] = mn;
#pragma unroll
        for (int e = 0; e < NPAIR; ++e)
        {
            float lo = o[g][2 * e] * alpha, hi = o[g][2 * e + 1] * alpha;
#pragma unroll
            for (int j = 0; j < PG; ++j)
            {
                lo = fmaf(ex[j], bf16_lo(vp[j][e]), lo);
                hi = fmaf(ex[j], bf16_hi(vp[j][e]), hi);
            }
            o[g][2 * e] = lo;
            o[g][2 * e + 1] = hi;
        }
    }
}

// the partial of (head, split): dst is its [HS + 4] row
template <int HS, int FE, bool SC1>
__device__ __forceinline__ void decode_store_partial(float* dst, const float (&acc)[FE], float M, float L, int lane, bool owner)
{
    if (owner)
    {
#pragma unroll
        for (int e = 0; e < FE; ++e) partial_st<SC1>(dst + lane * FE + e, acc[e]);
    }
    if (lane == 0) { partial_st<SC1>(dst + HS, M); partial_st<SC1>(dst + HS + 1, L); }
}

// What follows the loop: the lane segments' states (m, l, O) become Y or the split's partial.  sm: [8][GH][HS + 2] floats of LDS.  Contains one workgroup barrier:
// every thread of the workgroup must call it.
template <int HS, int GH, class Row>
__device__ __forceinline__ void decode_finish(const DecodeFinishArgs& a, float (&m)[GH], float (&l)[GH], float (&o)[GH][Row::EPL], float* sm)
{
    constexpr int NW = kDecodeWaves, EPL = Row::EPL, LPR = Row::LPR, RPW = Row::RPW, FE = Row::FE, STR = HS + 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = RPW > 1 ? lane / LPR : 0, ll = RPW > 1 ? lane % LPR : lane;      // the lane segment (the row of a wave-instruction), the lane within it
    const bool owner = Row::ACTIVE == LPR || ll < Row::ACTIVE;                       // the lane owns elements of its rows
    // ---- merge the RPW lane segments of the wave in registers: afterwards every segment holds the wave's state ----
    if constexpr (RPW > 1)
    {
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1)
        {
#pragma unroll
            for (int g = 0; g < GH; ++g)
            {
                const float mo = __shfl_xor(m[g], off, 64), lo_ = __shfl_xor(l[g], off, 64);
                const float M = fmaxf(m[g], mo);
                const float fa = (m[g] == -INFINITY) ? 0.0f : __expf(m[g] - M), fb = (mo == -INFINITY) ? 0.0f : __expf(mo - M);
                l[g] = l[g] * fa + lo_ * fb;
#pragma unroll
                for (int e = 0; e < EPL; ++e) o[g][e] = o[g][e] * fa + __shfl_xor(o[g][e], off, 64) * fb;
                m[g] = M;
            }
        }
    }

    // ---- merge the NW waves through LDS; wave w < GH finalises head w ----
#pragma unroll
    for (int g = 0; g < GH; ++g)
    {
        float* dst = sm + ((size_t)wave * GH + g) * STR;
        if (sub == 0 && owner)
        {
#pragma unroll
            for (int e = 0; e < EPL; ++e) dst[ll * EPL + e] = o[g][e];
        }
        if (lane == 0) { dst[HS] = m[g]; dst[HS + 1] = l[g]; }
    }
    __syncthreads();
    if (wave < GH)
    {
        const int g = wave;
        const bool fin = FE * 64 == HS || lane < HS / FE;      // the lanes that own FE output elements each
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sm[((size_t)w * GH + g) * STR + HS]);
        float L = 0.0f, acc[FE];
#pragma unroll
        for (int e = 0; e < FE; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w)
        {
            const float* src = sm + ((size_t)w * GH + g) * STR;
            const float mw = src[HS];
            const float f = (mw == -INFINITY) ? 0.0f : __expf(mw - M);
            L += src[HS + 1] * f;
            if (fin)
            {
#pragma unroll
                for (int e = 0; e < FE; ++e) acc[e] += src[lane * FE + e] * f;
            }
        }
        const int h = a.h0 + g;
        if (a.splits == 1)
        {
            const float inv = (L > 0.0f) ? 1.0f / L : 0.0f;
            uint16_t* y = a.Y + ((size_t)a.b * a.NH + h) * HS + lane * FE;
            if constexpr (FE == 1)
                y[0] = f32_to_bf16_bits(acc[0] * inv);
            else if (fin)
            {
#pragma unroll
                for (int e = 0; e < FE; e += 2) *reinterpret_cast<uint32_t*>(y + e) = pack_bf16x2(acc[e] * inv, acc[e + 1] * inv);
            }
        }
        else
        {
            float* dst = a.scratch + (((size_t)a.b * a.NH + h) * a.splits + a.split) * (HS + 4);
            if (!a.write_through)
                decode_store_partial<HS, FE, false>(dst, acc, M, L, lane, fin);
            else
            {
                // one-pass form: write-through (sc1) stores, drained by this wave before the workgroup's arrival is counted
                decode_store_partial<HS, FE, true>(dst, acc, M, L, lane, fin);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
    }
}

}  // namespace mila
