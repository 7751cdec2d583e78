// The tile body of the long-context matrix-core decode, shared by its two kernels: attn_decode_mfma_kernel (attention.hip, bf16 cache) and
// attn_decode_kvfp8_mfma_kernel (attention_kvfp8.hip, e4m3 cache + one fp32 scale per row).  A STAGING POLICY says how a 32-key tile of K and V gets from the cache
// into the two LDS images of attention_tiles.h (global -> registers -> LDS) and how many tiles it keeps in flight; from LDS on -- S^T = K Q^T, the in-lane softmax,
// P rounded to bf16, O^T += V^T P^T, the partial layout O | M | L -- there is one body, so both caches reduce the same values in the same order: the fp8 cache's
// result is bit for bit the bf16 kernel's on a bf16 cache that holds the dequantized values.
#pragma once
#include "attention_tiles.h"
#include "fp8_quant.h"

namespace mila {

// what the body reads of a kernel's parameter block
struct MfmaDecodeArgs
{
    const uint16_t* Q;        // [B, NH*HS]
    int64_t q_b_stride;       // elements between two batches' query rows (0 = NH*HS)
    float* scratch;           // [B, NH, splits, HS+4] partials: O (HS) | M | L | pad
    int NH, NKV, capacity, len, window, splits;      // len: the live length (position + 1), already read from the device in the device-position forms
    float scale;
};

// ---- staging policies: load(regs, kt) requests tile kt's chunks of this thread, store(regs, ldsK, ldsV) writes them into the images.  `end` is the split's end,
// `wraps` (uniform) says whether its rows need the ring's modulo.  Rows past the split's end re-read its last key: a real row (masked score, finite V). ----

// bf16 cache: 16-byte chunks of K and V rows, stored as loaded; two tiles in flight (64 staging registers each)
template <int HS>
struct MfmaStageBf16
{
    static constexpr int kDepth = 2;
    static constexpr int ROWB = HS * 2;
    static constexpr int CH = (kKeysPerTile * (ROWB / 16)) / 256;      // 16-byte chunks each thread stages per tile and operand
    const uint16_t* kbase;                                              // the (batch, KV head)'s rows
    const uint16_t* vbase;
    struct Regs { u32x4 k[CH], v[CH]; };

    __device__ __forceinline__ MfmaStageBf16 at(size_t first_row) const { return MfmaStageBf16{kbase + first_row * HS, vbase + first_row * HS}; }
    __device__ __forceinline__ void load(Regs& r, int kt, int end, bool wraps, int capacity, int tid) const
    {
#pragma unroll
        for (int i = 0; i < CH; ++i)
        {
            const int c = tid + 256 * i;
            const int row = c / (ROWB / 16), ch = c % (ROWB / 16);
            const int key = min(kt + row, end - 1);                 // rows past the split re-read its last key (masked below; a real, finite V row)
            const size_t off = (size_t)(wraps ? key % capacity : key) * HS + ch * 8;
            r.k[i] = ld16(kbase + off);
            r.v[i] = ld16(vbase + off);
        }
    }
    __device__ __forceinline__ void store(const Regs& r, unsigned char* ldsK, unsigned char* ldsV, int tid) const
    {
#pragma unroll
        for (int i = 0; i < CH; ++i)
        {
            const int c = tid + 256 * i;
            const int row = c / (ROWB / 16), ch = c % (ROWB / 16);
            *reinterpret_cast<u32x4*>(ldsK + k_off<HS>(row, ch)) = r.k[i];
            *reinterpret_cast<u32x4*>(ldsV + v_off<HS>(row, ch)) = r.v[i];
        }
    }
};

// e4m3 cache: a 16-byte chunk is 16 elements, so a thread stages HALF the chunks of the bf16 policy (4 per operand and tile at HS 512) plus the fp32 scale of each
// chunk's row (one address per 32 lanes: a broadcast load): 20 registers per operand and tile against 32.  The saving buys a THIRD tile in flight -- the kernel is a
// latency chain of 4-8 tiles per split, and 3 x 16 loads stay below the 63 a wave can have outstanding (a fourth set would not).  On the way into LDS a chunk is
// converted with e4m3x4_to_bf16x4 -- the cached value bf16_rne(float(e4m3) * scale) of the policy, the bits dequantize_to_bf16 gives -- and becomes the two adjacent
// bf16 chunks 2 ch, 2 ch + 1 of its row in the SAME images.  Store banking (MI355X_MICROARCH.md, LDS: ds_write_b128 is served in 8 groups of 8 contiguous lanes over
// 32 banks): the 8 lanes of a group hold 8 consecutive e4m3 chunks of one row, so one store instruction writes every second bf16 chunk of a 256-byte stretch -- the
// XOR of k_off / v_off permutes chunks inside 16, it cannot change that -- and lanes j, j + 4 of a group meet: 2-way, 16 LDS-array cycles against the 13 the
// instruction's data transfer takes anyway, 3 cycles on each of 16 stores per tile.  Undoing it means swapping the halves a lane converts first (4 selects per chunk,
// 32 vector instructions per tile and thread): dearer than what it saves, so the halves go out in order.
template <int HS>
struct MfmaStageKvFp8
{
    static constexpr int kDepth = 3;
    static constexpr int CPR = HS / 16;                                 // e4m3 chunks per row
    static constexpr int CH = (kKeysPerTile * CPR) / 256;
    const uint8_t* k8;                                                  // the (batch, KV head)'s rows
    const uint8_t* v8;
    const float* ks;
    const float* vs;
    struct Regs { u32x4 k[CH], v[CH]; float ks[CH], vs[CH]; };

    __device__ __forceinline__ MfmaStageKvFp8 at(size_t first_row) const { return MfmaStageKvFp8{k8 + first_row * HS, v8 + first_row * HS, ks + first_row, vs + first_row}; }
    __device__ __forceinline__ void load(Regs& r, int kt, int end, bool wraps, int capacity, int tid) const
    {
#pragma unroll
        for (int i = 0; i < CH; ++i)
        {
            const int c = tid + 256 * i;
            const int row = c / CPR, ch = c % CPR;
            const int key = min(kt + row, end - 1);                 // a live row always: a dead row's bytes and scale are never read
            const size_t rr = (size_t)(wraps ? key % capacity : key);
            r.k[i] = ld16(k8 + rr * HS + ch * 16);
            r.v[i] = ld16(v8 + rr * HS + ch * 16);
            r.ks[i] = ks[rr];
            r.vs[i] = vs[rr];
        }
    }
    __device__ __forceinline__ void store(const Regs& r, unsigned char* ldsK, unsigned char* ldsV, int tid) const
    {
#pragma unroll
        for (int i = 0; i < CH; ++i)
        {
            const int c = tid + 256 * i;
            const int row = c / CPR, ch = c % CPR;
            uint32_t a[8], b[8];
#pragma unroll
            for (int d = 0; d < 4; ++d)
            {
                e4m3x4_to_bf16x4(r.k[i][d], r.ks[i], a[2 * d], a[2 * d + 1]);
                e4m3x4_to_bf16x4(r.v[i][d], r.vs[i], b[2 * d], b[2 * d + 1]);
            }
            *reinterpret_cast<u32x4*>(ldsK + k_off<HS>(row, 2 * ch)) = u32x4{a[0], a[1], a[2], a[3]};
            *reinterpret_cast<u32x4*>(ldsK + k_off<HS>(row, 2 * ch + 1)) = u32x4{a[4], a[5], a[6], a[7]};
            *reinterpret_cast<u32x4*>(ldsV + v_off<HS>(row, 2 * ch)) = u32x4{b[0], b[1], b[2], b[3]};
            *reinterpret_cast<u32x4*>(ldsV + v_off<HS>(row, 2 * ch + 1)) = u32x4{b[4], b[5], b[6], b[7]};
        }
    }
};

// dynamic LDS of a launch: two [K | V] tile pairs + the 16 heads' Q rows (144 KB at HS 512), whatever the staging policy
template <int HS>
constexpr size_t mfma_decode_lds_bytes() { return 4 * (size_t)kKeysPerTile * HS * 2 + 16 * (size_t)HS * 2; }

// One workgroup (256 threads) = one split of the keys for the 16 query heads of one head group on one KV head; grid (splits, NKV * GS / 16, B).  `stage` addresses
// the whole cache; the body moves it to its (batch, KV head).  Gemma's global layers put 16 query heads on ONE KV head: at one decode position those 16 heads ARE a
// 16-row MFMA tile, and K / V rows are shared by all of them.  K / V tiles of 32 keys go global -> registers -> LDS (double-buffered images, the next tiles' loads
// in flight during this tile's products), S^T = K Q^T and O^T += V^T P^T run as in the flash prefill (transposed products: a head's keys sit in its lane's
// registers, the row statistics are in-lane plus two permlane steps, the exponentiated scores ARE the second product's B operand).  The four waves split the OUTPUT
// dimensions (each computes the whole S^T and softmax of the tile -- identical in all four -- and a quarter of O^T: 32 accumulator registers).
// CHAIN: batch row b reads the cache of batch row 0 (p.len is its own live length; fused_attn_decode_chain_bf16).
template <int HS, class Stage, bool CHAIN = false>
__device__ __forceinline__ void attn_decode_mfma_body(const MfmaDecodeArgs& p, const Stage& cache, unsigned char* smem_mfma)
{
    constexpr int KSTEPS = HS / 32, DT = HS / 16, DTW = DT / 4;
    constexpr int ROWB = HS * 2, TILE_BYTES = kKeysPerTile * ROWB;
    constexpr int DEPTH = Stage::kDepth;
    static_assert(DEPTH == 2 || DEPTH == 3, "two or three staging sets");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int GS = p.NH / p.NKV, n16 = GS / 16;
    const int split = blockIdx.x, kvh = blockIdx.y / n16, h0 = kvh * GS + (blockIdx.y % n16) * 16, b = blockIdx.z;
    const int len = p.len;
    const int band_begin = (p.window > 0) ? max(0, len - p.window) : 0;
    const int band = len - band_begin;
    const int chunk = (band + p.splits - 1) / p.splits;
    const int begin = band_begin + split * chunk;
    const int end = min(begin + chunk, len);
    float* part = p.scratch + (((size_t)b * p.NH + h0 + l15) * p.splits + split) * (HS + 4);      // this lane's head row

    f32x4 o[DTW];
#pragma unroll
    for (int d = 0; d < DTW; ++d) o[d] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m_run = -INFINITY, l_run = 0.0f;

    if (begin < end)      // workgroup-uniform
    {
        // Q: the 16 heads' rows as a 16-row image in LDS (the layout of a K tile's first 16 rows); the fragments of a k-step are read per tile -- held in registers they
        // cost 64 VGPRs, which buy the second staging set (two tiles of K / V in flight per workgroup instead of one: the kernel is a latency chain of 4-8 tiles)
        unsigned char* ldsQ = smem_mfma + 4 * TILE_BYTES;
        {
            const uint16_t* qb = p.Q + (size_t)b * (p.q_b_stride ? (size_t)p.q_b_stride : (size_t)p.NH * HS) + (size_t)h0 * HS;
#pragma unroll
            for (int i = 0; i < (16 * (ROWB / 16)) / 256; ++i)
            {
                const int c = tid + 256 * i;
                const int row = c / (ROWB / 16), ch = c % (ROWB / 16);
                *reinterpret_cast<u32x4*>(ldsQ + k_off<HS>(row, ch)) = ld16(qb + (size_t)row * HS + ch * 8);
            }
        }
        const Stage st = cache.at(((size_t)(CHAIN ? 0 : b) * p.NKV + kvh) * p.capacity);
        const bool wraps = end > p.capacity;                          // uniform: an unbounded cache (the global layers) needs no modulo per row
        const int ntiles = (end - begin + kKeysPerTile - 1) / kKeysPerTile;
        const int kt_last = begin + (ntiles - 1) * kKeysPerTile;
        // a load past the last tile re-reads it (never stored): branch-free, the waits stay counted
        auto stage_load = [&](typename Stage::Regs& r, int kt) { st.load(r, min(kt, kt_last), end, wraps, p.capacity, tid); };
        typename Stage::Regs ra, rb, rc;                              // (rc: the three-deep policies only)
        stage_load(ra, begin);
        stage_load(rb, begin + kKeysPerTile);
        if constexpr (DEPTH == 3) stage_load(rc, begin + 2 * kKeysPerTile);
        auto tile = [&](int t, typename Stage::Regs& regs) {
            const int kt = begin + t * kKeysPerTile;
            // two [K | V] buffers: tile t is stored while slower waves may still read tile t - 1 from the other one (the store follows the barrier of tile t - 1,
            // which every wave reaches only after its reads of tile t - 2): one barrier per tile, which also publishes the Q image before its first read
            unsigned char* ldsK = smem_mfma + (t & 1) * 2 * TILE_BYTES;
            unsigned char* ldsV = ldsK + TILE_BYTES;
            st.store(regs, ldsK, ldsV, tid);
            __syncthreads();
            stage_load(regs, kt + DEPTH * kKeysPerTile);              // DEPTH tiles ahead, in flight during this tile's and the next ones' products

            f32x4 s0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s)
            {
                const s16x8 qf = *reinterpret_cast<const s16x8*>(ldsQ + k_off<HS>(l15, 4 * s + g));
                const s16x8 ka = *reinterpret_cast<const s16x8*>(ldsK + k_off<HS>(l15, 4 * s + g));
                const s16x8 kb = *reinterpret_cast<const s16x8*>(ldsK + k_off<HS>(16 + l15, 4 * s + g));
                s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ka), __builtin_bit_cast(bf16x8, qf), s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kb), __builtin_bit_cast(bf16x8, qf), s1, 0, 0, 0);
            }
            // lane holds keys kt + 4 g + r (s0) and kt + 16 + 4 g + r (s1) of head row l15
            float sv[8], mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 8; ++r)
            {
                const int key = kt + ((r < 4) ? (4 * g + r) : (16 + 4 * g + (r - 4)));
                const float raw = (r < 4) ? s0[r] : s1[r - 4];
                sv[r] = (key < end) ? raw * p.scale : -INFINITY;
                mt = fmaxf(mt, sv[r]);
            }
            mt = quad_rows_max(mt);
            const float mn = fmaxf(m_run, mt);                      // finite: every tile holds at least one key of the split
            const float alpha = __expf(m_run - mn);                 // m_run = -inf -> 0
            float pe[8], rs = 0.0f;
#pragma unroll
            for (int r = 0; r < 8; ++r)
            {
                pe[r] = __expf(sv[r] - mn);
                rs += pe[r];
            }
            rs = quad_rows_sum(rs);
            l_run = l_run * alpha + rs;
            m_run = mn;
            u32x4 pb;
            pb[0] = pack_bf16x2(pe[0], pe[1]);
            pb[1] = pack_bf16x2(pe[2], pe[3]);
            pb[2] = pack_bf16x2(pe[4], pe[5]);
            pb[3] = pack_bf16x2(pe[6], pe[7]);
            const bf16x8 pfrag = __builtin_bit_cast(bf16x8, pb);
            const bool rescale = __any(alpha != 1.0f);
#pragma unroll
            for (int dd = 0; dd < DTW; ++dd)
            {
                const int d = wave * DTW + dd;
                const int q4 = l15 >> 2, pp = l15 & 3;
                const int col = 16 * d + 4 * pp;
                const int r_lo = 4 * g + q4, r_hi = 16 + 4 * g + q4;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(ldsV + v_off<HS>(r_lo, col >> 3) + ((col & 7) << 1)));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(ldsV + v_off<HS>(r_hi, col >> 3) + ((col & 7) << 1)));
                s16x8 va;
                va[0] = lo[0]; va[1] = lo[1]; va[2] = lo[2]; va[3] = lo[3];
                va[4] = hi[0]; va[5] = hi[1]; va[6] = hi[2]; va[7] = hi[3];
                if (rescale) { o[dd][0] *= alpha; o[dd][1] *= alpha; o[dd][2] *= alpha; o[dd][3] *= alpha; }
                o[dd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, va), pfrag, o[dd], 0, 0, 0);
            }
        };
        for (int t = 0; t < ntiles; t += DEPTH)
        {
            tile(t, ra);
            if (t + 1 < ntiles) tile(t + 1, rb);
            if constexpr (DEPTH == 3)
                if (t + 2 < ntiles) tile(t + 2, rc);
        }
    }
    // O^T[dim 16 d + 4 g + r][head l15] -> this head's partial row; (M, L) once per head (an empty split leaves O = 0, M = -inf, L = 0: the merge ignores it)
#pragma unroll
    for (int dd = 0; dd < DTW; ++dd) *reinterpret_cast<f32x4*>(part + 16 * (wave * DTW + dd) + 4 * g) = o[dd];
    if (wave == 0 && g == 0) { part[HS] = m_run; part[HS + 1] = l_run; }
}

}  // namespace mila
