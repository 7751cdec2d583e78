// Grouped-query attention over an FP8 KV cache: the PerChannelKvFp8<> policy of the reference (Quantization/KvCache/QuantPolicy.ixx:56-88 declares it -- e4m3 storage of
// K and V, one fp32 scale per KV head per cached token, absmax / 448, "dequantized to transient BF16 buffers ... never written back"; BACKLOG.md names the missing
// OperationTraits<GqaOp, Cuda, BF16, PerChannelKvFp8<>> row -- the reference has the policy type and no kernels).
//
//   layout   K8, V8 [B, NKV, capacity, HS] uint8, Ks, Vs [B, NKV, capacity] fp32; row = abs_pos % capacity (the bf16 cache's ring rule, Gqa.Cache.Bf16.cu:86-130)
//   write    a K / V row of one (batch, token, KV head) is quantized as quantize_fp8_per_channel quantizes a weight row (fp8_quant.h): bit-identical bytes and scales
//   read     a cached value is bf16_rne(float(e4m3) * scale) -- the bits dequantize_to_bf16 produces -- in the decode kernel's registers, or in a transient bf16
//            cache for the prefill, which then runs the bf16 flash kernels: both see the same K / V values, the attention arithmetic is the bf16 cache's.
//
// Decode (the hot path), two kernels chosen by attention.hip's plan_decode exactly as it chooses between the bf16 cache's two:
//   attn_decode_kvfp8_kernel       the split-K wave-per-position decode (Gqa.Decode.Bf16.cu:93-105, :212, :297-351): its own row loop (one byte per element + the row's
//     scale, dequantized in registers; a row is HS / 4 lanes wide, so a wave-instruction fetches 1, 2 or 4 rows: DecodeGeomKvFp8) around the phases of
//     attention_decode_scalar.h that attention.hip's attn_decode_kernel runs too: softmax step, both merges, finaliser, stores.  The splits are merged by attention.hip's combine kernel from partials in its layout.
//   attn_decode_kvfp8_mfma_kernel  16 query heads on one KV head at HS 512 over a long band (from the 8192-key bucket): the matrix-core decode -- the tile body of
//     attention_decode_mfma.h under the e4m3 staging policy (16-byte e4m3 chunks + row scales -> registers -> bf16 values in the bf16 kernel's LDS images), up to 256
//     splits merged by attn_combine_many_kernel.  From LDS on it IS attn_decode_mfma_kernel: the same bits as attn_decode_bf16 on the dequantized cache.
// Both take the live length either as a launch argument or (the device-position entries, for graph replay) from device memory.
//
// What this file owns: the quantizing append, the band dequant and the prefill over a transient bf16 cache; the two kernels above (the scalar one's row loop, the matrix-core one's wrapper)
// with their parameter block and launches; the fp8 entry points and their checks.  The arithmetic from the scores on (attention_decode_scalar.h), the matrix-core tile
// body (attention_decode_mfma.h), the plan and the
// (HS, heads per workgroup) dispatch (attention_decode_plan.h) are shared with the bf16 cache.
#include "attention_decode_mfma.h"
#include "attention_decode_plan.h"
#include "attention_decode_scalar.h"
#include "attention_tiles.h"      // kKeysPerTile: the flash prefill streams whole key tiles
#include "fp8_quant.h"

namespace mila {

// ---- quantizing KV append ---------------------------------------------------------------------------------------------------------------------------------------
// one wave per (K | V, batch, token, KV head) row: lanes below HS / EPL own EPL consecutive elements, the absmax is a wave reduction (exact, any order)
template <int HS>
__global__ __launch_bounds__(256) void kv_write_fp8_kernel(const int32_t* __restrict__ pos_dev, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                           uint8_t* __restrict__ K8, uint8_t* __restrict__ V8, int chunk, int NKV, int capacity, int start_pos,
                                                           int64_t rows, float* __restrict__ Ks, float* __restrict__ Vs)
{
    // (argument order: the position word, the source rows and what the row addresses derive from lead -- the 14 dwords the dispatcher preloads into SGPRs, build.py)
    constexpr int EPL = HS >= 512 ? 8 : 4, ACTIVE = HS / EPL;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform
    if (w >= 2 * rows) return;
    const bool is_v = w >= rows;
    int64_t r = is_v ? w - rows : w;                                     // source order [b, t, nkv]
    const int n = (int)(r % NKV);
    r /= NKV;
    const int t = (int)(r % chunk), b = (int)(r / chunk);
    const uint16_t* src = (is_v ? v : k) + (((size_t)b * chunk + t) * NKV + n) * HS;
    const int first = pos_dev ? *pos_dev : start_pos;                    // (the device-position form appends one token at *pos_dev)
    const size_t drow = ((size_t)b * NKV + n) * capacity + (size_t)((first + t) % capacity);
    const bool act = lane < ACTIVE;
    uint32_t x[EPL / 2];
#pragma unroll
    for (int e = 0; e < EPL / 2; ++e) x[e] = 0u;
    if (act)
    {
        if constexpr (EPL == 8)
        {
            const u32x4 q = ld16(src + lane * 8);
            x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3];
        }
        else
        {
            const u32x2 q = *reinterpret_cast<const u32x2*>(src + lane * 4);
            x[0] = q[0]; x[1] = q[1];
        }
    }
    float m = 0.0f;
#pragma unroll
    for (int e = 0; e < EPL / 2; ++e) m = fmaxf(m, fmaxf(fabsf(bf16_lo(x[e])), fabsf(bf16_hi(x[e]))));
    const float scale = fp8_row_scale(wave_max(m));
    const float inv = 1.0f / scale;
    if (lane == 0) (is_v ? Vs : Ks)[drow] = scale;
    if (act)
    {
        uint8_t* dst = (is_v ? V8 : K8) + drow * HS + lane * EPL;
        if constexpr (EPL == 8)
            *reinterpret_cast<u32x2*>(dst) = u32x2{bf16x4_to_e4m3x4(x[0], x[1], inv), bf16x4_to_e4m3x4(x[2], x[3], inv)};
        else
            *reinterpret_cast<uint32_t*>(dst) = bf16x4_to_e4m3x4(x[0], x[1], inv);
    }
}

// ---- band dequant (the prefill's transient bf16 cache) ------------------------------------------------------------------------------------------------------------
// rows of positions [first_pos, first_pos + count) of every (batch, KV head), K and V: one thread per 16 bytes -> 16 bf16 at the same row index of the destination
__global__ __launch_bounds__(256) void kv_dequant_fp8_kernel(uint16_t* __restrict__ Kd, uint16_t* __restrict__ Vd, const uint8_t* __restrict__ K8,
                                                             const uint8_t* __restrict__ V8, const float* __restrict__ Ks, const float* __restrict__ Vs,
                                                             int64_t total_vec, int HS, int capacity, int first_pos, int count)
{
    const int hv = HS / 16;
    const int64_t stride = (int64_t)gridDim.x * 256, half = total_vec / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_vec; i += stride)
    {
        const bool is_v = i >= half;
        int64_t r = is_v ? i - half : i;
        const int e = (int)(r % hv);
        r /= hv;
        const int t = (int)(r % count);
        const int64_t head = r / count;                                  // b * NKV + kv head
        const size_t row = (size_t)head * capacity + (size_t)((first_pos + t) % capacity);
        const float sc = (is_v ? Vs : Ks)[row];
        const u32x4 w = ld16((is_v ? V8 : K8) + row * HS + (size_t)e * 16);
        uint32_t o[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) e4m3x4_to_bf16x4(w[d], sc, o[2 * d], o[2 * d + 1]);
        uint16_t* dst = (is_v ? Vd : Kd) + row * HS + (size_t)e * 16;
        st16(dst, u32x4{o[0], o[1], o[2], o[3]});
        st16(dst + 8, u32x4{o[4], o[5], o[6], o[7]});
    }
}

// ---- decode attention -----------------------------------------------------------------------------------------------------------------------------------------
struct KvFp8DecodeParams
{
    uint16_t* Y;              // [B, NH*HS]
    const uint16_t* Q;        // [B, NH*HS]
    const uint8_t* K8;        // [B, NKV, capacity, HS] e4m3
    const uint8_t* V8;
    const float* Ks;          // [B, NKV, capacity]
    const float* Vs;
    float* scratch;           // [B, NH, splits, HS+4] partials when splits > 1 (attention.hip's layout)
    int NH, NKV, capacity, len, window, splits;
    float scale;
    const int32_t* pos_dev;   // when set: len = *pos_dev + 1, read by the kernels (graph replay); null in the eager form
};

// GH = query heads per workgroup; grid = (splits, NKV * GS/GH, B).  Wave w, lane segment s own positions begin + (w * RPW + s) + 8 * RPW * j of the split.
//
// Arguments, as attn_decode_kernel's (attention.hip): what the chain kernel arguments -> *pos_dev -> band and row addresses -> first K/V request reads comes as leading
// plain parameters (13 dwords, preloaded into SGPRs by the dispatcher); the tail is the launcher's whole parameter block, whose copies of those fields are never read.
#define MILA_KVFP8_LEAD_PARAMS const int32_t* pos_dev, const uint8_t* K8, const uint8_t* V8, const float* Ks, int NH, int NKV, int capacity, int window, int splits
#define MILA_KVFP8_LEAD_ARGS(p) (p).pos_dev, (p).K8, (p).V8, (p).Ks, (p).NH, (p).NKV, (p).capacity, (p).window, (p).splits
__device__ __forceinline__ KvFp8DecodeParams kvfp8_params(MILA_KVFP8_LEAD_PARAMS, const KvFp8DecodeParams& tail)
{
    KvFp8DecodeParams p = tail;
    p.pos_dev = pos_dev; p.K8 = K8; p.V8 = V8; p.Ks = Ks;
    p.NH = NH; p.NKV = NKV; p.capacity = capacity; p.window = window; p.splits = splits;
    return p;
}

// ROWS (attn_decode_kvfp8_rows): the batch rows are independent sequences -- row b = blockIdx.z attends over pos_dev[b] + 1 keys of its own caches; everything else
// (the band, the splits, the partial layout) is the one-row kernel's, so a row has the bits it has alone.
template <int HS, int GH, bool ROWS = false>
__global__ __launch_bounds__(kDecodeWaves * 64) void attn_decode_kvfp8_kernel(MILA_KVFP8_LEAD_PARAMS, const KvFp8DecodeParams tail)
{
    const KvFp8DecodeParams p = kvfp8_params(pos_dev, K8, V8, Ks, NH, NKV, capacity, window, splits, tail);
    using Row = DecodeGeomKvFp8<HS>;
    constexpr int NW = kDecodeWaves, EPL = Row::EPL, ND = Row::ND, NPAIR = Row::NPAIR, LPR = Row::LPR, RPW = Row::RPW, PG = Row::PG;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_kvfp8[];
    float* sm = reinterpret_cast<float*>(smem_kvfp8);      // [NW][GH][HS + 2]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, ll = lane % LPR;
    const int GS = p.NH / p.NKV, hgroups = GS / GH;
    const int split = blockIdx.x, grp = blockIdx.y;
    const int kvh = grp / hgroups, hg = grp % hgroups;
    const int h0 = kvh * GS + hg * GH;                     // first query head of this workgroup
    const int b = blockIdx.z;
    const int len = ROWS ? p.pos_dev[b] + 1 : (p.pos_dev ? *p.pos_dev + 1 : p.len);
    const int band_begin = (p.window > 0) ? max(0, len - p.window) : 0;
    const int band = len - band_begin;
    const int chunk = (band + p.splits - 1) / p.splits;
    const int begin = band_begin + split * chunk;
    const int end = min(begin + chunk, len);      // (a split past the live band: begin >= end, nothing is loaded, its partial is O = 0, M = -inf, L = 0)

    const size_t head = ((size_t)b * p.NKV + kvh) * p.capacity;
    const uint8_t* kbase = p.K8 + head * HS + ll * EPL;
    const uint8_t* vbase = p.V8 + head * HS + ll * EPL;
    const float* ksb = p.Ks + head;
    const float* vsb = p.Vs + head;

    struct KVG { uint32_t k[PG][ND], v[PG][ND]; float ks[PG], vs[PG]; };
    // wbase: the wave's first position of the group (wave-uniform); a lane's own rows are wbase + sub + NW * RPW * j
    auto load_group = [&](KVG& g, int wbase) {
#pragma unroll
        for (int j = 0; j < PG; ++j)
        {
            const int pp = wbase + sub + NW * RPW * j;
            if (pp < end)
            {
                const size_t r = (size_t)(pp % p.capacity);
                if constexpr (ND == 2)
                {
                    const u32x2 a = *reinterpret_cast<const u32x2*>(kbase + r * HS), c = *reinterpret_cast<const u32x2*>(vbase + r * HS);
                    g.k[j][0] = a[0]; g.k[j][1] = a[1]; g.v[j][0] = c[0]; g.v[j][1] = c[1];
                }
                else
                {
                    g.k[j][0] = *reinterpret_cast<const uint32_t*>(kbase + r * HS);
                    g.v[j][0] = *reinterpret_cast<const uint32_t*>(vbase + r * HS);
                }
                g.ks[j] = ksb[r];                          // one address per segment: a broadcast load
                g.vs[j] = vsb[r];
            }
            else
            {
#pragma unroll
                for (int e = 0; e < ND; ++e) { g.k[j][e] = 0u; g.v[j][e] = 0u; }
                g.ks[j] = 0.0f;
                g.vs[j] = 0.0f;
            }
        }
    };

    int base = begin + wave * RPW;
    KVG ga, gb;
    if (base < end) load_group(ga, base);                  // in flight while q is fetched

    uint32_t q[GH][NPAIR];
#pragma unroll
    for (int g = 0; g < GH; ++g)
    {
        const uint16_t* qp = p.Q + ((size_t)b * p.NH + h0 + g) * HS + ll * EPL;
        if constexpr (EPL == 8)
        {
            const u32x4 t = ld16(qp);
            q[g][0] = t[0]; q[g][1] = t[1]; q[g][2] = t[2]; q[g][3] = t[3];
        }
        else
        {
            const u32x2 t = *reinterpret_cast<const u32x2*>(qp);
            q[g][0] = t[0]; q[g][1] = t[1];
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

    auto compute_group = [&](const KVG& gbuf, int wbase) {
        float sc[PG][GH];
        uint32_t vp[PG][NPAIR];
#pragma unroll
        for (int j = 0; j < PG; ++j)
        {
            // the cached values, bf16_rne(float(e4m3) * scale), as packed bf16 pairs
            uint32_t kp[NPAIR];
#pragma unroll
            for (int d = 0; d < ND; ++d)
            {
                e4m3x4_to_bf16x4(gbuf.k[j][d], gbuf.ks[j], kp[2 * d], kp[2 * d + 1]);
                e4m3x4_to_bf16x4(gbuf.v[j][d], gbuf.vs[j], vp[j][2 * d], vp[j][2 * d + 1]);
            }
#pragma unroll
            for (int g = 0; g < GH; ++g)
            {
                float a = 0.0f;
#pragma unroll
                for (int e = 0; e < NPAIR; ++e) a = dot2_bf16(as_bf16x2(q[g][e]), as_bf16x2(kp[e]), a);
                sc[j][g] = a;
            }
        }
        decode_softmax_step<GH, Row>(sc, vp, m, l, o, wbase + sub, end, p.scale);
    };
    for (;;)                                               // (wave-uniform control: `base` is the wave's, not the lane segment's)
    {
        if (base >= end) break;
        int nb = base + NW * RPW * PG;
        if (nb < end) load_group(gb, nb);
        compute_group(ga, base);
        base = nb;
        if (base >= end) break;
        nb = base + NW * RPW * PG;
        if (nb < end) load_group(ga, nb);
        compute_group(gb, base);
        base = nb;
    }

    const DecodeFinishArgs a{p.Y, p.scratch, p.NH, p.splits, split, b, h0, false};
    decode_finish<HS, GH, Row>(a, m, l, o, sm);
}

template <int HS, int GH, bool ROWS = false>
static int launch_decode_kvfp8(const KvFp8DecodeParams& p, int B, int hgroups, hipStream_t s)
{
    note_form("attn_decode_kvfp8");
    const size_t lds = (size_t)kDecodeWaves * GH * (HS + 2) * sizeof(float);      // <= 33 KB (HS 256 x 4 heads, HS 512 x 2)
    hipLaunchKernelGGL((attn_decode_kvfp8_kernel<HS, GH, ROWS>), dim3(p.splits, p.NKV * hgroups, B), dim3(kDecodeWaves * 64), lds, s, MILA_KVFP8_LEAD_ARGS(p), p);
    int rc = check_hip(hipGetLastError(), "attn_decode_kvfp8");
    if (rc || p.splits <= 1) return rc;
    return launch_attn_combine(p.Y, p.scratch, B, p.NH, HS, p.splits, s);
}

// ---- the matrix-core decode (attention_decode_mfma.h): grid (splits, NKV * GS / 16, B), 256 threads ----
template <int HS, bool ROWS = false>
__global__ __launch_bounds__(256) void attn_decode_kvfp8_mfma_kernel(MILA_KVFP8_LEAD_PARAMS, const KvFp8DecodeParams tail)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_kvfp8_mfma[];
    const KvFp8DecodeParams p = kvfp8_params(pos_dev, K8, V8, Ks, NH, NKV, capacity, window, splits, tail);
    const int len = ROWS ? p.pos_dev[blockIdx.z] + 1 : (p.pos_dev ? *p.pos_dev + 1 : p.len);      // ROWS: row b = blockIdx.z of independent sequences, as above
    const MfmaDecodeArgs a{p.Q, 0, p.scratch, p.NH, p.NKV, p.capacity, len, p.window, p.splits, p.scale};
    attn_decode_mfma_body<HS>(a, MfmaStageKvFp8<HS>{p.K8, p.V8, p.Ks, p.Vs}, smem_kvfp8_mfma);
}
template <bool ROWS = false>
static int launch_decode_kvfp8_mfma(const KvFp8DecodeParams& p, int B, hipStream_t s)
{
    constexpr int HS = 512;
    note_form("attn_decode_kvfp8_mfma");
    static bool attr_set = false;
    const size_t lds = mfma_decode_lds_bytes<HS>();      // what attn_decode_mfma_kernel asks for: the images are the same
    if (!attr_set)
    {
        int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_decode_kvfp8_mfma_kernel<HS, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute(attn_decode_kvfp8_mfma)");
        if (rc) return rc;
        attr_set = true;
    }
    const int n16 = (p.NH / p.NKV) / 16;
    hipLaunchKernelGGL((attn_decode_kvfp8_mfma_kernel<HS, ROWS>), dim3(p.splits, p.NKV * n16, B), dim3(256), lds, s, MILA_KVFP8_LEAD_ARGS(p), p);
    int rc = check_hip(hipGetLastError(), "attn_decode_kvfp8_mfma");
    if (rc) return rc;
    return launch_attn_combine_many(p.Y, p.scratch, B, p.NH, HS, p.splits, s);
}

static size_t kvfp8_transient_bytes(int B, int NKV, int HS, int capacity) { return 2 * (size_t)B * NKV * capacity * HS * sizeof(uint16_t); }

}  // namespace mila

using namespace mila;

extern "C" {

// the append launch of both write entries: `chunk` tokens from start_pos, or (pos_dev) one token at *pos_dev
static int launch_kv_write_fp8(const char* who, uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* k, const uint16_t* v, int B, int chunk, int NKV, int HS, int start_pos,
                               const int32_t* pos_dev, int capacity, mila_stream_t stream)
{
    const int64_t rows = (int64_t)B * chunk * NKV;
    MILA_REQUIRE((2 * rows + 3) / 4 <= 0x7fffffffLL, "%s: too many rows for one launch", who);
    const dim3 grid((unsigned)((2 * rows + 3) / 4));
    hipStream_t s = as_stream(stream);
    switch (HS)
    {
        case 64: hipLaunchKernelGGL(kv_write_fp8_kernel<64>, grid, dim3(256), 0, s, pos_dev, k, v, K8, V8, chunk, NKV, capacity, start_pos, rows, Ks, Vs); break;
        case 128: hipLaunchKernelGGL(kv_write_fp8_kernel<128>, grid, dim3(256), 0, s, pos_dev, k, v, K8, V8, chunk, NKV, capacity, start_pos, rows, Ks, Vs); break;
        case 256: hipLaunchKernelGGL(kv_write_fp8_kernel<256>, grid, dim3(256), 0, s, pos_dev, k, v, K8, V8, chunk, NKV, capacity, start_pos, rows, Ks, Vs); break;
        default: hipLaunchKernelGGL(kv_write_fp8_kernel<512>, grid, dim3(256), 0, s, pos_dev, k, v, K8, V8, chunk, NKV, capacity, start_pos, rows, Ks, Vs); break;
    }
    return check_hip(hipGetLastError(), who);
}

int mila_cdna4_kv_write_fp8(uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* k, const uint16_t* v, int B, int chunk, int NKV, int HS, int start_pos,
                            int capacity, mila_stream_t stream)
{
    MILA_REQUIRE(K8 && V8 && Ks && Vs && k && v, "kv_write_fp8: null pointer");
    MILA_REQUIRE(B > 0 && chunk > 0 && NKV > 0 && capacity > 0, "kv_write_fp8: bad sizes");
    MILA_REQUIRE(decode_scalar_head_size(HS), "kv_write_fp8: HS=%d must be 64, 128, 256 or 512", HS);
    MILA_REQUIRE(start_pos >= 0, "kv_write_fp8: negative start position");
    MILA_REQUIRE(chunk <= capacity, "kv_write_fp8: chunk %d exceeds the cache capacity %d", chunk, capacity);
    return launch_kv_write_fp8("kv_write_fp8", K8, V8, Ks, Vs, k, v, B, chunk, NKV, HS, start_pos, nullptr, capacity, stream);
}

int mila_cdna4_kv_write_fp8_devpos(uint8_t* K8, uint8_t* V8, float* Ks, float* Vs, const uint16_t* k, const uint16_t* v, int B, int NKV, int HS, const int32_t* position_dev,
                                   int capacity, mila_stream_t stream)
{
    MILA_REQUIRE(K8 && V8 && Ks && Vs && k && v && position_dev, "kv_write_fp8_devpos: null pointer");
    MILA_REQUIRE(B > 0 && NKV > 0 && capacity > 0, "kv_write_fp8_devpos: bad sizes");
    MILA_REQUIRE(decode_scalar_head_size(HS), "kv_write_fp8_devpos: HS=%d must be 64, 128, 256 or 512", HS);
    return launch_kv_write_fp8("kv_write_fp8_devpos", K8, V8, Ks, Vs, k, v, B, 1, NKV, HS, 0, position_dev, capacity, stream);
}

int mila_cdna4_kv_dequant_fp8_bf16(uint16_t* Kc_bf16, uint16_t* Vc_bf16, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, int B, int NKV, int HS,
                                   int capacity, int first_pos, int count, mila_stream_t stream)
{
    MILA_REQUIRE(Kc_bf16 && Vc_bf16 && K8 && V8 && Ks && Vs, "kv_dequant_fp8_bf16: null pointer");
    MILA_REQUIRE(B > 0 && NKV > 0 && capacity > 0, "kv_dequant_fp8_bf16: bad sizes");
    MILA_REQUIRE(decode_scalar_head_size(HS), "kv_dequant_fp8_bf16: HS=%d must be 64, 128, 256 or 512", HS);
    MILA_REQUIRE(first_pos >= 0 && count > 0 && count <= capacity, "kv_dequant_fp8_bf16: positions [%d, %d + %d) do not fit the cache capacity %d", first_pos, first_pos,
                 count, capacity);
    const int64_t total_vec = 2 * (int64_t)B * NKV * count * (HS / 16);
    int blocks = ceil_div(total_vec, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(kv_dequant_fp8_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), Kc_bf16, Vc_bf16, K8, V8, Ks, Vs, total_vec, HS, capacity, first_pos, count);
    MILA_LAUNCH_CHECK("kv_dequant_fp8_bf16");
}

// what the two decode entries share: the checks (`who` names the entry in the messages; `len` is the live length of the eager entry, the captured bound max_len of
// the device-position one), the plan for that length's band bucket, the launch of the plan's form.  rows: pos_dev holds B words, row b's position at [b]; the plan
// is ONE row's (as fused_attn_decode_rows_bf16 plans), only the partials are sized for all B
static int kvfp8_decode(const char* who, uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch, size_t scratch_bytes,
                        int B, int NH, int NKV, int HS, int capacity, int len, const int32_t* pos_dev, int window, float scale, mila_stream_t stream, bool rows = false)
{
    MILA_REQUIRE(B > 0 && NH > 0 && NKV > 0 && NH % NKV == 0, "%s: bad head counts (NH=%d NKV=%d)", who, NH, NKV);
    MILA_REQUIRE(decode_scalar_head_size(HS), "%s: HS=%d must be 64, 128, 256 or 512", who, HS);
    const int GS = NH / NKV;
    MILA_REQUIRE(decode_group_size_ok(GS), "%s: group size %d (NH/NKV) must be 1,2,4,8,16 or 32", who, GS);
    MILA_REQUIRE(len > 0 && capacity > 0, "%s: %s and capacity must be positive (%s=%d capacity=%d)", who, pos_dev ? "max_len" : "len", pos_dev ? "max_len" : "len", len, capacity);
    MILA_REQUIRE(window >= 0, "%s: negative window", who);
    const int band = live_band(len, window);
    MILA_REQUIRE(band <= capacity, "%s: live band %d exceeds the cache capacity %d", who, band, capacity);
    KvFp8DecodeShape d = plan_decode_kvfp8(rows ? 1 : B, NH, NKV, HS, capacity, window, len);
    if (rows) d.scratch_need *= (size_t)B;      // partials [B, NH, splits, HS + 4]: no q rows in this plan (an unfused entry)
    MILA_REQUIRE(!d.scratch_need || (scratch && scratch_bytes >= d.scratch_need), "%s: scratch %zu bytes < required %zu (ask attn_decode_scratch_bytes)", who, scratch_bytes,
                 d.scratch_need);
    KvFp8DecodeParams p{Y, Q, K8, V8, Ks, Vs, reinterpret_cast<float*>(scratch), NH, NKV, capacity, len, window, d.splits, scale, pos_dev};
    hipStream_t s = as_stream(stream);
    if (d.mfma) return rows ? launch_decode_kvfp8_mfma<true>(p, B, s) : launch_decode_kvfp8_mfma<false>(p, B, s);      // (HS 512 by the plan's rule)
    // (<512, 4> runs only under the attn.heads_per_group_512 experiment, on the bf16 cache)
    const int rc = dispatch_decode_scalar<false>(HS, d.gh, [&](auto hs, auto g) {
        return rows ? launch_decode_kvfp8<decltype(hs)::value, decltype(g)::value, true>(p, B, d.hgroups, s)
                    : launch_decode_kvfp8<decltype(hs)::value, decltype(g)::value, false>(p, B, d.hgroups, s);
    });
    if (rc == kNoDecodeKernel) return set_error(MILA_E_UNSUPPORTED, "attn_decode_kvfp8: no kernel for %d heads per workgroup at HS=%d", d.gh, HS);
    return rc;
}

int mila_cdna4_attn_decode_kvfp8(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch, size_t scratch_bytes,
                                 int B, int NH, int NKV, int HS, int capacity, int len, int window, float scale, mila_stream_t stream)
{
    MILA_REQUIRE(Y && Q && K8 && V8 && Ks && Vs, "attn_decode_kvfp8: null pointer");
    return kvfp8_decode("attn_decode_kvfp8", Y, Q, K8, V8, Ks, Vs, scratch, scratch_bytes, B, NH, NKV, HS, capacity, len, nullptr, window, scale, stream);
}

int mila_cdna4_attn_decode_kvfp8_devpos(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch, size_t scratch_bytes,
                                        int B, int NH, int NKV, int HS, int capacity, const int32_t* position_dev, int max_len, int window, float scale, mila_stream_t stream)
{
    MILA_REQUIRE(Y && Q && K8 && V8 && Ks && Vs && position_dev, "attn_decode_kvfp8_devpos: null pointer");
    return kvfp8_decode("attn_decode_kvfp8_devpos", Y, Q, K8, V8, Ks, Vs, scratch, scratch_bytes, B, NH, NKV, HS, capacity, max_len, position_dev, window, scale, stream);
}

// attn_decode_kvfp8_devpos for B independent sequences (mila_cdna4.h).  The entry cannot see the device values: a positions_dev[b] outside [0, max_len) would read
// out of bounds or take a plan it was not captured for -- the caller keeps that invariant (GemmaTransformer: checkRowsStep, checkPosition).
int mila_cdna4_attn_decode_kvfp8_rows(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch, size_t scratch_bytes,
                                      int B, int NH, int NKV, int HS, int capacity, const int32_t* positions_dev, int max_len, int window, float scale, mila_stream_t stream)
{
    MILA_REQUIRE(Y && Q && K8 && V8 && Ks && Vs && positions_dev, "attn_decode_kvfp8_rows: null pointer");
    MILA_REQUIRE(B >= 2 && B <= 4, "attn_decode_kvfp8_rows: B=%d rows outside 2 .. 4", B);
    MILA_REQUIRE(max_len <= capacity, "attn_decode_kvfp8_rows: max_len %d beyond the capacity %d (a row's cache is unbounded: position p lives at cache row p)", max_len, capacity);
    return kvfp8_decode("attn_decode_kvfp8_rows", Y, Q, K8, V8, Ks, Vs, scratch, scratch_bytes, B, NH, NKV, HS, capacity, max_len, positions_dev, window, scale, stream, true);
}

size_t mila_cdna4_attn_prefill_kvfp8_scratch_bytes(int B, int NKV, int HS, int capacity)
{
    if (B <= 0 || NKV <= 0 || HS <= 0 || capacity <= 0) return 0;
    return kvfp8_transient_bytes(B, NKV, HS, capacity);
}

int mila_cdna4_attn_prefill_kvfp8(uint16_t* Y, const uint16_t* Q, const uint8_t* K8, const uint8_t* V8, const float* Ks, const float* Vs, void* scratch, size_t scratch_bytes,
                                  int B, int chunk, int NH, int NKV, int HS, int capacity, int pos_offset, int window, float scale, mila_stream_t stream)
{
    MILA_REQUIRE(Y && Q && K8 && V8 && Ks && Vs && scratch, "attn_prefill_kvfp8: null pointer");
    MILA_REQUIRE(B > 0 && chunk > 0 && NH > 0 && NKV > 0 && NH % NKV == 0, "attn_prefill_kvfp8: bad sizes");
    MILA_REQUIRE(decode_scalar_head_size(HS), "attn_prefill_kvfp8: HS=%d must be 64, 128, 256 or 512", HS);
    MILA_REQUIRE(pos_offset >= 0 && capacity > 0 && window >= 0, "attn_prefill_kvfp8: bad positions");
    // every key a query of this chunk may see must still be resident in the ring: the band [first, pos_offset + chunk)
    const int first = (window > 0) ? max(0, pos_offset - window + 1) : 0, count = pos_offset + chunk - first;
    MILA_REQUIRE(count <= capacity, "attn_prefill_kvfp8: keys [%d,%d] do not fit the cache capacity %d", first, pos_offset + chunk - 1, capacity);
    const size_t need = kvfp8_transient_bytes(B, NKV, HS, capacity);
    MILA_REQUIRE(scratch_bytes >= need, "attn_prefill_kvfp8: scratch %zu bytes < required %zu (ask attn_prefill_kvfp8_scratch_bytes)", scratch_bytes, need);
    MILA_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "attn_prefill_kvfp8: the scratch must be 16-byte aligned");
    // The transient bf16 caches, of the cache's own shape.  The flash kernels stream whole tiles of kKeysPerTile keys from the tile boundary at or below the band's
    // first key (attention_prefill.hip: kt0): the up to 31 rows in front of the band are multiplied by a probability of exactly zero, so they must hold finite
    // values -- the dequantized older tokens (or, in a ring too short to still hold them, the newer rows that took their place: the whole ring then).  Every other
    // row stays as it is: the kernels clamp their reads to the chunk's last key.
    const int end = pos_offset + chunk;
    int first_d = first & ~(kKeysPerTile - 1);
    if (end - first_d > capacity) first_d = end - capacity;      // (<= first, >= 0: count <= capacity <= end here)
    uint16_t* Kt = static_cast<uint16_t*>(scratch);
    uint16_t* Vt = Kt + (size_t)B * NKV * capacity * HS;
    int rc = mila_cdna4_kv_dequant_fp8_bf16(Kt, Vt, K8, V8, Ks, Vs, B, NKV, HS, capacity, first_d, end - first_d, stream);
    if (rc) return rc;
    return mila_cdna4_attn_prefill_bf16(Y, Q, Kt, Vt, B, chunk, NH, NKV, HS, capacity, pos_offset, window, scale, stream);
}

}  // extern "C"
