// Fork a row's KV prefix into other rows of a rows model's caches (include/mila_cdna4.h: kv_rows_fork_bf16).
//
// A rows model keeps, per layer, K and V as [rows, NKV, capacity, HS] bf16 on unbounded caches: position p of a sequence lives at cache index p of its row.  Two
// requests with the same prompt therefore hold the same bits at [0, len) of their rows after their prefills, and the second prefill can be replaced by a copy of the
// first row's prefix.  This file is that copy: per (K | V, head) one contiguous segment of len * HS * 2 bytes, read ONCE from row `src` and stored into every row of
// `dst_mask`, 16 bytes per lane and trip, in a flat grid-stride walk over the 16-byte units of both caches.  Plain loads and stores of bit patterns: a NaN or a -0
// passes through as it is.  No LDS, no atomics.  Every element offset is 64-bit: four rows of a global layer at a long context pass 2^31 elements.
#include "common.h"

namespace mila {

constexpr int kForkThreads = 256;
constexpr int kForkMaxBlocks = 2048;      // 256 CUs x 8 blocks: the memory-bound grid cap the other copy kernels use; the rest is strided over

__global__ __launch_bounds__(kForkThreads) void kv_rows_fork_bf16_kernel(uint16_t* __restrict__ K, uint16_t* __restrict__ V, int64_t total_units, int64_t cache_units,
                                                                         int64_t seg_units, int64_t head_elems, int64_t row_elems, int src, unsigned dst_mask, int rows)
{
    // total_units = 2 * cache_units (K then V), cache_units = NKV * seg_units, seg_units = len * HS / 8; head_elems = capacity * HS, row_elems = NKV * head_elems
    const int64_t stride = (int64_t)gridDim.x * kForkThreads;
    for (int64_t i = (int64_t)blockIdx.x * kForkThreads + threadIdx.x; i < total_units; i += stride)
    {
        const bool value = i >= cache_units;
        const int64_t c = value ? i - cache_units : i;
        const int64_t head = c / seg_units, u = c - head * seg_units;
        uint16_t* base = value ? V : K;
        const int64_t in_row = head * head_elems + u * 8;      // < row_elems: u * 8 < len * HS <= capacity * HS
        const u32x4 bits = ld16(base + (int64_t)src * row_elems + in_row);
        for (int r = 0; r < rows; ++r)
            if ((dst_mask >> r) & 1u) st16(base + (int64_t)r * row_elems + in_row, bits);
    }
}

// The same copy for n layers of different (K, V, NKV, capacity, HS) in ONE launch (kv_rows_fork_layers_bf16): a 48-layer fork of a short prefix is 48 launches of a few
// microseconds of work each, i.e. launch cost.  The layer is the grid's y index; its record comes by value in the kernel arguments (a uniform index into the argument
// block: scalar loads), so the call allocates nothing, copies nothing to the device and reads nothing back.  Within a layer: the walk of the kernel above.
constexpr int kForkLayersPerLaunch = 64;      // 64 x 32 bytes of records: half of the 4 KiB argument block; more layers take another launch
constexpr int kForkLayersMinBlocks = 8;       // per layer, however many layers share the grid cap

struct ForkLayer { uint16_t* K; uint16_t* V; int64_t seg_units, head_elems; int32_t NKV, pad; };      // seg_units = len * HS / 8, head_elems = capacity * HS
struct ForkLayers { ForkLayer l[kForkLayersPerLaunch]; };

__global__ __launch_bounds__(kForkThreads) void kv_rows_fork_layers_bf16_kernel(const ForkLayers layers, int src, unsigned dst_mask, int rows)
{
    const ForkLayer& L = layers.l[blockIdx.y];
    uint16_t* const K = L.K;
    uint16_t* const V = L.V;
    const int64_t seg_units = L.seg_units, head_elems = L.head_elems;
    const int64_t cache_units = (int64_t)L.NKV * seg_units, total_units = 2 * cache_units, row_elems = (int64_t)L.NKV * head_elems;
    const int64_t stride = (int64_t)gridDim.x * kForkThreads;
    for (int64_t i = (int64_t)blockIdx.x * kForkThreads + threadIdx.x; i < total_units; i += stride)
    {
        const bool value = i >= cache_units;
        const int64_t c = value ? i - cache_units : i;
        const int64_t head = c / seg_units, u = c - head * seg_units;
        uint16_t* base = value ? V : K;
        const int64_t in_row = head * head_elems + u * 8;      // < row_elems: head < NKV, u * 8 < len * HS <= capacity * HS
        const u32x4 bits = ld16(base + (int64_t)src * row_elems + in_row);
        for (int r = 0; r < rows; ++r)
            if ((dst_mask >> r) & 1u) st16(base + (int64_t)r * row_elems + in_row, bits);
    }
}

// The same for the FP8 KV cache (kv_rows_fork_layers_kvfp8): per layer K8 / V8 [rows, NKV, capacity, HS] e4m3 and Ks / Vs [rows, NKV, capacity] fp32.  One flat walk per
// layer over two kinds of unit: first the 16-byte units of the bytes (K8 then V8; per head len * HS / 16 of them, HS a multiple of 16), then the 4-byte words of the
// scales (Ks then Vs; per head len of them).  A head's scale run starts capacity * 4 bytes after the one before and is len * 4 long: neither is 16-byte aligned in
// general, so the scales go word by word, never wider.
struct ForkLayerFp8 { uint8_t* K8; uint8_t* V8; float* Ks; float* Vs; int64_t seg_units, head_bytes; int32_t NKV, capacity; };      // seg_units = len * HS / 16, head_bytes = capacity * HS
constexpr int kForkLayersFp8PerLaunch = 64;      // 64 x 56 bytes of records: 3.5 KiB of the 4 KiB argument block
struct ForkLayersFp8 { ForkLayerFp8 l[kForkLayersFp8PerLaunch]; };

__global__ __launch_bounds__(kForkThreads) void kv_rows_fork_layers_kvfp8_kernel(const ForkLayersFp8 layers, int src, unsigned dst_mask, int rows, int len)
{
    const ForkLayerFp8& L = layers.l[blockIdx.y];
    uint8_t* const K8 = L.K8;
    uint8_t* const V8 = L.V8;
    float* const Ks = L.Ks;
    float* const Vs = L.Vs;
    const int64_t seg_units = L.seg_units, head_bytes = L.head_bytes, capacity = L.capacity;
    const int64_t cache_units = (int64_t)L.NKV * seg_units, byte_units = 2 * cache_units, row_bytes = (int64_t)L.NKV * head_bytes;
    const int64_t cache_words = (int64_t)L.NKV * len, total = byte_units + 2 * cache_words, row_words = (int64_t)L.NKV * capacity;
    const int64_t stride = (int64_t)gridDim.x * kForkThreads;
    for (int64_t i = (int64_t)blockIdx.x * kForkThreads + threadIdx.x; i < total; i += stride)
    {
        if (i < byte_units)
        {
            const bool value = i >= cache_units;
            const int64_t c = value ? i - cache_units : i;
            const int64_t head = c / seg_units, u = c - head * seg_units;
            uint8_t* base = value ? V8 : K8;
            const int64_t in_row = head * head_bytes + u * 16;      // < row_bytes: head < NKV, u * 16 < len * HS <= capacity * HS
            const u32x4 bits = *reinterpret_cast<const u32x4*>(base + (int64_t)src * row_bytes + in_row);
            for (int r = 0; r < rows; ++r)
                if ((dst_mask >> r) & 1u) *reinterpret_cast<u32x4*>(base + (int64_t)r * row_bytes + in_row) = bits;
        }
        else
        {
            const int64_t j = i - byte_units;
            const bool value = j >= cache_words;
            const int64_t c = value ? j - cache_words : j;
            const int64_t head = c / len, u = c - head * len;
            uint32_t* base = reinterpret_cast<uint32_t*>(value ? Vs : Ks);      // bit patterns: a NaN, a -0 or a denormal passes as it is
            const int64_t in_row = head * capacity + u;             // < row_words: head < NKV, u < len <= capacity
            const uint32_t bits = base[(int64_t)src * row_words + in_row];
            for (int r = 0; r < rows; ++r)
                if ((dst_mask >> r) & 1u) base[(int64_t)r * row_words + in_row] = bits;
        }
    }
}

// The LIVE BAND of every layer in one launch (kv_rows_fork_layers_band_bf16): a rows model whose sliding-window layers sit on rings (GemmaConfig::bounded_local_kv_rows).
// Position p lives at cache index p % capacity, and a continuation from `len` reads no further back than len - window, so a layer's copy is positions [begin, len),
// begin = window > 0 ? max( 0, len - window ) : 0 -- a flat layer (window 0) is the whole prefix, as above.  Per (K | V, head) that is band * HS / 8 16-byte units that
// start at cache index begin % capacity and may run over the ring's end once (band <= capacity): unit u sits at start_elems + u * 8, less head_elems when that passes the
// head's end -- one conditional subtract per unit, no remainder in the walk.  Otherwise the walk of the layers kernel above: read once, stored to every destination row.
struct ForkLayerBand { uint16_t* K; uint16_t* V; int64_t seg_units, head_elems, start_elems; int32_t NKV, pad; };      // seg_units = band * HS / 8, head_elems = capacity * HS, start_elems = (begin % capacity) * HS
constexpr int kForkLayersBandPerLaunch = 64;      // 64 x 48 bytes of records: 3 KiB of the 4 KiB argument block
struct ForkLayersBand { ForkLayerBand l[kForkLayersBandPerLaunch]; };

__global__ __launch_bounds__(kForkThreads) void kv_rows_fork_layers_band_bf16_kernel(const ForkLayersBand layers, int src, unsigned dst_mask, int rows)
{
    const ForkLayerBand& L = layers.l[blockIdx.y];
    uint16_t* const K = L.K;
    uint16_t* const V = L.V;
    const int64_t seg_units = L.seg_units, head_elems = L.head_elems, start_elems = L.start_elems;
    const int64_t cache_units = (int64_t)L.NKV * seg_units, total_units = 2 * cache_units, row_elems = (int64_t)L.NKV * head_elems;
    const int64_t stride = (int64_t)gridDim.x * kForkThreads;
    for (int64_t i = (int64_t)blockIdx.x * kForkThreads + threadIdx.x; i < total_units; i += stride)
    {
        const bool value = i >= cache_units;
        const int64_t c = value ? i - cache_units : i;
        const int64_t head = c / seg_units, u = c - head * seg_units;
        uint16_t* base = value ? V : K;
        int64_t in_head = start_elems + u * 8;      // < 2 * head_elems: start_elems < head_elems, u * 8 < band * HS <= capacity * HS
        if (in_head >= head_elems) in_head -= head_elems;      // the band's second run, from the ring's first index
        const int64_t in_row = head * head_elems + in_head;      // < row_elems: head < NKV, in_head < head_elems
        const u32x4 bits = ld16(base + (int64_t)src * row_elems + in_row);
        for (int r = 0; r < rows; ++r)
            if ((dst_mask >> r) & 1u) st16(base + (int64_t)r * row_elems + in_row, bits);
    }
}

}  // namespace mila

using namespace mila;

extern "C" {

int mila_cdna4_kv_rows_fork_bf16(uint16_t* K, uint16_t* V, int rows, int NKV, int capacity, int HS, int src, unsigned dst_mask, int len, mila_stream_t stream)
{
    MILA_REQUIRE(K && V, "kv_rows_fork_bf16: null pointer");
    MILA_REQUIRE(rows >= 2 && rows <= 4, "kv_rows_fork_bf16: rows=%d out of range (2 .. 4)", rows);
    MILA_REQUIRE(NKV > 0 && capacity > 0 && HS > 0, "kv_rows_fork_bf16: bad sizes (NKV=%d capacity=%d HS=%d)", NKV, capacity, HS);
    MILA_REQUIRE(HS % 8 == 0, "kv_rows_fork_bf16: HS=%d must be a multiple of 8", HS);
    MILA_REQUIRE(src >= 0 && src < rows, "kv_rows_fork_bf16: src=%d outside the %d rows", src, rows);
    MILA_REQUIRE(dst_mask != 0, "kv_rows_fork_bf16: empty dst_mask");
    MILA_REQUIRE((dst_mask >> rows) == 0, "kv_rows_fork_bf16: dst_mask=0x%x names a row outside the %d rows", dst_mask, rows);
    MILA_REQUIRE(((dst_mask >> src) & 1u) == 0, "kv_rows_fork_bf16: dst_mask=0x%x names the source row %d", dst_mask, src);
    MILA_REQUIRE(len >= 1 && len <= capacity, "kv_rows_fork_bf16: len=%d out of range (1 .. capacity %d)", len, capacity);
    MILA_REQUIRE(((reinterpret_cast<uintptr_t>(K) | reinterpret_cast<uintptr_t>(V)) & 15) == 0, "kv_rows_fork_bf16: K and V must be 16-byte aligned");
    const int64_t seg_units = (int64_t)len * (HS / 8), cache_units = (int64_t)NKV * seg_units, total_units = 2 * cache_units;
    const int64_t head_elems = (int64_t)capacity * HS, row_elems = (int64_t)NKV * head_elems;
    const int64_t blocks = (total_units + kForkThreads - 1) / kForkThreads;
    hipLaunchKernelGGL(kv_rows_fork_bf16_kernel, dim3((unsigned)(blocks < kForkMaxBlocks ? blocks : kForkMaxBlocks)), dim3(kForkThreads), 0, as_stream(stream), K, V,
                       total_units, cache_units, seg_units, head_elems, row_elems, src, dst_mask, rows);
    MILA_LAUNCH_CHECK("kv_rows_fork_bf16");
}

int mila_cdna4_kv_rows_fork_layers_bf16(const mila_kv_fork_layer* layers, int n_layers, int rows, int src, unsigned dst_mask, int len, mila_stream_t stream)
{
    MILA_REQUIRE(layers, "kv_rows_fork_layers_bf16: null layer table");
    MILA_REQUIRE(n_layers > 0, "kv_rows_fork_layers_bf16: n_layers=%d must be positive", n_layers);
    MILA_REQUIRE(rows >= 2 && rows <= 4, "kv_rows_fork_layers_bf16: rows=%d out of range (2 .. 4)", rows);
    MILA_REQUIRE(src >= 0 && src < rows, "kv_rows_fork_layers_bf16: src=%d outside the %d rows", src, rows);
    MILA_REQUIRE(dst_mask != 0, "kv_rows_fork_layers_bf16: empty dst_mask");
    MILA_REQUIRE((dst_mask >> rows) == 0, "kv_rows_fork_layers_bf16: dst_mask=0x%x names a row outside the %d rows", dst_mask, rows);
    MILA_REQUIRE(((dst_mask >> src) & 1u) == 0, "kv_rows_fork_layers_bf16: dst_mask=0x%x names the source row %d", dst_mask, src);
    MILA_REQUIRE(len >= 1, "kv_rows_fork_layers_bf16: len=%d must be positive", len);
    for (int i = 0; i < n_layers; ++i)      // every layer before the first launch: a refusal leaves every cache as it was
    {
        const mila_kv_fork_layer& L = layers[i];
        MILA_REQUIRE(L.K && L.V, "kv_rows_fork_layers_bf16: layer %d: null pointer", i);
        MILA_REQUIRE(L.NKV > 0 && L.capacity > 0 && L.HS > 0, "kv_rows_fork_layers_bf16: layer %d: bad sizes (NKV=%d capacity=%d HS=%d)", i, L.NKV, L.capacity, L.HS);
        MILA_REQUIRE(L.HS % 8 == 0, "kv_rows_fork_layers_bf16: layer %d: HS=%d must be a multiple of 8", i, L.HS);
        MILA_REQUIRE(len <= L.capacity, "kv_rows_fork_layers_bf16: layer %d: len=%d out of range (1 .. capacity %d)", i, len, L.capacity);
        MILA_REQUIRE(((reinterpret_cast<uintptr_t>(L.K) | reinterpret_cast<uintptr_t>(L.V)) & 15) == 0, "kv_rows_fork_layers_bf16: layer %d: K and V must be 16-byte aligned", i);
    }
    for (int first = 0; first < n_layers; first += kForkLayersPerLaunch)
    {
        const int n = n_layers - first < kForkLayersPerLaunch ? n_layers - first : kForkLayersPerLaunch;
        ForkLayers args{};
        int64_t most = 0;      // the longest layer's units size the grid's x; a shorter layer's spare blocks fall through their loop
        for (int i = 0; i < n; ++i)
        {
            const mila_kv_fork_layer& L = layers[first + i];
            ForkLayer& a = args.l[i];
            a.K = L.K; a.V = L.V; a.NKV = L.NKV;
            a.seg_units = (int64_t)len * (L.HS / 8);
            a.head_elems = (int64_t)L.capacity * L.HS;
            const int64_t total_units = 2 * (int64_t)L.NKV * a.seg_units;
            most = total_units > most ? total_units : most;
        }
        const int64_t blocks = (most + kForkThreads - 1) / kForkThreads;
        const int64_t cap = kForkMaxBlocks / n > kForkLayersMinBlocks ? kForkMaxBlocks / n : kForkLayersMinBlocks;      // the grid cap of the one-layer kernel, shared by the layers
        hipLaunchKernelGGL(kv_rows_fork_layers_bf16_kernel, dim3((unsigned)(blocks < cap ? blocks : cap), (unsigned)n), dim3(kForkThreads), 0, as_stream(stream), args, src,
                           dst_mask, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return ::mila::check_hip(e, "kv_rows_fork_layers_bf16");
    }
    return MILA_OK;
}

int mila_cdna4_kv_rows_fork_layers_band_bf16(const mila_kv_fork_layer_band* layers, int n_layers, int rows, int src, unsigned dst_mask, int len, mila_stream_t stream)
{
    MILA_REQUIRE(layers, "kv_rows_fork_layers_band_bf16: null layer table");
    MILA_REQUIRE(n_layers > 0, "kv_rows_fork_layers_band_bf16: n_layers=%d must be positive", n_layers);
    MILA_REQUIRE(rows >= 2 && rows <= 4, "kv_rows_fork_layers_band_bf16: rows=%d out of range (2 .. 4)", rows);
    MILA_REQUIRE(src >= 0 && src < rows, "kv_rows_fork_layers_band_bf16: src=%d outside the %d rows", src, rows);
    MILA_REQUIRE(dst_mask != 0, "kv_rows_fork_layers_band_bf16: empty dst_mask");
    MILA_REQUIRE((dst_mask >> rows) == 0, "kv_rows_fork_layers_band_bf16: dst_mask=0x%x names a row outside the %d rows", dst_mask, rows);
    MILA_REQUIRE(((dst_mask >> src) & 1u) == 0, "kv_rows_fork_layers_band_bf16: dst_mask=0x%x names the source row %d", dst_mask, src);
    MILA_REQUIRE(len >= 1, "kv_rows_fork_layers_band_bf16: len=%d must be positive", len);
    for (int i = 0; i < n_layers; ++i)      // every layer before the first launch: a refusal leaves every cache as it was
    {
        const mila_kv_fork_layer_band& L = layers[i];
        MILA_REQUIRE(L.K && L.V, "kv_rows_fork_layers_band_bf16: layer %d: null pointer", i);
        MILA_REQUIRE(L.NKV > 0 && L.capacity > 0 && L.HS > 0, "kv_rows_fork_layers_band_bf16: layer %d: bad sizes (NKV=%d capacity=%d HS=%d)", i, L.NKV, L.capacity, L.HS);
        MILA_REQUIRE(L.HS % 8 == 0, "kv_rows_fork_layers_band_bf16: layer %d: HS=%d must be a multiple of 8", i, L.HS);
        MILA_REQUIRE(L.window >= 0, "kv_rows_fork_layers_band_bf16: layer %d: window=%d must not be negative", i, L.window);
        const int begin = L.window > 0 && len > L.window ? len - L.window : 0;
        MILA_REQUIRE(len - begin <= L.capacity, "kv_rows_fork_layers_band_bf16: layer %d: band=%d of len=%d (window %d) above capacity %d", i, len - begin, len, L.window, L.capacity);
        MILA_REQUIRE(((reinterpret_cast<uintptr_t>(L.K) | reinterpret_cast<uintptr_t>(L.V)) & 15) == 0, "kv_rows_fork_layers_band_bf16: layer %d: K and V must be 16-byte aligned", i);
    }
    for (int first = 0; first < n_layers; first += kForkLayersBandPerLaunch)
    {
        const int n = n_layers - first < kForkLayersBandPerLaunch ? n_layers - first : kForkLayersBandPerLaunch;
        ForkLayersBand args{};
        int64_t most = 0;      // the longest layer's units size the grid's x; a shorter layer's spare blocks fall through their loop
        for (int i = 0; i < n; ++i)
        {
            const mila_kv_fork_layer_band& L = layers[first + i];
            ForkLayerBand& a = args.l[i];
            const int begin = L.window > 0 && len > L.window ? len - L.window : 0;
            a.K = L.K; a.V = L.V; a.NKV = L.NKV;
            a.seg_units = (int64_t)(len - begin) * (L.HS / 8);
            a.head_elems = (int64_t)L.capacity * L.HS;
            a.start_elems = (int64_t)(begin % L.capacity) * L.HS;      // the one remainder of the call, on the host
            const int64_t total_units = 2 * (int64_t)L.NKV * a.seg_units;
            most = total_units > most ? total_units : most;
        }
        const int64_t blocks = (most + kForkThreads - 1) / kForkThreads;
        const int64_t cap = kForkMaxBlocks / n > kForkLayersMinBlocks ? kForkMaxBlocks / n : kForkLayersMinBlocks;      // the grid cap of the one-layer kernel, shared by the layers
        hipLaunchKernelGGL(kv_rows_fork_layers_band_bf16_kernel, dim3((unsigned)(blocks < cap ? blocks : cap), (unsigned)n), dim3(kForkThreads), 0, as_stream(stream), args, src,
                           dst_mask, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return ::mila::check_hip(e, "kv_rows_fork_layers_band_bf16");
    }
    return MILA_OK;
}

int mila_cdna4_kv_rows_fork_layers_kvfp8(const mila_kv_fork_layer_fp8* layers, int n_layers, int rows, int src, unsigned dst_mask, int len, mila_stream_t stream)
{
    MILA_REQUIRE(layers, "kv_rows_fork_layers_kvfp8: null layer table");
    MILA_REQUIRE(n_layers > 0, "kv_rows_fork_layers_kvfp8: n_layers=%d must be positive", n_layers);
    MILA_REQUIRE(rows >= 2 && rows <= 4, "kv_rows_fork_layers_kvfp8: rows=%d out of range (2 .. 4)", rows);
    MILA_REQUIRE(src >= 0 && src < rows, "kv_rows_fork_layers_kvfp8: src=%d outside the %d rows", src, rows);
    MILA_REQUIRE(dst_mask != 0, "kv_rows_fork_layers_kvfp8: empty dst_mask");
    MILA_REQUIRE((dst_mask >> rows) == 0, "kv_rows_fork_layers_kvfp8: dst_mask=0x%x names a row outside the %d rows", dst_mask, rows);
    MILA_REQUIRE(((dst_mask >> src) & 1u) == 0, "kv_rows_fork_layers_kvfp8: dst_mask=0x%x names the source row %d", dst_mask, src);
    MILA_REQUIRE(len >= 1, "kv_rows_fork_layers_kvfp8: len=%d must be positive", len);
    for (int i = 0; i < n_layers; ++i)      // every layer before the first launch: a refusal leaves every cache as it was
    {
        const mila_kv_fork_layer_fp8& L = layers[i];
        MILA_REQUIRE(L.K8 && L.V8 && L.Ks && L.Vs, "kv_rows_fork_layers_kvfp8: layer %d: null pointer", i);
        MILA_REQUIRE(L.NKV > 0 && L.capacity > 0 && L.HS > 0, "kv_rows_fork_layers_kvfp8: layer %d: bad sizes (NKV=%d capacity=%d HS=%d)", i, L.NKV, L.capacity, L.HS);
        MILA_REQUIRE(L.HS % 16 == 0, "kv_rows_fork_layers_kvfp8: layer %d: HS=%d must be a multiple of 16", i, L.HS);
        MILA_REQUIRE(len <= L.capacity, "kv_rows_fork_layers_kvfp8: layer %d: len=%d out of range (1 .. capacity %d)", i, len, L.capacity);
        MILA_REQUIRE(((reinterpret_cast<uintptr_t>(L.K8) | reinterpret_cast<uintptr_t>(L.V8)) & 15) == 0, "kv_rows_fork_layers_kvfp8: layer %d: K8 and V8 must be 16-byte aligned", i);
        MILA_REQUIRE(((reinterpret_cast<uintptr_t>(L.Ks) | reinterpret_cast<uintptr_t>(L.Vs)) & 3) == 0, "kv_rows_fork_layers_kvfp8: layer %d: Ks and Vs must be 4-byte aligned", i);
    }
    for (int first = 0; first < n_layers; first += kForkLayersFp8PerLaunch)
    {
        const int n = n_layers - first < kForkLayersFp8PerLaunch ? n_layers - first : kForkLayersFp8PerLaunch;
        ForkLayersFp8 args{};
        int64_t most = 0;      // the longest layer's units size the grid's x; a shorter layer's spare blocks fall through their loop
        for (int i = 0; i < n; ++i)
        {
            const mila_kv_fork_layer_fp8& L = layers[first + i];
            ForkLayerFp8& a = args.l[i];
            a.K8 = L.K8; a.V8 = L.V8; a.Ks = L.Ks; a.Vs = L.Vs; a.NKV = L.NKV; a.capacity = L.capacity;
            a.seg_units = (int64_t)len * (L.HS / 16);
            a.head_bytes = (int64_t)L.capacity * L.HS;
            const int64_t total = 2 * (int64_t)L.NKV * (a.seg_units + len);
            most = total > most ? total : most;
        }
        const int64_t blocks = (most + kForkThreads - 1) / kForkThreads;
        const int64_t cap = kForkMaxBlocks / n > kForkLayersMinBlocks ? kForkMaxBlocks / n : kForkLayersMinBlocks;
        hipLaunchKernelGGL(kv_rows_fork_layers_kvfp8_kernel, dim3((unsigned)(blocks < cap ? blocks : cap), (unsigned)n), dim3(kForkThreads), 0, as_stream(stream), args, src,
                           dst_mask, rows, len);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return ::mila::check_hip(e, "kv_rows_fork_layers_kvfp8");
    }
    return MILA_OK;
}

}  // extern "C"
