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

}  // extern "C"
