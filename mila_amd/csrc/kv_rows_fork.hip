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

}  // extern "C"
