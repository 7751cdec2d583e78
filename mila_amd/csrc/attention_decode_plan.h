// What the fp8-KV-cache decode (attention_kvfp8.hip) takes from the bf16 one (attention.hip): the plan of a shape -- plan_decode's, so that both caches take the same
// form and split a band the same way --, the launches that merge the split partials [B, NH, splits, HS + 4] (O | m | l | pad) into Y, and what both files do with a
// plan: the band a length leaves alive, and the ONE dispatch from (HS, heads per workgroup) to an instantiation of a wave-per-position kernel.
#pragma once
#include <climits>
#include <type_traits>
#include "common.h"

namespace mila {

struct KvFp8DecodeShape
{
    bool mfma;               // the matrix-core form (attn_decode_kvfp8_mfma_kernel: 16-head groups, up to 256 splits); else the wave-per-position kernel
    int splits;              // workgroups along the band
    int gh, hgroups;         // query heads per workgroup, workgroups per KV head (scalar form)
    size_t scratch_need;     // bytes of partials; 0 = unsplit, the launch touches no scratch
};
// plan_decode for an unfused entry over the fp8 cache; HS in {64, 128, 256, 512}; len_hint as in plan_decode
KvFp8DecodeShape plan_decode_kvfp8(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint);
// attn_combine_kernel over `splits` (<= 64) partials per head
int launch_attn_combine(uint16_t* Y, const float* partials, int B, int NH, int HS, int splits, hipStream_t s);
// attn_combine_many_kernel over `splits` (<= 256) partials per head: the matrix-core form's merge
int launch_attn_combine_many(uint16_t* Y, const float* partials, int B, int NH, int HS, int splits, hipStream_t s);


// the keys a query at live length `len` sees under `window` (0 = all of them): what must fit the cache
inline int live_band(int len, int window) { return (window > 0 && window < len) ? window : len; }
// the query heads per KV head (NH / NKV) the wave-per-position kernels divide into workgroups
inline bool decode_group_size_ok(int GS) { return GS == 1 || GS == 2 || GS == 4 || GS == 8 || GS == 16 || GS == 32; }
// the head sizes the wave-per-position kernels (and the fp8 cache's append / dequant) are instantiated for
inline bool decode_scalar_head_size(int HS) { return HS == 64 || HS == 128 || HS == 256 || HS == 512; }

// (HS, gh) -> launch(HS, GH), both as integral constants: gh is the plan's (DecodePlan::gh, KvFp8DecodeShape::gh) -- the rule for it lives in plan_decode alone.
// FOUR_AT_512: the caller has the <512, 4> instantiation (the attn.heads_per_group_512 experiment: bf16 cache only).  kNoDecodeKernel: no instantiation for the pair;
// the caller words the error.
constexpr int kNoDecodeKernel = INT_MIN;
template <int V> using DecodeInt = std::integral_constant<int, V>;
template <int HS, bool FOUR_AT_512, class Launch>
int dispatch_decode_gh(int gh, const Launch& launch)
{
    if (gh == 1) return launch(DecodeInt<HS>{}, DecodeInt<1>{});
    if (gh == 2) return launch(DecodeInt<HS>{}, DecodeInt<2>{});
    if constexpr (HS < 512 || FOUR_AT_512)
        if (gh == 4) return launch(DecodeInt<HS>{}, DecodeInt<4>{});
    return kNoDecodeKernel;
}
template <bool FOUR_AT_512, class Launch>
int dispatch_decode_scalar(int HS, int gh, const Launch& launch)
{
    switch (HS)
    {
        case 64: return dispatch_decode_gh<64, FOUR_AT_512>(gh, launch);
        case 128: return dispatch_decode_gh<128, FOUR_AT_512>(gh, launch);
        case 256: return dispatch_decode_gh<256, FOUR_AT_512>(gh, launch);
        case 512: return dispatch_decode_gh<512, FOUR_AT_512>(gh, launch);
        default: return kNoDecodeKernel;
    }
}

}  // namespace mila
