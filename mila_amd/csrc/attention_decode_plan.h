// What the fp8-KV-cache decode (attention_kvfp8.hip) takes from the bf16 one (attention.hip): the plan of a shape -- plan_decode's, so that both caches take the same
// form and split a band the same way -- and the launches that merge the split partials [B, NH, splits, HS + 4] (O | m | l | pad) into Y.
#pragma once
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

}  // namespace mila
