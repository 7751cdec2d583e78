// What the fp8-KV-cache decode (attention_kvfp8.hip) shares with the bf16 one (attention.hip): the scalar form's plan of a shape -- so that both caches split a band
// the same way -- and the launch that merges the split partials [B, NH, splits, HS + 4] (O | m | l | pad) into Y.
#pragma once
#include "common.h"

namespace mila {

struct ScalarDecodeShape
{
    int splits;              // workgroups along the band
    int gh, hgroups;         // query heads per workgroup, workgroups per KV head
    size_t scratch_need;     // bytes of partials; 0 = unsplit, the launch touches no scratch
};
// plan_decode's scalar form (attn_decode_kernel's grid) for an unfused entry; HS in {64, 128, 256, 512}
ScalarDecodeShape plan_decode_scalar(int B, int NH, int NKV, int HS, int capacity, int window, int len_hint);
// attn_combine_kernel over `splits` (<= 64) partials per head
int launch_attn_combine(uint16_t* Y, const float* partials, int B, int NH, int HS, int splits, hipStream_t s);

}  // namespace mila
