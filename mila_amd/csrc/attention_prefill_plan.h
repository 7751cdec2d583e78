// The prefill-attention plan: everything attn_prefill_bf16 / mha_bf16 decide before they launch -- the kernel, its workgroup shape and its grid -- as ONE pure host
// function of the shape and the "flash.form" tunable (attention_prefill.hip: plan_prefill).  flash_dispatch launches from it; mila_cdna4_attn_prefill_plan_describe
// prints it, so a test can hold a shape to the instantiation it is there for without a GPU.
#pragma once

namespace mila {

enum PrefillForm
{
    PF_FLASH,             // register-staged tiles: flash_prefill_kernel<HS, HB> (HS 512, under flash.form 1: flash_prefill_kernel_s1<512, HB, 1, 4>)
    PF_FLASH_DMA,         // LDS-DMA tiles: flash_prefill_kernel_s1<HS, HB, DS, NW>
    PF_FLASH_DMA_PIPE,    // ... with the software-pipelined loop: flash_prefill_kernel_s1<HS, HB, DS, NW, true>
    PF_FLASH_PP,          // the ping-pong 8-wave kernel: flash_prefill_pp_kernel<HS, HB, DS>
    PF_GENERIC,           // attention_generic.hip: any head size but 64 / 128 / 256 / 512, one wave per (head, row)
};
constexpr const char* kPrefillFormNames[] = {"flash", "flash_dma", "flash_dma_pipe", "flash_pp", "attn_generic"};

struct PrefillPlan
{
    PrefillForm form;
    int HS;
    int HB, DS, NW;            // heads, d-shares and waves per workgroup: a workgroup holds NW / (HB DS) blocks of 16 query rows (PF_GENERIC: 1, 1, 4 -- four rows of one head each)
    int QROWS;                 // query rows per workgroup
    int n_qtiles, n_hblk;      // query tiles of the chunk, head blocks: grid.x = n_items = n_qtiles * n_hblk per batch row (PF_GENERIC: the (head, row) pairs in fours)
    int n_items;
};

// HS > 0, NH % NKV == 0, chunk > 0
PrefillPlan plan_prefill(int HS, int NH, int NKV, int chunk, int pos_offset, int window);

}  // namespace mila
