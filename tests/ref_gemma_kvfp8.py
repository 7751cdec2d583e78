"""Oracle composition of the Gemma-4 forward over the FP8 KV cache (PerChannelKvFp8<>, GemmaConfig::kv_fp8): RefGemma with block() restated -- the appended K / V
rows, rounded to bf16 as the bf16 cache would hold them, pass through the oracle's row quantizer (orc.quantize_fp8_per_channel: scale = absmax / 448, 1 for an all-zero
row) and come back as bf16(e4m3 * scale), the value every later query reads.  Everything else is RefGemma's.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import orc
from ref_gemma import CONDITIONED_PROFILE, RefGemma


def quantize_rows(x):
    """rows x[..., HS] (bf16-representable floats) -> the values the FP8 KV cache returns for them: bf16(e4m3(x / scale) * scale), scale per row"""
    x = np.asarray(x, dtype=np.float32)
    q, s = orc.quantize_fp8_per_channel(orc.to_bf16_bits(x).reshape(-1, x.shape[-1]))
    return orc.round_bf16(orc.dequant_fp8(q, s)).reshape(x.shape)


class RefGemmaKvFp8(RefGemma):
    def block(self, x, L, pos, max_seq):
        """RefGemma.block with the quantizing append: x [T, D]; positions pos..pos+T-1"""
        T = x.shape[0]
        NH, NKV, HD = L["NH"], L["NKV"], L["HD"]
        qkv = self.linear(self.rms(x, L["input_norm"]), L["qkv"])
        q = qkv[:, :NH * HD].reshape(T, NH, HD)
        k = qkv[:, NH * HD:NH * HD + NKV * HD].reshape(T, NKV, HD)
        v = k if L["g"] else qkv[:, NH * HD + NKV * HD:].reshape(T, NKV, HD)
        qn = self.rms(q, L["q_norm"])
        kn = self.rms(k, L["k_norm"])
        cos, sin = self._rope_cache(L, max_seq)
        qr = self.r(orc.rope_rotate(qn[None], cos, sin, pos))[0]
        kr = self.r(orc.rope_rotate(kn[None], cos, sin, pos))[0]
        vn = self.rms(v, np.ones(HD, np.float32))
        L["K"] = np.concatenate([L["K"][:, :pos], quantize_rows(kr)[None]], axis=1)
        L["V"] = np.concatenate([L["V"][:, :pos], quantize_rows(vn)[None]], axis=1)
        window = 0 if L["g"] else self.c["window"]
        attn = self.r(orc.gqa_attention(qr[None], L["K"], L["V"], pos, window, 1.0))[0]
        o = self.linear(attn, L["o"])
        res1 = self.r(x + self.rms(o, L["post_attn"]))
        gu = self.linear(self.rms(res1, L["pre_ffn"]), L["gu"])
        act = self.r(orc.geglu(gu))
        dn = self.linear(act, L["down"])
        res2 = self.r(res1 + self.rms(dn, L["post_ffn"]))
        return self.r(res2 * np.float32(self.p["layer_scalar"]))


class RefGemmaKvFp8Fp32Norm(RefGemmaKvFp8):
    """the twin: a second correct implementation whose RMSNorm reduces in float32 in reverse order (tests/test_conditioned_cpu.py: _Fp32Norm) -- 1-ulp bf16 differences
    upstream of every Linear and of every quantized K / V row, where one may flip an e4m3 code (a 6 % step of that element)"""
    def rms(self, x, w):
        x = np.asarray(x, np.float32)
        ms = (x[..., ::-1] ** 2).sum(-1, dtype=np.float32, keepdims=True) / np.float32(x.shape[-1])
        return self.r(x * (np.float32(1) / np.sqrt(ms + np.float32(1e-6))) * np.asarray(w, np.float32))


# tests/test_conditioned_cpu.py's model and prompt
CPU_CFG = dict(vocab_size=1024, embedding_dim=512, num_layers=12, num_heads=4, num_kv_heads=2, head_dim=64, hidden_dim=1024,
               global_head_dim=128, num_global_kv_heads=1, window=8, sliding_window_pattern=6, global_rotary_dim=32)
CPU_TOK = [(7 * i + 3) % 1024 for i in range(12)]
BAR_FLOOR, BAR_CAP = 1e-3, 3e-3      # the bf16 whole-model bar; the project's bar for paths that re-quantize to e4m3


@functools.lru_cache(maxsize=None)
def cpu_distance():
    """max |a - b| / max |a| between the fp8-KV oracle and its float32-norm twin on the conditioned CPU model: the distance between two correct implementations"""
    a = RefGemmaKvFp8(CPU_CFG, "bf16", 7, profile=CONDITIONED_PROFILE).forward(CPU_TOK, 0, 32)
    b = RefGemmaKvFp8Fp32Norm(CPU_CFG, "bf16", 7, profile=CONDITIONED_PROFILE).forward(CPU_TOK, 0, 32)
    return float(np.abs(a - b).max() / np.abs(a).max())


def gpu_bar():
    """max(1e-3, 2 x the CPU distance) -- the device differs from the oracle in every reduction order, not only in the norms -- capped at 3e-3"""
    return min(BAR_CAP, max(BAR_FLOOR, 2.0 * cpu_distance()))
