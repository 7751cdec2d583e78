"""The FP8 KV cache through the host mirror (libmila_host.so: host/src/gqa_runner.cpp): GroupedQueryAttention<Rocm, BF16, PerChannelKvFp8<>> forwards to
RocmGqaKvFp8Op -- prefill, decode, rewind, the state bytes and the methods that exist for the fused bf16-cache entries only."""
import numpy as np
import pytest

import orc
from gpu_util import assert_bf16_close
from mila_amd import host

pytestmark = pytest.mark.gpu

NH, NKV, HS, WINDOW = 16, 8, 256, 64      # Gemma's local geometry, a window that starts inside the cache


def _bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def _b(x):
    return orc.to_bf16_bits(x)


def _quantize(x):
    q, s = orc.quantize_fp8_per_channel(_b(x).reshape(-1, x.shape[-1]))
    return q.reshape(x.shape), s.reshape(x.shape[:-1]), orc.round_bf16(orc.dequant_fp8(q, s)).reshape(x.shape)


def _tokens(seed, B, T):
    rng = np.random.default_rng(seed)
    return (_bf(rng.uniform(-1, 1, (B, T, NH, HS))), _bf(rng.uniform(-1, 1, (B, T, NKV, HS)) * 0.5),
            _bf(rng.uniform(-1, 1, (B, T, NKV, HS)) * rng.uniform(0.1, 1.0, (B, T, NKV, 1))))      # row scales that differ by up to 10 x, values inside the bar's [-1, 1]


def _run(g, q, k, v, start, prefill_to, chunk, end):
    """prefill [start, prefill_to) in chunks, then decode up to `end`: the output rows [start, end)"""
    B = q.shape[0]
    out = []
    for s in range(start, prefill_to, chunk):
        e = min(prefill_to, s + chunk)
        out.append(g.prefill(_b(q[:, s:e]).reshape(B, e - s, -1), _b(k[:, s:e]).reshape(B, e - s, -1), _b(v[:, s:e]).reshape(B, e - s, -1), s))
    for t in range(prefill_to, end):
        out.append(g.decode(_b(q[:, t]).reshape(B, -1), _b(k[:, t]).reshape(B, -1), _b(v[:, t]).reshape(B, -1), t)[:, None])
    return np.concatenate(out, axis=1)


def test_component_prefill_and_decode_against_the_oracle():
    """2 x 96 tokens of prefill, then 3 decodes, window 64: every row within the bf16 cache's bar of the oracle on the dequantized history; the cache arrays the op
    holds are the oracle's bytes and scales"""
    B, T = 1, 195
    q, k, v = _tokens(1, B, T)
    g = host.GqaComponent("fp8", NH, NKV, HS, window=WINDOW, attention_scale=1.0, batch=B, max_seq=256, prefill_chunk=96)
    try:
        got = _run(g, q, k, v, 0, 192, 96, T)
        (qk, sk, dk), (qv, sv, dv) = _quantize(k), _quantize(v)
        assert_bf16_close(got, orc.gqa_attention(q, dk, dv, 0, WINDOW, 1.0), 1, 2e-3, "GroupedQueryAttention<PerChannelKvFp8<>>")
        st = g.state()
        assert st["capacity"] == 256 and st["length"] == T
        K8, V8, Ks, Vs = g.read_cache()
        assert np.array_equal(K8[:, :, :T], qk.transpose(0, 2, 1, 3)) and np.array_equal(V8[:, :, :T], qv.transpose(0, 2, 1, 3))
        assert np.array_equal(Ks[:, :, :T].view(np.uint32), sk.transpose(0, 2, 1).view(np.uint32)) and np.array_equal(Vs[:, :, :T].view(np.uint32), sv.transpose(0, 2, 1).view(np.uint32))
    finally:
        g.close()


@pytest.mark.parametrize("hs", [128, 256, 512])
def test_state_bytes_follow_the_closed_form(hs):
    """2 B NKV capacity (HS + 4) bytes: (HS + 4) / (2 HS) of the bf16 op's -- under 0.52 from HS 128 on; the component's memory statistics count the same arrays"""
    B, nh, nkv, cap, chunk = 2, 8, 2, 96, 32
    g8 = host.GqaComponent("fp8", nh, nkv, hs, batch=B, max_seq=cap, prefill_chunk=chunk)
    g16 = host.GqaComponent("none", nh, nkv, hs, batch=B, max_seq=cap, prefill_chunk=chunk)
    try:
        s8, s16 = g8.state(), g16.state()
        want = 2 * B * nkv * cap * (hs + 4)
        assert s8["op_state_bytes"] == want and s8["op_required_state_bytes"] == want and s8["capacity"] == cap
        assert s16["op_state_bytes"] == 2 * B * nkv * cap * hs * 2
        assert s8["op_state_bytes"] < 0.52 * s16["op_state_bytes"]
        out_bytes = B * chunk * nh * hs * 2                      # the component's own output buffer
        assert s8["component_state_bytes"] == want + out_bytes and s8["component_required_state_bytes"] == want + out_bytes
    finally:
        g8.close()
        g16.close()


def test_rewind_then_a_different_continuation_equals_a_fresh_cache():
    B, keep = 1, 90
    q, k, v = _tokens(2, B, 99)
    q2, k2, v2 = _tokens(3, B, 112)
    for a, b_ in ((q2, q), (k2, k), (v2, v)):
        a[:, :keep] = b_[:, :keep]                                # the same first 90 tokens, then another continuation
    g = host.GqaComponent("fp8", NH, NKV, HS, window=WINDOW, attention_scale=1.0, batch=B, max_seq=128, prefill_chunk=96)
    fresh = host.GqaComponent("fp8", NH, NKV, HS, window=WINDOW, attention_scale=1.0, batch=B, max_seq=128, prefill_chunk=96)
    try:
        _run(g, q, k, v, 0, 96, 96, 99)
        with pytest.raises(ValueError):
            g.rewind(100)                                         # beyond what was written
        g.rewind(keep)
        assert g.state()["length"] == keep
        got = _run(g, q2, k2, v2, keep, 110, 96, 112)
        _run(fresh, q2, k2, v2, 0, keep, 96, keep)
        want = _run(fresh, q2, k2, v2, keep, 110, 96, 112)
        assert np.array_equal(got, want)
        assert_bf16_close(got, orc.gqa_attention(q2, _quantize(k2)[2], _quantize(v2)[2], 0, WINDOW, 1.0)[:, keep:], 1, 2e-3, "continuation after rewind")
    finally:
        g.close()
        fresh.close()


@pytest.mark.parametrize("which", ["prefillFromCache", "keyCache", "valueCache"])
def test_the_fused_entries_surface_throws_logic_error(which):
    q, k, v = _tokens(4, 1, 3)
    g8 = host.GqaComponent("fp8", NH, NKV, HS, batch=1, max_seq=16)
    g16 = host.GqaComponent("none", NH, NKV, HS, batch=1, max_seq=16)
    try:
        for g in (g8, g16):
            _run(g, q, k, v, 0, 3, 3, 3)
        g16.fused_surface_probe(which)                            # the bf16 policies have these methods
        with pytest.raises(TypeError, match="logic_error: RocmGqaKvFp8Op::%s: the fused q/k/v entries write a bf16 cache" % which):
            g8.fused_surface_probe(which)
        assert b"the fused q/k/v entries write a bf16 cache" in host.load().mila_host_last_error()
    finally:
        g8.close()
        g16.close()
