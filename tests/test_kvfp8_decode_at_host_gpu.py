"""RocmGqaKvFp8Op on the long band through the host mirror (libmila_host.so: host/src/gqa_runner.cpp): GroupedQueryAttention<Rocm, BF16, PerChannelKvFp8<>> at the
global-layer geometry with an 8192-row cache -- decode() from 4097 keys on runs the matrix-core kernel, decodeAt() is the same step with the position in device memory,
and noteCacheLength() is how the caller of decodeAt() reports the length afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gpu_util import assert_bf16_close, bits, dev_f32, dev_u8, dev_u16, empty_u16
from mila_amd import capi, host

pytestmark = pytest.mark.gpu

NH, NKV, HS, CAP = 16, 1, 512, 8192


def _bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def _b(x):
    return orc.to_bf16_bits(x)


def _dequantized(x):
    q, s = orc.quantize_fp8_per_channel(_b(x).reshape(-1, x.shape[-1]))
    return orc.round_bf16(orc.dequant_fp8(q, s)).reshape(x.shape)


def _capi_decode(g, q_bits, length):
    """attn_decode_kvfp8 on a copy of the cache arrays the component holds"""
    K8, V8, Ks, Vs = g.read_cache()
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(1, NH, HS)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    Y = empty_u16(1, NH * HS)
    capi.last_form()
    capi.call("attn_decode_kvfp8", Y, dev_u16(q_bits), dev_u8(K8), dev_u8(V8), dev_f32(Ks), dev_f32(Vs), scratch, C.c_size_t(nbytes), 1, NH, NKV, HS, CAP, length, 0, 1.0)
    assert capi.last_form() == ["attn_decode_kvfp8_mfma"]
    return bits(Y)


def test_decode_and_decode_at_on_the_long_band():
    """4100 tokens of prefill in chunks of 1025, three decode() steps, three decodeAt() steps from a device position: every step gives the bits of attn_decode_kvfp8 on
    the same cache contents (the matrix-core form: the 8192 bucket) and sits within the bar of the oracle on the dequantized history"""
    rng = np.random.default_rng(11)
    T0, T = 4100, 4106
    k = _bf(rng.uniform(-1, 1, (1, T, NKV, HS)) * 0.5)
    v = _bf(rng.uniform(-1, 1, (1, T, NKV, HS)))
    qd = _bf(rng.uniform(-1, 1, (1, T - T0, NH, HS)))                      # the decode steps' queries
    qp = _b(rng.uniform(-1, 1, (1, 1025, NH * HS)))                        # (the prefill's outputs are not looked at)
    dk, dv = _dequantized(k), _dequantized(v)
    g = host.GqaComponent("fp8", NH, NKV, HS, attention_scale=1.0, batch=1, max_seq=CAP, prefill_chunk=1025)
    try:
        for s in range(0, T0, 1025):
            g.prefill(qp, _b(k[:, s:s + 1025]).reshape(1, 1025, -1), _b(v[:, s:s + 1025]).reshape(1, 1025, -1), s)
        assert g.state()["length"] == T0 and g.state()["capacity"] == CAP
        for i, t in enumerate(range(T0, T)):
            q_bits, k_bits, v_bits = _b(qd[:, i]).reshape(1, -1), _b(k[:, t]).reshape(1, -1), _b(v[:, t]).reshape(1, -1)
            if t < T0 + 3:
                y = g.decode(q_bits, k_bits, v_bits, t)
                assert g.state()["length"] == t + 1
            else:
                # max_len: the live length itself, something in between, the bucket's upper end
                y = g.decode_at(q_bits, k_bits, v_bits, t, (t + 1, 6000, CAP)[t - T0 - 3])
                assert g.state()["length"] == T0 + 3                      # the op does not follow a device value
            assert np.array_equal(y, _capi_decode(g, q_bits, t + 1)), "step at position %d" % t
            assert_bf16_close(y, orc.gqa_attention(qd[:, i:i + 1], dk[:, :t + 1], dv[:, :t + 1], t, 0, 1.0)[:, 0], 1, 2e-3, "host fp8 decode at %d" % t)
        g.note_cache_length(T)
        assert g.state()["length"] == T
        g.rewind(T0)                                                      # ... and the lifecycle goes on from the reported length
        assert g.state()["length"] == T0
        with pytest.raises(ValueError, match="noteCacheLength"):
            g.note_cache_length(CAP + 1)
        with pytest.raises(ValueError):
            g.note_cache_length(-1)
        with pytest.raises(ValueError):
            g.decode_at(q_bits, k_bits, v_bits, T0, CAP + 1)              # max_len beyond the capacity: the entry's own check
    finally:
        g.close()


def test_the_bf16_policies_have_no_device_position_decode():
    g = host.GqaComponent("none", NH, NKV, HS, batch=1, max_seq=64)
    try:
        z = np.zeros((1, NH * HS), np.uint16)
        with pytest.raises(TypeError, match="only the PerChannelKvFp8<> op has a device-position decode"):
            g.decode_at(z, z[:, :NKV * HS], z[:, :NKV * HS], 0, 1)
    finally:
        g.close()
