"""GPU parity of the FP8 KV cache (Quant::KvCache::PerChannelKvFp8<>, csrc/attention_kvfp8.hip) through the C ABI: the quantizing append bit for bit against the
weight quantizer's oracle, the band dequant bit for bit, decode and chunked prefill against the float64 oracle ON THE DEQUANTIZED HISTORY -- a cached value is
bf16(float(e4m3) * scale), so given those values it is the bf16 cache's problem and the bf16 cache's bar: <= 1 bf16 ulp + 2e-3 abs (tests/test_attention_gpu.py).
Dead cache rows are poisoned with byte 0x7F (the e4m3 NaN) and a NaN scale: a result containing NaN means a dead row was read."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gpu_util import assert_bf16_close, bits, dev_u16, empty_u16, host
from mila_amd import capi
from test_attention_gpu import GEOMS

pytestmark = pytest.mark.gpu

POISON8, NAN_BITS = 0x7F, 0x7fc0
BF16_MAX = float(np.array([0x7f7f0000], dtype=np.uint32).view(np.float32)[0])      # the largest finite bf16


def _bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def _d(x):
    return dev_u16(orc.to_bf16_bits(x))


def _quantize(x):
    """oracle quantization of the rows x[..., HS] (bf16-representable floats): (bytes like x, scales x.shape[:-1], dequantized values like x)"""
    HS = x.shape[-1]
    q, s = orc.quantize_fp8_per_channel(orc.to_bf16_bits(x).reshape(-1, HS))
    deq = orc.round_bf16(orc.dequant_fp8(q, s))
    return q.reshape(x.shape), s.reshape(x.shape[:-1]), deq.reshape(x.shape)


class Cache8:
    """a poisoned FP8 cache on the device"""

    def __init__(self, B, NKV, cap, HS):
        self.B, self.NKV, self.cap, self.HS = B, NKV, cap, HS
        self.K8 = torch.full((B, NKV, cap, HS), POISON8, dtype=torch.uint8, device="cuda")
        self.V8 = torch.full((B, NKV, cap, HS), POISON8, dtype=torch.uint8, device="cuda")
        self.Ks = torch.full((B, NKV, cap), float("nan"), dtype=torch.float32, device="cuda")
        self.Vs = torch.full((B, NKV, cap), float("nan"), dtype=torch.float32, device="cuda")

    def arrays(self):
        return self.K8, self.V8, self.Ks, self.Vs

    def write(self, k, v, start):
        """k, v [B, chunk, NKV, HS] floats"""
        capi.call("kv_write_fp8", *self.arrays(), _d(k), _d(v), self.B, k.shape[1], self.NKV, self.HS, start, self.cap)

    def fill(self, hk, hv, chunk):
        for s in range(0, hk.shape[1], chunk):
            self.write(hk[:, s:s + chunk], hv[:, s:s + chunk], s)
        return self

    def poison_rows(self, lo, hi):
        for t in (self.K8, self.V8):
            t[:, :, lo:hi] = POISON8
        for t in (self.Ks, self.Vs):
            t[:, :, lo:hi] = float("nan")


def _decode(cache, q, NH, length, window, scale):
    B, HS = cache.B, cache.HS
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(B, NH, HS)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    Y = empty_u16(B, NH * HS)
    capi.call("attn_decode_kvfp8", Y, _d(q), *cache.arrays(), scratch, C.c_size_t(nbytes), B, NH, cache.NKV, HS, cache.cap, length, window, float(scale))
    return bits(Y)


def _prefill(cache, q, NH, pos, window, scale):
    B, HS, T = cache.B, cache.HS, q.shape[1]
    nbytes = capi.load().mila_cdna4_attn_prefill_kvfp8_scratch_bytes(B, cache.NKV, HS, cache.cap)
    assert nbytes == 2 * B * cache.NKV * cache.cap * HS * 2
    scratch = torch.full((nbytes // 2,), NAN_BITS, dtype=torch.int16, device="cuda")      # a dead row of the transient caches that is read gives NaN
    Y = empty_u16(B, T, NH * HS)
    capi.call("attn_prefill_kvfp8", Y, _d(q), *cache.arrays(), scratch, C.c_size_t(nbytes), B, T, NH, cache.NKV, HS, cache.cap, pos, window, float(scale))
    return bits(Y)


@pytest.mark.parametrize("HS", [64, 128, 256, 512])
def test_quantizing_write_is_bit_exact_and_follows_the_ring(HS):
    """23 tokens into a 10-row ring in chunks of 7 (it wraps twice): bytes and scales of every row equal orc.quantize_fp8_per_channel on that row -- an all-zero row
    (scale 1) and a row whose absmax is the largest finite bf16 among them -- and rows never written keep the poison"""
    rng = np.random.default_rng(HS)
    B, NKV, cap, T = 2, 2, 10, 23
    hk, hv = _bf(rng.standard_normal((B, T, NKV, HS))), _bf(rng.standard_normal((B, T, NKV, HS)))
    hk[0, 15, 1] = 0.0
    hv[1, 16, 0] = 0.0
    hk[1, 20, 0] = _bf(rng.uniform(-1, 1, HS) * BF16_MAX)
    hk[1, 20, 0, HS // 3] = BF16_MAX
    hv[0, 21, 1] = _bf(rng.uniform(-1, 1, HS) * BF16_MAX)
    hv[0, 21, 1, 5] = -BF16_MAX
    qk, sk, _ = _quantize(hk)
    qv, sv, _ = _quantize(hv)
    assert sk[0, 15, 1] == 1.0 and sk[1, 20, 0] == np.float32(BF16_MAX) / np.float32(448.0)
    eK8, eV8 = np.full((B, NKV, cap, HS), POISON8, np.uint8), np.full((B, NKV, cap, HS), POISON8, np.uint8)
    eKs, eVs = np.full((B, NKV, cap), np.nan, np.float32), np.full((B, NKV, cap), np.nan, np.float32)
    c = Cache8(B, NKV, cap, HS)
    for s in range(0, T, 7):
        e = min(T, s + 7)
        c.write(hk[:, s:e], hv[:, s:e], s)
        for t in range(s, e):
            eK8[:, :, t % cap], eV8[:, :, t % cap] = qk[:, t], qv[:, t]
            eKs[:, :, t % cap], eVs[:, :, t % cap] = sk[:, t], sv[:, t]
        # (after the first chunk rows 7 .. 9 have never been written: they must still hold the poison)
        assert np.array_equal(host(c.K8), eK8) and np.array_equal(host(c.V8), eV8), "bytes after the chunk at %d" % s
        assert np.array_equal(host(c.Ks).view(np.uint32), eKs.view(np.uint32)) and np.array_equal(host(c.Vs).view(np.uint32), eVs.view(np.uint32)), "scales after the chunk at %d" % s
    with pytest.raises(capi.InvalidArgument):
        capi.call("kv_write_fp8", *c.arrays(), _d(hk), _d(hv), B, T, NKV, HS, 0, cap)    # chunk > capacity


@pytest.mark.parametrize("HS", [64, 256])
def test_band_dequant_is_bit_exact_and_writes_the_band_only(HS):
    """positions 20 .. 34 of a 23-row ring that holds 17 .. 39: rows 20, 21, 22, 0 .. 11"""
    rng = np.random.default_rng(HS + 1)
    B, NKV, cap, T, first, count = 2, 3, 23, 40, 20, 15
    hk, hv = _bf(rng.standard_normal((B, T, NKV, HS))), _bf(rng.standard_normal((B, T, NKV, HS)) * 3.0)
    c = Cache8(B, NKV, cap, HS).fill(hk, hv, 9)
    Kd, Vd = empty_u16(B, NKV, cap, HS), empty_u16(B, NKV, cap, HS)
    capi.call("kv_dequant_fp8_bf16", Kd, Vd, *c.arrays(), B, NKV, HS, cap, first, count)
    eK, eV = np.full((B, NKV, cap, HS), NAN_BITS, np.uint16), np.full((B, NKV, cap, HS), NAN_BITS, np.uint16)
    dk, dv = _quantize(hk)[2], _quantize(hv)[2]
    for t in range(first, first + count):
        eK[:, :, t % cap], eV[:, :, t % cap] = orc.to_bf16_bits(dk[:, t]), orc.to_bf16_bits(dv[:, t])
    assert np.array_equal(bits(Kd), eK) and np.array_equal(bits(Vd), eV)
    with pytest.raises(capi.InvalidArgument):
        capi.call("kv_dequant_fp8_bf16", Kd, Vd, *c.arrays(), B, NKV, HS, cap, 0, cap + 1)


@pytest.mark.parametrize("name,NH,NKV,HS,window,scale", GEOMS)
@pytest.mark.parametrize("length", [1, 2, 37, 300, 1500])
def test_decode_attention(name, NH, NKV, HS, window, scale, length):
    rng = np.random.default_rng(length + HS)
    B, cap = (2 if HS <= 128 else 1), 2048
    hk = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, 1, NH, HS)))
    c = Cache8(B, NKV, cap, HS).fill(hk, hv, 512)
    if window > 0 and length > window:      # rows older than the band must never be read
        c.poison_rows(0, length - window)
    exp = orc.gqa_attention(q, _quantize(hk)[2], _quantize(hv)[2], length - 1, window, scale)[:, 0]
    capi.last_form()                        # (clears the record)
    assert_bf16_close(_decode(c, q, NH, length, window, scale), exp, 1, 2e-3, "fp8 decode %s len %d" % (name, length))
    assert capi.last_form() == ["attn_decode_kvfp8"]


@pytest.mark.parametrize("window,cap,length", [(8, 8, 30), (16, 23, 100), (1024, 1100, 2600)])
def test_decode_attention_bounded_ring_equals_unbounded(window, cap, length):
    """the same plan over the same values: the ring and the unbounded cache give the same bits (the reference's ring-vs-unbounded test, CudaGqaOp.Cuda.cpp:529-567)"""
    rng = np.random.default_rng(cap)
    B, NH, NKV, HS = 1, 16, 8, 256
    hk = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, 1, NH, HS)))
    ring = Cache8(B, NKV, cap, HS).fill(hk, hv, min(cap, 7) if cap < 64 else 64)
    flat = Cache8(B, NKV, length, HS).fill(hk, hv, 512)
    flat.poison_rows(0, length - window)
    exp = orc.gqa_attention(q, _quantize(hk)[2], _quantize(hv)[2], length - 1, window, 1.0)[:, 0]
    y_ring, y_flat = _decode(ring, q, NH, length, window, 1.0), _decode(flat, q, NH, length, window, 1.0)
    assert_bf16_close(y_ring, exp, 1, 2e-3, "fp8 ring decode")
    assert_bf16_close(y_flat, exp, 1, 2e-3, "fp8 unbounded decode")
    assert np.array_equal(y_ring, y_flat)
    with pytest.raises(capi.InvalidArgument):     # band larger than the ring
        _decode(ring, q, NH, length, 0, 1.0)


def test_decode_online_softmax_rescale_branch_is_exercised():
    """the construction of tests/test_attention_gpu.py on the fp8 cache: one spiked key late in the band (a later split holds the maximum) and one early"""
    rng = np.random.default_rng(9)
    B, NH, NKV, HS, length = 1, 16, 1, 512, 777
    hk = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)) * 0.1)
    hv = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, 1, NH, HS)))
    hk[0, 700, 0] = _bf(q[0, 0, 3] * 0.5)           # large positive score for head 3 at position 700
    hk[0, 5, 0] = _bf(q[0, 0, 7] * 0.5)
    c = Cache8(B, NKV, 1024, HS).fill(hk, hv, 256)
    dk, dv = _quantize(hk)[2], _quantize(hv)[2]
    exp = orc.gqa_attention(q, dk, dv, length - 1, 0, 1.0)[:, 0]
    # the spike survives the quantization: head 3's score at 700 towers over the rest of its band
    s3 = (dk[0, :, 0].astype(np.float64) @ q[0, 0, 3].astype(np.float64))
    assert s3.argmax() == 700 and s3[700] > np.delete(s3, 700).max() + 20.0
    assert capi.attn_decode_plan(B, NH, NKV, HS, 1024, 0, length)["splits"] > 1
    assert_bf16_close(_decode(c, q, NH, length, 0, 1.0), exp, 1, 2e-3, "spiked fp8 decode")


def _prefill_cases():
    for name, NH, NKV, HS, window, scale in GEOMS:
        yield name, NH, NKV, HS, window, scale
        if window > 0:
            yield name + "_w64", NH, NKV, HS, 64, scale


@pytest.mark.parametrize("name,NH,NKV,HS,window,scale", list(_prefill_cases()))
def test_prefill_attention_chunked(name, NH, NKV, HS, window, scale):
    """300 tokens in chunks of 128: the fp8 prefill (band dequant + the bf16 flash kernels) gives the bits of attn_prefill_bf16 on a bf16 cache filled with the
    dequantized values, and sits within the bar of the oracle"""
    rng = np.random.default_rng(HS + NH + window)
    B, T, cap = 1, 300, 320
    hk = _bf(rng.uniform(-1, 1, (B, T, NKV, HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (B, T, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, T, NH, HS)))
    dk, dv = _quantize(hk)[2], _quantize(hv)[2]
    c = Cache8(B, NKV, cap, HS)
    Kc = torch.full((B, NKV, cap, HS), NAN_BITS, dtype=torch.int16, device="cuda")
    Vc = torch.full((B, NKV, cap, HS), NAN_BITS, dtype=torch.int16, device="cuda")
    Y8, Y16 = np.empty((B, T, NH * HS), np.uint16), np.empty((B, T, NH * HS), np.uint16)
    for s in range(0, T, 128):
        e = min(T, s + 128)
        c.write(hk[:, s:e], hv[:, s:e], s)
        Y8[:, s:e] = _prefill(c, q[:, s:e], NH, s, window, scale)
        capi.call("kv_write_bf16", Kc, Vc, _d(dk[:, s:e]), _d(dv[:, s:e]), B, e - s, NKV, HS, s, cap)
        Yc = empty_u16(B, e - s, NH * HS)
        capi.call("attn_prefill_bf16", Yc, _d(q[:, s:e]), Kc, Vc, B, e - s, NH, NKV, HS, cap, s, window, float(scale))
        Y16[:, s:e] = bits(Yc)
    assert np.array_equal(Y8, Y16), "the fp8 prefill differs from the bf16 prefill on the dequantized cache"
    assert_bf16_close(Y8, orc.gqa_attention(q, dk, dv, 0, window, scale), 1, 2e-3, "fp8 prefill %s" % name)


@pytest.mark.parametrize("name,NH,NKV,HS,window,scale", [("gemma_local_w64", 16, 8, 256, 64, 1.0), ("gemma_global", 16, 1, 512, 0, 1.0), ("llama", 32, 8, 128, 0, 128 ** -0.5)])
def test_prefill_then_decode_on_one_cache(name, NH, NKV, HS, window, scale):
    """two chunks and three decode steps: a write / read disagreement about rows or scales shows at the first step that crosses it"""
    rng = np.random.default_rng(HS * 3 + NH)
    B, T, cap = 2, 94, 128
    hk = _bf(rng.uniform(-1, 1, (B, T, NKV, HS)) * 0.5)
    # row scales that differ by up to 10 x (a scale read from the wrong row is far outside the bar), values inside [-1, 1]: the bar is the bf16 cache's, whose flash
    # prefill rounds the probabilities to bf16 for the PV product -- an error that grows with |V|, and 2e-3 abs was set for V drawn from [-1, 1]
    hv = _bf(rng.uniform(-1, 1, (B, T, NKV, HS)) * rng.uniform(0.1, 1.0, (B, T, NKV, 1)))
    q = _bf(rng.uniform(-1, 1, (B, T, NH, HS)))
    exp = orc.gqa_attention(q, _quantize(hk)[2], _quantize(hv)[2], 0, window, scale)
    c = Cache8(B, NKV, cap, HS)
    for s, e in ((0, 50), (50, 91)):
        c.write(hk[:, s:e], hv[:, s:e], s)
        assert_bf16_close(_prefill(c, q[:, s:e], NH, s, window, scale), exp[:, s:e], 1, 2e-3, "%s prefill [%d, %d)" % (name, s, e))
    for t in range(91, 94):
        c.write(hk[:, t:t + 1], hv[:, t:t + 1], t)
        assert_bf16_close(_decode(c, q[:, t:t + 1], NH, t + 1, window, scale), exp[:, t], 1, 2e-3, "%s decode at %d" % (name, t))
