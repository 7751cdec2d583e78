"""The matrix-core decode over the FP8 KV cache (attn_decode_kvfp8_mfma_kernel: csrc/attention_decode_mfma.h under the e4m3 staging policy) and the device-position
forms of the fp8 cache's append and decode, through the C ABI.

Bars: the float64 oracle on the DEQUANTIZED history within <= 1 bf16 ulp + 2e-3 abs (tests/test_kvfp8_gpu.py: given the cached values bf16(float(e4m3) * scale) it is
the bf16 cache's problem and the bf16 cache's bar); and, wherever both caches take their matrix-core kernels, the BITS of attn_decode_bf16 on a bf16 cache filled with
the dequantized values -- same plan, same tile body, same values in the same order.  The small cases set attn.mfma_min_band to 256 so that a 1024-row cache takes the
matrix-core form with 8 splits of up to four 32-key tiles.  Dead rows hold byte 0x7F and NaN scales (NaN bf16 values in the bf16 cache): a NaN in an output means a
dead row was read."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import orc
from gpu_util import assert_bf16_close, bits, dev_i32, empty_u16, host
from mila_amd import capi
from test_kvfp8_gpu import NAN_BITS, POISON8, Cache8, _bf, _d, _decode, _quantize

pytestmark = pytest.mark.gpu

MFMA8, SCALAR8, MFMA16 = "attn_decode_kvfp8_mfma", "attn_decode_kvfp8", "attn_decode_mfma"


@pytest.fixture
def small_bands():
    """a 1024-row cache takes the matrix-core forms: attn.mfma_min_band 256"""
    capi.tune("attn.mfma_min_band", 256)
    try:
        yield
    finally:
        capi.tune_reset()


@functools.lru_cache(maxsize=None)
def _history(B, NKV, T, seed, HS=512):
    """K uniform +-0.5, V uniform +-1 (tests/test_kvfp8_gpu.py), their dequantized values, all [B, T, NKV, HS]; computed once per shape, never modified"""
    rng = np.random.default_rng(seed)
    hk, hv = _bf(rng.uniform(-1, 1, (B, T, NKV, HS)) * 0.5), _bf(rng.uniform(-1, 1, (B, T, NKV, HS)))
    return hk, hv, _quantize(hk)[2], _quantize(hv)[2]


def _query(B, NH, seed, HS=512):
    return _bf(np.random.default_rng(seed).uniform(-1, 1, (B, 1, NH, HS)))


class Cache16:
    """a bf16 cache whose dead rows hold NaN"""

    def __init__(self, B, NKV, cap, HS):
        self.B, self.NKV, self.cap, self.HS = B, NKV, cap, HS
        self.K = torch.full((B, NKV, cap, HS), NAN_BITS, dtype=torch.int16, device="cuda")
        self.V = torch.full((B, NKV, cap, HS), NAN_BITS, dtype=torch.int16, device="cuda")

    def fill(self, dk, dv, chunk):
        for s in range(0, dk.shape[1], chunk):
            e = min(dk.shape[1], s + chunk)
            capi.call("kv_write_bf16", self.K, self.V, _d(dk[:, s:e]), _d(dv[:, s:e]), self.B, e - s, self.NKV, self.HS, s, self.cap)
        return self

    def poison_rows(self, lo, hi):
        self.K[:, :, lo:hi] = NAN_BITS
        self.V[:, :, lo:hi] = NAN_BITS


def _scratch(B, NH, HS):
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(B, NH, HS)
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


def _decode16(cache, q, NH, length, window, scale):
    scratch, nbytes = _scratch(cache.B, NH, cache.HS)
    Y = empty_u16(cache.B, NH * cache.HS)
    capi.call("attn_decode_bf16", Y, _d(q), cache.K, cache.V, scratch, C.c_size_t(nbytes), cache.B, NH, cache.NKV, cache.HS, cache.cap, length, window, float(scale))
    return bits(Y)


def _decode_devpos(cache, q, NH, position, max_len, window, scale):
    scratch, nbytes = _scratch(cache.B, NH, cache.HS)
    Y = empty_u16(cache.B, NH * cache.HS)
    pos = dev_i32([position])
    capi.call("attn_decode_kvfp8_devpos", Y, _d(q), *cache.arrays(), scratch, C.c_size_t(nbytes), cache.B, NH, cache.NKV, cache.HS, cache.cap, pos, max_len, window, float(scale))
    return bits(Y)


def _both_forms(c8, c16, q, NH, length, window, scale, exp, what):
    """the fp8 decode against the oracle and against the bf16 decode's bits, each on its matrix-core kernel"""
    capi.last_form()
    y8 = _decode(c8, q, NH, length, window, scale)
    assert capi.last_form() == [MFMA8], what
    y16 = _decode16(c16, q, NH, length, window, scale)
    assert capi.last_form() == [MFMA16], what
    assert_bf16_close(y8, exp, 1, 2e-3, what)
    assert np.array_equal(y8, y16), "%s: the fp8 decode differs from attn_decode_bf16 on the dequantized cache" % what
    return y8


@pytest.mark.parametrize("length", [1, 5, 33, 130, 1000, 1024])
def test_matrix_core_decode_against_the_oracle_and_the_bf16_form(small_bands, length):
    """1: a single key; 5: splits 5-7 are empty; 33: one full tile plus one key; 130: 17 keys per split, one partial tile each; 1000: three full tiles and a 29-key one
    per split; 1024: four full tiles per split"""
    B, NH, NKV, HS, cap = 1, 16, 1, 512, 1024
    hk, hv, dk, dv = (a[:, :length] for a in _history(B, NKV, cap, 1))
    q = _query(B, NH, length)
    assert capi.attn_decode_kvfp8_plan(B, NH, NKV, HS, cap, 0, length)["splits"] == 8
    c8 = Cache8(B, NKV, cap, HS).fill(hk, hv, 512)
    c16 = Cache16(B, NKV, cap, HS).fill(dk, dv, 512)
    exp = orc.gqa_attention(q, dk, dv, length - 1, 0, 1.0)[:, 0]
    _both_forms(c8, c16, q, NH, length, 0, 1.0, exp, "fp8 matrix-core decode len %d" % length)


@pytest.mark.parametrize("B,NH,NKV", [(2, 32, 1), (1, 32, 2)], ids=["two_head_groups_on_one_kv_head", "two_kv_heads"])
def test_head_grouping(small_bands, B, NH, NKV):
    HS, cap, length = 512, 1024, 300
    hk, hv, dk, dv = (a[:, :length] for a in _history(B, NKV, cap, 2))
    q = _query(B, NH, NH + NKV)
    c8 = Cache8(B, NKV, cap, HS).fill(hk, hv, 512)
    c16 = Cache16(B, NKV, cap, HS).fill(dk, dv, 512)
    exp = orc.gqa_attention(q, dk, dv, length - 1, 0, 1.0)[:, 0]
    _both_forms(c8, c16, q, NH, length, 0, 1.0, exp, "fp8 matrix-core decode B %d NH %d NKV %d" % (B, NH, NKV))


def test_ring_equals_unbounded(small_bands):
    """window 300 in a 320-row ring at length 1000: the band wraps, 3 splits; an unbounded cache of 1000 rows whose rows below 700 are dead gives the same bits"""
    B, NH, NKV, HS, window, cap, length = 1, 16, 1, 512, 300, 320, 1000
    hk, hv, dk, dv = (a[:, :length] for a in _history(B, NKV, 1024, 3))
    q = _query(B, NH, 3)
    assert capi.attn_decode_kvfp8_plan(B, NH, NKV, HS, cap, window, length) == dict(capi.attn_decode_kvfp8_plan(B, NH, NKV, HS, length, window, length), form=MFMA8)
    assert capi.attn_decode_kvfp8_plan(B, NH, NKV, HS, cap, window, length)["splits"] == 3
    ring8, ring16 = Cache8(B, NKV, cap, HS).fill(hk, hv, 64), Cache16(B, NKV, cap, HS).fill(dk, dv, 64)
    flat8, flat16 = Cache8(B, NKV, length, HS).fill(hk, hv, 500), Cache16(B, NKV, length, HS).fill(dk, dv, 500)
    flat8.poison_rows(0, length - window)
    flat16.poison_rows(0, length - window)
    exp = orc.gqa_attention(q, dk, dv, length - 1, window, 1.0)[:, 0]
    y_ring = _both_forms(ring8, ring16, q, NH, length, window, 1.0, exp, "fp8 ring decode")
    y_flat = _both_forms(flat8, flat16, q, NH, length, window, 1.0, exp, "fp8 unbounded decode")
    assert np.array_equal(y_ring, y_flat)


def test_online_softmax_rescale_branch_is_exercised(small_bands):
    """the spiked-key construction of tests/test_kvfp8_gpu.py at length 777 in the 1024-row cache (8 splits of 98 keys, four tiles each): head 3's maximum sits in the
    last tile of split 7 (position 770: tiles before it are rescaled), head 7's in the first tile of split 0 (position 5)"""
    rng = np.random.default_rng(9)
    B, NH, NKV, HS, length, cap = 1, 16, 1, 512, 777, 1024
    hk = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)) * 0.1)
    hv = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, 1, NH, HS)))
    hk[0, 770, 0] = _bf(q[0, 0, 3] * 0.5)
    hk[0, 5, 0] = _bf(q[0, 0, 7] * 0.5)
    dk, dv = _quantize(hk)[2], _quantize(hv)[2]
    # the spikes survive the quantization: each towers over the rest of its head's band
    for head, at in ((3, 770), (7, 5)):
        s = dk[0, :, 0].astype(np.float64) @ q[0, 0, head].astype(np.float64)
        assert s.argmax() == at and s[at] > np.delete(s, at).max() + 20.0
    chunk = -(-length // 8)
    assert 770 // chunk == 7 and (770 - 7 * chunk) // 32 == 2 and 7 * chunk + 3 * 32 > length      # split 7's third and last tile
    c8 = Cache8(B, NKV, cap, HS).fill(hk, hv, 256)
    c16 = Cache16(B, NKV, cap, HS).fill(dk, dv, 256)
    exp = orc.gqa_attention(q, dk, dv, length - 1, 0, 1.0)[:, 0]
    _both_forms(c8, c16, q, NH, length, 0, 1.0, exp, "spiked fp8 matrix-core decode")


@functools.lru_cache(maxsize=None)
def _long_cache():
    """the 8192-row cache of the default rule (4 MB per operand), filled once"""
    B, NKV, HS, cap = 1, 1, 512, 8192
    hk, hv, dk, dv = _history(B, NKV, cap, 4)
    return Cache8(B, NKV, cap, HS).fill(hk, hv, 2048), dk, dv


@pytest.mark.parametrize("length,form,splits", [(4096, SCALAR8, 32), (4097, MFMA8, 64), (8192, MFMA8, 64)])
def test_default_rule_without_tuning(length, form, splits):
    """capacity 8192: up to 4096 keys (the 4096 bucket) the wave-per-position kernel, from 4097 (the 8192 bucket) the matrix-core one with 64 splits"""
    B, NH, NKV, HS, cap = 1, 16, 1, 512, 8192
    c8, dk, dv = _long_cache()
    q = _query(B, NH, length)
    p = capi.attn_decode_kvfp8_plan(B, NH, NKV, HS, cap, 0, length)
    assert p["form"] == form and p["splits"] == splits
    capi.last_form()
    y = _decode(c8, q, NH, length, 0, 1.0)
    assert capi.last_form() == [form]
    assert_bf16_close(y, orc.gqa_attention(q, dk[:, :length], dv[:, :length], length - 1, 0, 1.0)[:, 0], 1, 2e-3, "fp8 decode len %d" % length)


def test_the_other_kernel_serves_the_long_band_too():
    """attn.kvfp8_mfma_decode 0: the 8192-key case on the wave-per-position kernel, the same oracle bar -- two kernels, one function"""
    B, NH, NKV, HS, cap, length = 1, 16, 1, 512, 8192, 8192
    c8, dk, dv = _long_cache()
    q = _query(B, NH, length)
    exp = orc.gqa_attention(q, dk, dv, length - 1, 0, 1.0)[:, 0]
    try:
        capi.tune("attn.kvfp8_mfma_decode", 0)
        capi.last_form()
        y_scalar = _decode(c8, q, NH, length, 0, 1.0)
        assert capi.last_form() == [SCALAR8]
    finally:
        capi.tune_reset()
    y_mfma = _decode(c8, q, NH, length, 0, 1.0)
    assert capi.last_form() == [MFMA8]
    assert_bf16_close(y_scalar, exp, 1, 2e-3, "fp8 decode len 8192, scalar kernel")
    assert_bf16_close(y_mfma, exp, 1, 2e-3, "fp8 decode len 8192, matrix-core kernel")


def _devpos_append_and_decode(c8, hk, hv, q, NH, position, window, bucket_end, form):
    """the token at `position` appended through kv_write_fp8_devpos into c8 (which holds the tokens before it): bytes and scales of kv_write_fp8, no other row touched;
    then attn_decode_kvfp8_devpos at max_len = position + 1 and at the bucket's upper end gives attn_decode_kvfp8's bits"""
    B, NKV, HS, cap = c8.B, c8.NKV, c8.HS, c8.cap
    row = position % cap
    before = [host(t).copy() for t in c8.arrays()]
    k1, v1 = hk[:, position:position + 1], hv[:, position:position + 1]
    capi.call("kv_write_fp8_devpos", *c8.arrays(), _d(k1), _d(v1), B, NKV, HS, dev_i32([position]), cap)
    ref = Cache8(B, NKV, cap, HS)
    ref.write(k1, v1, position)
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8)      # (bit patterns: the dead rows' scales are NaN)
    for got, was, want in zip(c8.arrays(), before, ref.arrays()):
        got, want = host(got), host(want)
        assert np.array_equal(raw(got[:, :, row]), raw(want[:, :, row])), "the appended row at %d" % position
        was[:, :, row] = got[:, :, row]
        assert np.array_equal(raw(got), raw(was)), "another row changed at %d" % position
    capi.last_form()
    eager = _decode(c8, q, NH, position + 1, window, 1.0)
    assert capi.last_form() == [form]
    for max_len in (position + 1, bucket_end):
        y = _decode_devpos(c8, q, NH, position, max_len, window, 1.0)
        assert capi.last_form() == [form]
        assert np.array_equal(y, eager), "position %d, max_len %d" % (position, max_len)
    return eager


def test_device_position_on_the_small_cache(small_bands):
    """positions 129, 130 in the 1024-row cache: lengths 130 (17 keys per split) and 131 on either side of a split's tile count; the bucket is the capacity"""
    B, NH, NKV, HS, cap = 1, 16, 1, 512, 1024
    hk, hv, dk, dv = _history(B, NKV, cap, 1)
    c8 = Cache8(B, NKV, cap, HS).fill(hk[:, :129], hv[:, :129], 129)
    for position in (129, 130):
        q = _query(B, NH, position)
        y = _devpos_append_and_decode(c8, hk, hv, q, NH, position, 0, cap, MFMA8)
        assert_bf16_close(y, orc.gqa_attention(q, dk[:, :position + 1], dv[:, :position + 1], position, 0, 1.0)[:, 0], 1, 2e-3, "devpos decode at %d" % position)


def test_device_position_on_the_long_cache():
    """positions 4100, 4101 in an 8192-row cache, no tuning: the 8192 bucket, 64 splits of 65 keys, the last one of 6 and 7 keys"""
    B, NH, NKV, HS, cap = 1, 16, 1, 512, 8192
    hk, hv, dk, dv = _history(B, NKV, cap, 4)
    c8 = Cache8(B, NKV, cap, HS).fill(hk[:, :4100], hv[:, :4100], 2050)
    assert capi.load().mila_cdna4_attn_decode_band_bucket(4101, cap) == 8192
    for position in (4100, 4101):
        q = _query(B, NH, position)
        y = _devpos_append_and_decode(c8, hk, hv, q, NH, position, 0, 8192, MFMA8)
        assert_bf16_close(y, orc.gqa_attention(q, dk[:, :position + 1], dv[:, :position + 1], position, 0, 1.0)[:, 0], 1, 2e-3, "devpos decode at %d" % position)
    with pytest.raises(capi.InvalidArgument):
        _decode_devpos(c8, _query(B, NH, 0), NH, 4101, 8193, 0, 1.0)      # max_len beyond the capacity


def test_device_position_on_the_scalar_form():
    """HS 256, NKV 8, window 1024 in a 1100-row ring: the wave-per-position kernel reads the position from the device too; position 2599 wraps the ring"""
    B, NH, NKV, HS, window, cap = 1, 16, 8, 256, 1024, 1100
    T = 2601
    hk, hv, dk, dv = _history(B, NKV, T, 5, HS)
    c8 = Cache8(B, NKV, cap, HS).fill(hk[:, :2599], hv[:, :2599], 64)
    for position in (2599, 2600):
        q = _query(B, NH, position, HS)
        y = _devpos_append_and_decode(c8, hk, hv, q, NH, position, window, T, SCALAR8)
        assert_bf16_close(y, orc.gqa_attention(q, dk[:, :position + 1], dv[:, :position + 1], position, window, 1.0)[:, 0], 1, 2e-3, "devpos scalar decode at %d" % position)
