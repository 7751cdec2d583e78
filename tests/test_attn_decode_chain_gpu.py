"""GPU: fused_attn_decode_chain_bf16 -- T consecutive positions of ONE sequence on ONE cache in one call -- against T successive fused_attn_decode_bf16 calls
(B = 1, device-position form, the same max_len) at position .. position + T - 1 on a copy of the same cache: Y rows, the appended cache rows and every other cache row
bit for bit, in the eager and in the device-position form.  The cache is NaN-poisoned from `position` on (and carries one more, poisoned, batch row that no launch may
touch), so a row that read a later row of the chain, or a stale one, could not pass."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gpu_util import bits, dev_i32, dev_u16, empty_f32, empty_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = [  # NH NKV HS window capacity rotary base kv_shared
    (4, 2, 64, 8, 64, 0, 1e4, False),
    (4, 1, 128, 0, 64, 0, 1e4, False),
    (16, 8, 256, 32, 96, 0, 1e4, False),
    (16, 1, 512, 0, 96, 128, 1e6, True),          # HS 512 on the wave-per-position kernel (a short band)
]
LONG = (16, 1, 512, 0, 8192, 128, 1e6, True)      # ... and on the matrix-core kernel with its prologue (the 8192 bucket)


def _d(x):
    return dev_u16(orc.to_bf16_bits(orc.round_bf16(np.asarray(x, dtype=np.float32))))


class _Case:
    def __init__(self, NH, NKV, HS, window, cap, rot, base, kv_shared, seed):
        rng = np.random.default_rng(seed)
        self.geo = (NH, NKV, HS, cap, window)
        g = torch.Generator(device="cuda").manual_seed(seed)
        hist = lambda s, scale: ((torch.rand(s, device="cuda", generator=g) * 2 - 1) * scale).to(torch.bfloat16).view(torch.int16)
        self.Kc, self.Vc = hist((2, NKV, cap, HS), 0.5), hist((2, NKV, cap, HS), 1.0)
        qn, kn = NH * HS, NKV * HS
        self.packed = qn + kn * (1 if kv_shared else 2) + 24      # the row stride need not be the sum of the parts
        self.raw = _d(rng.standard_normal((5, self.packed)))
        self.k_off, self.v_off = qn, (qn if kv_shared else qn + kn)
        self.qw, self.kw = _d(1 + 0.1 * rng.uniform(-1, 1, HS)), _d(1 + 0.1 * rng.uniform(-1, 1, HS))
        self.cos, self.sin = empty_f32(cap, HS // 2), empty_f32(cap, HS // 2)
        capi.call("rope_build_cache", self.cos, self.sin, cap, HS, float(base), rot)
        lib = capi.load()
        self.nbytes = max(lib.mila_cdna4_attn_decode_chain_scratch_bytes(4, NH, HS), lib.mila_cdna4_attn_decode_scratch_bytes(1, NH, HS))
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def poisoned(self, position):
        """the history up to `position`, NaN from there on; batch row 1 NaN throughout"""
        K, V = self.Kc.clone(), self.Vc.clone()
        for t in (K, V):
            t[0, :, position:, :] = 0x7fc0
            t[1] = 0x7fc0
        return K, V

    def alone(self, T, position, max_len):
        NH, NKV, HS, cap, window = self.geo
        K, V = self.poisoned(position)
        Y = empty_u16(T, NH * HS)
        for t in range(T):
            capi.call("fused_attn_decode_bf16", Y[t], K, V, self.raw[t], self.raw[t, self.k_off:], self.raw[t, self.v_off:], self.qw, self.kw, None, self.cos, self.sin,
                      self.scratch, C.c_size_t(self.nbytes), NH, NKV, HS, cap, max_len, dev_i32(np.array([position + t])), window, 1.0, 1e-6)
        return bits(Y), bits(K), bits(V)

    def chain(self, T, position, max_len, devpos):
        NH, NKV, HS, cap, window = self.geo
        K, V = self.poisoned(position)
        Y = empty_u16(T + 1, NH * HS)
        pd = dev_i32(np.array([position, 1 << 20])) if devpos else None      # (a second word a strided read would trip over)
        capi.call("fused_attn_decode_chain_bf16", Y, K, V, self.raw[0], self.raw[0, self.k_off:], self.raw[0, self.v_off:], C.c_int64(self.packed), self.qw, self.kw, None,
                  self.cos, self.sin, self.scratch, C.c_size_t(self.nbytes), T, NH, NKV, HS, cap, 0 if devpos else position, pd, max_len if devpos else 0, window, 1.0, 1e-6)
        if devpos:
            assert pd.cpu().tolist() == [position, 1 << 20]      # the entry reads the position word, it does not advance it
        return bits(Y), bits(K), bits(V)


def _check(case, T, position, what):
    NH, NKV, HS, cap, window = case.geo
    max_len = position + T
    y1, k1, v1 = case.alone(T, position, max_len)
    forms = set()
    for devpos in (False, True):
        capi.last_form()
        Y, K, V = case.chain(T, position, max_len, devpos)
        forms.update(capi.last_form())
        w = "%s T=%d position=%d %s" % (what, T, position, "device position" if devpos else "eager")
        for t in range(T):
            assert np.array_equal(Y[t], y1[t]), "%s: row %d differs from the row decoded alone" % (w, t)
        assert (Y[T] == 0x7fc0).all(), w + ": an output row past the chain was written"
        rows = slice(position, position + T)
        assert np.array_equal(K[0][:, rows], k1[0][:, rows]) and np.array_equal(V[0][:, rows], v1[0][:, rows]), w + ": appended cache rows differ"
        assert not (K[0][:, rows] == 0x7fc0).all() and not (V[0][:, rows] == 0x7fc0).all()
        # every other row: what the sequential calls leave, which is what was there
        K0, V0 = (bits(x) for x in case.poisoned(position))
        for got, seq, before in ((K, k1, K0), (V, v1, V0)):
            assert np.array_equal(got, seq), w + ": the cache differs from the sequential calls'"
            keep = np.ones(got.shape[2], dtype=bool)
            keep[rows] = False
            assert np.array_equal(got[0][:, keep], before[0][:, keep]) and np.array_equal(got[1], before[1]), w + ": a cache row outside the chain was written"
    return forms


@pytest.mark.parametrize("T", [2, 3, 4])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_chain_rows_equal_the_sequential_one_row_calls(shape, T):
    NH, NKV, HS, window, cap, rot, base, kv_shared = SHAPES[shape]
    case = _Case(*SHAPES[shape], seed=shape + 1)
    # 0 | the band start moves inside the chain (window - 2: row 2 is the first whose band no longer starts at 0) | mid-cache | the last rows of the cache
    positions = [0, 37, cap - T] + ([window - 2] if window else [])
    for position in positions:
        forms = _check(case, T, position, "shape %d" % shape)
        assert forms == {"attn_decode"}, forms


def test_long_band_chain_takes_the_matrix_core_decode():
    case = _Case(*LONG, seed=11)
    forms = _check(case, 3, 4100, "long band")
    assert forms == {"attn_decode_mfma"}, forms


def test_bad_arguments_are_refused():
    NH, NKV, HS, window, cap, rot, base, kv_shared = SHAPES[0]
    case = _Case(*SHAPES[0], seed=5)
    K, V = case.poisoned(10)
    head = [empty_u16(4, NH * HS), K, V, case.raw[0], case.raw[0, case.k_off:], case.raw[0, case.v_off:], C.c_int64(case.packed), case.qw, case.kw, None, case.cos, case.sin,
            case.scratch, C.c_size_t(case.nbytes)]
    for T in (1, 5):
        with pytest.raises(capi.InvalidArgument):
            capi.call("fused_attn_decode_chain_bf16", *head, T, NH, NKV, HS, cap, 10, None, 0, window, 1.0, 1e-6)
    with pytest.raises(capi.InvalidArgument):
        capi.call("fused_attn_decode_chain_bf16", *head, 3, NH, NKV, HS, cap, cap - 2, None, 0, window, 1.0, 1e-6)      # the last row would wrap
    with pytest.raises(capi.InvalidArgument):
        capi.call("fused_attn_decode_chain_bf16", *head, 2, NH, NKV, HS, cap, 0, dev_i32(np.array([3])), cap + 1, window, 1.0, 1e-6)
    assert np.array_equal(bits(K), bits(case.poisoned(10)[0]))
