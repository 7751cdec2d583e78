"""GPU: fused_attn_decode_rows_bf16 -- B independent sequences, row b at positions_dev[b] -- is BATCH INVARIANT: row b's output and the whole K / V caches of every row
are bit-equal to fused_attn_decode_bf16 in its device-position form, run on a copy of row b's caches at pos[b] with the same max_len.  Caches and outputs carry one more
row than the batch, which must stay untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gpu_util import bits, dev_i32, dev_u16, empty_f32, empty_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

MAX_SEQ = 2048
GEOMETRIES = [  # NH NKV HS window capacity rotary base kv_shared
    (16, 8, 256, 1024, 2048, 0, 1e4, False),
    (16, 1, 512, 0, 2048, 128, 1e6, True),
    (4, 2, 64, 8, 16, 0, 1e4, False),          # a ring that wraps: row p lives at p % 16
]
POSITION_SETS = [[0, 63, 64], [1500, 5], [7, 8, 9, 200]]


def _bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def _d(x):
    return dev_u16(orc.to_bf16_bits(x))


def _history(shape, seed, scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand(shape, device="cuda", generator=g) * 2 - 1) * scale).to(torch.bfloat16).view(torch.int16)


class _Case:
    """one geometry's operands: B + 1 rows of caches and raw projections (the last row is never part of a launch)"""

    def __init__(self, NH, NKV, HS, window, cap, rot, base, kv_shared, B, seed, max_seq=MAX_SEQ):
        rng = np.random.default_rng(seed)
        self.geo = (NH, NKV, HS, cap, window)
        self.B = B
        self.Kc = _history((B + 1, NKV, cap, HS), seed, 0.5)
        self.Vc = _history((B + 1, NKV, cap, HS), seed + 1, 1.0)
        qn, kn = NH * HS, NKV * HS
        self.packed = qn + kn * (1 if kv_shared else 2) + 24      # the row stride need not be the sum of the parts
        self.raw = _d(_bf(rng.standard_normal((B + 1, self.packed))))
        self.k_off = qn
        self.v_off = qn if kv_shared else qn + kn
        self.qw, self.kw = _d(_bf(1 + 0.1 * rng.uniform(-1, 1, HS))), _d(_bf(1 + 0.1 * rng.uniform(-1, 1, HS)))
        self.cos, self.sin = empty_f32(max_seq, HS // 2), empty_f32(max_seq, HS // 2)
        capi.call("rope_build_cache", self.cos, self.sin, max_seq, HS, float(base), rot)
        self.nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(B + 1, NH, HS)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def alone(self, b, pos, max_len):
        """row b decoded alone: fused_attn_decode_bf16, device-position form, on a copy of its caches"""
        NH, NKV, HS, cap, window = self.geo
        K, V, y = self.Kc[b:b + 1].clone(), self.Vc[b:b + 1].clone(), empty_u16(NH * HS)
        capi.call("fused_attn_decode_bf16", y, K, V, self.raw[b], self.raw[b, self.k_off:], self.raw[b, self.v_off:], self.qw, self.kw, None, self.cos, self.sin,
                  self.scratch, C.c_size_t(self.nbytes), NH, NKV, HS, cap, max_len, dev_i32(np.array([pos])), window, 1.0, 1e-6)
        return bits(y), bits(K)[0], bits(V)[0]

    def rows(self, positions, max_len):
        NH, NKV, HS, cap, window = self.geo
        B = len(positions)
        K, V, Y = self.Kc.clone(), self.Vc.clone(), empty_u16(self.B + 1, NH * HS)
        pd = dev_i32(np.array(list(positions) + [3], dtype=np.int32))
        capi.call("fused_attn_decode_rows_bf16", Y, K, V, self.raw[0], self.raw[0, self.k_off:], self.raw[0, self.v_off:], C.c_int64(self.packed), self.qw, self.kw, None,
                  self.cos, self.sin, self.scratch, C.c_size_t(self.nbytes), B, NH, NKV, HS, cap, pd, max_len, window, 1.0, 1e-6)
        return bits(Y), bits(K), bits(V)


def _check(case, positions, max_len, what):
    B = len(positions)
    capi.last_form()
    Y, K, V = case.rows(positions, max_len)
    forms = capi.last_form()
    K0, V0 = bits(case.Kc), bits(case.Vc)
    for b, pos in enumerate(positions):
        y1, k1, v1 = case.alone(b, pos, max_len)
        assert np.array_equal(Y[b], y1), "%s: row %d (position %d) differs from the row decoded alone" % (what, b, pos)
        assert np.array_equal(K[b], k1) and np.array_equal(V[b], v1), "%s: caches of row %d differ from the row decoded alone" % (what, b)
    for b in range(B, K.shape[0]):
        assert np.array_equal(K[b], K0[b]) and np.array_equal(V[b], V0[b]), "%s: caches of row %d, past the batch, were written" % (what, b)
        assert (Y[b] == 0x7fc0).all(), "%s: output row %d, past the batch, was written" % (what, b)
    return forms


@pytest.mark.parametrize("geo", range(len(GEOMETRIES)))
def test_rows_at_their_own_positions_equal_the_rows_decoded_alone(geo):
    NH, NKV, HS, window, cap, rot, base, kv_shared = GEOMETRIES[geo]
    case = _Case(NH, NKV, HS, window, cap, rot, base, kv_shared, B=4, seed=geo + 1)
    for positions in POSITION_SETS:
        # the live-length bound of the longest row (a ring keeps at most its window)
        max_len = min(max(positions) + 1, cap)
        forms = _check(case, positions, max_len, "geometry %d positions %s" % (geo, positions))
        assert "attn_decode" in forms
    # a bound of 0 means the capacity, as beside a position_dev of the one-row entry
    _check(case, [5, 0], 0, "geometry %d, bound 0" % geo)


def test_long_band_rows_take_the_matrix_core_decode():
    """16 heads on one KV head over a band bucket of 8192 keys: the matrix-core kernel with its prologue chain (fused_qkv_post_devpos per row, each at ITS position); the
    short row rides in the long row's bucket"""
    case = _Case(16, 1, 512, 0, 8192, 128, 1e6, True, B=2, seed=11, max_seq=8192)
    forms = _check(case, [4500, 37], 4501, "long band")
    assert "attn_decode_mfma" in forms, forms


def test_an_existing_entry_keeps_its_bits_around_a_rows_launch():
    """the batch entry at one device position (position stride 0), before and after a rows launch in the same process: the same bits, and the eager form's"""
    NH, NKV, HS, window, cap, rot, base, kv_shared = GEOMETRIES[0]
    case = _Case(NH, NKV, HS, window, cap, rot, base, kv_shared, B=3, seed=21)
    pos = 777

    def batch(pd):
        K, V, Y = case.Kc.clone(), case.Vc.clone(), empty_u16(4, NH * HS)
        capi.call("fused_attn_decode_batch_bf16", Y, K, V, case.raw[0], case.raw[0, case.k_off:], case.raw[0, case.v_off:], C.c_int64(case.packed), case.qw, case.kw, None,
                  case.cos, case.sin, case.scratch, C.c_size_t(case.nbytes), 3, NH, NKV, HS, cap, pos if pd is None else pos + 1, pd, window, 1.0, 1e-6)
        return bits(Y), bits(K), bits(V)

    # [pos, 0, 0]: a launch that read positions with a non-zero stride would put rows 1 and 2 at position 0
    pd = dev_i32(np.array([pos, 0, 0]))
    before = batch(pd)
    case.rows([3, 900, 64], 901)
    after = batch(pd)
    eager = batch(None)
    for a, b, c in zip(before, after, eager):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_bad_arguments_are_refused():
    NH, NKV, HS, window, cap, rot, base, kv_shared = GEOMETRIES[2]
    case = _Case(NH, NKV, HS, window, cap, rot, base, kv_shared, B=2, seed=5)
    args = [empty_u16(3, NH * HS), case.Kc.clone(), case.Vc.clone(), case.raw[0], case.raw[0, case.k_off:], case.raw[0, case.v_off:], C.c_int64(case.packed), case.qw, case.kw,
            None, case.cos, case.sin, case.scratch, C.c_size_t(case.nbytes), 2, NH, NKV, HS, cap]
    with pytest.raises(capi.InvalidArgument):
        capi.call("fused_attn_decode_rows_bf16", *args, None, 0, window, 1.0, 1e-6)                          # no positions
    with pytest.raises(capi.InvalidArgument):
        capi.call("fused_attn_decode_rows_bf16", *args, dev_i32(np.array([1, 2])), cap + 1, window, 1.0, 1e-6)   # a bound beyond the cache
