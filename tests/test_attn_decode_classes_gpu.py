"""GPU parity of the split-K decode kernels (attn_decode_kernel, attn_decode_kvfp8_kernel and the combine they share) with the float64 oracle at every launch-index
class of tests/attn_decode_classes.py: workgroups per KV head of 1 .. 16 at every head size, heads per workgroup of 1, 2 and 4, batch rows beyond the first at HS 256
and 512, split counts {1, 2, 3, 10, 16, 17, 32, 33, 64}, and lengths that leave trailing splits empty, fill every split exactly, or sit on either side of the window.
tests/test_attn_decode_classes_cpu.py holds every row of the table to the plan it is there for.

Data as in tests/test_attention_gpu.py: K uniform(-1, 1) * 0.5, V and q uniform(-1, 1), bf16-rounded, scale 1 at HS >= 256 and HS ** -0.5 below; every batch row has a
history of its own, so a kernel that reads another row's cache, partials or query fails.  Dead cache rows -- at or beyond the live length, or older than the band --
hold NaN (byte 0x7F and a NaN scale in the fp8 cache): a kernel that reads one produces NaN and fails.  The bar is the project's: <= 1 bf16 ulp + 2e-3 abs against
orc.gqa_attention, for the fp8 cache on the dequantized history (tests/test_kvfp8_gpu.py).

A row's history is drawn and quantized once (functools.lru_cache) and lives on the device; the cache of one length is cut from it there."""
import ctypes as C
import functools
import types
import zlib

import numpy as np
import pytest
import torch

import orc
from attn_decode_classes import BY_NAME, FORM_KVFP8, FUSED_ROWS, GH512_ROW, GH512_TUNING, RING_ROWS, ROWS, ring_case
from gpu_util import assert_bf16_close, bits, dev_f32, dev_i32, dev_u16, dev_u8, empty_f32, empty_u16, host
from mila_amd import capi
from test_kvfp8_gpu import NAN_BITS, Cache8, _bf, _d, _quantize

pytestmark = pytest.mark.gpu

ALL = {r.name: r for r in ROWS + [GH512_ROW]}
CASES = [(r.name, n) for r in ROWS for n in r.lengths]
IDS = ["%s-%d" % c for c in CASES]
EPS = 1e-6


def _scale(HS):
    return 1.0 if HS >= 256 else HS ** -0.5


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _history_len(row):
    return max(max(row.lengths), ring_case(row)[2])


@functools.lru_cache(maxsize=3)
def _data(name):
    """the history of a row, [B, T, NKV, HS] on the host (hk, hv and their dequantized values dk, dv) and [B, NKV, T, HS] on the device (bf16 bits; e4m3 bytes and
    [B, NKV, T] scales): drawn once, never modified"""
    row = ALL[name]
    T = _history_len(row)
    rng = np.random.default_rng(_seed(name))
    hk = _bf(rng.uniform(-1, 1, (row.B, T, row.NKV, row.HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (row.B, T, row.NKV, row.HS)))
    k8, ks, dk = _quantize(hk)
    v8, vs, dv = _quantize(hv)
    t = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, 2))
    return types.SimpleNamespace(T=T, hk=hk, hv=hv, dk=dk, dv=dv, K=dev_u16(t(orc.to_bf16_bits(hk))), V=dev_u16(t(orc.to_bf16_bits(hv))),
                                 K8=dev_u8(t(k8)), V8=dev_u8(t(v8)), Ks=dev_f32(t(ks)), Vs=dev_f32(t(vs)))


def _query(row, *what):
    return _bf(np.random.default_rng(_seed(row.name, *what)).uniform(-1, 1, (row.B, 1, row.NH, row.HS)))


def _rows_of(first, end, cap):
    pos = torch.arange(first, end, device="cuda")
    return pos, pos % cap


def _cache16(d, row, cap, first, end):
    """a bf16 cache of `cap` rows that holds positions [first, end) of the history at row position % cap and NaN everywhere else"""
    K = torch.full((row.B, row.NKV, cap, row.HS), NAN_BITS, dtype=torch.int16, device="cuda")
    V = torch.full((row.B, row.NKV, cap, row.HS), NAN_BITS, dtype=torch.int16, device="cuda")
    pos, at = _rows_of(first, end, cap)
    K[:, :, at] = d.K[:, :, pos]
    V[:, :, at] = d.V[:, :, pos]
    return K, V


def _cache8(d, row, cap, first, end):
    """the same as an fp8 cache: dead rows hold byte 0x7F and a NaN scale"""
    c = Cache8(row.B, row.NKV, cap, row.HS)
    pos, at = _rows_of(first, end, cap)
    for dst, src in zip(c.arrays(), (d.K8, d.V8, d.Ks, d.Vs)):
        dst[:, :, at] = src[:, :, pos]
    return c


def _scratch(row):
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(row.B, row.NH, row.HS)
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), C.c_size_t(nbytes)


def _decode16(row, K, V, q, cap, length, window, position_dev=None, max_len=0):
    Y = empty_u16(row.B, row.NH * row.HS)
    scratch, nbytes = _scratch(row)
    if position_dev is None:
        capi.call("attn_decode_bf16", Y, _d(q), K, V, scratch, nbytes, row.B, row.NH, row.NKV, row.HS, cap, length, window, _scale(row.HS))
    else:
        capi.call("attn_decode_bf16_devpos", Y, _d(q), K, V, scratch, nbytes, row.B, row.NH, row.NKV, row.HS, cap, position_dev, max_len, window, _scale(row.HS))
    return bits(Y)


def _decode8(row, c, q, length, window, position_dev=None, max_len=0):
    Y = empty_u16(row.B, row.NH * row.HS)
    scratch, nbytes = _scratch(row)
    if position_dev is None:
        capi.call("attn_decode_kvfp8", Y, _d(q), *c.arrays(), scratch, nbytes, row.B, row.NH, row.NKV, row.HS, c.cap, length, window, _scale(row.HS))
    else:
        capi.call("attn_decode_kvfp8_devpos", Y, _d(q), *c.arrays(), scratch, nbytes, row.B, row.NH, row.NKV, row.HS, c.cap, position_dev, max_len, window, _scale(row.HS))
    return bits(Y)


def _band_first(length, window):
    return max(0, length - window) if window > 0 else 0


def _captured_bounds(row, length):
    """the live-length bounds a device-position launch for this length may have been captured with: the length itself, and the upper end of its bucket"""
    bucket = capi.load().mila_cdna4_attn_decode_band_bucket(length, row.capacity)
    return sorted({length, max(length, bucket)})


def _oracle(row, q, k, v, length, window):
    return orc.gqa_attention(q, k[:, :length], v[:, :length], length - 1, window, _scale(row.HS))[:, 0]


def _check_bf16(row, length):
    d = _data(row.name)
    q = _query(row, length)
    K, V = _cache16(d, row, row.capacity, _band_first(length, row.window), length)
    capi.last_form()                        # (clears the record)
    y = _decode16(row, K, V, q, row.capacity, length, row.window)
    assert capi.last_form() == [row.plan["form"]]
    what = "decode %s len %d" % (row.name, length)
    assert_bf16_close(y, _oracle(row, q, d.hk, d.hv, length, row.window), 1, 2e-3, what)
    position = dev_i32([length - 1])
    for max_len in _captured_bounds(row, length):
        y_dev = _decode16(row, K, V, q, row.capacity, length, row.window, position, max_len)
        assert capi.last_form() == [row.plan["form"]]
        assert np.array_equal(y_dev, y), "%s: the device-position form captured for %d keys differs from the eager bits" % (what, max_len)
    if (row.NKV * row.plan["head_groups"]) % 8 == 0:
        # the XCD-local grid (attn.xcd_local) is the same arithmetic per workgroup under another blockIdx.x -> (head group, split) map
        capi.tune("attn.xcd_local", 1)
        try:
            assert capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, row.capacity, row.window, length)["flat"] == 1
            y_flat = _decode16(row, K, V, q, row.capacity, length, row.window)
        finally:
            capi.tune_reset()
        assert np.array_equal(y_flat, y), "%s: the XCD-local grid changed bits" % what


@pytest.mark.parametrize("name,length", CASES, ids=IDS)
def test_bf16_decode_matches_the_oracle_in_every_class(name, length):
    """attn_decode_bf16 within the bar of the oracle on the kernel form the class names; attn_decode_bf16_devpos captured for exactly this length and for the upper end of
    its bucket gives the eager bits; so does the XCD-local grid wherever the head groups tile the 8 XCDs"""
    _check_bf16(ALL[name], length)


def _check_kvfp8(row, length):
    d = _data(row.name)
    q = _query(row, length)
    c = _cache8(d, row, row.capacity, _band_first(length, row.window), length)
    capi.last_form()
    y = _decode8(row, c, q, length, row.window)
    assert capi.last_form() == [FORM_KVFP8]
    what = "fp8 decode %s len %d" % (row.name, length)
    assert_bf16_close(y, _oracle(row, q, d.dk, d.dv, length, row.window), 1, 2e-3, what)
    position = dev_i32([length - 1])
    for max_len in _captured_bounds(row, length):
        y_dev = _decode8(row, c, q, length, row.window, position, max_len)
        assert capi.last_form() == [FORM_KVFP8]
        assert np.array_equal(y_dev, y), "%s: the device-position form captured for %d keys differs from the eager bits" % (what, max_len)


@pytest.mark.parametrize("name,length", CASES, ids=IDS)
def test_kvfp8_decode_matches_the_oracle_in_every_class(name, length):
    """attn_decode_kvfp8 within the bar of the oracle on the dequantized history; its device-position form gives the eager bits"""
    _check_kvfp8(ALL[name], length)


@pytest.mark.parametrize("length", GH512_ROW.lengths)
def test_four_heads_per_workgroup_at_hs512(length):
    """attn.heads_per_group_512 = 4: attn_decode_kernel<512, 4> with 4 workgroups per KV head, on the bf16 cache; the fp8 cache has no such kernel and says so"""
    row = GH512_ROW
    capi.tune(*GH512_TUNING)
    try:
        got = capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, row.capacity, row.window, length)
        assert (got["heads_per_group"], got["head_groups"], got["splits"]) == (4, 4, row.plan["splits"])
        d = _data(row.name)
        q = _query(row, length)
        K, V = _cache16(d, row, row.capacity, 0, length)
        capi.last_form()
        y = _decode16(row, K, V, q, row.capacity, length, row.window)
        assert capi.last_form() == [row.plan["form"]]
        assert_bf16_close(y, _oracle(row, q, d.hk, d.hv, length, row.window), 1, 2e-3, "decode %s len %d" % (row.name, length))
        with pytest.raises(capi.MilaError) as err:
            _decode8(row, _cache8(d, row, row.capacity, 0, length), q, length, row.window)
        assert err.value.code == capi.MILA_E_UNSUPPORTED
    finally:
        capi.tune_reset()


@pytest.mark.parametrize("name", RING_ROWS)
def test_ring_equals_unbounded_in_every_class(name):
    """a ring of window + 3 rows under a history that wraps it twice gives the bits of an unbounded cache whose rows older than the band hold NaN -- the same plan over
    the same values (the reference's ring-vs-unbounded test, CudaGqaOp.Cuda.cpp:529-567) --, on both caches, and sits within the bar of the oracle"""
    row = BY_NAME[name]
    window, cap, length = ring_case(row)
    d = _data(name)
    q = _query(row, "ring")
    first = length - window
    assert first > cap and first % cap != 0, "the band must wrap the ring"
    assert capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, cap, window, length)["splits"] > 1
    y_ring = _decode16(row, *_cache16(d, row, cap, first, length), q, cap, length, window)
    y_flat = _decode16(row, *_cache16(d, row, length, first, length), q, length, length, window)
    assert_bf16_close(y_ring, _oracle(row, q, d.hk, d.hv, length, window), 1, 2e-3, "ring decode %s" % name)
    assert np.array_equal(y_ring, y_flat), "the ring differs from the unbounded cache"
    y_ring8 = _decode8(row, _cache8(d, row, cap, first, length), q, length, window)
    y_flat8 = _decode8(row, _cache8(d, row, length, first, length), q, length, window)
    assert_bf16_close(y_ring8, _oracle(row, q, d.dk, d.dv, length, window), 1, 2e-3, "fp8 ring decode %s" % name)
    assert np.array_equal(y_ring8, y_flat8), "the fp8 ring differs from the unbounded fp8 cache"
    with pytest.raises(capi.InvalidArgument):     # band larger than the ring
        _decode16(row, *_cache16(d, row, cap, first, length), q, cap, length, 0)


# ---- the fused prologue: only workgroup hg == 0 of a KV head appends the new K / V row, the others patch it in from LDS ----
@functools.lru_cache(maxsize=None)
def _rope_cache(HS, max_seq=4608):
    cos, sin = empty_f32(max_seq, HS // 2), empty_f32(max_seq, HS // 2)
    capi.call("rope_build_cache", cos, sin, max_seq, HS, 1e4, 0)
    return cos, sin, host(cos), host(sin)


def _owner_split(row, window, cap, pos):
    """(the split whose range holds position `pos`, the split count) of the fused launch at that position"""
    splits = capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, cap, window, pos + 1, fused=True)["splits"]
    band = min(pos + 1, window) if window > 0 else pos + 1
    chunk = -(-band // splits)
    return (band - 1) // chunk, splits


def _fused_positions(row):
    """(window, capacity, position, the class of the position): the new row owned by the first split (position 0), by a split in the middle -- the last non-empty one,
    with empty splits behind it --, by the last split of a full band, and in a ring that the band wraps"""
    w, cap = row.window, row.capacity
    mid = next(p for p in range(_owner_split(row, w, cap, 0)[1], cap) if      # (from a band of splits + 1 keys on: two keys per split)
               0 < _owner_split(row, w, cap, p)[0] < _owner_split(row, w, cap, p)[1] - 1)
    full = w + 70 if w > 0 else cap - 1
    rw, rcap, rlen = ring_case(row)
    return [(w, cap, 0, "first"), (w, cap, mid, "middle"), (w, cap, full, "last"), (rw, rcap, rlen - 24, "ring")]


def _fused_case(row, window, cap, pos, kind):
    B, NH, NKV, HS = row.B, row.NH, row.NKV, row.HS
    owner, splits = _owner_split(row, window, cap, pos)
    assert splits > 1 and {"first": owner == 0, "middle": 0 < owner < splits - 1, "last": owner == splits - 1, "ring": pos >= 2 * cap and owner == splits - 1}[kind]
    d = _data(row.name)
    rng = np.random.default_rng(_seed(row.name, "fused", pos))
    first = _band_first(pos + 1, window)
    Kc0, Vc0 = _cache16(d, row, cap, first, pos)                               # positions first .. pos - 1: row pos % cap is dead until the launch appends it
    qn, kn = NH * HS, NKV * HS
    packed = qn + 2 * kn + 24                                                  # + 24: the row stride need not be the sum of the parts
    rows = _bf(rng.standard_normal((B, packed)))
    rows_d = _d(rows)
    q_off, k_off, v_off = 0, qn, qn + kn
    qw, kw = _bf(1 + 0.1 * rng.uniform(-1, 1, HS)), _bf(1 + 0.1 * rng.uniform(-1, 1, HS))
    qw_d, kw_d = _d(qw), _d(kw)
    cos, sin, cos_h, sin_h = _rope_cache(HS)
    scratch, nbytes = _scratch(row)
    scale = _scale(HS)
    # chain: fused_qkv_post row by row on that row's caches, then the batched decode
    K0, V0, q0, y0 = Kc0.clone(), Vc0.clone(), empty_u16(B, NH * HS), empty_u16(B, NH * HS)
    for b in range(B):
        capi.call("fused_qkv_post", q0[b], K0[b], V0[b], rows_d[b, q_off:], rows_d[b, k_off:], rows_d[b, v_off:], qw_d, kw_d, None, cos, sin, NH, NKV, HS, pos, cap, EPS)
    capi.call("attn_decode_bf16", y0, q0, K0, V0, scratch, nbytes, B, NH, NKV, HS, cap, pos + 1, window, scale)
    # one launch, position from the host and from the device
    for position, position_dev in ((pos, None), (pos + 1, dev_i32([pos]))):     # (under position_dev, `position` is the live-length bound of the launch)
        K1, V1, y1 = Kc0.clone(), Vc0.clone(), empty_u16(B, NH * HS)
        capi.last_form()
        capi.call("fused_attn_decode_batch_bf16", y1, K1, V1, rows_d[0, q_off:], rows_d[0, k_off:], rows_d[0, v_off:], C.c_int64(packed), qw_d, kw_d, None, cos, sin,
                  scratch, nbytes, B, NH, NKV, HS, cap, position, position_dev, window, scale, EPS)
        assert capi.last_form() == [row.plan["form"]]
        what = "%s at %d (%s)" % (row.name, pos, "device position" if position_dev is not None else "host position")
        assert np.array_equal(bits(K1), bits(K0)) and np.array_equal(bits(V1), bits(V0)), "cache rows differ: " + what
        assert np.array_equal(bits(y1), bits(y0)), "attention output differs: " + what
    # The oracle, stage by stage on every batch row.  (1) the q rows and the appended K / V rows are norm -> bf16 -> rope of the raw rows: the normed value is rounded to
    # bf16 before the rotation, so where the kernel's fp32 norm and the oracle's round to different neighbours (one bf16 ulp, <= 2^-7 |a|) the rotated value
    # a cos - b sin moves by up to 2^-7 (|a| |cos| + |b| |sin|) <= 2^-7 sqrt(2) max |a| on top of its own rounding; V is not rotated: one rounding, 1 ulp.
    q_raw = rows[:, q_off:q_off + qn].reshape(B, NH, HS)
    k_raw, v_raw = rows[:, k_off:k_off + kn].reshape(B, NKV, HS), rows[:, v_off:v_off + kn].reshape(B, NKV, HS)
    q_norm, k_norm = _bf(orc.rmsnorm(q_raw, qw, None, eps=EPS)), _bf(orc.rmsnorm(k_raw, kw, None, eps=EPS))
    q_exp = orc.rope_rotate(q_norm.reshape(B, 1, NH, HS), cos_h, sin_h, pos)
    k_exp = orc.rope_rotate(k_norm.reshape(B, 1, NKV, HS), cos_h, sin_h, pos)
    v_exp = orc.rmsnorm(v_raw, None, None, eps=EPS)
    k_new, v_new = bits(K0)[:, :, pos % cap], bits(V0)[:, :, pos % cap]          # [B, NKV, HS]
    assert_bf16_close(bits(q0), q_exp, 1, 2.0 ** -6.5 * np.abs(q_norm).max(), "fused q rows %s at %d" % (row.name, pos))
    assert_bf16_close(k_new, k_exp, 1, 2.0 ** -6.5 * np.abs(k_norm).max(), "appended K rows %s at %d" % (row.name, pos))
    assert_bf16_close(v_new, v_exp, 1, 0.0, "appended V rows %s at %d" % (row.name, pos))
    # (2) the attention of those q rows over the history and the appended rows, as the device holds them
    hist = lambda h, new: np.concatenate([h[:, :pos], orc.from_bf16_bits(new)[:, None]], axis=1)      # [B, pos + 1, NKV, HS]
    exp = orc.gqa_attention(orc.from_bf16_bits(bits(q0)).reshape(B, 1, NH, HS), hist(d.hk, k_new), hist(d.hv, v_new), pos, window, scale)[:, 0]
    assert_bf16_close(bits(y0), exp, 1, 2e-3, "fused decode %s at %d vs the oracle" % (row.name, pos))


@pytest.mark.parametrize("name", FUSED_ROWS)
def test_fused_prologue_equals_the_chain_and_the_oracle_in_every_class(name):
    """fused_attn_decode_batch_bf16 == per-row fused_qkv_post + attn_decode_bf16, bit for bit, cache contents included (all of them: a second workgroup that appended
    the row elsewhere, or a row appended for one head group only, shows), with the position from the host and from the device, at workgroups per KV head of 2, 4
    and 8 and in batches; and every batch row of the chain against orc.rmsnorm -> orc.rope_rotate (with the device's cos / sin cache) -> orc.gqa_attention"""
    row = BY_NAME[name]
    cases = _fused_positions(row)
    assert [k for _, _, _, k in cases] == ["first", "middle", "last", "ring"]
    for window, cap, pos, kind in cases:
        _fused_case(row, window, cap, pos, kind)
