"""The head of attn_decode_kernel (csrc/attention.hip): what runs between a wave's first instruction and its first K/V request, at the inputs the class tests
(test_attn_decode_classes_gpu.py, whose helpers are used here) do not reach.  Every leg compares fused_attn_decode_batch_bf16, with the position from the host and from
the device, bit for bit -- output and both whole caches, dead rows included -- with per-row fused_qkv_post + attn_decode_bf16:
  * a given V norm weight, and v_raw == k_raw (the global-layer form), at HS 64 / 256 / 512 with two KV heads of two query heads, and 16 heads on one KV head at HS 512;
  * the row walk: a ring of exactly the window and of window + 1, rings no longer than the eight-position step of a wave (8, 6, 3 rows), each at positions
    k cap - 1, k cap, k cap + 1 for k = 1, 2, 3, and a flat cache whose last row the launch fills (len == capacity);
  * the split quotient: 40 consecutive positions, so that the band passes m splits - 1, m splits, m splits + 1, windowed and unwindowed, position 0, and the
    positions at which the band first equals the window and first slides;
  * HS 512's register groups: 32, 33, 64 and 65 positions per split -- one group, two, two, three.
Shapes are the smallest that reach the code: the arithmetic is compared with the chain's own, not with a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_util import bits, dev_i32, empty_u16
from mila_amd import capi
from test_attn_decode_classes_gpu import EPS, _band_first, _rope_cache, _scale, _seed
from test_kvfp8_gpu import NAN_BITS, _bf, _d

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def _history(B, NKV, T, HS):
    """K and V of positions 0 .. T - 1 as [B, NKV, T, HS] bf16 bits on the device: drawn once per shape, never modified"""
    g = torch.Generator(device="cuda")
    g.manual_seed(_seed("head", B, NKV, T, HS))
    draw = lambda s: ((torch.rand((B, NKV, T, HS), device="cuda", generator=g) - 0.5) * s).to(torch.bfloat16).view(torch.int16)
    return draw(1.0), draw(2.0)


def _caches(B, NKV, HS, cap, first, end, T):
    """positions [first, end) at row position % cap, NaN in every other row"""
    hk, hv = _history(B, NKV, T, HS)
    K = torch.full((B, NKV, cap, HS), NAN_BITS, dtype=torch.int16, device="cuda")
    V = torch.full((B, NKV, cap, HS), NAN_BITS, dtype=torch.int16, device="cuda")
    pos = torch.arange(first, end, device="cuda")
    K[:, :, pos % cap] = hk[:, :, pos]
    V[:, :, pos % cap] = hv[:, :, pos]
    return K, V


def _splits(B, NH, NKV, HS, cap, window, pos):
    return capi.attn_decode_plan(B, NH, NKV, HS, cap, window, pos + 1, fused=True)["splits"]


def _leg(B, NH, NKV, HS, cap, window, pos, T, vw=False, v_is_k=False):
    assert pos < T and min(pos + 1, window or pos + 1) <= cap
    rng = np.random.default_rng(_seed("head leg", B, NH, NKV, HS, cap, window, pos, vw, v_is_k))
    K0, V0 = _caches(B, NKV, HS, cap, _band_first(pos + 1, window), pos, T)
    qn, kn = NH * HS, NKV * HS
    packed = qn + 2 * kn + 24
    rows_d = _d(_bf(rng.standard_normal((B, packed))))
    q_off, k_off, v_off = 0, qn, (qn if v_is_k else qn + kn)
    qw_d, kw_d = (_d(_bf(1 + 0.1 * rng.uniform(-1, 1, HS))) for _ in range(2))
    vw_d = _d(_bf(1 + 0.3 * rng.uniform(-1, 1, HS))) if vw else None
    cos, sin, _, _ = _rope_cache(HS)
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(B, NH, HS)
    scratch, nb = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), C.c_size_t(nbytes)
    scale = _scale(HS)
    Kc, Vc, qc, yc = K0.clone(), V0.clone(), empty_u16(B, NH * HS), empty_u16(B, NH * HS)
    for b in range(B):
        capi.call("fused_qkv_post", qc[b], Kc[b], Vc[b], rows_d[b, q_off:], rows_d[b, k_off:], rows_d[b, v_off:], qw_d, kw_d, vw_d, cos, sin, NH, NKV, HS, pos, cap, EPS)
    capi.call("attn_decode_bf16", yc, qc, Kc, Vc, scratch, nb, B, NH, NKV, HS, cap, pos + 1, window, scale)
    for position, position_dev in ((pos, None), (pos + 1, dev_i32([pos]))):
        K1, V1, y1 = K0.clone(), V0.clone(), empty_u16(B, NH * HS)
        capi.call("fused_attn_decode_batch_bf16", y1, K1, V1, rows_d[0, q_off:], rows_d[0, k_off:], rows_d[0, v_off:], C.c_int64(packed), qw_d, kw_d, vw_d, cos, sin,
                  scratch, nb, B, NH, NKV, HS, cap, position, position_dev, window, scale, EPS)
        what = "B %d NH %d NKV %d HS %d capacity %d window %d position %d (%s)%s%s" % (B, NH, NKV, HS, cap, window, pos, "device" if position_dev is not None else "host",
                                                                                   ", vw" if vw else "", ", v_raw == k_raw" if v_is_k else "")
        assert np.array_equal(bits(K1), bits(Kc)), "K cache differs: " + what
        assert np.array_equal(bits(V1), bits(Vc)), "V cache differs: " + what
        assert np.array_equal(bits(y1), bits(yc)), "attention output differs: " + what


# ---- a given vw; v_raw == k_raw ----
@pytest.mark.parametrize("NH,NKV,HS", [(4, 2, 64), (4, 2, 256), (4, 2, 512), (16, 1, 512)], ids=["hs64", "hs256", "hs512", "hs512_16_on_1"])
def test_given_v_weight_and_shared_kv_row(NH, NKV, HS):
    cap, T = 256, 256
    for pos in (0, 150, 255):                      # the owner is the first split, one in the middle, the last (and len == capacity)
        _leg(1, NH, NKV, HS, cap, 0, pos, T, vw=True)
        _leg(1, NH, NKV, HS, cap, 0, pos, T, vw=True, v_is_k=True)
        _leg(1, NH, NKV, HS, cap, 0, pos, T, v_is_k=True)


# ---- row addresses ----
RINGS = [(40, 40), (40, 41), (5, 8), (5, 6), (3, 3)]      # (window, capacity)


@pytest.mark.parametrize("window,cap", RINGS, ids=["w%d_cap%d" % r for r in RINGS])
def test_ring_rows_around_every_wrap(window, cap):
    for k in (1, 2, 3):
        for pos in (k * cap - 1, k * cap, k * cap + 1):
            _leg(1, 4, 2, 256, cap, window, pos, 3 * 41 + 2)


def test_flat_cache_filled_to_its_last_row():
    for cap in (96, 97):                            # len == capacity: nothing has wrapped yet
        _leg(1, 4, 2, 256, cap, 0, cap - 1, 97)
        _leg(1, 4, 2, 256, cap, 0, cap - 2, 97)


# ---- the split quotient ----
def test_split_quotient_over_consecutive_bands():
    # unwindowed, capacity 2048: 32 splits; bands 92 .. 131 pass 96 and 128 with a key either side
    B, NH, NKV, HS, cap = 1, 4, 2, 128, 2048
    assert _splits(B, NH, NKV, HS, cap, 0, 100) == 32
    for pos in [0] + list(range(91, 131)):
        _leg(B, NH, NKV, HS, cap, 0, pos, 160)
    # window 150: 3 splits; bands 101 .. 140 pass every multiple of 3 between them; then the band reaches the window (length 150) and slides (151, 152)
    window = 150
    assert _splits(B, NH, NKV, HS, cap, window, 100) == 3
    for pos in [0] + list(range(100, 140)) + [window - 2, window - 1, window, window + 1]:
        _leg(B, NH, NKV, HS, cap, window, pos, 160)


# ---- HS 512: one, two and three register groups per wave ----
@pytest.mark.parametrize("per_split", [32, 33, 64, 65])
def test_hs512_group_count(per_split):
    B, NH, NKV, HS, cap = 4, 16, 1, 512, 1024       # 8 workgroups per KV head, 4 rows: the workgroup budget leaves 8 splits
    pos = 8 * per_split - 1 - (3 if per_split in (33, 65) else 0)      # bands 256, 261, 512, 517
    splits = _splits(B, NH, NKV, HS, cap, 0, pos)
    assert splits == 8 and -(-(pos + 1) // splits) == per_split
    _leg(B, NH, NKV, HS, cap, 0, pos, 520)
