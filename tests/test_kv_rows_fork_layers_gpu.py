"""GPU: mila_cdna4_kv_rows_fork_layers_bf16 (csrc/kv_rows_fork.hip) -- kv_rows_fork_bf16 for n layers of different (NKV, capacity, HS) in one launch.  The
expectation is the one-layer entry itself: n calls of kv_rows_fork_bf16 on a copy of the same caches, and the two must agree byte for byte over the WHOLE allocation
of every layer -- what was copied and what was left alone.  The caches are uniformly random 16-bit patterns (NaN patterns of both kinds and -0 are among them, and a
few are planted in position 0, which every len copies); the destination rows are poisoned with one pattern, so a unit that was not written shows."""
import numpy as np
import pytest
import torch

from gpu_util import bits, dev_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

KIND_A = (2, 24, 64)        # (NKV, capacity, HS): the small model's local layers ...
KIND_B = (1, 40, 128)       # ... and its global ones, at another capacity
LAYERS = {1: [KIND_B], 2: [KIND_A, KIND_B], 3: [KIND_A, KIND_B, KIND_A]}
LENS = [1, 7, 24]
SPECIAL = [0x8000, 0x0000, 0x7fc0, 0xffc1, 0x7f81, 0xff80, 0x7f80, 0xffff]      # -0, +0, quiet NaNs, a signalling NaN, -inf, +inf, the all-ones NaN
POISON = 0x7fa5             # a NaN pattern of its own


def _mask(rows):
    return sum(1 << r for r in rows)


def _caches(rng, rows, kinds, src, dst):
    out = []
    for NKV, cap, HS in kinds:
        pair = []
        for _ in range(2):
            a = rng.integers(0, 1 << 16, size=(rows, NKV, cap, HS), dtype=np.uint16)
            for i, s in enumerate(SPECIAL):
                a[src, i % NKV, 0, (7 * i) % HS] = s
            for r in dst:
                a[r] = POISON
            pair.append(a)
        out.append(pair)
    return out


def _both_ways(rows, kinds, src, dst, n, host):
    """-> (one launch, n launches of the one-layer entry), each a list of (K bits, V bits) per layer"""
    mask = _mask(dst)
    one = [(dev_u16(k), dev_u16(v)) for k, v in host]
    table = (capi.KvForkLayer * len(kinds))()
    for i, ((NKV, cap, HS), (K, V)) in enumerate(zip(kinds, one)):
        table[i].K, table[i].V, table[i].NKV, table[i].capacity, table[i].HS = K.data_ptr(), V.data_ptr(), NKV, cap, HS
    capi.call("kv_rows_fork_layers_bf16", table, len(kinds), rows, src, mask, n)
    per_layer = [(dev_u16(k), dev_u16(v)) for k, v in host]
    for (NKV, cap, HS), (K, V) in zip(kinds, per_layer):
        capi.call("kv_rows_fork_bf16", K, V, rows, NKV, cap, HS, src, mask, n)
    return [(bits(K), bits(V)) for K, V in one], [(bits(K), bits(V)) for K, V in per_layer]


@pytest.mark.parametrize("rows, src, dst", [(2, 1, (0,)), (4, 2, (0,)), (4, 1, (3,)), (4, 1, (0, 2, 3))])
@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_one_launch_is_the_per_layer_calls_byte_for_byte(rows, src, dst, n_layers):
    kinds = LAYERS[n_layers]
    rng = np.random.default_rng(1000 * rows + 10 * src + n_layers)
    host = _caches(rng, rows, kinds, src, dst)
    for n in LENS:
        got, want = _both_ways(rows, kinds, src, dst, n, host)
        for i, ((gk, gv), (wk, wv), (k0, v0)) in enumerate(zip(got, want, host)):
            for name, g, w, before in (("K", gk, wk, k0), ("V", gv, wv, v0)):
                assert np.array_equal(g, w), (name, i, rows, src, dst, n, np.argwhere(g != w)[:4].tolist())
                # ... and the per-layer entry did what its own test pins: the prefix in the rows of the mask, nothing else
                for r in range(rows):
                    if r in dst:
                        assert np.array_equal(g[r, :, :n], before[src, :, :n]) and (g[r, :, n:] == POISON).all(), (name, i, r, n)
                    else:
                        assert np.array_equal(g[r], before[r]), (name, i, r, n)


def test_a_layer_with_more_units_than_its_share_of_the_grid_is_strided_over():
    """three layers share the grid cap of 2048 workgroups: 682 of 256 lanes each, 174 592 units per trip.  Layers of 2 x 6000 x 64 and 1 x 6000 x 128 have
    2 * 2 * 6000 * 8 = 192 000 units at len 6000: the walk's second trip runs, in a ragged tail, beside a short layer whose spare workgroups fall through"""
    kinds = [(2, 6000, 64), (1, 6040, 128), (2, 6016, 64)]
    rows, src, dst, n = 2, 1, (0,), 6000
    assert 2 * 2 * n * (64 // 8) > (2048 // 3) * 256
    rng = np.random.default_rng(7)
    host = _caches(rng, rows, kinds, src, dst)
    got, want = _both_ways(rows, kinds, src, dst, n, host)
    for i, ((gk, gv), (wk, wv), (k0, v0)) in enumerate(zip(got, want, host)):
        for name, g, w, before in (("K", gk, wk, k0), ("V", gv, wv, v0)):
            assert np.array_equal(g, w), (name, i, np.argwhere(g != w)[:4].tolist())
            assert np.array_equal(g[0, :, :n], before[src, :, :n]) and (g[0, :, n:] == POISON).all() and np.array_equal(g[src], before[src]), (name, i)


def test_more_layers_than_one_launch_carries():
    """70 layers: 64 in the first launch, 6 in the second"""
    kinds = [KIND_A, KIND_B] * 35
    rows, src, dst, n = 4, 3, (0, 1), 7
    rng = np.random.default_rng(70)
    host = _caches(rng, rows, kinds, src, dst)
    got, want = _both_ways(rows, kinds, src, dst, n, host)
    for i, ((gk, gv), (wk, wv)) in enumerate(zip(got, want)):
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), i
    torch.cuda.synchronize()
