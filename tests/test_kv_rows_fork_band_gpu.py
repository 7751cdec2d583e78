"""GPU: mila_cdna4_kv_rows_fork_layers_band_bf16 (csrc/kv_rows_fork.hip) -- the live band [begin, len) of every layer, begin = max(0, len - window) on a ring layer and 0
on a flat one, position p at cache index p % capacity, from row `src` into the rows of the mask, in one launch.  The expectation is a numpy copy of exactly those cache
indices, and the comparison is on bits over the WHOLE allocation of every layer: the band arrived, every other byte is what it was -- the source row, the rows the mask
does not name, the cells of the destination rows outside the band, and one spare row beyond `rows` that the entry is never told about.  The caches are uniformly random
16-bit patterns (NaN patterns of both kinds and -0 are among them, and a few are planted in the source's cells)."""
import itertools

import numpy as np
import pytest
import torch

from gpu_util import bits, dev_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

RING_11 = (2, 11, 64, 8)        # (NKV, capacity, HS, window): a ring of window + chunk - 1 cells at chunk 4, no power of two ...
RING_16 = (2, 16, 64, 8)        # ... one at chunk 9 ...
FLAT = (1, 64, 512, 0)          # ... and a global layer: the whole prefix
KINDS = [RING_11, RING_16, FLAT]
LENS = [1, 7, 8, 9, 11, 12, 20, 32, 64]      # below, at, just above the window; the first wrap of capacity 11; a band split across the end of both rings; a band that ends
                                             # at a multiple of 16; the flat layer's whole capacity
SPECIAL = [0x8000, 0x0000, 0x7fc0, 0xffc1, 0x7f81, 0xff80, 0x7f80, 0xffff]      # -0, +0, quiet NaNs, a signalling NaN, -inf, +inf, the all-ones NaN
SRC = 1
MASKS_4 = [m for n in (1, 2, 3) for m in itertools.combinations((0, 2, 3), n)]      # every non-empty subset of the rows that are not the source


def _caches(rng, rows, kinds, src):
    out = []
    for NKV, cap, HS, _ in kinds:
        pair = []
        for _ in range(2):
            a = rng.integers(0, 1 << 16, size=(rows + 1, NKV, cap, HS), dtype=np.uint16)      # one spare row beyond `rows`
            for i, s in enumerate(SPECIAL):
                a[src, i % NKV, (3 * i) % cap, (7 * i) % HS] = s
            pair.append(a)
        out.append(pair)
    return out


def _expected(before, kind, src, dst, n):
    _, cap, _, window = kind
    begin = max(0, n - window) if window > 0 else 0
    cells = [p % cap for p in range(begin, n)]
    want = before.copy()
    for r in dst:
        want[r][:, cells] = before[src][:, cells]
    return want


def _fork(rows, kinds, src, dst, n, host):
    dev = [(dev_u16(k), dev_u16(v)) for k, v in host]
    table = (capi.KvForkLayerBand * len(kinds))()
    for i, ((NKV, cap, HS, window), (K, V)) in enumerate(zip(kinds, dev)):
        table[i].K, table[i].V, table[i].NKV, table[i].capacity, table[i].HS, table[i].window = K.data_ptr(), V.data_ptr(), NKV, cap, HS, window
    capi.call("kv_rows_fork_layers_band_bf16", table, len(kinds), rows, src, sum(1 << r for r in dst), n)
    torch.cuda.synchronize()
    return [(bits(K), bits(V)) for K, V in dev]


def _check(rows, kinds, src, dst, n, host):
    got = _fork(rows, kinds, src, dst, n, host)
    for i, (kind, (gk, gv), (k0, v0)) in enumerate(zip(kinds, got, host)):
        for name, g, before in (("K", gk, k0), ("V", gv, v0)):
            want = _expected(before, kind, src, dst, n)
            assert np.array_equal(g, want), (name, i, kind, rows, src, dst, n, np.argwhere(g != want)[:4].tolist())      # the band, and every other byte as it was
            assert np.array_equal(g[src], before[src]) and np.array_equal(g[rows], before[rows]), (name, i, n)           # (said again: the source and the spare row)


@pytest.mark.parametrize("rows, src, dst", [(4, SRC, m) for m in MASKS_4] + [(2, 0, (1,))])
def test_the_band_arrives_and_every_other_byte_stays(rows, src, dst):
    rng = np.random.default_rng(100 * rows + 10 * src + sum(1 << r for r in dst))
    host = _caches(rng, rows, KINDS, src)
    for n in LENS:
        _check(rows, KINDS, src, dst, n, host)


def test_a_band_that_wraps_is_the_two_runs_of_cells():
    """what the numpy copy says at len 20, spelled out: ring 11 takes positions 12 .. 19 at cells 1 .. 8, ring 16 takes them at cells 12 .. 15 and 0 .. 3"""
    assert [p % 11 for p in range(12, 20)] == [1, 2, 3, 4, 5, 6, 7, 8] and [p % 16 for p in range(12, 20)] == [12, 13, 14, 15, 0, 1, 2, 3]
    assert [p % 11 for p in range(4, 12)] == [4, 5, 6, 7, 8, 9, 10, 0]      # len 12: the first wrap of capacity 11
    rng = np.random.default_rng(5)
    host = _caches(rng, 4, [RING_16], SRC)
    (gk, _), = _fork(4, [RING_16], SRC, (0,), 20, host)
    k0 = host[0][0]
    assert np.array_equal(gk[0][:, [12, 13, 14, 15, 0, 1, 2, 3]], k0[SRC][:, [12, 13, 14, 15, 0, 1, 2, 3]]) and np.array_equal(gk[0][:, 4:12], k0[0][:, 4:12])


def test_more_layers_than_one_launch_carries():
    """65 layers: 64 in the first launch, 1 in the second"""
    kinds = ([RING_11, RING_16, FLAT] * 22)[:65]
    rng = np.random.default_rng(65)
    host = _caches(rng, 4, kinds, 3)
    for n in (12, 20):
        _check(4, kinds, 3, (0, 1), n, host)
