"""GPU: mila_cdna4_kv_rows_fork_bf16 (csrc/kv_rows_fork.hip) -- positions [0, len) of one cache row into the rows of a mask, K and V, every head, bit for bit, and
nothing else written anywhere.  The expectation is numpy's, on the same 16-bit patterns (uniformly random ones, so NaN patterns of both kinds and -0 are among them,
and a few are planted in the copied range)."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, bits, dev_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

ROWS, NKV, CAP = 4, 2, 48
SRC = 1
MASKS = [(0,), (3,), (0, 2, 3)]
LENS = [1, 31, 32, 33, 48]
SPECIAL = [0x8000, 0x0000, 0x7fc0, 0xffc1, 0x7f81, 0xff80, 0x7f80, 0xffff]      # -0, +0, quiet NaNs, a signalling NaN, -inf, +inf, the all-ones NaN


def _mask(rows):
    return sum(1 << r for r in rows)


@pytest.mark.parametrize("HS", [64, 128, 256, 512])
def test_the_fork_copies_the_prefix_bitwise_and_writes_nothing_else(HS):
    rng = np.random.default_rng(HS)
    shape = (ROWS, NKV, CAP, HS)
    k0 = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    v0 = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    for i, s in enumerate(SPECIAL):      # in the first position, so every len copies them
        k0[SRC, i % NKV, 0, i] = s
        v0[SRC, (i + 1) % NKV, 0, HS - 1 - i] = s
    for dst in MASKS:
        for n in LENS:
            K, V = dev_u16(k0), dev_u16(v0)
            capi.call("kv_rows_fork_bf16", K, V, ROWS, NKV, CAP, HS, SRC, _mask(dst), n)
            for name, got, before in (("K", bits(K), k0), ("V", bits(V), v0)):
                want = before.copy()
                for r in dst:
                    want[r, :, :n, :] = before[SRC, :, :n, :]
                assert np.array_equal(got, want), (name, HS, dst, n, np.argwhere(got != want)[:4].tolist())


def test_row_offsets_beyond_31_bits():
    """four rows of 2 x 700000 x 512 elements: row 3 starts at element 2 150 400 000 > 2^31, where a 32-bit element offset has wrapped (5.7 GB per cache; everything
    stays on the device)."""
    HS, cap, n = 512, 700000, 33
    assert 3 * NKV * cap * HS > 1 << 31
    shape = (ROWS, NKV, cap, HS)
    g = torch.Generator(device=DEV).manual_seed(5)
    K = torch.randint(-(1 << 15), 1 << 15, shape, dtype=torch.int16, device=DEV, generator=g)
    V = torch.randint(-(1 << 15), 1 << 15, shape, dtype=torch.int16, device=DEV, generator=g)
    k0, v0 = K.clone(), V.clone()
    capi.call("kv_rows_fork_bf16", K, V, ROWS, NKV, cap, HS, 0, _mask((3,)), n)
    torch.cuda.synchronize()
    for got, before in ((K, k0), (V, v0)):
        assert torch.equal(got[3, :, :n], before[0, :, :n])
        assert torch.equal(got[3, :, n:], before[3, :, n:])
        assert torch.equal(got[:3], before[:3])
    del K, V, k0, v0
    torch.cuda.empty_cache()
