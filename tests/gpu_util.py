"""Helpers shared by the GPU parity tests: device buffers as torch tensors, bf16 bit handling,
ulp-aware comparison against the float64 oracle."""
import ctypes as C

import numpy as np
import torch

from mila_amd import capi

DEV = "cuda:0"


def dev_u16(bits):
    """uint16 numpy (bf16 bit patterns) -> int16 torch tensor on the GPU."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).to(DEV)


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


def dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


# Output buffers are handed out POISONED: the caching allocator returns blocks that an earlier case of the same shape filled with correct results, so an element a
# kernel never writes would otherwise pass.  bf16 0x7fc0 / fp32 0x7fc00000 are quiet NaNs (every comparison helper here rejects a non-finite output), 0xff is no
# e4m3 code a quantizer emits (it is the NaN code).
def empty_u16(*shape):
    return torch.full(shape, 0x7fc0, dtype=torch.int16, device=DEV)


def empty_f32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def empty_u8(*shape):
    return torch.full(shape, 0xff, dtype=torch.uint8, device=DEV)


def bits(t):
    """int16 device tensor -> uint16 numpy bit patterns."""
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """RNE, numpy only (the oracle's converter is checked against this in test_oracle_kats)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return r.astype(np.uint16)


def _ordered(bits16):
    b = np.asarray(bits16, dtype=np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7fff), b)


def assert_bf16_close(got_bits, expected, max_ulp=1, atol=0.0, what=""):
    """got (bf16 bits) must be within `max_ulp` bf16 ulps of RNE(expected) or within atol."""
    got_bits = np.asarray(got_bits).reshape(-1)
    expected = np.asarray(expected, dtype=np.float64).reshape(-1)
    assert got_bits.size == expected.size, (got_bits.size, expected.size)
    exp_bits = f32_to_bf16_bits(expected.astype(np.float32))
    ulp = np.abs(_ordered(got_bits) - _ordered(exp_bits))
    got = bf16_bits_to_f32(got_bits).astype(np.float64)
    bad = (ulp > max_ulp) & ~(np.abs(got - expected) <= atol)
    bad |= ~np.isfinite(got)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError("%s: %d/%d elements off by more than %d bf16 ulp (atol %g); first at %d: got %r exp %r (%d ulp)"
                             % (what, int(bad.sum()), bad.size, max_ulp, atol, i, got[i], expected[i], int(ulp[i])))
    return int(ulp.max()) if ulp.size else 0


# x sum_k |x w|: the project's slack for the accumulation error of a GEMM (test_linear_gpu._slack), here per element.  Measured on an MI355X over every element of the four
# Gemma-4 12B Linear shapes at M = 2048 and 2303 (test_gemm_fullshape_gpu.py), worst |got - exact| / mag among the elements over max_ulp:
#   bf16 x bf16 (v_mfma_f32_16x16x32_bf16, an fp32 chain)     2^-25.3 .. 2^-24.5     1.4e-5 .. 1.6e-5 of the elements go through the slack
#   fp8 x fp8, K = 3840 / 4096 (30 / 32 K-tiles)              2^-19.2 .. 2^-18.8     4.5e-4 (W4A8) .. 7.2e-4 (W8A8)
#   fp8 x fp8, K = 15360 (120 K-tiles)                         2^-20.1                the same share
# the same for every kernel form (256 x 256, 256 x 128 ring, split-K, column split), tile-row and band: the instruction's arithmetic, not a kernel's.  The fp8 share is
# 50 x the bf16 one because v_mfma_scale_f32_16x16x128_f8f6f4 does not sum its 128 products as an fp32 chain: one instruction on random e4m3 operands differs from the
# exact sum by up to 2^-11.6 of its LARGEST product (2^-16.1 of sum |a b| on Gaussian operands), and 2^16 - 2^16 + 1 within one instruction gives 0 -- products are aligned
# to the largest of the block and the bits below are dropped.  Errors of the K / 128 blocks are independent: 2^-16.1 / sqrt(30) = 2^-18.6, / sqrt(120) = 2^-19.6, which is
# what the GEMMs show.  2^-17 holds from 4 K-tiles on (2^-16.1 / sqrt(4)) and keeps a factor 3.5 at the Gemma shapes; a kernel that loses one of 120 K-tiles is off by
# about 2^-10 of mag, one that loses one k of 15360 by 2^-14 (test_gemm_bar_cpu.py: both fail on most of the elements they touch).
SLACK = 2.0 ** -17


def _where(idx2, N, row_ids=None):
    """which 256-row tile-rows, 64-row wave bands and 128-column tile-columns a set of flat indices lies in"""
    m, n = idx2 // N, idx2 % N
    if row_ids is not None:
        m = np.asarray(row_ids)[m]

    def fmt(v, cap=24):
        v = sorted(set(int(x) for x in v))
        return "%d: %s%s" % (len(v), v[:cap], " ..." if len(v) > cap else "")
    return "256-row tile-rows {%s}; 64-row bands {%s}; 128-column tile-columns {%s}" % (fmt(m // 256), fmt(m // 64), fmt(n // 128))


def _bf16_rounding_flip(g, post):
    """for exact values g that a composition rounds to bf16 BEFORE it goes on (x post, + bias): (distance of g from the rounding boundary nearest to it, the step the
    composition's result takes when the rounding goes to the other side of that boundary), both in units of the result (x |post|)"""
    gb = bf16_bits_to_f32(f32_to_bf16_bits(g.astype(np.float32))).astype(np.float64)
    frac, e = np.frexp(np.abs(gb))
    ulp = np.ldexp(1.0, e - 8)                                          # the bf16 spacing above |gb| ...
    ulp = np.where((frac == 0.5) & (np.abs(g) < np.abs(gb)), ulp / 2, ulp)      # ... and the one below a power of two, when g lies on that side
    side = np.where(g >= gb, 1.0, -1.0)
    return (0.5 * ulp - np.abs(g - gb)) * np.abs(post), side * ulp * post


def assert_gemm_close(got_bits, exact, mag, max_ulp, what, atol_global=0.0, stats=None, inner=None, row_ids=None):
    """EVERY element of a GEMM output [M, N] (bf16 bits) against its float64 expectation: an element passes if it is within `max_ulp` bf16 ulp of RNE(exact), or if
    |got - exact| <= min(atol_global, 2^-17 * mag[m, n]), mag[m, n] = sum_k |x w| times the scales (ref_matmul.abs_products): the slack for outputs that are the
    difference of large partial sums is taken from THAT element's partial sums, not from the largest output of the whole matrix, so a quiet row or channel is held to its
    own scale; atol_global (what the calling test used as its one atol before) stays the ceiling.  Non-finite outputs fail.
    mag: an [M, N] array, or a callable (m_idx, n_idx) -> vector, asked only for the elements over max_ulp (the second matmul is not needed for the rest).
    inner = (g [M, N] float64, post [M] or None), for a composition with TWO bf16 roundings (bf16 GEMM + bias: y = bf16(bf16(g) + bias); W4A8: y = bf16(bf16(g) s_m + bias)),
    where `exact` holds the composition with RNE(g): the expectation is then not unique.  The kernel's fp32 sum differs from g by up to the slack above, so when g lies
    within 2^-17 * mag (in g's units) of a bf16 rounding boundary, a correct kernel may round the intermediate to the other side, and its result is the composition of THAT
    neighbour: exact +- ulp_bf16(g) * post.  Where y is the small difference of bf16(g) and the bias, that one step of g is many ulp of y, and no slack taken from the
    accumulation covers it (measured: 10 - 14 of 7.9 M elements of the bf16 + bias legs at M = 2048, 344 - 773 of the W4A8 + bias legs).  For exactly those elements --
    g provably within the accumulation slack of a boundary -- the element also passes if it meets the same bar against that second expectation.  Nothing else is relaxed.
    stats (a dict) receives worst_ulp, over_ulp (elements over max_ulp that the slack let through), n, worst_ratio (max |got - exact| / mag over those) and inner_flips
    (elements that passed against the second expectation only).
    A failure reports the count, the worst element and where the failures lie; row_ids (the output's row number of each row handed in, for a test that looks at
    sampled rows) puts the report in the output's own rows."""
    got_bits = np.asarray(got_bits, dtype=np.uint16)
    exact = np.asarray(exact, dtype=np.float64)
    assert got_bits.ndim == 2 and got_bits.shape == exact.shape, (got_bits.shape, exact.shape)
    M, N = exact.shape
    gb, ex = got_bits.reshape(-1), exact.reshape(-1)
    ulp = np.abs(_ordered(gb) - _ordered(f32_to_bf16_bits(ex.astype(np.float32))))
    got = bf16_bits_to_f32(gb).astype(np.float64)
    finite = np.isfinite(got)
    over = np.flatnonzero((ulp > max_ulp) | ~finite)
    err = np.abs(got[over] - ex[over])
    if callable(mag):
        mg = np.asarray(mag(over // N, over % N), dtype=np.float64) if over.size else np.zeros(0)
    else:
        mg = np.asarray(mag, dtype=np.float64).reshape(-1)[over]
    with np.errstate(invalid="ignore"):
        ok = finite[over] & (err <= np.minimum(atol_global, SLACK * mg))
    flips = 0
    if inner is not None and over.size:
        g, post = inner
        post = np.ones(M) if post is None else np.asarray(post, dtype=np.float64)
        dist, step = _bf16_rounding_flip(np.asarray(g, dtype=np.float64).reshape(-1)[over], post[over // N])
        alt = ex[over] + step
        alt_ulp = np.abs(_ordered(gb[over]) - _ordered(f32_to_bf16_bits(alt.astype(np.float32))))
        with np.errstate(invalid="ignore"):
            ok2 = finite[over] & (dist <= SLACK * mg) & ((alt_ulp <= max_ulp) | (np.abs(got[over] - alt) <= np.minimum(atol_global, SLACK * mg)))
        flips = int((ok2 & ~ok).sum())
        ok2 &= ~ok
    else:
        ok2 = np.zeros(over.size, dtype=bool)
    if stats is not None:
        let = ok & (mg > 0)
        stats.update(n=int(ex.size), worst_ulp=int(ulp[finite].max()) if finite.any() else -1, over_ulp=int(ok.sum()),
                     worst_ratio=float((err[let] / mg[let]).max()) if let.any() else 0.0, inner_flips=flips)
    ok = ok | ok2
    bad = over[~ok]
    if bad.size:
        berr = np.where(np.isfinite(err[~ok]), err[~ok], np.inf)
        w = int(bad[int(np.argmax(berr))])
        j = int(np.flatnonzero(over == w)[0])
        e = AssertionError("%s: %d of %d elements (%d non-finite) off by more than %d bf16 ulp and more than min(%g, 2^-17 x %g); worst at [%d, %d]: got %r exact %r "
                           "(%d ulp); failures in %s" % (what, bad.size, ex.size, int((~finite).sum()), max_ulp, atol_global, float(mg[j]), w // N if row_ids is None else int(row_ids[w // N]), w % N,
                                                         got[w], ex[w], int(ulp[w]), _where(bad, N, row_ids)))
        e.bad_rows, e.bad_cols = (bad // N if row_ids is None else np.asarray(row_ids)[bad // N]), bad % N
        raise e
    return int(ulp.max()) if ulp.size else 0


def sample_rows(M, rng):
    """the rows a sampled oracle check looks at: every row for M <= 65; otherwise the first and last present row of every 256-row tile-row, one row (drawn from the seeded
    rng) in each 32-row band of the first, a middle and the last full tile-row, and of the remainder M % 256 its first and last row plus eight drawn ones.  Rows 0 and
    M - 1 are always in the set.  Every 256-row tile a persistent walk visits and every wave band of a tile is seen by the oracle."""
    if M <= 65:
        return list(range(M))
    rows = {0, M - 1}
    full = M // 256
    for t in range((M + 255) // 256):
        rows.update((t * 256, min(M, t * 256 + 256) - 1))
    for t in sorted({0, full // 2, full - 1}) if full else []:
        for b in range(8):
            rows.add(t * 256 + b * 32 + int(rng.integers(32)))
    rem = M % 256
    if rem:
        rows.update(full * 256 + int(r) for r in rng.integers(rem, size=8))
    return sorted(rows)


def rel_err(got, expected):
    got = np.asarray(got, dtype=np.float64)
    expected = np.asarray(expected, dtype=np.float64)
    return np.abs(got - expected).max() / max(np.abs(expected).max(), 1e-30)


def call(name, *args):
    capi.call(name, *args)


def size_t(v):
    return C.c_size_t(v)


def i64(v):
    return C.c_int64(v)
