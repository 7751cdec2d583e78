"""CPU: keeps gpu_util.assert_gemm_close (the elementwise bar of the full-shape GEMM tests) honest without a GPU.

An emulation of the device arithmetic of the fp8 x fp8 prefill GEMM at fc_down's K -- exact e4m3 products, fp32 accumulation of 32- or 128-wide partial sums K-tile by
K-tile, fp32 epilogue (x scale[n], x s_m, + bias), one bf16 rounding -- on the GPU tests' operands (channel scales over 4 octaves, token scales 0.2 - 3.0, a zero token)
must PASS the bar; four wrong kernels must FAIL it, and the report must say where:
  1. one of the 120 K-tiles left out in one 64-row wave band;
  2. one k left out everywhere;
  3. a 25 % scale error on the 64 quietest channels;
  4. a 25 % scale error on the 32 quietest tokens.
3 and 4 are what the bar exists for: one atol taken from the loudest output of the whole matrix is of the order of the quiet outputs themselves.
(The emulation is an fp32 chain over partial sums; the fp8 matrix-core instruction itself is coarser -- figures beside gpu_util.SLACK -- which is why the device lets 5e-4
of its elements through the slack where this emulation lets through a few in a million.  The mutants' distance from the bar does not depend on that.)"""
import numpy as np
import pytest

import orc
import ref_matmul
from gpu_util import SLACK, _bf16_rounding_flip, assert_bf16_close, assert_gemm_close, f32_to_bf16_bits, sample_rows

M, K, N = 512, 15360, 1024
BAND, KTILE, ONE_K = 5, 57, 7001


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(11)
    Wb = orc.to_bf16_bits((rng.standard_normal((N, K)) / np.sqrt(K) * rng.uniform(0.25, 4.0, (N, 1))).astype(np.float32))
    X = orc.round_bf16((rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32))
    X[7] = 0.0
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32))
    w8, sc = orc.quantize_fp8_per_channel(Wb)
    x8, ts = orc.quantize_act_fp8_per_token(X)
    exact = ref_matmul.linear_fp8a_fp8w(x8, ts, w8, sc, 1.0, bb)
    return dict(x8=x8, ts=ts, w8=w8, sc=sc, bb=bb, exact=exact, atol=1e-3 * float(np.abs(exact).max()),
                mag=lambda m, n: ref_matmul.abs_products("fp8a_fp8w", x8, w8, (ts, sc), at=(m, n)),         # the few elements in question (what the GPU tests pass)
                mag_all=ref_matmul.abs_products("fp8a_fp8w", x8, w8, (ts, sc)))                             # the whole matrix (a mutant puts most elements in question)


def _device(c, width=128, skip_tile_in_band=None, skip_k=None, sc=None, ts=None):
    """bf16 bits of the emulated kernel: fp32 accumulator, `width`-wide partial sums (exact, then rounded to fp32) added in K order"""
    Xd, Wd = ref_matmul.e4m3_to_f64(c["x8"]), ref_matmul.e4m3_to_f64(c["w8"])
    if skip_k is not None:
        Xd = Xd.copy()
        Xd[:, skip_k] = 0.0
    acc = np.zeros((M, N), dtype=np.float32)
    for k0 in range(0, K, width):
        part = (Xd[:, k0:k0 + width] @ Wd[:, k0:k0 + width].T).astype(np.float32)
        if skip_tile_in_band is not None and k0 // 128 == skip_tile_in_band[1]:
            b = skip_tile_in_band[0]
            part[b * 64:b * 64 + 64] = 0.0
        acc += part
    sc = c["sc"] if sc is None else sc
    ts = c["ts"] if ts is None else ts
    y = acc * sc.astype(np.float32)[None, :] * ts.astype(np.float32)[:, None] + orc.from_bf16_bits(c["bb"])[None, :]
    return f32_to_bf16_bits(y.astype(np.float32)).reshape(M, N)


@pytest.mark.parametrize("width", [32, 128])
def test_the_emulated_device_arithmetic_passes_the_elementwise_bar(case, width):
    stats = {}
    got = _device(case, width)
    assert_gemm_close(got, case["exact"], case["mag"], 2, "emulation, %d-wide partial sums" % width, case["atol"], stats)
    assert stats["n"] == M * N and stats["worst_ulp"] >= 1
    assert stats["over_ulp"] <= 1e-4 * M * N, stats                     # a few in a million go through the slack, not more
    assert stats["worst_ratio"] <= 2.0 ** -17
    # an [M, N] magnitude array is taken as well as the callable
    stats2 = {}
    assert_gemm_close(got, case["exact"], case["mag_all"], 2, "emulation, array magnitude", case["atol"], stats2)
    assert stats2["over_ulp"] == stats["over_ulp"] and stats2["worst_ulp"] == stats["worst_ulp"]


def _fails(case, got):
    with pytest.raises(AssertionError) as info:
        assert_gemm_close(got, case["exact"], case["mag_all"], 2, "mutant", case["atol"])
    return info.value, str(info.value)


def test_a_k_tile_left_out_in_one_wave_band_fails_and_the_report_names_the_band(case):
    e, text = _fails(case, _device(case, skip_tile_in_band=(BAND, KTILE)))
    assert set(e.bad_rows // 64) == {BAND}
    assert e.bad_rows.size > 0.5 * 64 * N
    assert "64-row bands {1: [%d]}" % BAND in text and "256-row tile-rows {1: [%d]}" % (BAND // 4) in text


def test_sampled_rows_are_reported_by_their_own_row_numbers(case):
    """a test that hands in sampled rows (the dispatch ladder) gets the report in the output's rows"""
    rows = [3, 64 * BAND + 9, 64 * BAND + 40, 500]
    got = _device(case, skip_tile_in_band=(BAND, KTILE))[rows]
    with pytest.raises(AssertionError) as info:
        assert_gemm_close(got, case["exact"][rows], case["mag_all"][rows], 2, "sampled", case["atol"], row_ids=rows)
    assert set(info.value.bad_rows.tolist()) == {64 * BAND + 9, 64 * BAND + 40} and "64-row bands {1: [%d]}" % BAND in str(info.value)


def test_one_k_left_out_everywhere_fails(case):
    e, text = _fails(case, _device(case, skip_k=ONE_K))
    assert e.bad_rows.size > 0.1 * M * N
    assert set(e.bad_rows // 64) == set(range(M // 64)) and set(e.bad_cols // 128) == set(range(N // 128))


def test_a_scale_error_on_the_quietest_channels_fails_where_one_global_atol_passes_elements(case):
    quiet = np.argsort(case["sc"])[:64]
    sc = case["sc"].copy()
    sc[quiet] *= np.float32(1.25)
    got = _device(case, sc=sc)
    e, text = _fails(case, got)
    assert set(e.bad_cols) == set(quiet.tolist())
    assert e.bad_cols.size > 0.9 * 64 * (M - 1)
    assert "128-column tile-columns {%d:" % len(set((quiet // 128).tolist())) in text
    # the bar this one replaces sees fewer of the same wrong elements
    with pytest.raises(AssertionError) as old:
        assert_bf16_close(got, case["exact"], 2, case["atol"], "global atol")
    assert int(str(old.value).split(":")[1].split("/")[0]) < e.bad_cols.size


def test_a_scale_error_on_the_quietest_tokens_fails_and_the_report_names_their_bands(case):
    ts = case["ts"].copy()
    order = [m for m in np.argsort(ts) if m != 7][:32]              # (row 7 is the zero token: its outputs are the bias alone)
    ts[order] *= np.float32(1.25)
    e, text = _fails(case, _device(case, ts=ts))
    assert set(e.bad_rows) == set(int(m) for m in order)
    assert e.bad_rows.size > 0.8 * 32 * N
    assert "64-row bands {%d:" % len(set(int(m) // 64 for m in order)) in text


def test_unwritten_and_non_finite_outputs_fail(case):
    got = _device(case)
    got[300:364, 128:256] = 0x7fc0                                  # the poison of gpu_util.empty_u16: a 64 x 128 patch nobody wrote
    e, text = _fails(case, got)
    assert e.bad_rows.size == 64 * 128 and set(e.bad_rows // 64) == {4, 5} and set(e.bad_cols // 128) == {1}
    assert "(8192 non-finite)" in text


def test_two_roundings_the_second_expectation_is_taken_only_at_a_rounding_boundary(case):
    """W4A8-like composition y = bf16(bf16(g) s_m + bias) on the same operands: where bf16(g) s_m nearly cancels the bias, an fp32 sum that lands on the other side of a
    bf16 rounding boundary of g moves y by many ulp.  With inner = (g, s_m) the emulation passes, an element moved by one step of g AWAY from a boundary fails, and so does
    the left-out K-tile."""
    c = case
    ws = np.float32(2e-5)                                           # (a per-tensor weight scale that puts the outputs at the size of the bias, +- 0.1)
    g = ref_matmul.linear_fp8a_fp8w(c["x8"], np.ones(M, dtype=np.float32), c["w8"], None, ws)
    ts64 = c["ts"].astype(np.float64)
    bias = orc.from_bf16_bits(c["bb"]).astype(np.float64)[None, :]
    exact = orc.round_bf16(g.astype(np.float32)).astype(np.float64) * ts64[:, None] + bias
    mag = lambda m, n: ref_matmul.abs_products("fp8a_fp8w", c["x8"], c["w8"], (c["ts"], ws), at=(m, n))
    atol = 1e-3 * float(np.abs(exact).max())

    def device(skip=None):
        Xd, Wd = ref_matmul.e4m3_to_f64(c["x8"]), ref_matmul.e4m3_to_f64(c["w8"])
        acc = np.zeros((M, N), dtype=np.float32)
        for k0 in range(0, K, 128):
            part = (Xd[:, k0:k0 + 128] @ Wd[:, k0:k0 + 128].T).astype(np.float32)
            if skip is not None and k0 // 128 == skip[1]:
                part[skip[0] * 64:skip[0] * 64 + 64] = 0.0
            acc += part
        gb = orc.round_bf16(acc * ws)
        return f32_to_bf16_bits((gb * c["ts"][:, None] + orc.from_bf16_bits(c["bb"])[None, :]).astype(np.float32)).reshape(M, N)

    got = device()
    stats = {}
    assert_gemm_close(got, exact, mag, 2, "two roundings", atol, stats, inner=(g, ts64))
    assert stats["inner_flips"] <= 1e-3 * M * N
    # one bf16 step of g on an element whose g is nowhere near a rounding boundary: not excused
    dist, step = _bf16_rounding_flip(g.reshape(-1), np.repeat(ts64, N))
    safe = np.flatnonzero((dist > 0.25 * np.abs(step)) & (np.abs(exact.reshape(-1)) < 0.3 * np.abs(step)) & (np.repeat(ts64, N) > 1e-6))
    safe = safe[np.abs(step[safe]) > 2 * SLACK * mag(safe // N, safe % N)]          # (... and the step is not inside the accumulation slack anyway)
    assert safe.size, "no element with bf16(g) s_m close to -bias in this case"
    i = int(safe[0])
    wrong = got.copy()
    wrong.reshape(-1)[i] = f32_to_bf16_bits(np.array([exact.reshape(-1)[i] + step[i]], dtype=np.float32))[0]
    with pytest.raises(AssertionError) as info:
        assert_gemm_close(wrong, exact, mag, 2, "one step of g, away from a boundary", atol, inner=(g, ts64))
    assert info.value.bad_rows.tolist() == [i // N] and info.value.bad_cols.tolist() == [i % N]
    with pytest.raises(AssertionError) as info:
        assert_gemm_close(device(skip=(BAND, KTILE)), exact, mag, 2, "K-tile left out", atol, inner=(g, ts64))
    assert set(info.value.bad_rows // 64) == {BAND} and info.value.bad_rows.size > 0.5 * 64 * N


@pytest.mark.parametrize("rows", [1, 2, 65, 66, 255, 256, 300, 512, 2048, 2049, 2303])
def test_sample_rows_sees_every_tile_row_and_every_band(rows):
    r = sample_rows(rows, np.random.default_rng(rows))
    assert r == sorted(set(r)) and r[0] == 0 and r[-1] == rows - 1 and all(0 <= x < rows for x in r)
    assert r == sample_rows(rows, np.random.default_rng(rows))
    if rows <= 65:
        assert r == list(range(rows))
        return
    for t in range((rows + 255) // 256):
        assert t * 256 in r and min(rows, t * 256 + 256) - 1 in r
    full = rows // 256
    for t in {0, full // 2, full - 1} if full else ():
        assert {x // 32 for x in r if x // 256 == t} == set(range(t * 8, t * 8 + 8))
    if rows % 256:
        assert len([x for x in r if x >= full * 256]) >= min(rows % 256, 3)
    assert len(r) <= 2 * ((rows + 255) // 256) + 24 + 10
