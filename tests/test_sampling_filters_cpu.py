"""CPU: the sampling filters' host side.  The NumPy oracle of tests/ref_sampling_filters.py is tied to the restated reference (orc.sample_stochastic) at neutral
filters before any GPU test relies on it; the inputs of the GPU identity tests are shown to exercise the penalties; host.py's validation and the plan text."""
import numpy as np
import pytest

import orc
import ref_sampling_filters as R
from mila_amd import capi, host
from test_sample_radix_gpu import CASES, DRAWS, _logits


@pytest.mark.parametrize("V,softcap,t,k,p", CASES)
def test_the_numpy_oracle_agrees_with_the_reference_oracle_at_neutral_filters(V, softcap, t, k, p):
    """every draw of DRAWS for every case of the radix sampler's tests: on a decisive draw (that file's rule, by the reference oracle's margins) the two oracles name
    the same token, with and without an all-zero table"""
    lg = _logits(V, k)
    plain = R.Distribution(lg, softcap, t, k, p)
    tabled = R.Distribution(lg, softcap, t, k, p, R.NEUTRAL, np.zeros(V, dtype=np.int32))
    assert np.array_equal(plain.x, tabled.x)                # neutral penalties leave every logit's bits
    decisive = 0
    for r in DRAWS:
        tok, m = orc.sample_stochastic(lg, softcap, t, k, p, r)
        if m[0] > 1e-6 and m[2] > 2e-3:
            decisive += 1
            assert plain.draw(r)[0] == tok == tabled.draw(r)[0], "r=%g: %d != reference oracle %d (margins %s)" % (r, plain.draw(r)[0], tok, m)
    if not (k == 0 and p >= 1.0):                           # (the untruncated case: every probability is ~1e-5, no draw is decisive -- as in the radix tests)
        assert decisive >= 12


def test_the_adjusted_logit_by_hand():
    """x3 on numbers whose products and differences are exact in fp32"""
    lg = np.array([2.0, -2.0, 2.0, -2.0, 3.0, 3.0, 0.0], dtype=np.float32)
    flag = -2 ** 31
    table = np.array([0, 0, flag, flag, 3, flag | 1, 2], dtype=np.int64).astype(np.int32)
    x3 = R.adjusted_logits(lg, table, 0.0, 2.0, 0.25, 0.5)
    #  untouched | prompt only: x / rep, x * rep | generated 3 times: 3 / 2 - 1.5 - 0.25 | prompt + once: 1.5 - 0.5 - 0.25 | zero logit, twice: 0 * rep - 1 - 0.25
    assert x3.tolist() == [2.0, -2.0, 1.0, -4.0, -0.25, 0.75, -1.25]
    assert x3.dtype == np.float32
    assert np.array_equal(R.adjusted_logits(lg, table, 0.0, 1.0, 0.0, 0.0), lg)
    assert R.argmax_filtered(lg, 0.0, (0.0, 2.0, 0.25, 0.5), table) == 0
    # inv_rep is the rounded reciprocal, not a division per element
    x = np.float32(7.0)
    got = R.adjusted_logits(np.array([x]), np.array([1], dtype=np.int32), 0.0, 1.3, 0.0, 0.0)[0]
    assert got == x * (np.float32(1.0) / np.float32(1.3))


def test_the_generator_reproduces_libstdcxx_mt19937_64_uniform():
    """the first raw output and the first five draws of std::mt19937_64(seed) through uniform_real_distribution<float>(0, 1), libstdc++ (printed by a C++ program)"""
    want = {40: (4346996961871706838, [0.23565118, 0.736638546, 0.590784132, 0.158514664, 0.383457541]),
            5489: (14514284786278117030, [0.786820948, 0.250480354, 0.710671246, 0.94666779, 0.019271059])}
    for seed, (raw, draws) in want.items():
        assert R.Mt19937_64(seed).raw() == raw
        g = R.Mt19937_64(seed)
        assert [float(np.float32(d)) for d in draws] == [float(g.uniform()) for _ in range(5)]


def test_min_p_in_the_oracle():
    lg = np.log(np.array([0.5, 0.25, 0.15, 0.06, 0.04], dtype=np.float64)).astype(np.float32)
    d = R.Distribution(lg, 0.0, 1.0, 0, 1.0, (0.2, 1.0, 0.0, 0.0))             # 0.2 * 0.5 = 0.1: the last two go
    assert (d.e > 0).tolist() == [True, True, True, False, False]
    assert d.m_minp == pytest.approx(1.0 - 0.12 / 0.2, abs=1e-5)               # the nearest ratio e / min_p is 0.12 / 0.2
    assert [d.draw(r)[0] for r in (0.0, 0.5, 0.6, 0.99)] == [0, 0, 1, 2]
    peak = np.zeros(100, dtype=np.float32)
    peak[71] = 60.0
    assert {R.sample_filtered(peak, 0.0, 1.0, 0, 1.0, r, (1e-6, 1.0, 0.0, 0.0))[0] for r in DRAWS} == {71}


@pytest.mark.parametrize("V", sorted(R.IDENTITY_SETTINGS))
def test_the_identity_tests_inputs_exercise_the_penalties(V):
    """what tests/test_sample_filtered_gpu.py relies on: with the table of make_table, at every vocabulary >= 257 and for every penalty triple, at least one draw's
    token differs from the unpenalized token; the greedy token moves under at least one triple of GREEDY_PENALTIES"""
    t, k, p = R.IDENTITY_SETTINGS[V]
    lg = R.random_logits(V)
    table = R.make_table(lg)
    w = table.view(np.uint32)
    assert ((w & R.FLAG) != 0).sum() >= 8 and ((w & R.COUNT_MASK) != 0).sum() >= 8
    base = R.Distribution(lg, 0.0, t, k, p)
    for pen in R.PENALTIES:
        d = R.Distribution(lg, 0.0, t, k, p, (0.0,) + pen, table)
        changed = sum(d.draw(r)[0] != base.draw(r)[0] for r in DRAWS)
        if V >= 257:
            assert changed >= 1, (V, pen)
    glg = R.greedy_logits(V)
    gtable = R.make_table(glg)
    if V >= 257:
        assert any(R.argmax_filtered(glg, 0.0, (0.0,) + pen, gtable) != int(np.argmax(glg)) for pen in R.GREEDY_PENALTIES)


def test_host_validation_of_the_filters():
    assert host._filters() == R.NEUTRAL
    assert host._filters(0.05, 1.3, 0.5, 0.25) == (0.05, 1.3, 0.5, 0.25)
    assert host._filters(min_p=0.999, presence_penalty=-2.0)[0] == 0.999       # a negative penalty (a reward) is allowed
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")), dict(min_p=float("nan")),
                dict(presence_penalty=float("inf")), dict(frequency_penalty=float("-inf")), dict(min_p=1.0), dict(min_p=-0.1), dict(min_p=1.5)):
        with pytest.raises(ValueError):
            host._filters(**bad)


@pytest.mark.parametrize("V,k,p", [(262144, 64, 0.95), (262144, 0, 0.9), (262144, 40, 1.0), (262144, 0, 1.0), (1000, 5, 0.99), (65, 8, 0.5)])
def test_a_filtered_call_launches_what_the_unfiltered_call_launches(V, k, p):
    """one deciding function: the filters choose instantiations of launches the plan already has"""
    plain = capi.sample_radix_plan(V, k, p)
    for filters, with_table, want in ((None, False, (0, 0)), (R.NEUTRAL, False, (0, 0)), ((0.05, 1.0, 0.0, 0.0), False, (0, 1)), ((0.0, 1.3, 0.5, 0.25), True, (1, 0)),
                                      ((0.3, 1.15, 0.5, 0.25), True, (1, 1)), ((0.0, 1.3, 0.0, 0.0), False, (0, 0)), (R.NEUTRAL, True, (1, 0))):
        got = capi.sample_filters_plan(V, k, p, filters, with_table)
        assert {f: got[f] for f in capi.RADIX_PLAN_FIELDS} == plain, (filters, with_table)
        assert (got["scale_filtered"], got["mask_filtered"]) == want, (filters, with_table)
    for bad in ((1.0, 1.0, 0.0, 0.0), (-0.5, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, float("nan"), 0.0, 0.0), (0.0, 1.0, float("inf"), 0.0)):
        assert capi.sample_filters_plan(V, k, p, bad, True) is None


def test_the_filtered_entries_refuse_bad_filters_before_any_device_work():
    """validation comes first: the pointers are never dereferenced"""
    import ctypes as C
    lib = capi.load()
    one, null = C.c_void_p(16), C.c_void_p(None)
    for bad in ((0.0, 0.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), (-0.1, 1.0, 0.0, 0.0), (float("nan"), 1.0, 0.0, 0.0), (0.0, float("inf"), 0.0, 0.0),
                (0.0, 1.0, float("nan"), 0.0), (0.0, 1.0, 0.0, float("-inf"))):
        f = capi.sample_filters(*bad)
        assert lib.mila_cdna4_sample_radix_filtered_fp32(one, one, 100, 0.0, 1.0, 0, 1.0, 0.5, C.byref(f), one, one, C.c_size_t(1 << 20), null) == capi.MILA_E_INVALID_ARGUMENT, bad
        assert lib.mila_cdna4_sample_argmax_filtered_fp32(one, one, 100, 0.0, C.byref(f), one, one, C.c_size_t(1 << 20), null) == capi.MILA_E_INVALID_ARGUMENT, bad
        assert lib.mila_cdna4_sample_radix_filtered_rows_fp32(one, C.c_size_t(100), one, 2, 100, 0.0, 1.0, 0, 1.0, one, C.byref(f), one, C.c_size_t(100), one, C.c_size_t(1 << 22),
                                                              null) == capi.MILA_E_INVALID_ARGUMENT, bad
    good = capi.sample_filters(*R.NEUTRAL)
    assert lib.mila_cdna4_sample_radix_filtered_rows_fp32(one, C.c_size_t(100), one, 2, 100, 0.0, 1.0, 0, 1.0, one, C.byref(good), one, C.c_size_t(99), one, C.c_size_t(1 << 22),
                                                          null) == capi.MILA_E_INVALID_ARGUMENT                    # table_stride < vocab
    assert b"table_stride" in lib.mila_cdna4_last_error()
    assert lib.mila_cdna4_token_table_bytes(262144) == 1 << 20 and lib.mila_cdna4_token_table_bytes(0) == 0
    assert lib.mila_cdna4_token_table_mark_prompt(null, C.c_size_t(0), 0, 100, one, 4, null) == capi.MILA_E_INVALID_ARGUMENT
