"""The decode-attention plan (csrc/attention.hip: plan_decode -- shape -> kernel form, split count, band, grid, scratch) checked without a GPU: the plan is data.

Parity with the build the fixtures were recorded from (tools/attn_decode_plan_fixtures.py queries, run BEFORE the rules were gathered into plan_decode; re-record only on
purpose): tests/golden/attn_decode_plan_queries.json holds attn_decode_split_count over 3 batch sizes x 6 head layouts x 5 head sizes x 8 capacities x 3 windows and
attn_decode_scratch_bytes over their (B, NH, HS), at the defaults and under 7 single tunings.  The queries answer the same, and so does the plan the partials entry runs
at len_hint 0.  Soundness over the same sweep and seven live-length hints: the scratch query bounds every plan, the matrix-core form is chosen exactly by its rule, the
band bucket is monotone, idempotent and covers the live length, and split_count(len_hint) is the split count of the partials entry's plan."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from mila_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("attn_decode_plan_fixtures", os.path.join(ROOT, "tools", "attn_decode_plan_fixtures.py"))
fixtures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fixtures)

QUERIES = json.load(open(os.path.join(ROOT, "tests", "golden", "attn_decode_plan_queries.json")))
CASES = fixtures.sweep_cases(QUERIES["sweep"])
SETTINGS = ["default"] + sorted(QUERIES["tuned"])
MFMA_MIN_BAND = 8192      # the default of attn.mfma_min_band


@pytest.fixture
def tuned():
    """set single tunings through the returned function; every default is back afterwards"""
    def set_(setting):
        fixtures.apply_setting(setting)
        return dict([(setting.split("=")[0], int(setting.split("=")[1]))] if setting != "default" else [])
    yield set_
    capi.tune_reset()


_buf = C.create_string_buffer(256)


def _plan(B, NH, NKV, HS, cap, window, hint, fused, hooks):
    """capi.attn_decode_plan without its per-call set-up (the sweeps below ask for several hundred thousand plans)"""
    assert capi.load().mila_cdna4_attn_decode_plan_describe(B, NH, NKV, HS, cap, window, hint, fused, hooks, _buf, 256) > 0
    f = _buf.value.decode().split(":")
    return dict(zip(capi.PLAN_FIELDS, [f[0]] + [int(v) for v in f[1:]]))


def _recorded(setting, what):
    row = QUERIES["default"][what] if setting == "default" else QUERIES["tuned"][setting][what]
    return QUERIES["default"][what] if row == "same" else row


def _hints(capacity):
    return [0, 1, 4096, 4097, 8192, 8193, capacity]


def test_the_sweep_is_the_one_the_fixtures_were_recorded_over():
    assert capi.attn_decode_plan(1, 16, 1, 512, 8300, 0, 4097, fused=True) == _plan(1, 16, 1, 512, 8300, 0, 4097, True, False) == dict(
        form="attn_decode_mfma", splits=64, band_max=8192, heads_per_group=2, head_groups=8, flat=0, prologue=1, partial_floats=16 * 64 * 516, scratch_need=4 * 16 * 64 * 516 + 2 * 16 * 512)
    assert QUERIES["sweep"] == fixtures.SWEEP and len(CASES) == 2160 and len(QUERIES["default"]["splits"]) == len(CASES)
    assert sorted(QUERIES["tuned"]) == sorted("%s=%d" % t for t in fixtures.TUNINGS)


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_queries_and_the_partials_plan_answer_as_the_recorded_build_did(tuned, setting):
    tuned(setting)
    lib = capi.load()
    want = _recorded(setting, "splits")
    got = [int(lib.mila_cdna4_attn_decode_split_count(*c, 0)) for c in CASES]
    diff = [(c, g, w) for c, g, w in zip(CASES, got, want) if g != w]
    assert not diff, "%d split counts differ from tests/golden/attn_decode_plan_queries.json, first: %s" % (len(diff), diff[:5])
    plans = [_plan(*c, 0, True, True)["splits"] for c in CASES]      # hooks: the partials entry's no_combine
    diff = [(c, g, w) for c, g, w in zip(CASES, plans, want) if g != w]
    assert not diff, "%d plans differ from the recorded split counts, first: %s" % (len(diff), diff[:5])
    assert len(set(want)) > 4, "the sweep is vacuous"
    scratch = [int(lib.mila_cdna4_attn_decode_scratch_bytes(*c)) for c in fixtures.scratch_cases(QUERIES["sweep"])]
    assert scratch == _recorded(setting, "scratch")


@pytest.mark.parametrize("setting", SETTINGS)
def test_every_plan_fits_the_scratch_query_and_takes_the_matrix_core_form_exactly_by_its_rule(tuned, setting):
    tune = tuned(setting)
    lib = capi.load()
    mfma_on, min_band = tune.get("attn.mfma_decode", 1), tune.get("attn.mfma_min_band", MFMA_MIN_BAND)
    forms = set()
    for B, NH, NKV, HS, cap, window in CASES:
        bound = int(lib.mila_cdna4_attn_decode_scratch_bytes(B, NH, HS))
        for hint in _hints(cap):
            for fused, hooks in ((False, False), (True, False), (True, True)):
                p = _plan(B, NH, NKV, HS, cap, window, hint, fused, hooks)
                what = (setting, B, NH, NKV, HS, cap, window, hint, fused, hooks, p)
                assert p["scratch_need"] <= bound, what
                bucket = lib.mila_cdna4_attn_decode_band_bucket(hint, cap) if hint > 0 else cap
                assert p["band_max"] == (window if 0 < window < cap else bucket), what
                mfma = bool(mfma_on) and HS == 512 and (NH // NKV) % 16 == 0 and p["band_max"] >= min_band and not hooks
                assert (p["form"] == "attn_decode_mfma") == mfma, what
                assert p["form"] == ("attn_decode_mfma" if mfma else "attn_decode" if HS in (64, 128, 256, 512) else "attn_generic"), what
                assert p["prologue"] == int(mfma and fused) and p["splits"] >= 1 and p["partial_floats"] == B * NH * p["splits"] * (HS + 4), what
                assert p["scratch_need"] == (0 if p["form"] == "attn_generic" or (not mfma and p["splits"] == 1) else
                                             4 * p["partial_floats"] + (2 * B * NH * HS if p["prologue"] else 0)), what
                forms.add(p["form"])
                if hooks:      # the partials entry's plan: what a caller sizes and merges the partials by
                    assert lib.mila_cdna4_attn_decode_split_count(B, NH, NKV, HS, cap, window, hint) == p["splits"], what
    assert forms == ({"attn_decode", "attn_generic"} | ({"attn_decode_mfma"} if mfma_on else set()))


def test_the_band_bucket_is_monotone_idempotent_and_covers_the_live_length():
    bucket = capi.load().mila_cdna4_attn_decode_band_bucket
    for cap in QUERIES["sweep"]["capacity"] + [1, 4095, 16384, 16385, 40000]:
        lens = sorted({1, 2, 63, 64, 4095, 4096, 4097, 8191, 8192, 8193, 12000, 12288, 12289, 16384, 16385, 32768, 32769, cap - 1, cap, cap + 1} - {0})
        got = [bucket(n, cap) for n in lens]
        assert got == sorted(got), (cap, got)
        for n, b in zip(lens, got):
            assert b >= min(n, cap) and b <= cap and bucket(b, cap) == b, (cap, n, b)
            assert b == min(cap, max(4096, 1 << (n - 1).bit_length())), (cap, n, b)      # the doubling rule: 4096, 8192, 16384, ..., clipped to the capacity
    assert bucket(9001, 12000) == 12000 and bucket(7001, 12000) == 8192 and bucket(100, 0) == 0
