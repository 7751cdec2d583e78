"""The radix pipeline of the stochastic sampler, the part that needs no GPU: what a call launches (csrc/sampling.hip: plan_radix, read through
sample_radix_plan_describe by the same host function the entries launch from) and the argument checks, which answer before any device work."""
import ctypes as C

import pytest

from mila_amd import build, capi

VOCABS = (1, 65, 1000, 50257, 262144)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


@pytest.mark.parametrize("V", VOCABS)
def test_the_plan_counts_at_most_twelve_launches_and_fewer_per_truncation_that_is_off(lib, V):
    both = capi.sample_radix_plan(V, 64, 0.95)
    only_p = capi.sample_radix_plan(V, 0, 0.95)
    only_k = capi.sample_radix_plan(V, 64, 1.0)
    none = capi.sample_radix_plan(V, 0, 1.0)
    assert both["launches"] <= 12
    assert both["p_passes"] > 0 and only_p["p_passes"] == both["p_passes"] and only_k["p_passes"] == 0 and none["p_passes"] == 0
    if 64 < V:
        # top-k is on: each truncation costs launches of its own
        assert both["k_passes"] > 0 and only_k["k_passes"] == both["k_passes"] and only_p["k_passes"] == 0
        assert only_p["launches"] < both["launches"] and only_k["launches"] < both["launches"]
        assert none["launches"] < min(only_p["launches"], only_k["launches"])
        assert both["launches"] - only_p["launches"] == both["k_passes"]          # one launch per top-k digit pass
    else:
        # top_k >= V keeps everything: planned like top_k = 0
        assert both == only_p and only_k == none
        assert none["launches"] < only_p["launches"]
    assert none["k_passes"] == 0
    # the first nucleus pass rides in the probability launch: one launch per FURTHER digit pass
    assert only_p["launches"] - none["launches"] == only_p["p_passes"] - 1
    for plan in (both, only_p, only_k, none):
        assert plan["scratch_need"] == capi.sample_radix_scratch_bytes(V) == lib.mila_cdna4_sample_radix_scratch_bytes(V)
        assert plan["scratch_need"] >= 4 * V


@pytest.mark.parametrize("V", VOCABS)
def test_top_k_at_or_beyond_the_vocabulary_plans_like_top_k_off(lib, V):
    for p in (0.5, 1.0):
        assert capi.sample_radix_plan(V, V, p) == capi.sample_radix_plan(V, 0, p) == capi.sample_radix_plan(V, V + 7, p)
    if V > 1:
        assert capi.sample_radix_plan(V, V - 1, 1.0)["k_passes"] > 0


def test_the_plan_answers_nothing_for_arguments_no_call_accepts(lib):
    buf = C.create_string_buffer(64)
    for V, k, p in ((0, 0, 1.0), (-5, 0, 1.0), (100, -1, 1.0), (100, 0, 0.0), (100, 0, -0.5)):
        assert lib.mila_cdna4_sample_radix_plan_describe(V, k, p, buf, C.c_size_t(64)) == 0 and buf.value == b""
    assert lib.mila_cdna4_sample_radix_scratch_bytes(0) == 0 and lib.mila_cdna4_sample_radix_scratch_bytes(-3) == 0
    # a short buffer: the size needed comes back, the text is cut and terminated
    need = lib.mila_cdna4_sample_radix_plan_describe(262144, 64, 0.95, buf, C.c_size_t(4))
    assert need > 4 and len(buf.value) == 3
    assert lib.mila_cdna4_sample_radix_plan_describe(262144, 64, 0.95, None, C.c_size_t(0)) == need


def test_argument_checks_answer_before_any_launch(lib):
    """every pointer below is a small integer that no check dereferences: a call that got as far as a launch would fault, and a process without a device would
    fail in the runtime instead of answering INVALID_ARGUMENT / SCRATCH_TOO_SMALL with the entry's name"""
    null, one = C.c_void_p(None), C.c_void_p(16)
    V = 1000
    nb = C.c_size_t(capi.sample_radix_scratch_bytes(V))
    INV, SMALL = capi.MILA_E_INVALID_ARGUMENT, capi.MILA_E_SCRATCH_TOO_SMALL
    err = lib.mila_cdna4_last_error

    def by_value(fn, logits=one, tok=one, vocab=V, t=0.8, k=64, p=0.95, r=0.5, scratch=one, bytes_=nb):
        return fn(logits, tok, vocab, 30.0, t, k, p, r, scratch, bytes_, null)

    for name in ("sample_radix_fp32", "sample_radix_bf16"):
        fn = getattr(lib, "mila_cdna4_" + name)
        assert by_value(fn, logits=null) == INV and b"null pointer" in err() and name.encode() in err()
        assert by_value(fn, tok=null) == INV and b"null pointer" in err()
        assert by_value(fn, vocab=0) == INV and b"vocab" in err()
        assert by_value(fn, t=0.0) == INV and b"temperature" in err()
        assert by_value(fn, t=-1.0) == INV and b"temperature" in err()
        assert by_value(fn, p=0.0) == INV and b"top_p > 0" in err()
        assert by_value(fn, k=-1) == INV and b"top_k >= 0" in err()
        assert by_value(fn, r=-0.01) == INV and b"0 <= r <= 1" in err()
        assert by_value(fn, r=1.5) == INV and b"0 <= r <= 1" in err()
        assert by_value(fn, scratch=null) == SMALL and b"scratch" in err()
        assert by_value(fn, bytes_=C.c_size_t(nb.value - 1)) == SMALL and b"required %d" % nb.value in err()
        assert by_value(fn, scratch=C.c_void_p(20)) == INV and b"aligned" in err()

    adv = lib.mila_cdna4_sample_radix_advance_fp32

    def advance(logits=one, tok=one, t=0.8, p=0.95, draws=one, draws_size=8, scratch=one, bytes_=nb, pos=one, seq=one, ring=one, ring_size=8):
        return adv(logits, tok, V, 30.0, t, 64, p, draws, draws_size, scratch, bytes_, pos, seq, ring, ring_size, null)

    for kw in ({"logits": null}, {"tok": null}, {"draws": null}, {"pos": null}, {"seq": null}):
        assert advance(**kw) == INV and b"sample_radix_advance_fp32: null pointer" in err(), kw
    assert advance(t=0.0) == INV and b"temperature" in err()
    assert advance(p=0.0) == INV and b"top_p > 0" in err()
    assert advance(draws_size=0) == INV and b"draws_size" in err()
    assert advance(draws_size=-2) == INV and b"draws_size" in err()
    assert advance(ring=one, ring_size=0) == INV and b"ring" in err()
    assert advance(ring=null, ring_size=8) == INV and b"ring" in err()
    assert advance(scratch=null) == SMALL
    assert advance(bytes_=C.c_size_t(64)) == SMALL and b"scratch 64 bytes" in err()
