"""Logit bias, the part that needs no GPU: the entries at the drop-in boundary (declared, listed, exported, named in INTEGRATION.md), their argument checks -- which
answer before any device work -- the ValueErrors of the Python layer, and the host-only composition of a request's four controls (Mila/TokenBias.h)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("sample_radix_biased_fp32", "sample_radix_biased_advance_fp32", "sample_radix_biased_rows_fp32", "sample_radix_biased_rows_advance_fp32",
            "sample_argmax_biased_fp32", "sample_argmax_biased_advance_fp32", "sample_argmax_biased_rows_advance_fp32")
ENTRIES = ("token_bias_bytes", "token_bias_fill", "token_bias_set") + SAMPLERS
INV, SMALL = capi.MILA_E_INVALID_ARGUMENT, capi.MILA_E_SCRATCH_TOO_SMALL
V = 1000


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_entries_are_declared_listed_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    declared = set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", text))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in ENTRIES:
        assert "mila_cdna4_" + n in declared and n in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + n), n
        assert ("mila_cdna4_" + n) in integration, n
    for n in SAMPLERS:      # one sibling per filtered entry
        assert n.replace("_biased", "_filtered") in capi.EXPORTED
    assert lib.mila_cdna4_abi_version() == 4      # additive
    assert capi.token_bias_bytes(V) == 4 * V and capi.token_bias_bytes(0) == 0 and capi.token_bias_bytes(-3) == 0


def _calls(lib):
    """each entry as a function of keyword overrides; every pointer is a small integer that no check dereferences"""
    null, one = C.c_void_p(None), C.c_void_p(16)
    z = C.c_size_t
    rows_need = capi.sample_radix_rows_scratch_bytes(4, V)
    one_need = capi.sample_radix_scratch_bytes(V)
    greedy_need = 4 * int(lib.mila_cdna4_sample_scratch_bytes())

    def radix(bias=one, bstride=0, table=one, tok=one, logits=one, vocab=V, t=0.8, scratch=one, rows=None, tstride=None):
        return lib.mila_cdna4_sample_radix_biased_fp32(logits, tok, vocab, 30.0, t, 64, 0.95, 0.5, None, table, bias, z(bstride), scratch, z(one_need), null)

    def radix_advance(bias=one, bstride=0, table=one, tok=one, logits=one, vocab=V, t=0.8, scratch=one, rows=None, tstride=None):
        return lib.mila_cdna4_sample_radix_biased_advance_fp32(logits, tok, vocab, 30.0, t, 64, 0.95, one, 8, None, table, bias, z(bstride), scratch, z(one_need), one, one, one, 8, null)

    def radix_rows(bias=one, bstride=0, table=one, tok=one, logits=one, vocab=V, t=0.8, scratch=one, rows=4, tstride=V):
        return lib.mila_cdna4_sample_radix_biased_rows_fp32(logits, z(V), tok, rows, vocab, 30.0, t, 64, 0.95, one, None, table, z(tstride), bias, z(bstride), scratch, z(rows_need),
                                                            null)

    def radix_rows_advance(bias=one, bstride=0, table=one, tok=one, logits=one, vocab=V, t=0.8, scratch=one, rows=4, tstride=V):
        return lib.mila_cdna4_sample_radix_biased_rows_advance_fp32(logits, z(V), tok, rows, vocab, 30.0, t, 64, 0.95, one, None, table, z(tstride), bias, z(bstride), scratch,
                                                                    z(rows_need), one, one, null)

    def argmax(bias=one, bstride=0, table=one, tok=one, logits=one, vocab=V, t=None, scratch=one, rows=None, tstride=None):
        return lib.mila_cdna4_sample_argmax_biased_fp32(logits, tok, vocab, 30.0, None, table, bias, z(bstride), scratch, z(greedy_need), null)

    def argmax_advance(bias=one, bstride=0, table=one, tok=one, logits=one, vocab=V, t=None, scratch=one, rows=None, tstride=None):
        return lib.mila_cdna4_sample_argmax_biased_advance_fp32(logits, tok, vocab, 30.0, None, table, bias, z(bstride), scratch, z(greedy_need), one, one, one, 8, null)

    def argmax_rows_advance(bias=one, bstride=0, table=one, tok=one, logits=one, vocab=V, t=None, scratch=one, rows=4, tstride=V):
        return lib.mila_cdna4_sample_argmax_biased_rows_advance_fp32(logits, z(V), tok, rows, vocab, 30.0, None, table, z(tstride), bias, z(bstride), scratch, z(greedy_need), one, one,
                                                                     null)

    return dict(zip(SAMPLERS, (radix, radix_advance, radix_rows, radix_rows_advance, argmax, argmax_advance, argmax_rows_advance)))


@pytest.mark.parametrize("name", SAMPLERS)
def test_the_sampler_entries_refuse_before_any_launch(lib, name):
    """a call that got as far as a launch would fault on these pointers, and a process without a device would fail in the runtime instead of answering
    INVALID_ARGUMENT / SCRATCH_TOO_SMALL"""
    null = C.c_void_p(None)
    err = lib.mila_cdna4_last_error
    fn = _calls(lib)[name]
    rows_entry = "rows" in name
    # what the mirrored entry refuses, with a bias table given
    assert fn(logits=null) == INV and b"null pointer" in err()
    assert fn(tok=null) == INV and b"null pointer" in err()
    assert fn(vocab=0) == INV and b"vocab" in err()
    assert fn(scratch=null) == SMALL and b"scratch" in err()
    assert name.encode() in err(), "a biased call reports under its own name"
    if "radix" in name:
        assert fn(t=0.0) == INV and b"temperature" in err()
    assert fn(bias=C.c_void_p(18)) == INV and b"bias must be 4-byte aligned" in err()
    # the stride rule: with more than one row 0 (shared) or >= vocab
    if rows_entry:
        for bad in (1, V // 2, V - 1):
            assert fn(bstride=bad) == INV and b"bias_stride" in err(), bad
        assert fn(rows=5) == INV and b"outside 1 .. 4" in err()
        assert fn(tstride=V - 1) == INV and b"table_stride" in err()
        assert fn(rows=1, bstride=V - 1, scratch=null) == SMALL      # one row: any stride passes the rule (the call then stops at the scratch)
        assert fn(bstride=0, scratch=null) == SMALL and fn(bstride=V, scratch=null) == SMALL and fn(bstride=V + 5, scratch=null) == SMALL
    else:
        assert fn(bstride=V - 1, scratch=null) == SMALL
    # bias = NULL is the filtered entry: its name, its refusals
    assert fn(bias=null, scratch=null) == SMALL and name.replace("_biased", "_filtered").encode() in err()
    if name == "sample_argmax_biased_rows_advance_fp32":
        assert fn(bias=null, table=null) == INV and b"null pointer" in err()      # the filtered rows greedy entry needs its table
        assert fn(table=null, scratch=null) == SMALL                               # with a bias it does not


def test_the_table_entries_refuse_before_any_launch(lib):
    null, one, z = C.c_void_p(None), C.c_void_p(16), C.c_size_t
    err = lib.mila_cdna4_last_error
    fill, set_ = lib.mila_cdna4_token_bias_fill, lib.mila_cdna4_token_bias_set
    for bad in (float("nan"), float("inf")):
        assert fill(one, z(V), 0, V, bad, null) == INV and b"finite or -inf" in err(), bad
    assert fill(null, z(V), 0, V, 0.0, null) == INV and b"null pointer" in err()
    assert fill(one, z(V), 0, 0, 0.0, null) == INV
    assert fill(one, z(V), -1, V, 0.0, null) == INV
    assert fill(one, z(V - 1), 1, V, 0.0, null) == INV and b"bias_stride" in err()
    assert set_(one, z(V), 0, V, one, one, -1, null) == INV and b"negative" in err()
    assert set_(null, z(V), 0, V, one, one, 3, null) == INV and b"null pointer" in err()
    assert set_(one, z(V), 0, V, null, one, 3, null) == INV and b"null pointer" in err()
    assert set_(one, z(V), 0, V, one, null, 3, null) == INV and b"null pointer" in err()
    assert set_(one, z(V - 1), 2, V, one, one, 3, null) == INV and b"bias_stride" in err()
    assert set_(one, z(V), 0, V, null, null, 0, null) == capi.MILA_OK      # nothing to do: no launch


def test_python_raises_value_error_before_any_call():
    from mila_amd import host
    rq = host._bias_request
    assert rq() is None and rq(logit_bias={}, banned_tokens=[], allowed_tokens=(), min_tokens=0, vocab=V) is None
    ok, arrays = rq(logit_bias={3: 1.5, 7: -2.0}, banned_tokens=[1], allowed_tokens=[3, 7, 9], min_tokens=2, stop_tokens=[9], max_new_tokens=2, vocab=V)
    assert (ok.n_bias, ok.n_banned, ok.n_allowed, ok.min_tokens) == (2, 1, 3, 2) and len(arrays) == 4
    assert rq(min_tokens=3, vocab=V) is not None      # min_tokens alone is a request (the model's default stop set is held back)
    bad = [dict(logit_bias={-1: 1.0}), dict(logit_bias={V: 1.0}), dict(banned_tokens=[V]), dict(allowed_tokens=[2, -5]), dict(stop_tokens=[V + 3], min_tokens=1),
           dict(logit_bias={1: float("nan")}), dict(logit_bias={1: float("inf")}), dict(logit_bias={1: float("-inf")}), dict(logit_bias=[(1, 1.0), (2, 0.5), (1, 2.0)]),
           dict(logit_bias={1.5: 1.0}), dict(allowed_tokens=[5, 6], banned_tokens=[6, 5]), dict(allowed_tokens=[5, 6], stop_tokens=[5, 6], min_tokens=1),
           dict(min_tokens=-1), dict(min_tokens=1.5), dict(min_tokens=5, max_new_tokens=4)]
    for kw in bad:
        with pytest.raises(ValueError):
            rq(vocab=V, **kw)
    with pytest.raises(ValueError):
        rq(banned_tokens=[0, 1, 2], vocab=3)
    assert rq(allowed_tokens=[5, 6], stop_tokens=[5, 6], min_tokens=0, vocab=V) is not None
    for fn in (host.GemmaModel.generate, host.GemmaModel.generate_batch):
        sig = inspect.signature(fn).parameters
        assert sig["logit_bias"].default is None and sig["banned_tokens"].default == () and sig["allowed_tokens"].default == () and sig["min_tokens"].default == 0
    assert hasattr(host.Gemma, "set_token_bias") and hasattr(host.Gemma, "token_bias")
    build.build()
    h = host.load()
    for n in ("set_token_bias", "read_token_bias", "model_generate_biased", "model_generate_spec_biased", "model_generate_rows_biased", "model_vocab_size"):
        assert hasattr(h, "mila_gemma_" + n), n


def test_the_request_to_table_composition(tmp_path):
    """tests/cpp/token_bias_compose.cpp against Mila/TokenBias.h alone (no HIP include): each control alone and all four together, the ban-over-allow rule, the
    restore list and index, every invalid_argument"""
    cxx = shutil.which("g++") or build.HOSTCXX
    exe = tmp_path / "token_bias_compose"
    subprocess.check_call([cxx, "-std=c++20", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "mila_amd", "host", "include"),
                           os.path.join(ROOT, "tests", "cpp", "token_bias_compose.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "token bias compose OK" in r.stdout, r.stdout
    text = open(os.path.join(ROOT, "mila_amd", "host", "include", "Mila", "TokenBias.h")).read()
    assert "#include <hip" not in text and "#include \"" not in text, "TokenBias.h is host only and stands alone"
