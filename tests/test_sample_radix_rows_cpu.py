"""The radix sampler over rows and speculative sampling, the part that needs no GPU: the entries at the drop-in boundary (declared, listed, exported), their
argument checks -- which answer before any device work -- the rows scratch size, and the host-only draw bookkeeping of the speculative loop."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sample_radix_rows_scratch_bytes", "sample_radix_rows_fp32", "sample_radix_rows_advance_fp32", "sample_radix_chain_accept_fp32")
INV, SMALL = capi.MILA_E_INVALID_ARGUMENT, capi.MILA_E_SCRATCH_TOO_SMALL
V = 1000


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_entries_are_declared_listed_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    declared = set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", text))
    for n in ENTRIES:
        assert "mila_cdna4_" + n in declared and n in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + n), n
        assert ("_" + n) in open(os.path.join(ROOT, "INTEGRATION.md")).read(), n
    assert lib.mila_cdna4_abi_version() == 4      # additive


@pytest.mark.parametrize("vocab", [1, 65, 1000, 50257, 262144, 300001])
def test_the_rows_scratch_is_rows_times_the_aligned_one_row_need(lib, vocab):
    one = capi.sample_radix_scratch_bytes(vocab)
    aligned = (one + 7) & ~7
    assert aligned - one in (0, 4)
    for rows in (1, 2, 3, 4):
        assert capi.sample_radix_rows_scratch_bytes(rows, vocab) == rows * aligned == lib.mila_cdna4_sample_radix_rows_scratch_bytes(rows, vocab)
    for rows, v in ((0, vocab), (5, vocab), (-1, vocab), (2, 0), (2, -7)):
        assert lib.mila_cdna4_sample_radix_rows_scratch_bytes(rows, v) == 0


def _rows_calls(lib):
    """each entry as a function of keyword overrides; every pointer is a small integer that no check dereferences"""
    null, one = C.c_void_p(None), C.c_void_p(16)

    def rows_fp32(logits=one, stride=V, tok=one, rows=4, vocab=V, t=0.8, k=64, p=0.95, draws=one, scratch=one, bytes_=None):
        nb = C.c_size_t(capi.sample_radix_rows_scratch_bytes(4, V) if bytes_ is None else bytes_)
        return lib.mila_cdna4_sample_radix_rows_fp32(logits, C.c_size_t(stride), tok, rows, vocab, 30.0, t, k, p, draws, scratch, nb, null)

    def rows_advance(logits=one, stride=V, tok=one, rows=4, vocab=V, t=0.8, k=64, p=0.95, draws=one, scratch=one, bytes_=None, pos=one, active=one):
        nb = C.c_size_t(capi.sample_radix_rows_scratch_bytes(4, V) if bytes_ is None else bytes_)
        return lib.mila_cdna4_sample_radix_rows_advance_fp32(logits, C.c_size_t(stride), tok, rows, vocab, 30.0, t, k, p, draws, scratch, nb, pos, active, null)

    def chain(logits=one, stride=V, tok=one, rows=4, vocab=V, t=0.8, k=64, p=0.95, draws=one, scratch=one, bytes_=None, pos=one, result=one):
        nb = C.c_size_t(capi.sample_radix_rows_scratch_bytes(4, V) if bytes_ is None else bytes_)
        return lib.mila_cdna4_sample_radix_chain_accept_fp32(tok, result, logits, C.c_size_t(stride), rows, vocab, 30.0, t, k, p, draws, scratch, nb, pos, null)

    return {"sample_radix_rows_fp32": rows_fp32, "sample_radix_rows_advance_fp32": rows_advance, "sample_radix_chain_accept_fp32": chain}


@pytest.mark.parametrize("name", ENTRIES[1:])
def test_argument_checks_answer_before_any_launch(lib, name):
    """a call that got as far as a launch would fault on these pointers, and a process without a device would fail in the runtime instead of answering
    INVALID_ARGUMENT / SCRATCH_TOO_SMALL with the entry's name"""
    null = C.c_void_p(None)
    err = lib.mila_cdna4_last_error
    fn = _rows_calls(lib)[name]
    pointers = ["logits", "tok", "draws"] + {"sample_radix_rows_fp32": [], "sample_radix_rows_advance_fp32": ["pos", "active"], "sample_radix_chain_accept_fp32": ["pos", "result"]}[name]
    for kw in pointers:
        assert fn(**{kw: null}) == INV and (name + ": null pointer").encode() in err(), kw
    if name == "sample_radix_chain_accept_fp32":
        for T in (1, 5, 0, -2):
            assert fn(rows=T) == INV and b"outside 2 .. 4" in err(), T
    else:
        for rows in (0, 5, -1):
            assert fn(rows=rows) == INV and b"outside 1 .. 4" in err(), rows
    assert fn(vocab=0) == INV and b"vocab" in err()
    assert fn(t=0.0) == INV and b"temperature" in err()
    assert fn(t=-1.0) == INV and b"temperature" in err()
    assert fn(k=-1) == INV and b"top_k >= 0" in err()
    assert fn(p=0.0) == INV and b"top_p > 0" in err()
    assert fn(p=-0.5) == INV and b"top_p > 0" in err()
    assert fn(stride=V - 1) == INV and b"logits_stride" in err()
    assert fn(scratch=null) == SMALL and b"scratch" in err() and name.encode() in err()
    need = capi.sample_radix_rows_scratch_bytes(4, V)
    assert fn(bytes_=need - 1) == SMALL and b"required %d" % need in err()
    assert fn(bytes_=capi.sample_radix_rows_scratch_bytes(3, V)) == SMALL      # sized for one row fewer
    assert fn(rows=3, bytes_=capi.sample_radix_rows_scratch_bytes(3, V), scratch=C.c_void_p(20)) == INV and b"aligned" in err()


def test_a_rows_call_launches_what_one_row_launches(lib):
    """the plan is the one-row plan: nothing in the C ABI multiplies launches by rows (the rows ride in the grid); the rows entries share plan_radix with
    sample_radix_plan_describe, whose launch count the graph tests compare node counts against"""
    for k, p, want in ((64, 0.95, 9), (0, 0.95, 6), (64, 1.0, 7), (0, 1.0, 4)):
        assert capi.sample_radix_plan(262144, k, p)["launches"] == want


def test_the_draw_bookkeeping_of_the_speculative_loop(tmp_path):
    """tests/cpp/spec_sampling_draws.cpp, compiled with the host flags and RUN (host code only, no device call): peekDraws( T ) then consumeDraws( n ) leaves the
    generator where n plain draws leave it, n = 1 .. T, T = 2 .. 4; GenerateParams{}.speculative_sampling is false"""
    build.build()
    src = os.path.join(ROOT, "tests", "cpp", "spec_sampling_draws.cpp")
    exe = str(tmp_path / "spec_sampling_draws")
    libdir = os.path.dirname(capi.LIB_PATH)
    flags = [f for f in build.HOST_FLAGS if f not in ("-fPIC", "-fvisibility=hidden")]
    p = subprocess.run([build.HOSTCXX] + flags + [src, "-o", exe, "-L" + libdir, "-lmila_cdna4", "-L/opt/rocm/lib", "-lamdhip64", "-lrocprofiler-sdk-roctx",
                                                  "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "spec sampling draws OK" in r.stdout, r.stdout


def test_the_host_binding_carries_the_sampled_steps(lib):
    import inspect

    from mila_amd import host
    names = [n for n, _ in host.GemmaConfigC._fields_]
    assert names[-2:] == ["bounded_local_kv", "kv_fp8"]      # mila_gemma_config is unchanged
    h = host.load()
    for n in ("decode_rows_sampled", "chain_decode_sampled", "model_generate_spec_sampling"):
        assert hasattr(h, "mila_gemma_" + n), n
    assert inspect.signature(host.GemmaModel.generate).parameters["speculative_sampling"].default is False
    for fn in (host.Gemma.decode_rows, host.Gemma.decode_chain):
        sig = inspect.signature(fn).parameters
        assert sig["sampling"].default is None and sig["draws"].default is None
