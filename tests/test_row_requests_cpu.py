"""CPU-only checks of row requests (include/mila_cdna4.h: row requests; Mila/GemmaModel.h: generateRequests): the layout of the device records on both sides of the
binding, the exported entries and their refusals before any device work, the host binding's surface, and tests/cpp/row_requests_compose.cpp -- the per-row request
checks, bias plans and restore indices -- compiled with the host flags and run."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sample_row_params_bytes", "sample_row_params_set", "sample_radix_requests_rows_fp32", "sample_radix_requests_rows_advance_fp32",
           "sample_argmax_requests_rows_fp32", "sample_argmax_requests_rows_advance_fp32", "token_automaton_rows_bytes", "token_automaton_rows_set",
           "token_automaton_rows_compose", "token_automaton_rows_step")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_records_have_the_layout_the_header_states(lib):
    f = capi.sample_row_params
    assert C.sizeof(f) == 32 and [(n, getattr(f, n).offset) for n, _ in f._fields_] == [
        ("temperature", 0), ("top_k", 4), ("top_p", 8), ("min_p", 12), ("repetition_penalty", 16), ("inv_rep", 20), ("presence_penalty", 24), ("frequency_penalty", 28)]
    a = capi.token_automaton_row
    assert C.sizeof(a) == 24 and [getattr(a, n).offset for n, _ in a._fields_] == [0, 8, 16, 20]
    assert [capi.sample_row_params_bytes(r) for r in (0, 1, 4, 5)] == [0, 32, 128, 0]
    assert [capi.token_automaton_rows_bytes(r) for r in (0, 1, 4, 5)] == [0, 24, 96, 0]


def test_the_entries_are_exported_and_the_abi_version_stays(lib):
    for n in ENTRIES:
        assert n in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + n), n
    assert lib.mila_cdna4_abi_version() == 4


def test_the_setters_and_entries_refuse_bad_arguments_without_touching_the_device(lib):
    """every pointer here is a small integer that is never dereferenced: validation fails first"""
    null, one = C.c_void_p(None), C.c_void_p(64)
    z, f = C.c_size_t, C.c_float
    E = capi.MILA_E_INVALID_ARGUMENT

    def rec(**kw):
        base = dict(temperature=1.0, top_k=5, top_p=0.9, min_p=0.0, repetition_penalty=1.0, inv_rep=0.0, presence_penalty=0.0, frequency_penalty=0.0)
        base.update(kw)
        return C.byref(capi.sample_row_params(**base))

    st = lib.mila_cdna4_sample_row_params_set
    for bad in (dict(temperature=float("nan")), dict(temperature=float("-inf")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=float("nan")), dict(repetition_penalty=0.0),
                dict(min_p=1.0), dict(min_p=float("nan")), dict(presence_penalty=float("inf")), dict(frequency_penalty=float("nan"))):
        assert st(one, 0, rec(**bad), null) == E, bad
    assert b"min_p" in (st(one, 0, rec(min_p=1.0), null), lib.mila_cdna4_last_error())[1]
    assert st(one, -1, rec(), null) == E and st(one, 4, rec(), null) == E and st(null, 0, rec(), null) == E and st(one, 0, null, null) == E
    assert st(C.c_void_p(66), 0, rec(), null) == E      # misaligned

    V = 1003
    radix = lib.mila_cdna4_sample_radix_requests_rows_fp32
    need = capi.sample_radix_rows_scratch_bytes(4, V)

    def r(rows=4, vocab=V, stride=V, params=one, draws=one, scratch=one, nbytes=need, table_stride=V, bias_stride=0, bias=null):
        return radix(one, z(stride), one, rows, vocab, f(30.0), params, draws, one, z(table_stride), bias, z(bias_stride), scratch, z(nbytes), null)

    assert r(rows=0) == E and r(rows=5) == E and r(vocab=0) == E and r(stride=V - 1) == E and r(params=null) == E and r(draws=null) == E
    assert r(table_stride=V - 1) == E and r(bias=one, bias_stride=V - 1) == E and r(scratch=C.c_void_p(68)) == E
    assert r(nbytes=need - 1) == capi.MILA_E_SCRATCH_TOO_SMALL and r(scratch=null) == capi.MILA_E_SCRATCH_TOO_SMALL
    adv = lib.mila_cdna4_sample_radix_requests_rows_advance_fp32
    assert adv(one, z(V), one, 4, V, f(30.0), one, one, one, z(V), null, z(0), one, z(need), null, one, null) == E      # positions_dev missing
    assert adv(one, z(V), one, 4, V, f(30.0), one, one, one, z(V), null, z(0), one, z(need), one, null, null) == E      # active_dev missing

    argmax = lib.mila_cdna4_sample_argmax_requests_rows_fp32
    aneed = 4 * lib.mila_cdna4_sample_scratch_bytes()

    def a(rows=4, vocab=V, stride=V, params=one, scratch=one, nbytes=aneed):
        return argmax(one, z(stride), one, rows, vocab, f(30.0), params, one, z(V), null, z(0), scratch, z(nbytes), null)

    assert a(rows=0) == E and a(rows=5) == E and a(vocab=-1) == E and a(stride=1) == E and a(params=null) == E and a(scratch=C.c_void_p(66)) == E
    assert a(nbytes=aneed - 1) == capi.MILA_E_SCRATCH_TOO_SMALL

    aset = lib.mila_cdna4_token_automaton_rows_set
    assert aset(one, 4, one, one, 2, 2, V, null) == E and aset(null, 0, one, one, 2, 2, V, null) == E and aset(one, 0, one, null, 2, 2, V, null) == E
    assert aset(one, 0, one, one, 0, 2, V, null) == E and aset(one, 0, one, one, 2, 70000, V, null) == E and aset(C.c_void_p(68), 0, one, one, 2, 2, V, null) == E
    step = lib.mila_cdna4_token_automaton_rows_step
    assert step(one, z(V), null, z(0), null, one, one, null, one, 4, V, null) == E and step(one, z(V), null, z(0), one, one, null, null, one, 4, V, null) == E
    assert step(one, z(V), null, z(0), one, one, one, null, one, 5, V, null) == E and step(one, z(V - 1), null, z(0), one, one, one, null, one, 4, V, null) == E
    assert lib.mila_cdna4_token_automaton_rows_compose(one, z(V), one, z(5), one, one, 4, V, null) == E      # a base_stride from 1 to vocab - 1


def test_the_host_binding_carries_the_requests_entries():
    from mila_amd import host
    h = host.load()
    for n in ("mila_gemma_set_rows_requests", "mila_gemma_set_row_token_bias", "mila_gemma_set_row_token_automaton", "mila_gemma_row_token_automaton_state",
              "mila_gemma_model_generate_requests", "mila_gemma_model_rows_graph_info"):
        assert hasattr(h, n), n
    assert [n for n, _ in host.GemmaConfigC._fields_][-2:] == ["bounded_local_kv", "kv_fp8"]      # mila_gemma_config is unchanged
    assert list(inspect.signature(host.GemmaModel.generate_requests).parameters) == ["self", "requests", "logprobs"]
    assert inspect.signature(host.GemmaModel.generate_requests).parameters["logprobs"].default is None
    assert C.sizeof(host.GemmaRowRequestC) == 96
    assert {"prompt", "seed", "automaton", "min_tokens", "logit_bias", "temperature"} <= set(host.ROW_REQUEST_KEYS)
    # generate_batch keeps its signature and its refusal
    assert "automaton" in inspect.signature(host.GemmaModel.generate_batch).parameters


def test_the_per_row_request_checks_and_bias_plans(tmp_path, lib):
    """tests/cpp/row_requests_compose.cpp, compiled with the host flags and RUN (host code only, no device call)"""
    src = os.path.join(ROOT, "tests", "cpp", "row_requests_compose.cpp")
    exe = str(tmp_path / "row_requests_compose")
    libdir = os.path.dirname(capi.LIB_PATH)
    flags = [f for f in build.HOST_FLAGS if f not in ("-fPIC", "-fvisibility=hidden")]
    p = subprocess.run([build.HOSTCXX] + flags + [src, "-o", exe, "-L" + libdir, "-lmila_cdna4", "-L/opt/rocm/lib", "-lamdhip64", "-lrocprofiler-sdk-roctx",
                                                  "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "row requests compose OK" in r.stdout, r.stdout
