"""CPU-only: the token automaton at the drop-in boundary and on the host -- the three entries are declared, exported, bound and refuse bad arguments before any device
work; host.TokenAutomaton.from_transitions is the dense table it was built from; every validation error of Mila/TokenAutomaton.h is raised, in Python and (through
tests/cpp/token_automaton_traits.cpp) in the C++ header, dead ends and min_tokens included."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ref_token_automaton as A
from mila_amd import build, capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("token_automaton_bytes", "token_automaton_compose", "token_automaton_step")
INVALID = -1      # MILA_E_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_entries_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    declared = set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", text))
    for n in ENTRIES:
        assert "mila_cdna4_" + n in declared and n in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + n), n
    assert lib.mila_cdna4_abi_version() == 4, "additive: the ABI stays 4"


def test_the_image_size_and_its_limits(lib):
    assert capi.token_automaton_bytes(262144, 300, 7) == 2 * (262144 + 300 * 7)
    assert capi.token_automaton_bytes(1, 1, 1) == 4
    assert capi.token_automaton_bytes(10, 65535, 2048) == 2 * (10 + 65535 * 2048)      # 256 MiB - 4 KiB of transitions
    for bad in ((0, 1, 1), (-1, 1, 1), (10, 0, 1), (10, 1, 0), (10, 65536, 1), (10, 1, 65536), (10, 65535, 2049)):
        assert capi.token_automaton_bytes(*bad) == 0, bad


def test_the_entries_refuse_bad_arguments_before_any_device_work(lib):
    """no GPU here: a call that reached the device would fail with another status (or crash); every one of these returns INVALID_ARGUMENT"""
    p = C.c_void_p(0x1000)      # never dereferenced on the host
    good = dict(eff=p, es=16, base=None, bs=0, cls=p, nxt=p, S=3, C=2, state=p, tok=p, act=None, ticket=p, rows=1, vocab=16)

    def compose(**kw):
        a = dict(good, **kw)
        return lib.mila_cdna4_token_automaton_compose(a["eff"], a["es"], a["base"], a["bs"], a["cls"], a["nxt"], a["S"], a["C"], a["state"], a["rows"], a["vocab"], None)

    def step(**kw):
        a = dict(good, **kw)
        return lib.mila_cdna4_token_automaton_step(a["eff"], a["es"], a["base"], a["bs"], a["cls"], a["nxt"], a["S"], a["C"], a["state"], a["tok"], a["act"], a["ticket"],
                                                   a["rows"], a["vocab"], None)

    bad = [dict(eff=None), dict(cls=None), dict(nxt=None), dict(state=None), dict(rows=0), dict(rows=5), dict(vocab=0), dict(vocab=-3), dict(S=0), dict(S=65536), dict(C=0),
           dict(C=65536), dict(S=65535, C=2049), dict(rows=2, es=15), dict(base=p, bs=15)]
    for kw in bad:
        assert compose(**kw) == INVALID, ("compose", kw)
        assert step(**kw) == INVALID, ("step", kw)
    for kw in (dict(tok=None), dict(ticket=None)):
        assert step(**kw) == INVALID, ("step", kw)
    assert b"token_automaton" in lib.mila_cdna4_last_error()


def test_from_transitions_is_the_dense_table_it_was_built_from():
    rng = np.random.default_rng(7)
    V, S = 300, 7
    dense = rng.integers(0, S, size=(S, V)).astype(np.uint16)
    dense[rng.random((S, V)) < 0.4] = A.FORBIDDEN
    dense[:, 40:] = dense[:, rng.integers(0, 40, size=V - 40)]      # at most 40 distinct columns
    tr = {s: {t: int(dense[s, t]) for t in range(V) if dense[s, t] != A.FORBIDDEN} for s in range(S)}
    a = host.TokenAutomaton.from_transitions(V, S, tr, start=3)
    assert a.vocab == V and a.num_states == S and a.start == 3 and a.class_of.dtype == np.uint16 and a.next.dtype == np.uint16
    assert a.num_classes == len(np.unique(dense.T, axis=0)) <= 40
    assert np.array_equal(a.dense(), dense)
    assert a.class_of[0] == 0 and (np.diff(np.maximum.accumulate(a.class_of)) <= 1).all(), "classes are numbered in the order of their first token"
    for s in range(S):
        assert np.array_equal(a.allowed(s), dense[s] != A.FORBIDDEN)
        assert np.array_equal(A.mask(a.class_of, a.next, s), np.where(dense[s] != A.FORBIDDEN, np.float32(0), -np.inf).astype(np.float32))
        for t in (0, 17, 299):
            assert a.step(s, t) == A.step(a.class_of, a.next, s, t) == (s if dense[s, t] == A.FORBIDDEN else int(dense[s, t]))
    # identity classes: every column its own
    ident = host.TokenAutomaton.from_dense(np.arange(5, dtype=np.uint16)[None, :] % 1)      # one state, all columns equal -> one class
    assert ident.num_classes == 1


def test_the_python_constructor_raises_every_validation_error():
    cls, nxt = np.zeros(8, dtype=np.uint16), np.zeros((3, 2), dtype=np.uint16)
    host.TokenAutomaton(cls, nxt, start=2)
    for bad in (lambda: host.TokenAutomaton(cls, nxt, start=3), lambda: host.TokenAutomaton(cls, nxt, start=-1),
                lambda: host.TokenAutomaton(np.full(8, 2), nxt), lambda: host.TokenAutomaton(cls, np.full((3, 2), 3)),
                lambda: host.TokenAutomaton(cls, np.zeros((0, 2), dtype=np.uint16)), lambda: host.TokenAutomaton(cls, np.zeros((3, 0), dtype=np.uint16)),
                lambda: host.TokenAutomaton(cls, np.zeros((65536, 1), dtype=np.uint16)), lambda: host.TokenAutomaton(cls, np.zeros((1, 65536), dtype=np.uint16)),
                lambda: host.TokenAutomaton(cls, np.zeros((65535, 2049), dtype=np.uint16)), lambda: host.TokenAutomaton(cls, np.zeros(6, dtype=np.uint16)),
                lambda: host.TokenAutomaton.from_transitions(8, 2, {0: {8: 0}}), lambda: host.TokenAutomaton.from_transitions(8, 2, {0: {1: 2}}),
                lambda: host.TokenAutomaton.from_transitions(8, 2, {2: {1: 0}})):
        with pytest.raises(ValueError):
            bad()
    assert host.TokenAutomaton(cls, np.full((3, 2), A.FORBIDDEN)).allowed(0).sum() == 0      # FORBIDDEN is a legal entry; the dead-end check is generate()'s


def test_the_dead_end_restatement_agrees_with_itself_on_small_cases():
    """the restatement the GPU tests trust, on cases small enough to read"""
    F = A.FORBIDDEN
    cls = np.array([0, 0, 0, 0, 0, 0, 1, 1], dtype=np.uint16)
    nxt = np.array([[0, 1], [F, 2], [2, F]], dtype=np.uint16)
    assert A.dead_end(cls, nxt, 0) is None
    bias = np.zeros(8, dtype=np.float32)
    bias[[6, 7]] = -np.inf
    assert A.dead_end(cls, nxt, 0, bias) is None, "state 1 is unreachable once class 1 is banned"
    bias = np.zeros(8, dtype=np.float32)
    bias[:6] = -np.inf
    assert A.dead_end(cls, nxt, 0, bias) == 2


def test_the_header_validates_and_the_surface_exists(lib, tmp_path):
    """tests/cpp/token_automaton_traits.cpp, compiled with the host flags and RUN (host code only, no device call)"""
    src = os.path.join(ROOT, "tests", "cpp", "token_automaton_traits.cpp")
    exe = str(tmp_path / "token_automaton_traits")
    libdir = os.path.dirname(capi.LIB_PATH)
    flags = [f for f in build.HOST_FLAGS if f not in ("-fPIC", "-fvisibility=hidden")]
    p = subprocess.run([build.HOSTCXX] + flags + [src, "-o", exe, "-L" + libdir, "-lmila_cdna4", "-L/opt/rocm/lib", "-lamdhip64", "-lrocprofiler-sdk-roctx",
                                                  "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "token automaton traits OK" in r.stdout, r.stdout


def test_the_host_binding_carries_the_automaton():
    import inspect
    assert "automaton" in inspect.signature(host.GemmaModel.generate).parameters and "automaton" in inspect.signature(host.GemmaModel.generate_batch).parameters
    for n in ("set_token_automaton", "reset_token_automaton", "token_automaton_state"):
        assert hasattr(host.Gemma, n), n
    assert hasattr(host.GemmaModel, "last_automaton_state")
    names = [n for n, _ in host.GemmaConfigC._fields_]
    assert names[-2:] == ["bounded_local_kv", "kv_fp8"]      # mila_gemma_config is unchanged
