"""CPU-only: constrained speculative decode at the drop-in boundary and on the host.  The four chain entries (include/mila_cdna4.h: the constrained chain step) are
declared, exported, bound and refuse bad arguments before any device work; TokenAutomaton::forcedTokens is the brute-force answer on random small automata, in the C++
header (tests/cpp/token_automaton_forced.cpp, with bans, an allow-list and a held stop token) and through host.TokenAutomaton.forced_tokens; the Python surface carries
the flag."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from mila_amd import build, capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("token_automaton_chain_compose", "token_automaton_chain_step", "sample_radix_biased_chain_accept_fp32", "sample_argmax_biased_chain_accept_fp32")
INVALID = -1      # MILA_E_INVALID_ARGUMENT
FORBIDDEN = 0xFFFF


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_entries_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    declared = set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", text))
    for n in ENTRIES:
        assert "mila_cdna4_" + n in declared and n in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + n), n
        assert getattr(lib, "mila_cdna4_" + n).argtypes, n
    assert lib.mila_cdna4_abi_version() == 4, "additive: the ABI stays 4"
    for n in ("token_automaton_chain_compose", "token_automaton_chain_step", "sample_radix_biased_chain_accept", "sample_argmax_biased_chain_accept"):
        assert callable(getattr(capi, n)), n


def test_the_automaton_chain_entries_refuse_bad_arguments_before_any_device_work(lib):
    """no GPU here: a call that reached the device would fail with another status (or crash); every one of these returns INVALID_ARGUMENT"""
    p = C.c_void_p(0x1000)      # never dereferenced on the host
    good = dict(eff=p, es=16, base=None, bs=0, cls=p, nxt=p, S=3, C=2, state=p, tok=p, states=p, result=p, T=3, ticket=p, vocab=16)

    def compose(**kw):
        a = dict(good, **kw)
        return lib.mila_cdna4_token_automaton_chain_compose(a["eff"], a["es"], a["base"], a["bs"], a["cls"], a["nxt"], a["S"], a["C"], a["state"], a["tok"], a["states"], a["T"],
                                                            a["vocab"], None)

    def step(**kw):
        a = dict(good, **kw)
        return lib.mila_cdna4_token_automaton_chain_step(a["eff"], a["es"], a["base"], a["bs"], a["cls"], a["nxt"], a["S"], a["C"], a["state"], a["tok"], a["states"], a["result"],
                                                         a["T"], a["ticket"], a["vocab"], None)

    bad = [dict(eff=None), dict(cls=None), dict(nxt=None), dict(state=None), dict(tok=None), dict(states=None), dict(T=1), dict(T=5), dict(T=0), dict(vocab=0), dict(vocab=-3),
           dict(S=0), dict(S=65536), dict(C=0), dict(C=65536), dict(S=65535, C=2049), dict(es=15), dict(es=0), dict(base=p, bs=15)]
    for kw in bad:
        assert compose(**kw) == INVALID, ("chain_compose", kw)
        assert step(**kw) == INVALID, ("chain_step", kw)
    for kw in (dict(result=None), dict(ticket=None)):
        assert step(**kw) == INVALID, ("chain_step", kw)
    assert b"token_automaton_chain" in lib.mila_cdna4_last_error()


def test_the_biased_chain_tails_refuse_bad_arguments_before_any_device_work(lib):
    p = C.c_void_p(0x1000)
    V = 4097
    good = dict(tok=p, result=p, logits=p, ls=V, T=3, vocab=V, temp=0.8, k=0, top_p=1.0, draws=p, bias=p, bs=V, scratch=p, nb=1 << 30, pos=p)

    def radix(**kw):
        a = dict(good, **kw)
        return lib.mila_cdna4_sample_radix_biased_chain_accept_fp32(a["tok"], a["result"], a["logits"], a["ls"], a["T"], a["vocab"], 30.0, a["temp"], a["k"], a["top_p"], a["draws"],
                                                                    a["bias"], a["bs"], a["scratch"], a["nb"], a["pos"], None)

    def greedy(**kw):
        a = dict(good, **kw)
        return lib.mila_cdna4_sample_argmax_biased_chain_accept_fp32(a["tok"], a["result"], a["logits"], a["ls"], a["T"], a["vocab"], 30.0, a["bias"], a["bs"], a["scratch"], a["nb"],
                                                                     a["pos"], None)

    both = [dict(tok=None), dict(result=None), dict(logits=None), dict(pos=None), dict(T=1), dict(T=5), dict(vocab=0), dict(ls=V - 1), dict(bs=1), dict(bs=V - 1),
            dict(bias=C.c_void_p(0x1002))]
    for kw in both:
        assert radix(**kw) == INVALID, ("radix", kw)
        assert greedy(**kw) == INVALID, ("greedy", kw)
    for kw in (dict(draws=None), dict(temp=0.0), dict(k=-1), dict(top_p=0.0), dict(scratch=C.c_void_p(0x1004))):
        assert radix(**kw) == INVALID, ("radix", kw)
    assert greedy(bias=None) == INVALID, "the greedy chain from the logits needs a table: without one its partials come from the lm_head"
    for f in (radix, greedy):      # a short scratch has a status of its own
        assert f(nb=64) not in (0, INVALID) and f(scratch=None) not in (0, INVALID)
    assert radix(bias=None, nb=64) not in (0, INVALID), "bias == NULL is the unbiased entry: refused for the same reasons"
    assert radix(bias=None, T=1) == INVALID


def _brute_force(a, banned=()):
    dense = a.dense()
    out = np.full(a.num_states, -1, dtype=np.int32)
    ok = np.ones(a.vocab, dtype=bool)
    ok[list(banned)] = False
    for s in range(a.num_states):
        ids = np.flatnonzero((dense[s] != FORBIDDEN) & ok)
        if ids.size == 1:
            out[s] = ids[0]
    return out


def test_forced_tokens_is_the_brute_force_answer_with_and_without_bans(lib):
    rng = np.random.default_rng(11)
    forced_only_by_a_ban = 0
    for _ in range(60):
        V, S = int(rng.integers(1, 41)), int(rng.integers(1, 7))
        dense = rng.integers(0, S, size=(S, V)).astype(np.uint16)
        dense[rng.random((S, V)) < 0.8] = FORBIDDEN
        a = host.TokenAutomaton.from_dense(dense, start=0)
        plain = a.forced_tokens()
        assert plain.dtype == np.int32 and np.array_equal(plain, _brute_force(a))
        banned = [int(t) for t in np.flatnonzero(rng.random(V) < 0.3)][:V - 1]
        with_bans = a.forced_tokens(banned=banned)
        assert np.array_equal(with_bans, _brute_force(a, banned)), (dense, banned)
        forced_only_by_a_ban += int(((plain < 0) & (with_bans >= 0)).sum())
    assert forced_only_by_a_ban > 0, "the cases include states that are forced only because of a ban"
    # the one case by hand: state 1 allows tokens 6 and 7
    a = host.TokenAutomaton(np.array([0, 0, 0, 0, 0, 0, 1, 1]), np.array([[0, 1], [FORBIDDEN, 2], [2, FORBIDDEN]]))
    assert a.forced_tokens().tolist() == [-1, -1, -1] and a.forced_tokens(banned=[6]).tolist() == [-1, 7, -1]
    with pytest.raises(ValueError):
        a.forced_tokens(banned=[8])


def test_the_header_computes_forced_tokens_and_the_surface_exists(lib, tmp_path):
    """tests/cpp/token_automaton_forced.cpp, compiled with the host flags and RUN (host code only, no device call)"""
    src = os.path.join(ROOT, "tests", "cpp", "token_automaton_forced.cpp")
    exe = str(tmp_path / "token_automaton_forced")
    libdir = os.path.dirname(capi.LIB_PATH)
    flags = [f for f in build.HOST_FLAGS if f not in ("-fPIC", "-fvisibility=hidden")]
    p = subprocess.run([build.HOSTCXX] + flags + [src, "-o", exe, "-L" + libdir, "-lmila_cdna4", "-L/opt/rocm/lib", "-lamdhip64", "-lrocprofiler-sdk-roctx",
                                                  "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "token automaton forced OK" in r.stdout, r.stdout


def test_the_host_binding_carries_the_flag():
    sig = inspect.signature(host.GemmaModel.generate)
    assert sig.parameters["speculate_constrained"].default is False
    assert hasattr(host.GemmaModel, "speculation_stats_forced") and hasattr(host.TokenAutomaton, "forced_tokens")
    assert "speculate_constrained" not in inspect.signature(host.GemmaModel.generate_batch).parameters      # out of scope: automata in generate_batch
