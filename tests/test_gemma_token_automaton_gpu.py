"""GPU: grammar-constrained decoding through the Gemma host mirror -- GemmaTransformer (host.Gemma: eager samplers, the captured step's extra node, captures, memory)
and GemmaModel (generate(automaton=...), the decode-ahead loop, speculative models, refusals).  The kernel is held to its restatement in
tests/test_token_automaton_gpu.py; here the question is whether every layer routes to it with the right table at the right time.  The oracles are the existing
bias path (a one-state automaton is a bias table), host-tracked states, and a logits readback."""
import numpy as np
import pytest

import ref_sampling_filters as R
import ref_token_automaton as A
from mila_amd import capi, host
from test_gemma_host_gpu import SMALL, TOKENS

pytestmark = pytest.mark.gpu

MAX_SEQ = 32
SEED = 11
SOFTCAP = 30.0
V = SMALL["vocab_size"]
PROMPT, FIRST = TOKENS[:7], TOKENS[7]
NEG_INF = float("-inf")
S_TOK = 654                                       # a stop token
NEVER = [V - 1]
ST = dict(temperature=0.9, top_k=12, top_p=0.9, seed=5, pipeline="radix")
F = A.FORBIDDEN


def _model(policy="bf16", **kw):
    return host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, **kw)


def _gemma_model(**kw):
    return host.GemmaModel.synthetic("bf16", SMALL, context=MAX_SEQ, prefill_chunk=16, seed=SEED, **kw)


def _mod3():
    """state k allows the ids = k (mod 3) and goes to k + 1 (mod 3)"""
    nxt = np.full((3, 3), F, dtype=np.uint16)
    for k in range(3):
        nxt[k, k] = (k + 1) % 3
    return host.TokenAutomaton((np.arange(V) % 3).astype(np.uint16), nxt)


def _set_automaton(allowed, states=1):
    """`states` states in a cycle, every one allowing exactly the ids in `allowed`"""
    class_of = np.zeros(V, dtype=np.uint16)
    class_of[list(allowed)] = 1
    nxt = np.array([[F, (k + 1) % states] for k in range(states)], dtype=np.uint16)
    return host.TokenAutomaton(class_of, nxt)


def _both(g, fn, before=None):
    """fn(mode) behind a fresh prefill (and `before()`), fused and graph: the same tokens"""
    out = {}
    for mode in ("fused", "graph"):
        g.prefill(PROMPT)
        if before:
            before()
        out[mode] = fn(mode)
    assert out["fused"] == out["graph"], out
    return out["graph"]


# ---- host.Gemma
@pytest.mark.parametrize("policy", ["bf16", "fp4"])
def test_fused_and_graph_agree_and_every_token_is_allowed_in_its_state(policy):
    g = _model(policy)
    a = _mod3()
    try:
        plain_greedy = _both(g, lambda mode: g.generate(FIRST, 7, 12, mode).tolist())
        plain_radix = _both(g, lambda mode: g.generate_sampled(FIRST, 7, 12, mode=mode, **ST).tolist())
        g.set_token_automaton(a)
        for n in (12, 7):
            states = []
            greedy = _both(g, lambda mode: (g.generate(FIRST, 7, n, mode).tolist(), states.append(g.token_automaton_state()))[0], g.reset_token_automaton)
            radix = _both(g, lambda mode: (g.generate_sampled(FIRST, 7, n, mode=mode, **ST).tolist(), states.append(g.token_automaton_state()))[0], g.reset_token_automaton)
            for toks in (greedy, radix):
                s = a.start
                for i, t in enumerate(toks):
                    assert a.allowed(s)[t], "token %d (%d) is not allowed in state %d: %s" % (i, t, s, toks)
                    s = a.step(s, t)
                assert s == n % 3
            assert states == [n % 3] * 4, states
        assert greedy != plain_greedy[:7] or radix != plain_radix[:7], "the automaton changed nothing: the case shows nothing"
        # off again: the plain tokens
        g.set_token_automaton(None)
        assert _both(g, lambda mode: g.generate(FIRST, 7, 12, mode).tolist()) == plain_greedy
        assert _both(g, lambda mode: g.generate_sampled(FIRST, 7, 12, mode=mode, **ST).tolist()) == plain_radix
    finally:
        g.close()


def test_a_one_state_automaton_is_the_bias_table_and_a_cycle_with_one_mask_too():
    g = _model()
    rng = np.random.default_rng(2)
    allowed = sorted(rng.choice(V - 1, size=60, replace=False).tolist())
    try:
        g.set_token_bias({int(t): 0.0 for t in allowed}, fill=NEG_INF)
        want_greedy = _both(g, lambda mode: g.generate(FIRST, 7, 11, mode).tolist())
        want_radix = _both(g, lambda mode: g.generate_sampled(FIRST, 7, 11, mode=mode, **ST).tolist())
        g.set_token_bias(None)
        assert set(want_greedy) | set(want_radix) <= set(allowed) and len(set(want_radix)) > 1
        for states in (1, 3):
            g.set_token_automaton(_set_automaton(allowed, states))
            assert _both(g, lambda mode: g.generate(FIRST, 7, 11, mode).tolist(), g.reset_token_automaton) == want_greedy, states
            assert g.token_automaton_state() == 11 % states
            assert _both(g, lambda mode: g.generate_sampled(FIRST, 7, 11, mode=mode, **ST).tolist(), g.reset_token_automaton) == want_radix, states
            assert g.token_automaton_state() == 11 % states
        # over a bias table: the effective table follows its base when the base is updated while the automaton is on
        g.set_token_bias({allowed[0]: 100.0})
        assert _both(g, lambda mode: g.generate(FIRST, 7, 5, mode).tolist(), g.reset_token_automaton) == [allowed[0]] * 5
        g.set_token_bias({allowed[1]: 100.0, allowed[0]: NEG_INF}, update=True)
        state, eff = g.token_automaton_state(table=True)
        assert eff[allowed[1]] == 100.0 and np.isneginf(eff[allowed[0]]) and np.isfinite(eff).sum() == len(allowed) - 1
        assert _both(g, lambda mode: g.generate(FIRST, 7, 5, mode).tolist(), g.reset_token_automaton) == [allowed[1]] * 5
        g.set_token_bias(None)
        assert np.isfinite(g.token_automaton_state(table=True)[1]).sum() == len(allowed)
    finally:
        g.close()


def test_the_constrained_greedy_token_is_the_argmax_of_the_masked_capped_logits():
    """twelve fused steps with the logits read back: each greedy token is argmax(capped logits + mask of the host-tracked state) wherever the two largest are further
    apart than tanhf's ulps -- the rule and the margin of the biased greedy sampler's test"""
    g = _model()
    a = _mod3()
    try:
        g.set_token_automaton(a)
        g.prefill(PROMPT)
        toks = g.generate(FIRST, 7, 12, "fused").tolist()
        g.set_token_automaton(None)      # the readback steps below run no sampler; nothing constrains them
        g.prefill(PROMPT)
        fed, clear, s = FIRST, 0, a.start
        for i in range(12):
            logits = g.decode(fed, 7 + i, "fused")
            xb = R.capped(logits, SOFTCAP) + A.mask(a.class_of, a.next, s)
            top2 = np.sort(xb)[-2:]
            if top2[1] - top2[0] > 1e-3:
                assert toks[i] == int(np.argmax(xb)), (i, toks[i], int(np.argmax(xb)))
                clear += 1
            s = a.step(s, toks[i])
            fed = toks[i]
        assert clear >= 8
    finally:
        g.close()


def test_node_counts_captures_and_memory():
    g, fresh = _model(), _model()
    try:
        mem = lambda m: {k: v for k, v in m.memory_stats().items() if k != "scratch_bytes"}
        base = mem(fresh)
        st = dict(ST, mode="graph")
        # a model that never saw an automaton: the parent's graphs
        fresh.decode(5, 0, "graph")
        samplerless = fresh.graph_node_count()
        fresh.generate(5, 0, 6, "graph")
        parent_greedy = fresh.graph_node_count()
        fresh.generate_sampled(5, 0, 6, **st)
        parent_stochastic = fresh.graph_node_count()
        assert mem(fresh) == base
        # off: the same counts on the model under test
        g.decode(5, 0, "graph")
        assert g.graph_node_count() == samplerless
        plain_greedy = g.generate(5, 0, 6, "graph").tolist()
        assert g.graph_node_count() == parent_greedy
        plain_radix = g.generate_sampled(5, 0, 6, **st).tolist()
        assert g.graph_node_count() == parent_stochastic and mem(g) == base, "a model that never saw an automaton allocated something"
        c0 = g.graph_capture_count()
        # on: exactly one node more than the step that reads a bias table -- the stochastic step keeps its launches, the greedy step ends at the logits and takes the
        # biased greedy sampler's two
        a = _mod3()
        g.set_token_automaton(a)
        ms = mem(g)
        image = (capi.token_automaton_bytes(V, a.num_states, a.num_classes) + 3) // 4 * 4
        assert ms["required"] == ms["actual"] and ms["actual"]["device_state_bytes"] == base["actual"]["device_state_bytes"] + 4 * V + 8 + image
        on_radix = g.generate_sampled(5, 0, 6, **st).tolist()
        assert (g.graph_node_count(), g.graph_capture_count()) == (parent_stochastic + 1, c0 + 1)
        # resetting, and replacing the automaton by another of the same size, never re-captures
        g.reset_token_automaton()
        assert g.generate_sampled(5, 0, 6, **st).tolist() == on_radix and g.graph_capture_count() == c0 + 1
        b = host.TokenAutomaton(a.class_of, np.roll(a.next, 1, axis=1))      # state k now allows the ids = k + 1 (mod 3)
        g.set_token_automaton(b)
        got = g.generate_sampled(5, 0, 6, **st).tolist()
        assert [t % 3 for t in got] == [(i + 1) % 3 for i in range(6)] and g.graph_capture_count() == c0 + 1
        assert mem(g) == ms
        g.set_token_automaton(a)
        on_greedy = g.generate(5, 0, 6, "graph").tolist()
        assert [t % 3 for t in on_greedy] == [i % 3 for i in range(6)]
        assert (g.graph_node_count(), g.graph_capture_count()) == (samplerless - 1 + 2 + 1, c0 + 2)
        # on -> off -> on: one capture per change
        g.set_token_automaton(None)
        assert g.generate(5, 0, 6, "graph").tolist() == plain_greedy and (g.graph_node_count(), g.graph_capture_count()) == (parent_greedy, c0 + 3)
        g.set_token_automaton(a)
        assert g.generate(5, 0, 6, "graph").tolist() == on_greedy and (g.graph_node_count(), g.graph_capture_count()) == (samplerless - 1 + 2 + 1, c0 + 4)
        g.set_token_automaton(None)
        assert g.generate_sampled(5, 0, 6, **st).tolist() == plain_radix and g.graph_node_count() == parent_stochastic
        assert mem(g) == ms, "the automaton stays allocated and counted"
        with pytest.raises(ValueError):
            g.set_token_automaton(host.TokenAutomaton(np.zeros(V + 1, dtype=np.uint16), np.zeros((1, 1), dtype=np.uint16)))      # another vocabulary
    finally:
        g.close()
        fresh.close()


# ---- GemmaModel.generate
def _exactly(n):
    """n states that allow everything but S_TOK, then a state that allows only S_TOK"""
    class_of = np.zeros(V, dtype=np.uint16)
    class_of[S_TOK] = 1
    nxt = np.array([[k + 1, F] for k in range(n)] + [[F, n]], dtype=np.uint16)
    return host.TokenAutomaton(class_of, nxt)


def test_exactly_n_tokens_then_stop():
    m = _gemma_model()
    prompt = TOKENS[:6]
    try:
        plain = m.generate(prompt, max_new_tokens=12, stop_tokens=NEVER)[0]
        for kw in (dict(), dict(temperature=1.2, top_k=0, top_p=1.0, seed=8)):
            want = m.generate(prompt, max_new_tokens=12, stop_tokens=[S_TOK], banned_tokens=[S_TOK], **kw)[0]
            assert len(want) == 12 and S_TOK not in want
            for n in (1, 2, 6, 11):
                out = m.generate(prompt, max_new_tokens=12, stop_tokens=[S_TOK], automaton=_exactly(n), **kw)
                assert out[:2] == (want[:n], "stop"), "n=%d %s: %s, want the first %d of %s" % (n, kw, out, n, want)
                assert out[-1] == n == m.last_automaton_state()
        # a plain request after constrained ones gives the plain tokens
        assert m.generate(prompt, max_new_tokens=12, stop_tokens=NEVER)[0] == plain
        assert m.last_automaton_state() is None
    finally:
        m.close()


def test_log_probabilities_stay_those_of_the_unconstrained_logits():
    m = _gemma_model()
    prompt = TOKENS[:6]
    try:
        plain = m.generate(prompt, max_new_tokens=6, stop_tokens=NEVER, logprobs=3)
        class_of = np.zeros(V, dtype=np.uint16)
        class_of[plain[0][0]] = 1
        a = host.TokenAutomaton(class_of, np.array([[0, F]], dtype=np.uint16))      # everything but the plain request's first token
        out = m.generate(prompt, max_new_tokens=6, stop_tokens=NEVER, logprobs=3, automaton=a)
        assert out[0][0] != plain[0][0] and plain[0][0] not in out[0] and out[-1] == 0
        (lp0, ids0, tlp0), (lp1, ids1, tlp1) = plain[3][0], out[3][0]
        assert np.array_equal(ids0, ids1) and np.array_equal(tlp0.view(np.uint32), tlp1.view(np.uint32)), "the automaton changed the reported distribution"
        assert ids0[0] == plain[0][0] and lp1 < tlp1[0], "the constrained request reports its own token under the same distribution"
    finally:
        m.close()


def test_a_constrained_request_on_a_draft_model_takes_the_plain_loop():
    plain, spec = _gemma_model(), _gemma_model(draft_tokens=2)
    try:
        ref = plain.generate(TOKENS[:6], max_new_tokens=12, stop_tokens=NEVER)
        a = _mod3()
        for req in (dict(temperature=1.0, top_k=1), dict(temperature=0.9, top_k=12, top_p=0.9, speculative_sampling=True)):
            req = dict(max_new_tokens=12, stop_tokens=NEVER, seed=3, automaton=a, **req)
            want = plain.generate(TOKENS[:6], **{k: v for k, v in req.items() if k != "speculative_sampling"})
            assert [t % 3 for t in want[0]] == [i % 3 for i in range(12)] and want[-1] == 0
            got = spec.generate(TOKENS[:6], draft_hint=ref[0], **req)
            assert got[:2] == want[:2] and got[-1] == want[-1], req
            assert spec.speculation_stats()["chain_steps"] == 0, req
        assert spec.generate(TOKENS[:6], max_new_tokens=12, stop_tokens=NEVER, draft_hint=ref[0])[:2] == ref[:2]
        assert spec.speculation_stats()["chain_steps"] > 0, "an unconstrained request must still speculate"
    finally:
        plain.close()
        spec.close()


def test_refusals_leave_the_model_as_it_was():
    m, batch = _gemma_model(), _gemma_model(max_batch=2)
    prompt = TOKENS[:6]
    try:
        req = dict(max_new_tokens=8, stop_tokens=NEVER)
        plain = m.generate(prompt, **req)[0]
        dead = host.TokenAutomaton(np.zeros(V, dtype=np.uint16), np.array([[1], [F]], dtype=np.uint16))      # state 1 allows nothing
        with pytest.raises(ValueError, match="state 1"):
            m.generate(prompt, automaton=dead, **req)
        assert m.generate(prompt, **req)[0] == plain
        # a dead end that exists only because of a ban: state 1 allows token 9 alone
        class_of = np.zeros(V, dtype=np.uint16)
        class_of[9] = 1
        narrow = host.TokenAutomaton(class_of, np.array([[1, F], [F, 0]], dtype=np.uint16))
        assert m.generate(prompt, automaton=narrow, **req)[0][1::2] == [9] * 4
        with pytest.raises(ValueError, match="state 1"):
            m.generate(prompt, automaton=narrow, banned_tokens=[9], **req)
        assert m.generate(prompt, **req)[0] == plain
        with pytest.raises(ValueError, match="min_tokens"):
            m.generate(prompt, automaton=narrow, min_tokens=2, **req)
        with pytest.raises(ValueError):
            m.generate(prompt, automaton=host.TokenAutomaton(np.zeros(V - 1, dtype=np.uint16), np.zeros((1, 1), dtype=np.uint16)), **req)      # another vocabulary
        assert m.generate(prompt, **req)[0] == plain
        with pytest.raises(ValueError, match="generateBatch"):
            batch.generate_batch([prompt, TOKENS[3:8]], automaton=narrow, **req)
        assert batch.generate_batch([prompt], **req)[0][0] == plain
    finally:
        m.close()
        batch.close()
