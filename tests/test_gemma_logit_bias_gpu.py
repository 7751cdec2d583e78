"""GPU: logit bias, banned / allowed tokens and min_tokens through the Gemma host mirror -- GemmaTransformer (host.Gemma: eager samplers, captured steps, memory) and
GemmaModel (generate / generate_batch keywords, the decode-ahead loop's restore, speculative models).  The kernels are held to their oracles in
tests/test_sample_biased_gpu.py; here the question is whether every layer routes to them with the right table at the right time.  Every expectation is sharp: the
softcap bounds the capped logit by 30, so a bias of +100 forces a token and -inf forbids one."""
import numpy as np
import pytest

import ref_sampling_filters as R
from mila_amd import capi, host
from test_gemma_host_gpu import SMALL, TOKENS

pytestmark = pytest.mark.gpu

MAX_SEQ = 32
SEED = 11
SOFTCAP = 30.0
V = SMALL["vocab_size"]
PROMPT, FIRST = TOKENS[:7], TOKENS[7]
NEG_INF = float("-inf")
A, S = 321, 654                                   # a forced token and a stop token
NEVER = [V - 1]                                   # a stop set nobody reaches: V - 1 is banned wherever this is used with a bias, and checked where it is not


def _model(policy="bf16", kv_fp8=False, **kw):
    return host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, kv_fp8=kv_fp8, **kw)


def _gemma_model(**kw):
    return host.GemmaModel.synthetic("bf16", SMALL, context=MAX_SEQ, prefill_chunk=16, seed=SEED, **kw)


# ---- host.Gemma: graph against eager
@pytest.mark.parametrize("policy,kv_fp8", [("bf16", False), ("fp4", False), ("bf16", True)])
def test_the_captured_step_with_a_bias_equals_the_fused_step(policy, kv_fp8):
    g = _model(policy, kv_fp8)
    st = dict(temperature=0.9, top_k=12, top_p=0.9, seed=5, pipeline="radix")
    try:
        def both(fn):
            out = {}
            for mode in ("fused", "graph"):
                g.prefill(PROMPT)
                out[mode] = fn(mode)
            assert out["fused"] == out["graph"], out
            return out["graph"]
        plain_greedy = both(lambda mode: g.generate(FIRST, 7, 12, mode).tolist())
        plain_radix = both(lambda mode: g.generate_sampled(FIRST, 7, 12, mode=mode, **st).tolist())
        banned = sorted(set(plain_greedy[1:]) | set(plain_radix[1:]))
        g.set_token_bias({t: NEG_INF for t in banned} | {A: 4.0})
        table, on = g.token_bias()
        assert on and np.isneginf(table[banned]).all() and table[A] == 4.0 and np.count_nonzero(table) == len(banned) + 1
        greedy = both(lambda mode: g.generate(FIRST, 7, 12, mode).tolist())
        radix = both(lambda mode: g.generate_sampled(FIRST, 7, 12, mode=mode, **st).tolist())
        assert greedy != plain_greedy and radix != plain_radix, "the bias changed nothing: the case shows nothing"
        assert not set(greedy) & set(banned) and not set(radix) & set(banned), "a banned token was sampled"
        # an update of the table that is on: A forced from now on, in both modes
        g.set_token_bias({A: 100.0}, update=True)
        assert both(lambda mode: g.generate(FIRST, 7, 6, mode).tolist()) == [A] * 6
        assert both(lambda mode: g.generate_sampled(FIRST, 7, 6, mode=mode, **st).tolist()) == [A] * 6
        assert np.isneginf(g.token_bias()[0][banned]).all(), "an update leaves the other entries"
        # off again: the plain tokens
        g.set_token_bias(None)
        assert not g.token_bias()[1]
        assert both(lambda mode: g.generate(FIRST, 7, 12, mode).tolist()) == plain_greedy
        assert both(lambda mode: g.generate_sampled(FIRST, 7, 12, mode=mode, **st).tolist()) == plain_radix
        with pytest.raises(ValueError):
            g.set_token_bias({V: 1.0})
        with pytest.raises(ValueError):
            g.set_token_bias({1: float("nan")})
        with pytest.raises(ValueError):
            g.set_token_bias({1: 1.0}, fill=float("inf"))
    finally:
        g.close()


def test_the_eager_biased_greedy_sampler_is_the_argmax_of_the_biased_capped_logits():
    """twelve fused steps with the logits read back: each greedy token is argmax(capped logits + bias) wherever the two largest are further apart than tanhf's ulps"""
    g = _model()
    try:
        rng = np.random.default_rng(3)
        ids = rng.choice(V, size=200, replace=False)
        bias = np.zeros(V, dtype=np.float32)
        bias[ids] = (rng.standard_normal(200) * 6.0).astype(np.float32)
        bias[ids[:40]] = -np.inf
        g.set_token_bias({int(i): float(bias[i]) for i in ids})
        g.prefill(PROMPT)
        toks = g.generate(FIRST, 7, 12, "fused").tolist()
        g.prefill(PROMPT)
        fed, clear = FIRST, 0
        for i in range(12):
            logits = g.decode(fed, 7 + i, "fused")
            xb = R.capped(logits, SOFTCAP) + bias
            top2 = np.sort(xb)[-2:]
            if top2[1] - top2[0] > 1e-3:
                assert toks[i] == int(np.argmax(xb)), (i, toks[i], int(np.argmax(xb)))
                clear += 1
            fed = toks[i]
        assert clear >= 8
    finally:
        g.close()


# ---- GemmaModel.generate
def test_generate_forces_bans_and_allows():
    m = _gemma_model()
    prompt = TOKENS[:6]
    try:
        req = dict(max_new_tokens=12, stop_tokens=NEVER)
        T = m.generate(prompt, **req)[0]
        assert len(T) == 12
        assert m.generate(prompt, logit_bias={A: 100.0}, **req)[0] == [A] * 12
        out = m.generate(prompt, banned_tokens=[T[3]], **req)[0]
        assert T[3] not in T[:3], "choose another prompt: the banned token occurs before index 3"
        assert out[:3] == T[:3] and out[3] != T[3] and T[3] not in out
        # a closed answer set under a hot, untruncated distribution
        allowed = [9, 333, 512, 700, 1001]
        kw = dict(max_new_tokens=24, stop_tokens=NEVER, temperature=1.5, top_k=0, top_p=1.0, allowed_tokens=allowed)
        first = m.generate(prompt, seed=21, **kw)
        assert len(first[0]) == 24 and set(first[0]) <= set(allowed), first
        assert len(set(first[0])) > 1, "one token only: the case does not show sampling"
        assert m.generate(prompt, seed=21, **kw)[:2] == first[:2], "the same seed twice"
        assert m.generate(prompt, seed=22, **kw)[0] != first[0]
        # an allowed token with a bias and a ban inside the list
        out = m.generate(prompt, seed=21, **dict(kw, logit_bias={333: 100.0}))[0]
        assert out == [333] * 24
        out = m.generate(prompt, seed=21, **dict(kw, banned_tokens=[333, 9]))[0]
        assert set(out) <= {512, 700, 1001}
        # after biased requests a plain request gives the plain tokens
        assert m.generate(prompt, **req)[0] == T
        for bad in (dict(logit_bias={V: 1.0}), dict(banned_tokens=[-1]), dict(logit_bias={1: float("inf")}), dict(allowed_tokens=[4], banned_tokens=[4]), dict(min_tokens=-1),
                    dict(min_tokens=13)):
            with pytest.raises(ValueError):
                m.generate(prompt, **dict(req, **bad))
        assert m.generate(prompt, **req)[0] == T
    finally:
        m.close()


def test_min_tokens_holds_the_stop_token_back_for_exactly_that_many_samples():
    m = _gemma_model()
    prompt = TOKENS[:6]
    try:
        want = m.generate(prompt, max_new_tokens=12, stop_tokens=NEVER, banned_tokens=[S])[0]
        assert len(want) == 12 and S not in want
        for n in (1, 2, 6, 11):
            out = m.generate(prompt, max_new_tokens=12, stop_tokens=[S], logit_bias={S: 100.0}, min_tokens=n)
            assert out[:2] == (want[:n], "stop"), "min_tokens=%d: %s, want the first %d of %s" % (n, out, n, want)
        out = m.generate(prompt, max_new_tokens=12, stop_tokens=[S], logit_bias={S: 100.0}, min_tokens=12)
        assert out[:2] == (want, "length")
        assert m.generate(prompt, max_new_tokens=12, stop_tokens=[S], logit_bias={S: 100.0}, min_tokens=0)[:2] == ([], "stop")
        # stochastic: the same restore in the captured stochastic step
        kw = dict(max_new_tokens=12, temperature=1.2, top_k=0, top_p=1.0, seed=8)
        free = m.generate(prompt, stop_tokens=NEVER, banned_tokens=[S], **kw)[0]
        assert len(free) == 12
        out = m.generate(prompt, stop_tokens=[S], logit_bias={S: 100.0}, min_tokens=6, **kw)
        assert out[:2] == (free[:6], "stop"), (out, free)
    finally:
        m.close()


@pytest.mark.parametrize("n_prompts", [2, 4])
def test_generate_batch_rows_equal_their_own_generate(n_prompts):
    alone, batch = _gemma_model(), _gemma_model(max_batch=4)
    prompts = [TOKENS[:9], TOKENS[3:8], TOKENS[5:15], TOKENS[1:7]][:n_prompts]
    try:
        plain = [alone.generate(p, max_new_tokens=10, stop_tokens=NEVER)[0] for p in prompts]
        banned = sorted({t for row in plain for t in row[2:5]})
        bias = dict(logit_bias={A: 3.0, 17: -2.0}, banned_tokens=banned)
        req = dict(max_new_tokens=10, stop_tokens=NEVER, **bias)
        rows = batch.generate_batch(prompts, **req)
        for b, p in enumerate(prompts):
            assert tuple(rows[b]) == tuple(alone.generate(p, **req)[:2]), b
            assert not set(rows[b][0]) & set(banned)
        assert [r[0] for r in rows] != plain
        # min_tokens, every row: the stop token is forced, and comes exactly at sample index 6
        held = [alone.generate(p, max_new_tokens=12, stop_tokens=NEVER, banned_tokens=[S])[0] for p in prompts]
        rows = batch.generate_batch(prompts, max_new_tokens=12, stop_tokens=[S], logit_bias={S: 100.0}, min_tokens=6)
        for b in range(n_prompts):
            assert tuple(rows[b]) == (held[b][:6], "stop"), (b, rows[b], held[b])
        assert [tuple(r) for r in batch.generate_batch(prompts, max_new_tokens=12, stop_tokens=[S], logit_bias={S: 100.0})] == [([], "stop")] * n_prompts
        # stochastic rows under an allow-list
        allowed = [9, 333, 512, 700, 1001]
        rows = batch.generate_batch(prompts, max_new_tokens=12, stop_tokens=NEVER, temperature=1.5, top_k=0, top_p=1.0, seed=30, allowed_tokens=allowed)
        for b, p in enumerate(prompts):
            assert set(rows[b][0]) <= set(allowed) and len(rows[b][0]) == 12
            assert tuple(rows[b]) == tuple(alone.generate(p, max_new_tokens=12, stop_tokens=NEVER, temperature=1.5, top_k=0, top_p=1.0, seed=30 + b, allowed_tokens=allowed)[:2])
        # a bias-off batch afterwards is what it always was
        assert [r[0] for r in batch.generate_batch(prompts, max_new_tokens=10, stop_tokens=NEVER)] == plain
        with pytest.raises(ValueError):
            batch.generate_batch(prompts, logit_bias={V: 1.0})
    finally:
        alone.close()
        batch.close()


def test_a_biased_request_on_a_draft_model_takes_the_plain_loop():
    plain, spec = _gemma_model(), _gemma_model(draft_tokens=3)
    try:
        ref = plain.generate(TOKENS[:6], max_new_tokens=12, stop_tokens=NEVER)
        for bias in (dict(banned_tokens=[ref[0][3]]), dict(logit_bias={A: 2.0}), dict(allowed_tokens=[9, 333, 512]), dict(min_tokens=4)):
            for req in (dict(temperature=1.0, top_k=1), dict(temperature=0.9, top_k=12, top_p=0.9, speculative_sampling=True)):
                req = dict(max_new_tokens=12, stop_tokens=NEVER, seed=3, **req, **bias)
                want = plain.generate(TOKENS[:6], **{k: v for k, v in req.items() if k != "speculative_sampling"})
                assert spec.generate(TOKENS[:6], draft_hint=ref[0], **req)[:2] == want[:2], req
                assert spec.speculation_stats()["chain_steps"] == 0, req
        assert spec.generate(TOKENS[:6], max_new_tokens=12, stop_tokens=NEVER, draft_hint=ref[0])[:2] == ref[:2]
        assert spec.speculation_stats()["chain_steps"] > 0, "an unbiased request must still speculate"
    finally:
        plain.close()
        spec.close()


def test_log_probabilities_stay_those_of_the_unbiased_logits():
    m = _gemma_model()
    prompt = TOKENS[:6]
    try:
        plain = m.generate(prompt, max_new_tokens=6, stop_tokens=NEVER, logprobs=3)
        banned = m.generate(prompt, max_new_tokens=6, stop_tokens=NEVER, logprobs=3, banned_tokens=[plain[0][0]])
        assert banned[0][0] != plain[0][0]
        (lp0, ids0, tlp0), (lp1, ids1, tlp1) = plain[3][0], banned[3][0]
        assert np.array_equal(ids0, ids1) and np.array_equal(tlp0.view(np.uint32), tlp1.view(np.uint32)), "the ban changed the reported distribution"
        assert ids0[0] == plain[0][0] and abs(float(lp0) - float(tlp0[0])) <= 1e-6 and lp1 < tlp1[0], "the banned request reports its own token under the same distribution"
    finally:
        m.close()


# ---- captures and memory
def test_node_counts_captures_and_memory():
    g, fresh = _model(), _model()
    try:
        mem = lambda m: {k: v for k, v in m.memory_stats().items() if k != "scratch_bytes"}
        base = mem(fresh)
        g.decode(5, 0, "graph")
        samplerless = g.graph_node_count()
        a = g.generate(5, 0, 6, "graph").tolist()
        greedy_nodes = g.graph_node_count()
        st = dict(temperature=0.9, top_k=12, top_p=0.9, seed=5, mode="graph", pipeline="radix")
        b = g.generate_sampled(5, 0, 6, **st).tolist()
        stochastic_nodes, c1 = g.graph_node_count(), g.graph_capture_count()
        assert stochastic_nodes == samplerless - 1 + capi.sample_radix_plan(V, 12, 0.9)["launches"]
        assert mem(g) == base, "a model that never saw a bias allocated something"
        # bias on: the stochastic step keeps its node count (the biased instantiations of the same launches), one capture; the contents never capture
        g.set_token_bias({int(t): NEG_INF for t in set(b)})
        ms = mem(g)
        assert ms["required"] == ms["actual"] and ms["actual"]["device_state_bytes"] == base["actual"]["device_state_bytes"] + 4 * (V + 4 * 1024)
        bb = g.generate_sampled(5, 0, 6, **st).tolist()
        assert not set(bb) & set(b)
        assert (g.graph_node_count(), g.graph_capture_count()) == (stochastic_nodes, c1 + 1)
        g.set_token_bias({A: 100.0})
        assert g.generate_sampled(5, 0, 6, **st).tolist() == [A] * 6 and g.graph_capture_count() == c1 + 1
        with pytest.raises(ValueError):
            g.generate_sampled(5, 0, 2, temperature=0.9, top_k=12, top_p=0.9, seed=5, mode="fused", pipeline="search")      # the search pipeline takes no bias
        # a greedy capture with a bias: the sampler-less capture's nodes, minus the position bump, plus the two launches of the penalized greedy sampler
        assert g.generate(5, 0, 6, "graph").tolist() == [A] * 6
        assert g.graph_node_count() == samplerless - 1 + 2
        c2 = g.graph_capture_count()
        g.set_token_bias({A: NEG_INF, 7: 100.0})
        assert g.generate(5, 0, 6, "graph").tolist() == [7] * 6 and g.graph_capture_count() == c2
        # bias off: today's graphs, today's tokens, one capture each
        g.set_token_bias(None)
        assert g.generate(5, 0, 6, "graph").tolist() == a and g.graph_node_count() == greedy_nodes and g.graph_capture_count() == c2 + 1
        assert g.generate_sampled(5, 0, 6, **st).tolist() == b and g.graph_node_count() == stochastic_nodes
        assert mem(g) == ms, "the table stays allocated and counted"
    finally:
        g.close()
        fresh.close()
