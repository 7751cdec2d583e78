"""GPU: the sampling filters through the Gemma host mirror -- GemmaTransformer (host.Gemma: eager samplers, captured steps, token table, memory) and GemmaModel
(generate / generate_batch keywords, decode-ahead, prefix reuse, speculative models).  The kernels themselves are held to their oracles in
tests/test_sample_filtered_gpu.py; here the question is whether every layer routes to them with the right table at the right time."""
import numpy as np
import pytest

import ref_sampling_filters as R
from mila_amd import capi, host
from test_gemma_host_gpu import SMALL, TOKENS

pytestmark = pytest.mark.gpu

MAX_SEQ = 32
SEED = 11
SOFTCAP = 30.0          # GemmaConfig::final_logit_softcapping of the synthetic models
V = SMALL["vocab_size"]
PROMPT, FIRST = TOKENS[:7], TOKENS[7]          # the prompt is prefilled, FIRST is fed at position 7; both are "in the prompt" for the table
SETTINGS = [dict(temperature=0.9, top_k=12, top_p=0.9, min_p=0.05, repetition_penalty=1.3), dict(temperature=1.2, top_k=0, top_p=0.95, presence_penalty=0.6, frequency_penalty=0.4)]
PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)


def _model(policy="bf16", kv_fp8=False, **kw):
    return host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, kv_fp8=kv_fp8, **kw)


def _start(g):
    """a new request: the prompt into the caches and into the token table"""
    g.prefill(PROMPT)
    g.set_token_table(0, PROMPT + [FIRST])


def _table(prompt, generated):
    w = np.zeros(V, dtype=np.uint32)
    w[np.asarray(prompt)] = R.FLAG
    for t in generated:
        w[t] += np.uint32(1)
    return w


def _draws(seed, n):
    """std::mt19937(seed) + uniform_real_distribution<float>(0, 1), libstdc++ arithmetic: the draws of generate_sampled"""
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed))
    u = bg.random_raw(n).astype(np.uint32).astype(np.float32) / np.float32(4294967296.0)
    return np.minimum(u, np.nextafter(np.float32(1), np.float32(0)))


def _filters(kw):
    return host._filters(**{k: v for k, v in kw.items() if k not in ("temperature", "top_k", "top_p")})


# ---- 9. graph against eager
@pytest.mark.parametrize("policy,kv_fp8", [("bf16", False), ("fp4", False), ("bf16", True)])
def test_the_captured_step_with_filters_equals_the_fused_step_and_the_eager_sampler(policy, kv_fp8):
    g = _model(policy, kv_fp8)
    try:
        for kw in SETTINGS:
            out = {}
            for mode in ("fused", "graph"):
                _start(g)
                out[mode] = g.generate_sampled(FIRST, 7, 12, seed=5, mode=mode, pipeline="radix", **kw).tolist()
                if _filters(kw)[1:] != R.NEUTRAL[1:]:
                    assert np.array_equal(g.token_table(), _table(PROMPT + [FIRST], out[mode])), "the table is not prompt flags + counts of the sampled tokens"
            assert out["graph"] == out["fused"], (kw, out)
        out = {}
        for mode in ("fused", "graph"):
            _start(g)
            out[mode] = g.generate(FIRST, 7, 12, mode, **PENALTIES).tolist()
            assert np.array_equal(g.token_table(), _table(PROMPT + [FIRST], out[mode]))
        assert out["graph"] == out["fused"], out
        _start(g)
        assert g.generate(FIRST, 7, 12, "graph").tolist() != out["graph"], "the penalties changed nothing: the case shows nothing"
    finally:
        g.close()


# ---- 10. eager against the oracle
def test_the_eager_filtered_sampler_matches_the_oracle_on_the_models_logits():
    """twelve fused steps with the logits read back: each token is the NumPy oracle's on those logits, with the table implied by the prompt mark and the tokens so far,
    wherever the draw is decisive"""
    g = _model()
    try:
        # (SETTINGS[1]'s untruncated nucleus at temperature 1.2 spreads the mass over hundreds of tokens of ~1e-3 each: no draw is decisive by the 2e-3 bracket rule,
        # whatever the sampler -- 0 of 12 measured; its penalties are held to the oracle under a top-k of 8 instead)
        for kw, seed in zip([SETTINGS[0], dict(temperature=0.8, top_k=8, top_p=0.95, presence_penalty=0.6, frequency_penalty=0.4)], (5, 9)):
            _start(g)
            toks = g.generate_sampled(FIRST, 7, 12, seed=seed, mode="fused", pipeline="radix", **kw).tolist()
            draws = _draws(seed, 12)
            g.prefill(PROMPT)
            decisive, fed, generated = 0, FIRST, []
            for i in range(12):
                logits = g.decode(fed, 7 + i, "fused")
                d = R.Distribution(logits, SOFTCAP, kw["temperature"], kw["top_k"], kw["top_p"], _filters(kw), _table(PROMPT + [FIRST], generated).view(np.int32))
                tok, m = d.draw(draws[i])
                if d.decisive(m) and d.m_minp > 1e-4:
                    assert toks[i] == tok, "step %d: %d != oracle %d (margins %s)" % (i, toks[i], tok, m)
                    decisive += 1
                generated.append(toks[i])
                fed = toks[i]
            print("%s seed %d: %d of 12 steps decisive" % (kw, seed, decisive))
            assert decisive >= 8
    finally:
        g.close()


# ---- 11. a sharp property
def test_a_huge_presence_penalty_forbids_every_repeat():
    m = host.GemmaModel.synthetic("bf16", SMALL, context=MAX_SEQ, prefill_chunk=16, seed=SEED)
    try:
        req = dict(max_new_tokens=24, stop_tokens=[V - 1])
        plain = m.generate(TOKENS[:5], **req)[0]
        pen = m.generate(TOKENS[:5], presence_penalty=1000.0, **req)[0]          # far beyond the +-30 of the capped logits
        assert len(plain) == 24 and len(pen) == 24, "a stop token was reached"
        assert len(set(plain)) < 24, "the unpenalized request repeats nothing: choose another prompt"
        assert len(set(pen)) == 24, "a token was repeated under presence_penalty = 1000: %s" % pen
    finally:
        m.close()


# ---- 12. decode-ahead against the step-level eager loop
ORACLE_SETTINGS = [SETTINGS[0], dict(temperature=0.8, top_k=8, top_p=0.95, presence_penalty=0.6, frequency_penalty=0.4)]


def _step_level_check(g, prompt, toks, kw, seed):
    """the tokens `toks` that GemmaModel.generate gave for `prompt` against the step-level loop on the twin transformer `g`: the logits of the fused path read back,
    the NumPy oracle on them with the table implied by the WHOLE prompt's marks and the tokens so far, at the draws of std::mt19937_64(seed) -- one per sample, in
    order.  Returns the number of decisive steps (each of which was asserted)."""
    rng = R.Mt19937_64(seed)
    logits = g.prefill(prompt)
    decisive, generated = 0, []
    for i, got in enumerate(toks):
        r = rng.uniform()
        d = R.Distribution(logits, SOFTCAP, kw["temperature"], kw["top_k"], kw["top_p"], _filters(kw), _table(prompt, generated).view(np.int32))
        tok, m = d.draw(r)
        if d.decisive(m) and d.m_minp > 1e-4:
            assert got == tok, "step %d: generate() gave %d, the oracle %d (margins %s)" % (i, got, tok, m)
            decisive += 1
        generated.append(got)
        if i + 1 < len(toks):
            logits = g.decode(got, len(prompt) + i, "fused")
    return decisive


def test_generate_with_filters_gives_the_tokens_of_the_step_level_eager_loop():
    """GemmaModel.generate (prefill, eager first sample, then the captured step decoding ahead of the host) with filters, stochastic, seed fixed.  The prompt repeats
    tokens and is longer than one prefill chunk, and the second identical request reuses the prefix: a table that missed the prompt, or took only the chunks that
    were uploaded, would show under repetition_penalty."""
    m = host.GemmaModel.synthetic("bf16", SMALL, context=MAX_SEQ, prefill_chunk=8, seed=SEED)
    g = _model()
    prompt = TOKENS[:11] + TOKENS[2:5]                       # 14 tokens: two chunks of 8; three ids twice
    try:
        for kw, seed in zip(ORACLE_SETTINGS, (40, 41)):
            req = dict(max_new_tokens=12, stop_tokens=[V - 1], seed=seed, **kw)
            first = m.generate(prompt, **req)
            assert len(first[0]) == 12, "a stop token was reached: %s" % (first,)
            n = _step_level_check(g, prompt, first[0], kw, seed)
            print("%s seed %d: %d of 12 steps decisive" % (kw, seed, n))
            assert n >= 8
            again = m.generate(prompt, **req)
            assert again[2] > 0 and again[:2] == first[:2], "the request that reuses the prefix: %s / %s" % (first, again)
        # greedy with penalties: argmax of the adjusted logits of the same step-level loop, wherever the two largest are further apart than tanhf's ulps
        kw = dict(temperature=1.0, top_k=1, **PENALTIES)
        toks = m.generate(prompt, max_new_tokens=12, stop_tokens=[V - 1], **kw)[0]
        assert len(toks) == 12
        logits, generated, clear = g.prefill(prompt), [], 0
        for i, got in enumerate(toks):
            x3 = R.adjusted_logits(logits, _table(prompt, generated).view(np.int32), SOFTCAP, *_filters(kw)[1:])
            top2 = np.sort(x3)[-2:]
            if top2[1] - top2[0] > 1e-3:
                assert got == int(np.argmax(x3)), (i, got, int(np.argmax(x3)))
                clear += 1
            generated.append(got)
            logits = g.decode(got, len(prompt) + i, "fused")
        assert clear >= 8
        assert toks != m.generate(prompt, max_new_tokens=12, stop_tokens=[V - 1])[0], "the penalties changed nothing: the case shows nothing"
    finally:
        m.close()
        g.close()


# ---- 12 / 13. reproducibility, prefix reuse, batch
def test_generate_with_filters_is_reproducible_reuses_the_prefix_and_equals_the_batch_rows():
    kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED)
    alone, batch = host.GemmaModel.synthetic("bf16", SMALL, **kw), host.GemmaModel.synthetic("bf16", SMALL, max_batch=4, **kw)
    prompts = [TOKENS[:9], TOKENS[3:8], TOKENS[5:15]]
    try:
        for s in SETTINGS + [dict(temperature=1.0, top_k=1, **PENALTIES)]:
            req = dict(max_new_tokens=10, stop_tokens=[V - 1], **s)
            first = alone.generate(prompts[0], seed=40, **req)
            again = alone.generate(prompts[0], seed=40, **req)
            assert again[:2] == first[:2] and again[2] > 0, "the second request reuses the prefix and must rebuild the table for it: %s / %s" % (first, again)
            unfiltered = alone.generate(prompts[0], seed=40, max_new_tokens=10, stop_tokens=[V - 1], temperature=s["temperature"], top_k=s["top_k"], top_p=s.get("top_p", 1.0))
            assert unfiltered[0] != first[0], "the filters changed nothing: the case shows nothing"
            rows = batch.generate_batch(prompts, seed=40, **req)
            for b, p in enumerate(prompts):
                assert tuple(rows[b]) == tuple(alone.generate(p, seed=40 + b, **req)[:2]), (s, b)
        # a filter-off batch after the filtered ones is what it always was
        assert [tuple(r) for r in batch.generate_batch(prompts[:2], max_new_tokens=6, stop_tokens=[V - 1])] == \
               [tuple(alone.generate(p, max_new_tokens=6, stop_tokens=[V - 1])[:2]) for p in prompts[:2]]
        with pytest.raises(ValueError):
            alone.generate(prompts[0], repetition_penalty=0.0)
        with pytest.raises(ValueError):
            batch.generate_batch(prompts, min_p=1.0)
    finally:
        alone.close()
        batch.close()


# ---- 14. speculative models
def test_a_filtered_request_on_a_draft_model_takes_the_plain_loop():
    kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED)
    plain, spec = host.GemmaModel.synthetic("bf16", SMALL, **kw), host.GemmaModel.synthetic("bf16", SMALL, draft_tokens=3, **kw)
    try:
        for req in (dict(temperature=1.0, top_k=1, **PENALTIES), dict(speculative_sampling=True, **SETTINGS[0])):
            req = dict(max_new_tokens=12, stop_tokens=[V - 1], seed=3, **req)
            want = plain.generate(TOKENS[:6], **{k: v for k, v in req.items() if k != "speculative_sampling"})
            assert spec.generate(TOKENS[:6], **req)[:2] == want[:2]
            st = spec.speculation_stats()
            assert st["chain_steps"] == 0, st
        ref = plain.generate(TOKENS[:6], max_new_tokens=12, stop_tokens=[V - 1])
        assert spec.generate(TOKENS[:6], max_new_tokens=12, stop_tokens=[V - 1], draft_hint=ref[0])[:2] == ref[:2]
        assert spec.speculation_stats()["chain_steps"] > 0, "an unfiltered request must still speculate"
    finally:
        plain.close()
        spec.close()


# ---- 15. log-probabilities with filters
@pytest.mark.parametrize("mode", ["fused", "graph"])
def test_log_probabilities_stay_those_of_the_unpenalized_logits(mode):
    g, plain = _model(), _model()
    try:
        _start(g)
        plain.prefill(PROMPT)
        g.set_sampling_filters(**PENALTIES)
        fed, moved = FIRST, 0
        for i in range(6):
            logits, tok, lp, _, _ = g.decode(fed, 7 + i, mode, logprobs=0)
            ref_logits, ref_tok = plain.decode(fed, 7 + i, mode, logprobs=0)[:2]
            assert np.array_equal(logits.view(np.uint32), ref_logits.view(np.uint32)), "the sampler touched the logits"
            z = R.capped(logits, SOFTCAP).astype(np.float64)
            want = z - z.max() - np.log(np.exp(z - z.max()).sum())
            assert abs(float(lp) - want[tok]) <= 1e-4, (i, tok, lp, want[tok])
            moved += tok != ref_tok
            fed = tok
        assert moved > 0, "the penalties moved no token: the case shows nothing"
    finally:
        g.close()
        plain.close()


# ---- 16. captures and memory
def test_node_counts_captures_and_memory():
    g, fresh = _model(), _model()
    try:
        mem = lambda m: {k: v for k, v in m.memory_stats().items() if k != "scratch_bytes"}
        base = mem(fresh)
        assert mem(g) == base
        g.decode(5, 0, "graph")
        samplerless = g.graph_node_count()
        # filter-off calls with and without the keywords: the same tokens, the same graphs, nothing allocated
        a = g.generate(5, 0, 6, "graph").tolist()
        greedy_nodes, c0 = g.graph_node_count(), g.graph_capture_count()
        assert g.generate(5, 0, 6, "graph", repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0).tolist() == a
        assert (g.graph_node_count(), g.graph_capture_count()) == (greedy_nodes, c0)
        st = dict(temperature=0.9, top_k=12, top_p=0.9, seed=5, mode="graph", pipeline="radix")
        b = g.generate_sampled(5, 0, 6, **st).tolist()
        stochastic_nodes, c1 = g.graph_node_count(), g.graph_capture_count()
        assert stochastic_nodes == samplerless - 1 + capi.sample_radix_plan(V, 12, 0.9)["launches"]
        assert g.generate_sampled(5, 0, 6, min_p=0.0, repetition_penalty=1.0, **st).tolist() == b
        assert (g.graph_node_count(), g.graph_capture_count()) == (stochastic_nodes, c1)
        assert mem(g) == base, "a model that never saw a filter allocated something"
        # a stochastic capture with filters has the node count it has without them; a change captures once, the same values capture none
        g.set_token_table(0, [5])
        g.generate_sampled(5, 0, 6, min_p=0.05, **PENALTIES, **st)
        assert (g.graph_node_count(), g.graph_capture_count()) == (stochastic_nodes, c1 + 1)
        g.set_token_table(0, [5])
        g.generate_sampled(5, 0, 6, min_p=0.05, **PENALTIES, **st)
        assert g.graph_capture_count() == c1 + 1
        g.generate_sampled(5, 0, 6, min_p=0.1, **PENALTIES, **st)
        assert (g.graph_node_count(), g.graph_capture_count()) == (stochastic_nodes, c1 + 2)
        # a greedy capture with penalties: the sampler-less capture's nodes, minus the position bump, plus the two launches of the penalized sampler
        g.set_token_table(0, [5])
        g.generate(5, 0, 6, "graph", **PENALTIES)
        assert g.graph_node_count() == samplerless - 1 + 2
        c2 = g.graph_capture_count()
        g.generate(5, 0, 6, "graph", **PENALTIES)
        assert g.graph_capture_count() == c2
        g.generate(5, 0, 6, "graph", repetition_penalty=1.1)
        assert g.graph_capture_count() == c2 + 1
        assert g.generate(5, 0, 6, "graph").tolist() == a and g.graph_node_count() == greedy_nodes
        # min_p does not enter a greedy step: setting it alone re-captures nothing and moves no token
        c3 = g.graph_capture_count()
        g.set_sampling_filters(min_p=0.3)
        assert g.generate(5, 0, 6, "graph").tolist() == a and g.graph_capture_count() == c3
        g.set_sampling_filters()
        ms = mem(g)
        assert ms["required"] == ms["actual"] and ms["actual"]["device_state_bytes"] == base["actual"]["device_state_bytes"] + 4 * (V + 1024)
        with pytest.raises(ValueError):
            g.set_sampling_filters(repetition_penalty=-1.0)
        with pytest.raises(ValueError):
            g.generate_sampled(5, 0, 2, min_p=0.1, pipeline="search")
        # a draft-token model's rows are positions of one sequence: one table, not draft_tokens + 1
        d = _model(draft_tokens=3)
        try:
            before = mem(d)
            d.set_token_table(0, [5])
            after = mem(d)
            assert after["required"] == after["actual"] and after["actual"]["device_state_bytes"] == before["actual"]["device_state_bytes"] + 4 * (V + 1024)
        finally:
            d.close()
    finally:
        g.close()
        fresh.close()
