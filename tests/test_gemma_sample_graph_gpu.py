"""The stochastic sampler as the tail of the captured decode step (GemmaTransformer::setGraphSampling / setDrawRing, mila_cdna4_sample_radix_advance_fp32) and the
GemmaModel::generate loop that runs on it: a replayed step samples what the fused step followed by the eager radix sampler samples, from the same draws."""
import numpy as np
import pytest

from mila_amd import capi, host

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1024, embedding_dim=256, num_layers=6, num_heads=4, num_kv_heads=2, head_dim=64, hidden_dim=512,
             global_head_dim=128, num_global_kv_heads=1, window=8, sliding_window_pattern=6, global_rotary_dim=32)
PROMPT = [5, 17, 900, 3, 44, 260, 7, 7, 31, 512, 99, 2]
TRUNCATIONS = [(8, 0.95), (0, 0.9), (50, 1.0), (0, 1.0)]
N = 12


def _pair(policy, kv_fp8=False):
    return [host.Gemma(policy, SMALL, max_seq=32, max_prefill=1, seed=11, kv_fp8=kv_fp8) for _ in range(2)]


@pytest.mark.parametrize("policy,kv_fp8", [("bf16", False), ("fp4", False), ("bf16", True)])
def test_the_captured_stochastic_step_samples_what_the_fused_step_and_the_eager_radix_sampler_sample(policy, kv_fp8):
    fused, graph = _pair(policy, kv_fp8)
    try:
        for k, p in TRUNCATIONS if not kv_fp8 else TRUNCATIONS[:1]:
            kw = dict(temperature=0.9, top_k=k, top_p=p, seed=7 + k, pipeline="radix")
            want = fused.generate_sampled(5, 0, N, mode="fused", **kw)
            got = graph.generate_sampled(5, 0, N, mode="graph", **kw)
            assert np.array_equal(got, want), (k, p, got, want)
            assert all(0 <= t < 1024 for t in got)
        # a second request on the same capture, from another position and another seed
        kw = dict(temperature=0.9, top_k=8, top_p=0.95, seed=99, pipeline="radix")
        assert np.array_equal(graph.generate_sampled(9, 3, 6, mode="graph", **kw), fused.generate_sampled(9, 3, 6, mode="fused", **kw))
    finally:
        fused.close()
        graph.close()


def test_the_radix_pipeline_eagerly_is_seeded_and_stays_inside_the_top_k_set():
    g, ref = _pair("bf16")
    try:
        a = g.generate_sampled(5, 0, N, temperature=0.9, top_k=8, top_p=0.95, seed=7, mode="fused", pipeline="radix")
        b = g.generate_sampled(5, 0, N, temperature=0.9, top_k=8, top_p=0.95, seed=7, mode="reference", pipeline="radix")
        assert np.array_equal(a, b)
        tok = 5
        for i, t in enumerate(a):
            logits = ref.decode(tok, i, "reference")
            assert int(t) in set(np.argsort(-logits)[:8].tolist()), (i, t)
            tok = int(t)
        with pytest.raises(ValueError):
            g.generate_sampled(5, 0, 4, temperature=0.9, mode="graph", pipeline="search")      # the captured step ends with the radix pipeline only
        with pytest.raises(ValueError):
            g.generate_sampled(5, 0, 4, temperature=0.0, mode="graph", pipeline="radix")       # greedy in the graph: generate(mode="graph")
    finally:
        g.close()
        ref.close()


def test_node_count_re_capture_rule_and_memory_accounting():
    g = host.Gemma("bf16", SMALL, max_seq=32, max_prefill=1, seed=11)
    try:
        g.decode(5, 0, "graph")                                    # the sampler-less capture: the step, then advance_position
        bare, c0 = g.graph_node_count(), g.graph_capture_count()
        kw = dict(temperature=0.9, top_k=8, top_p=0.95, seed=7, mode="graph", pipeline="radix")
        first = g.generate_sampled(5, 0, 6, **kw)
        assert g.graph_node_count() == bare - 1 + capi.sample_radix_plan(1024, 8, 0.95)["launches"]      # the pipeline's last node replaces the position bump
        assert g.graph_capture_count() == c0 + 1
        assert np.array_equal(g.generate_sampled(5, 0, 6, **kw), first)
        assert g.graph_capture_count() == c0 + 1                    # the same parameters: the capture serves
        for change in (dict(temperature=0.8), dict(top_k=0), dict(top_p=1.0)):
            before = g.graph_capture_count()
            k2 = dict(kw, **change)
            g.generate_sampled(5, 0, 3, **k2)
            assert g.graph_capture_count() == before + 1, change
            assert g.graph_node_count() == bare - 1 + capi.sample_radix_plan(1024, k2["top_k"], k2["top_p"])["launches"]
            g.generate_sampled(5, 0, 3, **k2)
            assert g.graph_capture_count() == before + 1, change
            kw = k2
        st = g.memory_stats()
        assert st["required"] == st["actual"], st
        # the greedy capture keeps its nodes: argmax in the head's epilogue, one final launch in the place of the position bump
        greedy = g.generate(5, 0, 6, "graph")
        assert g.graph_node_count() == bare
        assert np.array_equal(greedy, g.generate(5, 0, 6, "fused"))
    finally:
        g.close()


@pytest.mark.parametrize("kv_fp8", [False, True])
def test_generate_runs_stochastic_requests_on_the_captured_sampler(kv_fp8):
    g = host.GemmaModel.synthetic("bf16", SMALL, context=64, prefill_chunk=16, seed=21, kv_fp8=kv_fp8)
    try:
        kw = dict(max_new_tokens=10, stop_tokens=[1023])
        greedy, _, _ = g.generate(PROMPT, top_k=1, **kw)
        s1, why, _ = g.generate(PROMPT, temperature=1.3, top_k=50, top_p=0.95, seed=42, **kw)
        s2, _, _ = g.generate(PROMPT, temperature=1.3, top_k=50, top_p=0.95, seed=42, **kw)
        s3, _, _ = g.generate(PROMPT, temperature=1.3, top_k=50, top_p=0.95, seed=43, **kw)
        assert s1 == s2 and len(s1) == 10 and why == "length" and all(0 <= t < 1024 for t in s1)
        assert s1 != greedy or s3 != greedy
        also, _, _ = g.generate(PROMPT, temperature=0.7, top_k=1, top_p=0.9, **kw)
        assert also == greedy                                       # top_k = 1 is still the greedy token list, after stochastic captures too
    finally:
        g.close()


def test_a_request_that_ends_on_a_stop_token_leaves_the_generator_where_the_eager_loop_left_it():
    """the replay that decodes token n also samples token n + 1, so its draw is taken before token n is known; when token n is a stop token the eager loop had not
    drawn it.  Two models, one seed: A serves a request that stops early and then a second one WITHOUT reseeding; B replays the draws A must have used -- the
    first request's (one per emitted token and one for the stop token), then the second request's."""
    a = host.GemmaModel.synthetic("bf16", SMALL, context=64, prefill_chunk=16, seed=21)
    b = host.GemmaModel.synthetic("bf16", SMALL, context=64, prefill_chunk=16, seed=21)
    try:
        sp = dict(temperature=1.3, top_k=50, top_p=0.95)
        for seed in range(5, 13):                               # a continuation with a token at 1 .. 6 that none before it equals: the request can stop exactly there
            full, _, _ = b.generate(PROMPT, max_new_tokens=8, stop_tokens=[1023], seed=seed, **sp)
            fresh = [i for i in range(1, 7) if full[i] not in full[:i]]
            if fresh:
                break
        assert fresh, "eight seeds, no continuation with a first occurrence at positions 1 .. 6: %s" % full
        stop_at = fresh[-1]
        first, why, _ = a.generate(PROMPT, max_new_tokens=8, stop_tokens=[full[stop_at]], seed=seed, **sp)
        assert first == full[:stop_at] and why == "stop"
        # A has consumed stop_at + 1 draws.  B: the same stop_at + 1 draws through a request of exactly that many samples, then the follow-up on both
        b.generate(PROMPT, max_new_tokens=stop_at + 1, stop_tokens=[1023], seed=seed, **sp)
        nxt_a, _, _ = a.generate(PROMPT[:7], max_new_tokens=6, stop_tokens=[1023], **sp)
        nxt_b, _, _ = b.generate(PROMPT[:7], max_new_tokens=6, stop_tokens=[1023], **sp)
        assert nxt_a == nxt_b
    finally:
        a.close()
        b.close()
