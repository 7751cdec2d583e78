"""GPU: the FP8 KV cache under batched rows in the Gemma model (GemmaConfig::kv_fp8_rows) -- up to four independent sequences per step, each on its own e4m3 caches.
THE ORACLE is the same sequence alone on a kv_fp8 one-row model of the same weights, compared as bit patterns: batch invariance of the rows step (the oracle of
tests/test_gemma_rows_gpu.py), and above it the contracts of generate_requests, serve_requests and the prefix cache (tests/test_gemma_row_requests_gpu.py,
tests/test_gemma_serve_requests_gpu.py, tests/test_gemma_prefix_cache_gpu.py), whose helpers and rule these tests run on FP8 models.  The SMALL geometry: head
dimensions 64 / 128, window 8, MAX_SEQ 64 -- every position in one live-length bucket."""
import numpy as np
import pytest

from mila_amd import host
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_prefix_cache_gpu import _check, _Rule
from test_gemma_row_requests_gpu import FOUR, _alone, _mod3, _same_row
from test_gemma_rows_gpu import NEW_PROMPT, PROMPTS, SEED, _admit, _same
from test_gemma_serve_requests_gpu import _fresh

pytestmark = pytest.mark.gpu

V = SMALL["vocab_size"]
POLICIES = ["bf16", "fp8"]
ST = dict(temperature=0.9, top_k=12, top_p=0.9)


class _Alone:
    """one sequence on a kv_fp8 one-row model: prefill, then greedy steps through the fused decode"""

    def __init__(self, policy, prompt):
        self.g = host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, kv_fp8=True)
        self.prefill_logits = self.g.prefill(prompt)
        self.pos, self.tok = len(prompt), int(np.argmax(self.prefill_logits))

    def step(self):
        logits = self.g.decode(self.tok, self.pos, "fused")
        self.pos, self.tok = self.pos + 1, int(np.argmax(logits))
        return logits

    def close(self):
        self.g.close()


def _rows_model(policy, max_batch=4):
    return host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=max_batch, kv_fp8_rows=True)


@pytest.mark.parametrize("policy", POLICIES)
def test_fp8_rows_equal_the_sequences_alone(policy):
    """prompts of 3, 9 and 15 tokens in rows 0 .. 2, row 3 inactive, eight greedy steps: prefill logits, step logits, sampled tokens and positions of every row equal
    the kv_fp8 alone runs bit for bit; the eager rows step equals the graph replay; one capture"""
    alone = [_Alone(policy, p) for p in PROMPTS]
    models = {m: _rows_model(policy) for m in ("fused", "graph")}
    try:
        for g in models.values():
            for b, a in enumerate(alone):
                _admit(g, b, PROMPTS[b], a)      # (asserts the row prefill's logits) row 3 stays inactive: position 0, token 0
        for step in range(8):
            max_pos = max(a.pos for a in alone)
            out = {m: g.decode_rows(4, max_pos, m) for m, g in models.items()}
            want = [a.step() for a in alone]
            for m, (logits, toks, pos) in out.items():
                for b, a in enumerate(alone):
                    assert _same(logits[b], want[b]), "%s step %d: row %d differs from the sequence alone" % (m, step, b)
                    assert int(toks[b]) == a.tok and int(pos[b]) == a.pos, (m, step, b, toks, pos)
                assert int(pos[3]) == 0 and int(toks[3]) == 0, "the inactive row moved"
            assert _same(out["fused"][0], out["graph"][0]), "eager rows step != graph replay at step %d" % step
        assert models["graph"].rows_graph_info()["captures"] == 1 and models["fused"].rows_graph_info()["captures"] == 0
        assert models["graph"].rows_graph_info()["nodes"] > 0
    finally:
        for x in alone + list(models.values()):
            x.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_an_fp8_row_retires_and_a_new_prompt_is_admitted_into_it(policy):
    """after four steps row 1 retires (its position and token stay while rows 0 and 2 go on), is reset and takes a new prompt over its old cache rows; all three rows
    still equal their alone runs"""
    alone = [_Alone(policy, p) for p in PROMPTS]
    g = _rows_model(policy)
    try:
        for b, a in enumerate(alone):
            _admit(g, b, PROMPTS[b], a)

        def step(live, what):
            logits, toks, pos = g.decode_rows(3, max(alone[b].pos for b in live), "graph")
            for b in live:
                assert _same(logits[b], alone[b].step()), "%s: row %d differs from the sequence alone" % (what, b)
                assert int(toks[b]) == alone[b].tok and int(pos[b]) == alone[b].pos
            return toks, pos

        for i in range(4):
            step([0, 1, 2], "step %d" % i)
        g.set_active(1, False)
        frozen_pos, frozen_tok = alone[1].pos, alone[1].tok
        for i in range(2):
            toks, pos = step([0, 2], "row 1 retired, step %d" % i)
            assert int(pos[1]) == frozen_pos and int(toks[1]) == frozen_tok, "the retired row moved"
        g.reset_row(1)
        alone[1].close()
        alone[1] = _Alone(policy, NEW_PROMPT)
        _admit(g, 1, NEW_PROMPT, alone[1])
        for i in range(4):
            step([0, 1, 2], "after re-admission, step %d" % i)
        assert g.rows_graph_info()["captures"] == 1
    finally:
        for x in alone + [g]:
            x.close()


def _kv_bytes(rows, per_element_and_scale):
    """resident KV bytes of `rows` rows from the configuration: per kind of layer 2 (K, V) x NKV x capacity x the bytes of one cached row"""
    total = 0
    for i in range(SMALL["num_layers"]):
        glob = (i + 1) % SMALL["sliding_window_pattern"] == 0
        nkv, hs = (SMALL["num_global_kv_heads"], SMALL["global_head_dim"]) if glob else (SMALL["num_kv_heads"], SMALL["head_dim"])
        total += rows * 2 * nkv * MAX_SEQ * per_element_and_scale(hs)
    return total


def test_memory_required_equals_actual_and_the_cache_is_hs_plus_4_of_2_hs():
    """what the configuration says a built model holds is what it holds; against the bf16 max_batch = 4 model the state shrinks by exactly the KV difference --
    (HS + 4) against 2 HS bytes per cached row, per kind of layer -- less the rows q buffer [4, NH * HD] the two-launch step needs; and with max_batch = 1 the switch
    builds the kv_fp8 model: same bytes, same graph"""
    fp8, bf16 = _rows_model("bf16"), host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4)
    one, plain = _rows_model("bf16", max_batch=1), host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, kv_fp8=True)
    try:
        s8, s16, s1, sp = fp8.memory_stats(), bf16.memory_stats(), one.memory_stats(), plain.memory_stats()
        assert s8["required"]["device_state_bytes"] == s8["actual"]["device_state_bytes"]
        assert s8["actual"]["device_parameter_bytes"] == s16["actual"]["device_parameter_bytes"]
        q_rows = 4 * SMALL["num_heads"] * max(SMALL["head_dim"], SMALL["global_head_dim"]) * 2
        saved = _kv_bytes(4, lambda hs: 2 * hs) - _kv_bytes(4, lambda hs: hs + 4)
        assert saved > 0 and s16["actual"]["device_state_bytes"] - s8["actual"]["device_state_bytes"] == saved - q_rows, (s16, s8, saved, q_rows)
        assert s8["actual"]["device_state_bytes"] < s16["actual"]["device_state_bytes"]
        assert s1["actual"] == sp["actual"] and s1["required"] == sp["required"]
        a, b = plain.decode(5, 0, "graph"), one.decode(5, 0, "graph")
        assert _same(a, b) and plain.graph_node_count() == one.graph_node_count() > 0
        with pytest.raises(ValueError):      # plain kv_fp8 keeps its refusal
            host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=2, kv_fp8=True)
    finally:
        for x in (fp8, bf16, one, plain):
            x.close()


# ---- serving ------------------------------------------------------------------------------------------------------------------------------------------------------
def _serving(policy, max_batch=4):
    kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED)
    return host.GemmaModel.synthetic(policy, SMALL, kv_fp8=True, **kw), host.GemmaModel.synthetic(policy, SMALL, max_batch=max_batch, kv_fp8_rows=True, **kw)


@pytest.mark.parametrize("policy", POLICIES)
def test_generate_requests_gives_each_fp8_row_what_generate_gives_it_alone(policy):
    """four differing requests -- greedy, stochastic with a seed, biased, a small automaton -- each with the alone model's tokens, finish reason and log-probability bits"""
    alone, batch = _serving(policy)
    try:
        reqs = [dict(prompt=FOUR[3], max_new_tokens=6),
                dict(prompt=FOUR[1], max_new_tokens=8, seed=11, **ST),
                dict(prompt=FOUR[2], max_new_tokens=7, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17]),
                dict(prompt=FOUR[0], max_new_tokens=7, automaton=_mod3())]
        want = [_alone(alone, q, logprobs=3) for q in reqs]
        got = batch.generate_requests(reqs, logprobs=3)
        for b in range(4):
            _same_row(got[b], want[b], True)
        assert all(t % 3 == i % 3 for i, t in enumerate(got[3][0])) and isinstance(got[3][-1], int), got[3]
    finally:
        alone.close()
        batch.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_serve_requests_forks_fp8_rows_and_captures_once(policy):
    """six stochastic requests of prompt lengths 15, 5, 3, 9, 5 and 3 on four rows, the first with n = 3: its copies share one prefill through the FP8 fork.  Row 3
    carries a request that outlasts all the others (asserted on the alone model), so every step has four rows and one class: one capture"""
    alone, batch = _serving(policy)
    try:
        long_free = alone.generate(FOUR[3], max_new_tokens=30, seed=2, **ST)[0]
        never = [t for t in range(V) if t not in long_free][:2]
        head = dict(prompt=FOUR[2], seed=5, max_new_tokens=8, **ST)
        reqs = [dict(head, n=3),
                dict(prompt=FOUR[3], max_new_tokens=30, seed=2, stop_tokens=never, **ST),
                dict(prompt=FOUR[0], max_new_tokens=4, seed=3, **ST),
                dict(prompt=FOUR[1], max_new_tokens=6, seed=4, **ST),
                dict(prompt=NEW_PROMPT, max_new_tokens=3, seed=6, **ST),
                dict(prompt=FOUR[0], max_new_tokens=5, seed=7, **ST)]
        flat = [dict(head, seed=s) for s in (5, 6, 7)] + reqs[1:]
        want = [_fresh(alone, q, logprobs=2) for q in flat]
        assert len(want[3][0]) == 30 and want[3][1] == "length", "the request in row 3 must outlast the others"
        assert len({tuple(w[0]) for w in want[:3]}) > 1, "the three seeds must not agree, or a fork that copied the sampler too would pass"
        got, stats = batch.serve_requests(reqs, logprobs=2)
        assert len(got) == 8
        for i in range(8):
            _same_row(got[i], want[i], True)
        assert stats["forks"] == 2 and stats["prefills"] == 6 and stats["rows"][:4] == [0, 1, 2, 3], stats
        assert stats["captures"] == 1 and batch.rows_graph_info()["captures"] == 1, stats
    finally:
        alone.close()
        batch.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_serve_requests_prefix_reuses_fp8_prefixes(policy):
    """five requests that share a 12-token header (longer than the window of 8) and go on with distinct tails, on two rows: every one but the first takes the header
    from a row that holds it -- a fork of e4m3 bytes and scale words, or in place -- and prefills its tail at offset 12 through the policy's attention-only prefill on
    the selected row.  The oracle is the prefix cache's own: generate() on the kv_fp8 alone model on which the donor chain ran before, itself reusing 12 positions"""
    alone, batch = _serving(policy, max_batch=2)
    try:
        header = FOUR[2][:12]
        tails = [[33, 701, 2], [555, 64, 9, 310], [77], [640, 8, 256, 42, 0], [901, 12]]
        reqs = [dict(prompt=header + t, max_new_tokens=3 + i % 3, **(dict(seed=20 + i, **ST) if i % 2 else {})) for i, t in enumerate(tails)]
        batch.clear_prefix_cache()
        _, stats, _ = _check(_Rule(2, alone), batch, reqs, logprobs=2)
        assert stats["reused_tokens"][0] == 0 and all(r == 12 for r in stats["reused_tokens"][1:]), stats
        assert stats["prefix_forks"] >= 1, stats
    finally:
        alone.close()
        batch.close()
