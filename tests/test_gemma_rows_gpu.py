"""GPU: batched decode in the Gemma model (GemmaConfig::max_batch > 1) -- up to four independent sequences per step, each at its own position on its own KV caches.
The oracle is batch invariance: row b's logits at every step are BIT-IDENTICAL to a max_batch = 1 model with the same seed running that sequence alone through the
fused step (every position here is in one live-length bucket).  Needs no new CPU reference."""
import numpy as np
import pytest

from mila_amd import host
from test_gemma_host_gpu import MAX_SEQ, MEDIUM, SMALL

pytestmark = pytest.mark.gpu

SEED = 7
PROMPTS = [[5, 900, 17], [3, 512, 77, 1023, 0, 42, 256, 8, 640], [99, 1, 300, 5, 900, 17, 3, 512, 77, 1023, 0, 42, 256, 8, 640]]      # lengths 3, 9, 15
NEW_PROMPT = [640, 8, 256, 42, 0]


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


class _Alone:
    """one sequence on a max_batch = 1 model: prefill, then greedy steps through the fused decode"""

    def __init__(self, policy, cfg, prompt):
        self.g = host.Gemma(policy, cfg, max_seq=MAX_SEQ, max_prefill=16, seed=SEED)
        self.prefill_logits = self.g.prefill(prompt)
        self.pos, self.tok = len(prompt), int(np.argmax(self.prefill_logits))

    def step(self):
        logits = self.g.decode(self.tok, self.pos, "fused")
        self.pos, self.tok = self.pos + 1, int(np.argmax(logits))
        return logits

    def close(self):
        self.g.close()


def _admit(rows, b, prompt, alone):
    logits = rows.prefill_row(b, prompt)
    assert _same(logits, alone.prefill_logits), "row %d: the row prefill differs from the prefill of the sequence alone" % b
    rows.set_active(b, True, token=alone.tok)


def _rows_equal_alone(policy, cfg, steps=8):
    alone = [_Alone(policy, cfg, p) for p in PROMPTS]
    models = {m: host.Gemma(policy, cfg, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4) for m in ("fused", "graph")}
    try:
        for g in models.values():
            for b, a in enumerate(alone):
                _admit(g, b, PROMPTS[b], a)      # row 3 stays inactive: position 0, token 0
        for step in range(steps):
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


@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_rows_equal_the_sequences_alone(policy):
    """prompts of 3, 9 and 15 tokens in rows 0 .. 2, row 3 inactive, eight greedy steps: logits, sampled tokens and positions of every row equal the alone runs;
    the eager rows step equals the graph replay; one capture"""
    _rows_equal_alone(policy, SMALL)


def test_rows_equal_the_sequences_alone_with_more_than_one_weight_step_per_row():
    """the MEDIUM geometry (D 1280, F 2560): the Linears see more than one pipeline step per weight row"""
    _rows_equal_alone("bf16", MEDIUM, steps=4)


@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_a_row_retires_and_a_new_prompt_is_admitted_into_it(policy):
    """after four steps row 1 retires (its position and token stay while rows 0 and 2 go on), is reset and takes a new prompt; all three rows still equal their alone runs"""
    alone = [_Alone(policy, SMALL, p) for p in PROMPTS]
    g = host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4)
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
        alone[1] = _Alone(policy, SMALL, NEW_PROMPT)
        _admit(g, 1, NEW_PROMPT, alone[1])
        for i in range(4):
            step([0, 1, 2], "after re-admission, step %d" % i)
        assert g.rows_graph_info()["captures"] == 1      # retiring and admitting rows changes device words, not the captured step
    finally:
        for x in alone + [g]:
            x.close()


def test_max_batch_one_is_the_model_it_was():
    """a model created through the rows entry with max_batch = 1 holds the bytes and captures the graph of the plain model; with max_batch = 4 the required memory
    (from the configuration alone) still equals what the built model holds, and the state grows by the rows' caches and buffers"""
    plain = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED)
    one = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=1)
    four = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4)
    try:
        sp, s1, s4 = plain.memory_stats(), one.memory_stats(), four.memory_stats()
        assert sp["actual"] == s1["actual"] and sp["required"] == s1["required"]
        assert s4["required"]["device_state_bytes"] == s4["actual"]["device_state_bytes"] > sp["actual"]["device_state_bytes"]
        assert s4["actual"]["device_parameter_bytes"] == sp["actual"]["device_parameter_bytes"]
        a, b = plain.decode(5, 0, "graph"), one.decode(5, 0, "graph")
        assert _same(a, b) and plain.graph_node_count() == one.graph_node_count() > 0
        assert _same(four.decode(5, 0, "graph"), a) and four.graph_node_count() == plain.graph_node_count()      # the one-row path of a rows model is the same path
        with pytest.raises(RuntimeError):
            one.decode_rows(2, 0)      # no rows on a one-sequence model
        for bad in (0, 5):
            with pytest.raises(ValueError):
                host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=bad)
        with pytest.raises(ValueError):
            host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=2, kv_fp8=True)
    finally:
        for x in (plain, one, four):
            x.close()


CONTEXT = 24


def _models(policy):
    kw = dict(context=CONTEXT, prefill_chunk=16, seed=SEED)
    return host.GemmaModel.synthetic(policy, SMALL, **kw), host.GemmaModel.synthetic(policy, SMALL, max_batch=4, **kw)


@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_generate_batch_gives_generates_tokens_and_statuses(policy):
    """greedy generateBatch against generate() per prompt, with the same parameters: a row that stops on a stop token, one that runs to max_new_tokens and one that hits
    the context limit (a 21-token prompt in a context of 24) finish at different steps of one batch"""
    alone, batch = _models(policy)
    try:
        prompts = [PROMPTS[0], PROMPTS[1], (PROMPTS[2] + NEW_PROMPT + [7])[:21]]
        free = [alone.generate(p, max_new_tokens=6)[0] for p in prompts]
        stop = free[0][2]      # the third token row 0 would emit ends it
        want = [alone.generate(p, max_new_tokens=6, stop_tokens=[stop])[:2] for p in prompts]
        got = batch.generate_batch(prompts, max_new_tokens=6, stop_tokens=[stop])
        assert [tuple(g) for g in got] == [tuple(w) for w in want], (got, want)
        assert got[0][1] == "stop" and len(got[0][0]) <= 2
        assert {g[1] for g in got} == {"stop", "length", "context_limit"}, got
        # the same batch again on the same model: rows are reset, the result is the same
        assert batch.generate_batch(prompts, max_new_tokens=6, stop_tokens=[stop]) == got
        # fewer prompts than rows, and one prompt (a rows step still carries two rows, the second inactive)
        assert tuple(batch.generate_batch(prompts[:1], max_new_tokens=5, stop_tokens=[1023 - stop])[0]) == tuple(alone.generate(prompts[0], max_new_tokens=5, stop_tokens=[1023 - stop])[:2])
        with pytest.raises(ValueError):
            batch.generate_batch(prompts + prompts[:2], max_new_tokens=2)      # five prompts
        with pytest.raises(ValueError):
            alone.generate_batch(prompts[:2], max_new_tokens=2)                # a one-sequence model
    finally:
        alone.close()
        batch.close()


def test_generate_batch_samples_each_row_from_its_own_generator():
    """stochastic: the same seed twice gives the same tokens; top_k = 1 is greedy; a one-prompt batch with seed s gives generate()'s tokens after seedSampler(s)"""
    alone, batch = _models("bf16")
    try:
        prompts = [PROMPTS[0], PROMPTS[1], NEW_PROMPT]
        kw = dict(max_new_tokens=8, stop_tokens=[1], temperature=0.9, top_k=12, top_p=0.9)
        a, b = batch.generate_batch(prompts, seed=31, **kw), batch.generate_batch(prompts, seed=31, **kw)
        assert a == b
        assert batch.generate_batch(prompts, seed=32, **kw) != a, "another seed gave the same tokens in every row"
        greedy = batch.generate_batch(prompts, max_new_tokens=8, stop_tokens=[1])
        assert batch.generate_batch(prompts, max_new_tokens=8, stop_tokens=[1], temperature=0.9, top_k=1, top_p=0.5, seed=5) == greedy
        for s in (31, 77):
            one = batch.generate_batch(prompts[1:2], seed=s, **kw)[0]
            assert tuple(one) == tuple(alone.generate(prompts[1], seed=s, **kw)[:2]), s
        # row b draws from seed + b: row 1 of a batch seeded s is a one-prompt batch seeded s + 1
        assert batch.generate_batch(prompts[:2], seed=40, **kw)[1] == batch.generate_batch(prompts[1:2], seed=41, **kw)[0]
    finally:
        alone.close()
        batch.close()
