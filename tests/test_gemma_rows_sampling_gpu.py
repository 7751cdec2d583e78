"""GPU: the stochastic sampler inside the rows step (GemmaTransformer::setRowsSampling; GemmaModel::generateBatch with a stochastic request).  The radix pipeline runs
over all rows behind the logits, each row at its own draw, and its tail -- token and position bump of every active row -- takes the place of the position bump.
Oracles: the one-row radix entry on each row's logits at that row's draw, and for generate_batch a recording of the tokens the per-row sampler calls gave before the
sampler moved into the graph (tests/golden/generate_batch_stochastic.json, written by tests/golden/record_generate_batch_stochastic.py on the parent commit)."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_util import dev_f32, dev_i32
from mila_amd import capi, host
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_rows_gpu import PROMPTS

pytestmark = pytest.mark.gpu

SEED = 7
SOFTCAP = 30.0      # GemmaConfig::final_logit_softcapping of the synthetic models
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_batch_stochastic.json")


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _one_row_sample(logits_row, setting, r):
    t, k, p = setting
    scratch = torch.empty(capi.sample_radix_scratch_bytes(logits_row.size), dtype=torch.uint8, device="cuda:0")
    tok = dev_i32(np.array([-1]))
    capi.sample_radix(dev_f32(logits_row), tok, SOFTCAP, t, k, p, float(np.float32(r)), scratch)
    return int(tok.cpu()[0])


@pytest.mark.parametrize("setting", [(0.9, 12, 0.9), (1.0, 64, 0.95), (1.3, 0, 1.0)])
@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_the_sampled_rows_step_eager_and_replayed(policy, setting):
    """prompts of 3, 9 and 15 tokens in rows 0 .. 2, row 3 inactive, six sampled steps: the eager step and the graph replay give the same logits bits, tokens and
    positions; each active row's token is the one-row radix entry's on that row's logits at that row's draw; the inactive row is unmoved; one capture, whose kernel
    nodes are the logits-only step's minus the position bump plus the launches of ONE one-row pipeline"""
    models = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4) for m in ("fused", "graph", "plain")}
    rng = np.random.default_rng(11)
    try:
        pos = [len(p) for p in PROMPTS]
        for g in models.values():
            for b, prompt in enumerate(PROMPTS):
                g.set_active(b, True, token=int(np.argmax(g.prefill_row(b, prompt))))
        for step in range(6):
            draws = rng.uniform(0, 1, 4).astype(np.float32)
            out = {m: models[m].decode_rows(4, max(pos), m, greedy=False, sampling=setting, draws=draws) for m in ("fused", "graph")}
            (lf, tf, pf), (lg, tg, pg) = out["fused"], out["graph"]
            assert _same(lf, lg), "step %d: the eager rows step differs from the graph replay" % step
            assert tf.tolist() == tg.tolist() and pf.tolist() == pg.tolist(), (step, tf, tg, pf, pg)
            for b in range(3):
                pos[b] += 1
                assert int(tg[b]) == _one_row_sample(lg[b], setting, draws[b]), "step %d row %d: not the one-row sampler's token" % (step, b)
                assert int(pg[b]) == pos[b]
            assert int(pg[3]) == 0 and int(tg[3]) == 0, "the inactive row moved"
        info = models["graph"].rows_graph_info()
        assert info["captures"] == 1 and models["fused"].rows_graph_info()["captures"] == 0
        # the logits-only step of the same shape on a model of its own, from the same positions
        for b in range(3):
            models["plain"].set_active(b, True, token=5)
        models["plain"].decode_rows(4, 15, "graph", greedy=False)
        plain = models["plain"].rows_graph_info()
        launches = capi.sample_radix_plan(SMALL["vocab_size"], setting[1], setting[2])["launches"]
        assert info["nodes"] == plain["nodes"] - 1 + launches, (info, plain, launches)
        # other parameters are another capture; the sampler-less step after it one more, and it moves no token
        models["graph"].decode_rows(4, max(pos), "graph", greedy=False, sampling=(setting[0] * 0.5, setting[1], setting[2]), draws=np.full(4, 0.5, dtype=np.float32))
        assert models["graph"].rows_graph_info()["captures"] == 2
        before = models["graph"].decode_rows(4, max(pos) + 1, "graph", greedy=False)[1].tolist()
        after = models["graph"].decode_rows(4, max(pos) + 2, "graph", greedy=False)[1].tolist()
        assert before == after and models["graph"].rows_graph_info() == dict(captures=3, nodes=plain["nodes"])
    finally:
        for g in models.values():
            g.close()


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_generate_batch_gives_the_recorded_tokens_of_the_per_row_sampler(policy):
    """the fixture is a PARENT-COMMIT recording: what generate_batch gave when every active row was sampled by a one-row radix call of its own after each replay"""
    rec = _golden()
    m = host.GemmaModel.synthetic(policy, SMALL, context=rec["context"], prefill_chunk=16, seed=rec["model_seed"], max_batch=4)
    try:
        cases = [c for c in rec["cases"] if c["policy"] == policy]
        assert len(cases) >= 5
        statuses = set()
        for c in cases:
            kw = {k: c[k] for k in ("max_new_tokens", "stop_tokens", "temperature", "top_k", "top_p", "seed")}
            got = [[toks, status] for toks, status in m.generate_batch(c["prompts"], **kw)]
            assert got == c["want"], (c, got)
            statuses |= {g[1] for g in got}
        assert statuses == {"stop", "length", "context_limit"}, statuses
    finally:
        m.close()


def test_a_one_prompt_batch_still_equals_generate_after_seeding():
    kw = dict(context=24, prefill_chunk=16, seed=SEED)
    alone, batch = host.GemmaModel.synthetic("bf16", SMALL, **kw), host.GemmaModel.synthetic("bf16", SMALL, max_batch=4, **kw)
    try:
        req = dict(max_new_tokens=8, stop_tokens=[1], temperature=0.9, top_k=12, top_p=0.9)
        for s in (31, 77):
            one = batch.generate_batch(PROMPTS[1:2], seed=s, **req)[0]
            assert tuple(one) == tuple(alone.generate(PROMPTS[1], seed=s, **req)[:2]), s
        # greedy batches are untouched by the sampler setting of the stochastic ones before them
        greedy = batch.generate_batch(PROMPTS[:2], max_new_tokens=6, stop_tokens=[1])
        assert [tuple(g) for g in greedy] == [tuple(alone.generate(p, max_new_tokens=6, stop_tokens=[1])[:2]) for p in PROMPTS[:2]]
    finally:
        alone.close()
        batch.close()
