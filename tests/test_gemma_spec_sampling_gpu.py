"""GPU: speculative SAMPLING -- a stochastic generate() with GenerateParams::speculative_sampling on a withDraftTokens model.  The chain step's tail samples row t from
its own logits at the uniform draw the plain loop would use for that token and accepts a draft exactly when it equals that sample; every chain row keeps the bits it
has alone.  So the oracle is exact: the tokens and the finish reason are those of a draft_tokens = 0 model sent the same request with the same seed, whatever the
drafter proposes, and the request leaves the model's generator where the plain loop leaves it.

As in tests/test_gemma_spec_generate_gpu.py every speculative model has a plain TWIN that is sent the same requests in the same order."""
import numpy as np
import pytest
import torch

from gpu_util import dev_f32, dev_i32
from mila_amd import capi, host
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_rows_gpu import PROMPTS
from test_gemma_spec_generate_gpu import REPETITIVE, SEED, ZERO, _ceil

pytestmark = pytest.mark.gpu

CONTEXT = 48
SAMPLING = dict(temperature=0.9, top_k=12, top_p=0.9)
SOFTCAP = 30.0      # GemmaConfig::final_logit_softcapping of the synthetic models


class _Pair:
    def __init__(self, policy, k, context=CONTEXT):
        kw = dict(context=context, prefill_chunk=16, seed=SEED)
        self.k = k
        self.twin, self.spec = host.GemmaModel.synthetic(policy, SMALL, **kw), host.GemmaModel.synthetic(policy, SMALL, draft_tokens=k, **kw)

    def both(self, prompt, hint=None, **kw):
        """the stochastic request on the twin, then with speculative_sampling on the speculative model (hint: None = the default drafter, "true" = the twin's tokens,
        "wrong" = every one of them off by one): the same tokens and finish reason.  Returns (tokens, finish reason, the speculative loop's counters)."""
        args = dict(SAMPLING)
        args.update(kw)
        ref = self.twin.generate(prompt, **args)
        assert self.twin.speculation_stats() == ZERO
        h = {None: None, "true": ref[0], "wrong": [(t + 1) % SMALL["vocab_size"] for t in ref[0]]}[hint]
        got = self.spec.generate(prompt, draft_hint=h, speculative_sampling=True, **args)
        assert got[:2] == ref[:2], (self.k, hint, prompt, args, got, ref)
        return ref[0], ref[1], self.spec.speculation_stats()

    def quiet_stop(self, prompt, n, seed):
        """a stop token the free run of n tokens at this seed never emits (the synthetic model knows no EOS)"""
        for s in (1023, 1022, 1021, 1020, 1019):
            if self.both(prompt, max_new_tokens=n, stop_tokens=[s], seed=seed)[1] != "stop":
                return s
        raise AssertionError("five stop candidates all stopped the run")

    def close(self):
        self.twin.close()
        self.spec.close()


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_speculative_sampling_gives_the_plain_stochastic_tokens(policy, k):
    p = _Pair(policy, k)
    try:
        for prompt in PROMPTS[:2] + [REPETITIVE]:
            stop = p.quiet_stop(prompt, 18, 31)
            kw = dict(max_new_tokens=18, stop_tokens=[stop], seed=31)
            # the default drafter (prompt lookup over prompt + output): right or wrong, the tokens are the plain ones
            toks, status, st = p.both(prompt, **kw)
            assert status == "length" and len(toks) == 18
            assert st != ZERO and st["steps"] >= st["chain_steps"] >= 0 and st["accepted"] <= st["drafted"] <= k * st["chain_steps"], st
            assert 1 <= st["steps"] <= 17 and st["steps"] + st["accepted"] <= 17 + k, st
            # the twin's tokens as the hint: every draft is the sample, every step is a chain step
            toks, status, st = p.both(prompt, hint="true", **kw)
            assert st["chain_steps"] == st["steps"] == _ceil(17, k + 1), (k, st)
            assert st["accepted"] == st["drafted"] > 0, st
            # off by one: nothing is accepted, one token per step, the same tokens
            toks31, status, st = p.both(prompt, hint="wrong", **kw)
            assert st["accepted"] == 0 and st["chain_steps"] == st["steps"] == 17, st
            # a second seed: other tokens, on both models the same
            kw["seed"] = 77
            if p.both(prompt, **kw)[1] == "stop":
                kw["stop_tokens"] = [p.quiet_stop(prompt, 18, 77)]
            toks77 = p.both(prompt, hint="true", **kw)[0]
            assert toks77 != toks31, "two seeds, the same 18 tokens"
            # no seed: the request goes on in the stream the seeded one left -- the generator is where the plain loop leaves it (here after a run that ended inside
            # accepted runs, and after one that took a draw for every step)
            p.both(prompt, seed=None, max_new_tokens=7, stop_tokens=kw["stop_tokens"])
            p.both(prompt, hint="wrong", seed=None, max_new_tokens=5, stop_tokens=kw["stop_tokens"])
            p.both(prompt, hint="true", seed=None, max_new_tokens=6, stop_tokens=kw["stop_tokens"])
    finally:
        p.close()


@pytest.mark.parametrize("k", [1, 3])
def test_stop_token_and_token_budget_inside_an_accepted_run(k):
    p = _Pair("bf16", k)
    try:
        prompt, seed = PROMPTS[1], 31
        stop0 = p.quiet_stop(prompt, 18, seed)
        want = p.both(prompt, max_new_tokens=18, stop_tokens=[stop0], seed=seed)[0]
        # with k = 3 and the true hint the runs are want[1:5], want[5:9], ...: a stop token at index j = 2 or 3 sits inside the first run, at 6 inside the second
        tried = 0
        for j in (2, 3, 6):
            if want[j] in want[:j]:
                continue
            tried += 1
            for hint in ("true", None):
                toks, status, st = p.both(prompt, hint=hint, max_new_tokens=18, stop_tokens=[want[j]], seed=seed)
                assert (toks, status) == (want[:j], "stop"), (j, toks, status)
                if hint:
                    assert 1 <= st["steps"] <= _ceil(j, k + 1), (j, k, st)
                # the draws behind the stop token were peeked, not taken: the stream goes on as the twin's does
                p.both(prompt, hint=hint, seed=None, max_new_tokens=4, stop_tokens=[stop0])
        assert tried > 0
        # max_new_tokens mid-run
        for n in (1, 2, 3, 4, 6, 7):
            toks, status, st = p.both(prompt, hint="true", max_new_tokens=n, stop_tokens=[stop0], seed=seed)
            assert (toks, status) == (want[:n], "length"), (n, toks, status)
            assert st["chain_steps"] == st["steps"] == _ceil(n - 1, k + 1), (n, k, st)
            p.both(prompt, seed=None, max_new_tokens=3, stop_tokens=[stop0])
    finally:
        p.close()


@pytest.mark.parametrize("k", [1, 3])
def test_near_the_context_end_the_one_row_step_takes_over(k):
    """a context of 24 and a prompt of 15: the chain step needs position + k + 1 <= 24, so the last positions are decoded one row at a time by the captured
    stochastic one-row step; the tokens and the context_limit finish are the plain model's"""
    p = _Pair("bf16", k, context=24)
    try:
        prompt, seed = PROMPTS[2], 31
        stop = p.quiet_stop(prompt, 64, seed)
        toks, status, st = p.both(prompt, stop_tokens=[stop], seed=seed)
        assert status == "context_limit" and len(toks) == 24 - 15 + 1
        toks, status, st = p.both(prompt, hint="true", stop_tokens=[stop], seed=seed)
        assert status == "context_limit" and len(toks) == 24 - 15 + 1
        chain = (24 - 15) // (k + 1)
        assert st["chain_steps"] == chain and st["steps"] == chain + (24 - 15) - chain * (k + 1) > chain, (k, st)
        p.both(prompt[:9], seed=None, max_new_tokens=5, stop_tokens=[stop])
    finally:
        p.close()


def test_with_the_flag_clear_a_stochastic_request_keeps_the_plain_path():
    p = _Pair("bf16", 3)
    try:
        kw = dict(max_new_tokens=10, stop_tokens=[1], seed=31, **SAMPLING)
        ref = p.twin.generate(PROMPTS[1], **kw)
        assert p.spec.generate(PROMPTS[1], **kw) == ref and p.spec.speculation_stats() == ZERO
        assert p.spec.generate(PROMPTS[1], speculative_sampling=False, **kw)[:2] == ref[:2] and p.spec.speculation_stats() == ZERO
        assert p.spec.generate(PROMPTS[1], speculative_sampling=True, **kw)[:2] == ref[:2] and p.spec.speculation_stats() != ZERO
        # the flag does nothing on a model without draft tokens
        assert p.twin.generate(PROMPTS[1], speculative_sampling=True, **kw)[:2] == ref[:2] and p.twin.speculation_stats() == ZERO
    finally:
        p.close()


# ---- transformer level: the chain step with the sampling tail ----
def _one_row_sample(logits_row, setting, r):
    t, k, p = setting
    V = logits_row.size
    scratch = torch.empty(capi.sample_radix_scratch_bytes(V), dtype=torch.uint8, device="cuda:0")
    tok = dev_i32(np.array([-1]))
    capi.sample_radix(dev_f32(logits_row), tok, SOFTCAP, t, k, p, float(np.float32(r)), scratch)
    return int(tok.cpu()[0])


@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_the_sampled_chain_step_eager_and_replayed(policy):
    """Gemma.decode_chain(sampling=, draws=): the eager step and the graph replay give the same (count, tokens, position) and the same logits bits; accepted[i] is the
    one-row radix sampler's token from row i's logits at draws[i]; the accepted run is the longest prefix of drafts that equal those samples.  Each step is first run
    with wrong drafts and then again from the same position with one more draft set to the sample just seen, until every draft verifies."""
    setting = (SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"])
    prompt = PROMPTS[1]
    models = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=3) for m in ("fused", "graph")}
    rng = np.random.default_rng(5)
    try:
        pre = {m: g.prefill(prompt) for m, g in models.items()}
        assert np.array_equal(pre["fused"].view(np.uint32), pre["graph"].view(np.uint32))
        tok, pos = _one_row_sample(pre["graph"], setting, 0.5), len(prompt)
        partial = 0
        for step, T in enumerate((4, 2, 3)):
            draws = rng.uniform(0, 1, T).astype(np.float32)
            drafts = [tok] + [(tok + 1 + t) % SMALL["vocab_size"] for t in range(T - 1)]
            for rounds in range(T):
                out = {m: g.decode_chain(drafts, pos, m, sampling=setting, draws=draws) for m, g in models.items()}
                (lf, cf, af, pf), (lg, cg, ag, pg) = out["fused"], out["graph"]
                what = "step %d round %d" % (step, rounds)
                assert (cf, af, pf) == (cg, ag, pg), (what, out["fused"][1:], out["graph"][1:])
                assert np.array_equal(lf.view(np.uint32), lg.view(np.uint32)), "%s: the eager chain step differs from the graph replay" % what
                s = [_one_row_sample(lg[t], setting, draws[t]) for t in range(cg)]
                assert ag == s, (what, ag, s)
                assert 1 <= cg <= T and pg == pos + cg, (what, cg, pg)
                assert all(s[t] == drafts[t + 1] for t in range(cg - 1)), (what, s, drafts)
                if cg == T:
                    break
                assert s[cg - 1] != drafts[cg], (what, s, drafts)
                partial += 1
                drafts[cg] = s[cg - 1]      # the sample of row cg - 1 is the draft that verifies there: the next round accepts one more
            assert cg == T, "T rounds did not reach a fully accepted run"
            if step == 0:
                assert models["graph"].chain_graph_info()["captures"] == 1      # rounds change device words and draws, not the captured step
            tok, pos = ag[-1], pg
        assert partial > 0
        assert models["fused"].chain_graph_info()["captures"] == 0
        # the greedy chain step on the same model afterwards: another capture (the tail changed) and the greedy rule
        before = models["graph"].chain_graph_info()["captures"]
        logits, count, accepted, new_pos = models["graph"].decode_chain([tok, 0], pos, "graph")
        assert accepted[0] == int(np.argmax(logits[0])) and models["graph"].chain_graph_info()["captures"] == before + 1
    finally:
        for g in models.values():
            g.close()
