"""GPU: speculative greedy generate() (GemmaModelConfig::withDraftTokens) -- up to k drafted tokens verified per step, up to k + 1 tokens emitted per step.  Every chain
row keeps the bits it has alone, so the oracle is exact: the tokens and the finish reason are those of a draft_tokens = 0 model, whatever the drafter proposes.

Every speculative model has a plain TWIN that is sent the same requests in the same order: generate() reuses the prompt prefix its caches hold, and a prompt prefilled
whole and one prefilled behind a reused prefix go through different prefill kernels (equal to the oracle's tolerance, not bit for bit), so the oracle of a request
is the twin's answer to that request at the same point of the same history."""
import pytest

from mila_amd import host
from test_gemma_host_gpu import SMALL
from test_gemma_rows_gpu import PROMPTS

pytestmark = pytest.mark.gpu

SEED = 7
CONTEXT = 48
REPETITIVE = [5, 900, 17, 3] * 3 + [5, 900]
ZERO = dict(steps=0, chain_steps=0, drafted=0, accepted=0)


class _Pair:
    def __init__(self, policy, k, context=CONTEXT):
        kw = dict(context=context, prefill_chunk=16, seed=SEED)
        self.k = k
        self.twin, self.spec = host.GemmaModel.synthetic(policy, SMALL, **kw), host.GemmaModel.synthetic(policy, SMALL, draft_tokens=k, **kw)

    def both(self, prompt, hint=None, **kw):
        """the request on the twin, then on the speculative model (hint: None = the default drafter, "true" = the twin's tokens, "wrong" = every one of them off by
        one): the same tokens and finish reason.  Returns (tokens, finish reason, the speculative loop's counters)."""
        ref = self.twin.generate(prompt, **kw)
        assert self.twin.speculation_stats() == ZERO
        h = {None: None, "true": ref[0], "wrong": [(t + 1) % SMALL["vocab_size"] for t in ref[0]]}[hint]
        got = self.spec.generate(prompt, draft_hint=h, **kw)
        assert got[:2] == ref[:2], (self.k, hint, prompt, kw, got, ref)
        if h is None:
            assert got[2] == ref[2], "the speculative model reused another prefix than its twin"
        return ref[0], ref[1], self.spec.speculation_stats()

    def quiet_stop(self, prompt, n):
        """a stop token the free run of n tokens never emits (the synthetic model knows no EOS)"""
        for s in (1023, 1022, 1021, 1020, 1019):
            if self.both(prompt, max_new_tokens=n, stop_tokens=[s])[1] != "stop":
                return s
        raise AssertionError("five stop candidates all stopped the run")

    def close(self):
        self.twin.close()
        self.spec.close()


def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_speculative_generate_gives_the_plain_greedy_tokens(policy, k):
    p = _Pair(policy, k)
    try:
        for prompt in PROMPTS + [REPETITIVE]:
            stop = p.quiet_stop(prompt, 18)
            kw = dict(max_new_tokens=18, stop_tokens=[stop])
            # the default drafter (prompt lookup over prompt + output): right or wrong, the tokens are the plain ones
            toks, status, st = p.both(prompt, **kw)
            assert status == "length" and len(toks) == 18
            assert st["steps"] >= st["chain_steps"] >= 0 and st["accepted"] <= st["drafted"] <= k * st["chain_steps"], st
            assert 1 <= st["steps"] <= 17 and st["steps"] + st["accepted"] <= 17 + k, st      # 17 tokens behind the prefill's: one per step plus the accepted drafts (the last step may overshoot by k)
            if prompt is REPETITIVE:
                assert st["chain_steps"] > 0, st
            # the true continuation as the hint: every draft is accepted, every step is a chain step
            toks, status, st = p.both(prompt, hint="true", **kw)
            assert st["chain_steps"] == st["steps"] == _ceil(17, k + 1), (k, st)      # the first token comes from the prefill's logits, k + 1 more per step
            assert st["accepted"] == st["drafted"] > 0, st                               # (padding is counted in neither)
            # a wrong hint costs steps, never tokens
            toks, status, st = p.both(prompt, hint="wrong", **kw)
            assert st["accepted"] == 0 and st["chain_steps"] == st["steps"] == 17, st
    finally:
        p.close()


@pytest.mark.parametrize("k", [1, 3])
def test_stop_token_and_token_budget_inside_an_accepted_run(k):
    p = _Pair("bf16", k)
    try:
        prompt = PROMPTS[1]
        stop0 = p.quiet_stop(prompt, 18)
        want = p.both(prompt, max_new_tokens=18, stop_tokens=[stop0])[0]
        # with k = 3 and the true hint the runs are want[1:5], want[5:9], ...: a stop token at index j = 2 or 3 sits inside the first run, at 6 inside the second
        tried = 0
        for j in (2, 3, 6):
            if want[j] in want[:j]:
                continue
            tried += 1
            for hint in ("true", None):
                toks, status, st = p.both(prompt, hint=hint, max_new_tokens=18, stop_tokens=[want[j]])
                assert (toks, status) == (want[:j], "stop"), (j, toks, status)
                if hint:
                    # the hint (the twin's output) ends before the stop token, which arrives as the successor of the last accepted draft, or from a one-row step where
                    # no draft is left: j tokens and the stop token, the first of them from the prefill, k + 1 per step
                    assert 1 <= st["steps"] <= _ceil(j, k + 1), (j, k, st)
        assert tried > 0
        # max_new_tokens mid-run
        for n in (1, 2, 3, 4, 6, 7):
            toks, status, st = p.both(prompt, hint="true", max_new_tokens=n, stop_tokens=[stop0])
            assert (toks, status) == (want[:n], "length"), (n, toks, status)
            assert st["chain_steps"] == st["steps"] == _ceil(n - 1, k + 1), (n, k, st)
        # a request that extends the last one reuses the caches the speculative loop left -- accepted tokens only -- as the twin reuses its own
        a = p.both(prompt, max_new_tokens=9, stop_tokens=[stop0])[0]
        ref = p.twin.generate(prompt + a[:4], max_new_tokens=5, stop_tokens=[stop0])
        got = p.spec.generate(prompt + a[:4], max_new_tokens=5, stop_tokens=[stop0])
        assert got == ref and got[2] == len(prompt) + 3, (got, ref)
    finally:
        p.close()


@pytest.mark.parametrize("k", [1, 3])
def test_near_the_context_end_the_one_row_step_takes_over(k):
    """a context of 24 and a prompt of 15: the chain step needs position + k + 1 <= 24, so the last positions are decoded one row at a time; the tokens and the
    context_limit finish are the plain model's"""
    p = _Pair("bf16", k, context=24)
    try:
        prompt = PROMPTS[2]
        stop = p.quiet_stop(prompt, 64)
        toks, status, st = p.both(prompt, stop_tokens=[stop])
        assert status == "context_limit" and len(toks) == 24 - 15 + 1
        toks, status, st = p.both(prompt, hint="true", stop_tokens=[stop])
        assert status == "context_limit" and len(toks) == 24 - 15 + 1
        # positions 15 .. 23 are decoded: chain steps of k + 1 positions while position + k + 1 <= 24, one-row steps for the rest
        chain = (24 - 15) // (k + 1)
        assert st["chain_steps"] == chain and st["steps"] == chain + (24 - 15) - chain * (k + 1) > chain, (k, st)
    finally:
        p.close()


def test_stochastic_requests_keep_the_plain_path():
    p = _Pair("bf16", 3)
    try:
        kw = dict(max_new_tokens=10, stop_tokens=[1], temperature=0.9, top_k=12, top_p=0.9)
        for prompt in PROMPTS[:2]:
            for seed in (31, 77):
                st = p.both(prompt, max_new_tokens=6, stop_tokens=[1])[2]      # a greedy (speculative) request in between changes nothing
                assert st != ZERO
                assert p.both(prompt, seed=seed, **kw)[2] == ZERO
    finally:
        p.close()
