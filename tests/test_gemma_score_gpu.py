"""GPU: prompt log-probabilities through the Gemma host mirror -- GemmaTransformer::prefillScored (host.Gemma.prefill_scored) and GemmaModel::score -- on the conditioned
12-layer model that tests/test_gemma_conditioned_gpu.py holds to 1e-3 of max |logit|.

Bar on a log-probability (tests/ref_score.py): softcap and log-sum-exp are 1-Lipschitz in the max norm, so logits within (logit bar) * max |logit_oracle| of the oracle's
move z_t and log S by at most that much each: |d logprob| <= 2 * (logit bar) * max |logit_oracle| + BAR[softcap] (the kernel's own bar, test_token_logprobs_gpu.py).
The logit bar is the project's: 1e-3 for bf16 and fp8 weights, BAR_W4A8_PREFILL for fp4, ref_gemma_kvfp8.gpu_bar() over the FP8 KV cache.  The argmax is compared on
rows whose two best oracle tokens are further apart than that bound; the oracle alone is first held to leaving out at most one row in ten."""
import functools

import numpy as np
import pytest

import ref_gemma_kvfp8 as rk
from mila_amd import host
from ref_gemma import CONDITIONED_PROFILE, RefGemma
from ref_score import clear_rows, logprob_bar, oracle_scores
from test_gemma_conditioned_gpu import BAR, BAR_W4A8_PREFILL, CFG, MAX_SEQ, TOKENS

pytestmark = pytest.mark.gpu

T = len(TOKENS)
LAST_TARGET = 5                                           # prefill_scored takes a target for every row, the last included
TARGETS = TOKENS[1:] + [LAST_TARGET]
LOGIT_BAR = {"bf16": BAR, "fp8": BAR, "fp4": BAR_W4A8_PREFILL}
CHUNK = 16


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist()


@functools.lru_cache(maxsize=None)
def _oracle(policy, kv_fp8=False, tokens=tuple(TOKENS)):
    """(log-probabilities [T, V], the bound, the rows whose argmax is decided) of the oracle composition, once per policy for the whole module"""
    if kv_fp8:
        ref = rk.RefGemmaKvFp8(CFG, policy, seed=7, profile=CONDITIONED_PROFILE)
        ref.staged_prefill = True
        logit_bar = rk.gpu_bar()
    else:
        ref = RefGemma(CFG, policy, seed=7, profile=CONDITIONED_PROFILE, staged_prefill=True, w4a8_prefill=True)
        logit_bar = LOGIT_BAR[policy]
    lp, logits = oracle_scores(ref, list(tokens), MAX_SEQ)
    bound = logprob_bar(logit_bar, logits)
    clear = clear_rows(lp, bound)
    # the oracle alone: this token sequence leaves at most one row in ten undecided
    assert (~clear).sum() * 10 <= clear.size, "the test's own sequence: %d of %d rows have an undecided argmax" % ((~clear).sum(), clear.size)
    return lp, bound, clear


def _check(what, oracle, rows, targets, lp, am, alp):
    ref, bound, clear = oracle
    rows = np.asarray(rows)
    err = np.abs(lp.astype(np.float64) - ref[rows, np.asarray(targets)])
    worst = float(err.max())
    if am is not None:
        assert np.array_equal(am[clear[rows]], ref[rows].argmax(axis=1)[clear[rows]]), what
        worst = max(worst, float(np.abs(alp.astype(np.float64) - ref[rows, am]).max()))
    print("%s: max |logprob - oracle| = %.3e (bound %.3e)" % (what, worst, bound))
    assert worst <= bound, (what, worst, bound)


def _gemma(policy, max_prefill=32, **kw):
    return host.Gemma(policy, CFG, max_seq=MAX_SEQ, max_prefill=max_prefill, seed=7, profile=CONDITIONED_PROFILE, **kw)


def _model(policy, cfg=CFG, **kw):
    return host.GemmaModel.synthetic(policy, cfg, context=MAX_SEQ, prefill_chunk=CHUNK, seed=7, profile=CONDITIONED_PROFILE, **kw)


def _two_chunks(g, split=CHUNK):
    """prefill_scored over TOKENS as two chunks; the concatenated (logprob, argmax, argmax_logprob) of all T rows and the last logits"""
    _, lp0, am0, alp0 = g.prefill_scored(TOKENS[:split], TARGETS[:split], 0)
    logits, lp1, am1, alp1 = g.prefill_scored(TOKENS[split:], TARGETS[split:], split)
    return logits, np.concatenate([lp0, lp1]), np.concatenate([am0, am1]), np.concatenate([alp0, alp1])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# transformer level
@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_prefill_scored_against_the_oracle_in_one_chunk_and_in_two(policy):
    oracle = _oracle(policy)
    g = _gemma(policy)
    plain = g.prefill(TOKENS)
    logits, lp, am, alp = g.prefill_scored(TOKENS, TARGETS)
    assert _bits(logits) == _bits(plain), "the last row's logits are not prefill()'s"
    _check("%s prefill_scored T=%d" % (policy, T), oracle, range(T), TARGETS, lp, am, alp)
    # rows from first_row on: the tail of the full result, bit for bit; without the argmax the same log-probabilities
    _, lp7, am7, alp7 = g.prefill_scored(TOKENS, TARGETS, first_row=7)
    assert _bits(lp7) == _bits(lp[7:]) and _bits(am7) == _bits(am[7:]) and _bits(alp7) == _bits(alp[7:])
    _, lp_only, none_a, none_b = g.prefill_scored(TOKENS, TARGETS, argmax=False)
    assert none_a is None and none_b is None and _bits(lp_only) == _bits(lp)
    # a target of -1 reports NaN and leaves the other rows alone
    tg = list(TARGETS)
    tg[3] = -1
    _, lpn, _, _ = g.prefill_scored(TOKENS, tg)
    assert np.isnan(lpn[3]) and _bits(np.delete(lpn, 3)) == _bits(np.delete(lp, 3))
    for split in (12, CHUNK):
        plain2 = g.prefill(TOKENS[:split])
        plain2 = g.prefill(TOKENS[split:], split)
        logits2, lp2, am2, alp2 = _two_chunks(g, split)
        assert _bits(logits2) == _bits(plain2)
        _check("%s prefill_scored %d + %d" % (policy, split, T - split), oracle, range(T), TARGETS, lp2, am2, alp2)
    with pytest.raises(ValueError):
        g.prefill_scored(TOKENS, TARGETS, first_row=T)
    with pytest.raises(ValueError):
        g.prefill_scored(TOKENS, TARGETS[:-1])
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# model level
@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_score_is_the_transformers_rows_and_their_float64_sum(policy):
    g = _gemma(policy, max_prefill=CHUNK)
    _, lp, am, alp = _two_chunks(g)                      # the model's chunking: 16 + 4
    g.close()
    m = _model(policy)
    res = m.score(TOKENS, argmax=True)
    assert res["reused_prefix"] == 0
    assert len(res["logprob"]) == T - 1
    assert _bits(res["logprob"]) == _bits(lp[:-1]) and _bits(res["argmax"]) == _bits(am[:-1]) and _bits(res["argmax_logprob"]) == _bits(alp[:-1])
    assert res["sum"] == float(np.sum(res["logprob"].astype(np.float64)))
    _check("%s score" % policy, _oracle(policy), range(T - 1), TOKENS[1:], res["logprob"], res["argmax"], res["argmax_logprob"])
    plain = m.score(TOKENS)                              # the same sequence again: nothing below first - 1 = 0 can be reused
    assert plain["reused_prefix"] == 0 and "argmax" not in plain and _bits(plain["logprob"]) == _bits(res["logprob"])
    m.close()
    # first = k on a fresh model: the tail of the full result, bit for bit
    for k in (8, CHUNK, CHUNK + 1, T - 1):
        f = _model(policy)
        tail = f.score(TOKENS, first=k, argmax=True)
        f.close()
        assert tail["reused_prefix"] == 0
        assert _bits(tail["logprob"]) == _bits(res["logprob"][k - 1:]) and _bits(tail["argmax"]) == _bits(res["argmax"][k - 1:]), k
        assert tail["sum"] == float(np.sum(tail["logprob"].astype(np.float64)))


def test_continuations_of_one_context_prefill_it_once():
    """the multiple-choice pattern.  The bound is the bf16 oracle's of TOKENS, whose first 12 tokens are the context: max |logit| is the tied table's peak at the
    position's own token, the same for every sequence of this model"""
    ctx, a, b = TOKENS[:12], [5, 9, 11], [100, 200, 300, 17]
    bound = _oracle("bf16")[1]
    m = _model("bf16")
    first = m.score(ctx + a, first=len(ctx))
    assert first["reused_prefix"] == 0 and len(first["logprob"]) == len(a)
    again = m.score(ctx + b, first=len(ctx), argmax=True)
    assert again["reused_prefix"] == len(ctx) - 1 and len(again["logprob"]) == len(b)
    m.close()
    f = _model("bf16")
    fresh = f.score(ctx + b, first=len(ctx), argmax=True)
    f.close()
    assert fresh["reused_prefix"] == 0
    d = float(np.abs(again["logprob"].astype(np.float64) - fresh["logprob"]).max())
    print("continuation: reused vs unreused differ by %.3e (bound %.3e)" % (d, bound))
    assert np.isfinite(again["logprob"]).all() and d <= bound


def _generate(m, prompt, n=4):
    toks, status, reused = m.generate(prompt, max_new_tokens=n, stop_tokens=[CFG["vocab_size"] - 1])[:3]
    return toks, reused


def test_echo_is_score_then_generate_and_refusals_leave_everything_alone():
    f = _model("bf16")
    want, reused = _generate(f, TOKENS)
    f.close()
    assert reused == 0 and len(want) == 4
    m = _model("bf16")
    m.score(TOKENS)
    got, reused = _generate(m, TOKENS)
    assert reused == T - 1 and got == want
    V = CFG["vocab_size"]
    for bad, kw in (([], {}), ([3], {}), (TOKENS, dict(first=0)), (TOKENS, dict(first=T)), (TOKENS, dict(first=-2)), (list(range(MAX_SEQ + 1)), {}),
                    (TOKENS[:5] + [V], {}), (TOKENS[:5] + [-1], {})):
        with pytest.raises(ValueError):
            m.score(bad, **kw)
        got, reused = _generate(m, TOKENS)                # the caches and the history are what they were: the prompt is still reused, the tokens are the same
        assert reused == T - 1 and got == want, (bad, kw)
    m.close()


def test_score_over_the_fp8_kv_cache():
    oracle = _oracle("bf16", kv_fp8=True)
    m = _model("bf16", kv_fp8=True)
    res = m.score(TOKENS, argmax=True)
    m.close()
    _check("kv-fp8 score", oracle, range(T - 1), TOKENS[1:], res["logprob"], res["argmax"], res["argmax_logprob"])


def test_score_over_the_bounded_local_kv():
    """SlidingWindowKvCache on the sliding-window layers: a ring of window + chunk - 1 rows; the same function as the unbounded cache, so the same oracle and bar"""
    m = _model("bf16", cfg=dict(CFG, bounded_local_kv=1))
    res = m.score(TOKENS, argmax=True)
    again = m.score(TOKENS[:14] + [9, 8, 7], first=14)
    m.close()
    _check("bounded local KV score", _oracle("bf16"), range(T - 1), TOKENS[1:], res["logprob"], res["argmax"], res["argmax_logprob"])
    assert np.isfinite(again["logprob"]).all() and len(again["logprob"]) == 3
