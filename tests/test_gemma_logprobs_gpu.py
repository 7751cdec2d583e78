"""GPU: token log-probabilities in the Gemma decode steps (GemmaTransformer::setStepLogprobs, GenerateParams::logprobs).

Runner level: the arrays a step returns are, bit for bit, the kernel entry (token_logprobs_rows_fp32) applied to the logits and the tokens the same call returned; the
logits, tokens and positions are those of the same call without log-probabilities on a twin; a captured step has exactly two more kernel nodes with the setting on,
and the nodes it always had with it off.

Model level: generate() / generate_batch() give the tokens, status and reuse count they give without the option; every emitted token has one entry; the speculative
loops and the rows loop report, bit for bit, what the plain loop reports.  Twins are sent the same requests in the same order (test_gemma_spec_generate_gpu.py says why).
No live-length bucket edge lies within MAX_SEQ = 64 (the first is at 4096 keys), so none is crossed here."""
import numpy as np
import pytest
import torch

from gpu_util import dev_f32, dev_i32
from mila_amd import capi, host
from test_gemma_chain_gpu import PROMPT as CHAIN_PROMPT
from test_gemma_chain_gpu import _truth
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_rows_gpu import NEW_PROMPT, PROMPTS

pytestmark = pytest.mark.gpu

SEED = 7
SOFTCAP = 30.0      # GemmaConfig::final_logit_softcapping of the synthetic models
POLICIES = ["bf16", "fp8", "fp4"]
SETTING = (0.9, 12, 0.9)
V = SMALL["vocab_size"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _kernel(logits_row, token, n):
    """the kernel entry on one row of logits: (logprob, ids [n], logprobs [n])"""
    lp = torch.empty(1, dtype=torch.float32, device="cuda:0")
    ids = torch.empty(max(n, 1), dtype=torch.int32, device="cuda:0")
    tlp = torch.empty(max(n, 1), dtype=torch.float32, device="cuda:0")
    scratch = torch.empty(capi.token_logprobs_scratch_bytes(1, V, n), dtype=torch.uint8, device="cuda:0")
    capi.token_logprobs_rows(dev_f32(np.asarray(logits_row).reshape(1, V)), dev_i32([int(token)]), SOFTCAP, n, lp, ids[:n] if n else None, tlp[:n] if n else None, scratch)
    return lp.cpu().numpy()[0], ids.cpu().numpy()[:n], tlp.cpu().numpy()[:n]


def _assert_is_the_kernels(what, logits_row, token, n, lp, ids, tlp):
    klp, kids, ktlp = _kernel(logits_row, token, n)
    assert _bits(np.float32(lp)) == _bits(klp) and _bits(ids) == _bits(kids) and _bits(tlp) == _bits(ktlp), what
    assert np.isfinite(klp) and klp <= 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# runner level
@pytest.mark.parametrize("policy", POLICIES)
def test_the_one_row_step_reports_the_kernels_logprobs(policy):
    modes = ("reference", "fused", "graph")
    on = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED) for m in modes}
    off = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED) for m in modes}
    try:
        pre = [g.prefill(PROMPTS[1]) for g in list(on.values()) + list(off.values())]
        tok, pos = int(np.argmax(pre[0])), len(PROMPTS[1])
        for n in (5, 0, 20, 1):
            chosen = set()
            for m in modes:
                logits, t, lp, ids, tlp = on[m].decode(tok, pos, m, logprobs=n)
                assert _same(logits, off[m].decode(tok, pos, m)), (m, n)
                assert t == int(np.argmax(logits)) and ids.shape == (n,) and tlp.shape == (n,)
                _assert_is_the_kernels((policy, m, n), logits, t, n, lp, ids, tlp)
                if n:
                    assert ids[0] == t and _bits(tlp[0]) == _bits(lp)          # greedy: the first alternative is the token
                chosen.add(t)
            assert len(chosen) == 1
            tok, pos = chosen.pop(), pos + 1
        # the captured step: two more nodes with the setting on; off again, the nodes of a model that never had it
        with_lp = on["graph"].graph_node_count()
        assert _same(on["graph"].decode(tok, pos, "graph"), off["graph"].decode(tok, pos, "graph"))
        assert on["graph"].graph_node_count() == off["graph"].graph_node_count() > 0
        assert with_lp == off["graph"].graph_node_count() + 2
        for bad in (21, -1):
            with pytest.raises(ValueError):
                on["fused"].decode(tok, pos, "fused", logprobs=bad)
        # the scratch and the outputs exist from the first enable on, and are counted on both sides of the footprint from then on
        had, never = on["fused"].memory_stats(), off["fused"].memory_stats()
        grown = had["actual"]["device_state_bytes"] - never["actual"]["device_state_bytes"]
        assert grown >= capi.token_logprobs_scratch_bytes(1, V, 20) + 4 + 2 * 20 * 4
        assert had["required"]["device_state_bytes"] - never["required"]["device_state_bytes"] == grown
        assert had["actual"]["device_parameter_bytes"] == never["actual"]["device_parameter_bytes"]
    finally:
        for g in list(on.values()) + list(off.values()):
            g.close()


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("policy", POLICIES)
def test_the_rows_step_reports_the_kernels_logprobs(policy, B):
    modes = ("fused", "graph")
    on = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4) for m in modes}
    off = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4) for m in modes}
    live = min(B, 3)      # B = 4: row 3 stays inactive
    rng = np.random.default_rng(5)
    try:
        for g in list(on.values()) + list(off.values()):
            for b in range(live):
                g.set_active(b, True, token=int(np.argmax(g.prefill_row(b, PROMPTS[b]))))
        pos = [len(p) for p in PROMPTS[:live]]
        for n, sampled in ((5, False), (20, True), (0, True), (1, False)):
            draws = rng.uniform(0, 1, B).astype(np.float32)
            kw = dict(greedy=False, sampling=SETTING, draws=draws) if sampled else dict(greedy=True)
            for m in modes:
                logits, toks, p, lp, ids, tlp = on[m].decode_rows(B, max(pos), m, logprobs=n, **kw)
                l0, t0, p0 = off[m].decode_rows(B, max(pos), m, **kw)
                assert _same(logits, l0) and toks.tolist() == t0.tolist() and p.tolist() == p0.tolist(), (m, n, sampled)
                assert lp.shape == (B,) and ids.shape == (B, n) and tlp.shape == (B, n)
                for b in range(live):
                    _assert_is_the_kernels((policy, B, m, n, sampled, b), logits[b], toks[b], n, lp[b], ids[b], tlp[b])
                    if n and not sampled:
                        assert ids[b, 0] == toks[b]
            pos = [x + 1 for x in pos]
        with_lp = on["graph"].rows_graph_info()["nodes"]
        on["graph"].decode_rows(B, max(pos), "graph", greedy=True)
        off["graph"].decode_rows(B, max(pos), "graph", greedy=True)
        assert on["graph"].rows_graph_info()["nodes"] == off["graph"].rows_graph_info()["nodes"] > 0
        assert with_lp == off["graph"].rows_graph_info()["nodes"] + 2
        with pytest.raises(ValueError):      # a step without a sampler tail has no token to report
            on["fused"].decode_rows(B, max(pos) + 1, "fused", greedy=False, logprobs=3)
    finally:
        for g in list(on.values()) + list(off.values()):
            g.close()


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("policy", POLICIES)
def test_the_chain_step_reports_the_kernels_logprobs(policy, T):
    pre, truth, _ = _truth(policy, "small", SMALL)
    modes = ("fused", "graph")
    on = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=3) for m in modes}
    off = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=3) for m in modes}
    rng = np.random.default_rng(9)
    try:
        for g in list(on.values()) + list(off.values()):
            assert _same(g.prefill(CHAIN_PROMPT), pre)
        P, i = len(CHAIN_PROMPT), 0
        # true drafts (all accepted), a corrupted first draft (one token), then sampled steps from wherever the sequence is, the last one greedy again
        plan = [(5, "true", False), (20, "wrong", False), (1, "true", True), (0, "any", True), (5, "any", False)]
        cur, position = None, P
        for n, drafts, sampled in plan:
            if drafts == "true" and cur is None:
                tokens = truth[i:i + T]
            elif drafts == "wrong":
                tokens = [truth[i]] + [(t + 1) % V for t in truth[i + 1:i + T]]
            else:
                tokens = [truth[i] if cur is None else cur] + [int(x) for x in rng.integers(0, V, T - 1)]
            draws = rng.uniform(0, 1, T).astype(np.float32)
            kw = dict(sampling=SETTING, draws=draws) if sampled else {}
            outs = set()
            for m in modes:
                logits, count, accepted, new_pos, lp, ids, tlp = on[m].decode_chain(tokens, position, m, logprobs=n, **kw)
                l0, c0, a0, np0 = off[m].decode_chain(tokens, position, m, **kw)
                assert _same(logits, l0) and (count, accepted, new_pos) == (c0, a0, np0), (m, n, drafts, sampled)
                assert lp.shape == (count,) and ids.shape == (count, n) and tlp.shape == (count, n)
                for t in range(count):
                    _assert_is_the_kernels((policy, T, m, n, drafts, sampled, t), logits[t], accepted[t], n, lp[t], ids[t], tlp[t])
                outs.add((count, tuple(accepted), new_pos))
            assert len(outs) == 1
            count, accepted, position = outs.pop()
            if drafts == "true" and not sampled:
                assert count == T
            if drafts == "wrong":
                assert count == 1
            if sampled or cur is not None:
                cur = accepted[-1]
            else:
                i += count
        with_lp = on["graph"].chain_graph_info()["nodes"]
        tokens = [cur] + [0] * (T - 1)
        on["graph"].decode_chain(tokens, position, "graph")
        off["graph"].decode_chain(tokens, position, "graph")
        assert on["graph"].chain_graph_info()["nodes"] == off["graph"].chain_graph_info()["nodes"] > 0
        assert with_lp == off["graph"].chain_graph_info()["nodes"] + 2
    finally:
        for g in list(on.values()) + list(off.values()):
            g.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# model level
CONTEXT = 48
KW = dict(context=CONTEXT, prefill_chunk=16, seed=SEED)


def _entries_bits(entries):
    return [(_bits(lp), _bits(ids), _bits(tlp)) for lp, ids, tlp in entries]


def _quiet_stop(model_a, model_b, prompt, n):
    """a stop token the free greedy run of n tokens never emits, found on both twins alike"""
    free = model_a.generate(prompt, max_new_tokens=n)[0]
    assert model_b.generate(prompt, max_new_tokens=n)[0] == free
    return next(s for s in (1023, 1022, 1021, 1020, 1019) if s not in free)


@pytest.mark.parametrize("policy", POLICIES)
def test_generate_with_logprobs_gives_the_same_tokens_and_one_entry_per_token(policy):
    plain, lp = host.GemmaModel.synthetic(policy, SMALL, **KW), host.GemmaModel.synthetic(policy, SMALL, **KW)
    try:
        for bad in (21, -1):
            with pytest.raises(ValueError):
                lp.generate(PROMPTS[0], max_new_tokens=2, logprobs=bad)
        for prompt in PROMPTS:
            stop = _quiet_stop(plain, lp, prompt, 12)
            kw = dict(max_new_tokens=12, stop_tokens=[stop])
            # greedy
            want = plain.generate(prompt, **kw)
            toks, status, reused, entries = lp.generate(prompt, logprobs=5, **kw)
            assert (toks, status, reused) == want and status == "length" and len(entries) == len(toks) == 12
            for t, (l, ids, tl) in zip(toks, entries):
                assert ids.shape == (5,) and ids[0] == t and _bits(l) == _bits(tl[0]) and l <= 0.0
                assert (np.diff(tl) <= 0).all()
            # n = 0 and n = 20 report the same log-probability
            for n in (0, 20):
                assert plain.generate(prompt, **kw) == want
                got = lp.generate(prompt, logprobs=n, **kw)
                assert got[:3] == want and [_bits(e[0]) for e in got[3]] == [_bits(e[0]) for e in entries] and all(e[1].shape == (n,) for e in got[3])
            # a stop token ends the run: an entry for every emitted token, none for the stop token; the first-token path alone
            j = next(k for k in range(2, 12) if toks[k] not in toks[:k])
            want_stop = plain.generate(prompt, max_new_tokens=12, stop_tokens=[toks[j]])
            got = lp.generate(prompt, max_new_tokens=12, stop_tokens=[toks[j]], logprobs=5)
            assert got[:3] == want_stop and got[1] == "stop" and len(got[3]) == len(got[0]) == j
            assert _entries_bits(got[3]) == _entries_bits(entries[:j])
            want_one = plain.generate(prompt, max_new_tokens=1, stop_tokens=[stop])
            got = lp.generate(prompt, max_new_tokens=1, stop_tokens=[stop], logprobs=5)
            assert got[:3] == want_one and len(got[3]) == 1 and _entries_bits(got[3]) == _entries_bits(entries[:1])
            # stochastic with a seed: the same tokens; the log-probability is the model's, whatever the sampler's temperature and truncation
            skw = dict(max_new_tokens=10, stop_tokens=[stop], temperature=SETTING[0], top_k=SETTING[1], top_p=SETTING[2], seed=31)
            want = plain.generate(prompt, **skw)
            got = lp.generate(prompt, logprobs=5, **skw)
            assert got[:3] == want and len(got[3]) == len(got[0])
            for t, (l, ids, tl) in zip(got[0], got[3]):
                assert l <= 0.0
                if t in ids.tolist():
                    assert _bits(l) == _bits(tl[ids.tolist().index(t)])
            # without the option again: what it always was
            assert lp.generate(prompt, **kw) == plain.generate(prompt, **kw)
    finally:
        plain.close()
        lp.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_the_speculative_loops_report_the_plain_loops_logprobs(policy):
    twin, spec = host.GemmaModel.synthetic(policy, SMALL, **KW), host.GemmaModel.synthetic(policy, SMALL, draft_tokens=3, **KW)
    try:
        for prompt in PROMPTS[1:]:
            stop = _quiet_stop(twin, spec, prompt, 14)
            for skw in (dict(), dict(temperature=SETTING[0], top_k=SETTING[1], top_p=SETTING[2], seed=23, speculative_sampling=True)):
                kw = dict(max_new_tokens=14, stop_tokens=[stop], logprobs=5)
                tkw = {k: v for k, v in skw.items() if k != "speculative_sampling"}
                for hint in ("true", "wrong", None):
                    ref = twin.generate(prompt, **kw, **tkw)
                    h = {None: None, "true": ref[0], "wrong": [(t + 1) % V for t in ref[0]]}[hint]
                    got = spec.generate(prompt, draft_hint=h, **kw, **skw)
                    assert got[:2] == ref[:2] and len(got[3]) == len(got[0]) > 0, (hint, skw, got[:2], ref[:2])
                    assert _entries_bits(got[3]) == _entries_bits(ref[3]), (hint, skw)
                    if hint == "true":
                        assert spec.speculation_stats()["accepted"] > 0
    finally:
        twin.close()
        spec.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_generate_batch_reports_each_prompts_logprobs_alone(policy):
    """every prompt starts with another token, so the one-sequence twin prefills each of them whole, as the rows model does"""
    alone, batch = host.GemmaModel.synthetic(policy, SMALL, **KW), host.GemmaModel.synthetic(policy, SMALL, max_batch=4, **KW)
    prompts = PROMPTS + [NEW_PROMPT]
    assert len({p[0] for p in prompts}) == 4
    try:
        for skw in (dict(), dict(temperature=SETTING[0], top_k=SETTING[1], top_p=SETTING[2])):
            kw = dict(max_new_tokens=7, stop_tokens=[1])
            want = [alone.generate(p, logprobs=5, **kw, **(dict(skw, seed=40 + b) if skw else {})) for b, p in enumerate(prompts)]
            assert all(w[2] == 0 for w in want), "a prompt of the twin was served from its caches"
            for count in (1, 2, 4):
                plain = batch.generate_batch(prompts[:count], seed=40, **kw, **skw)
                got = batch.generate_batch(prompts[:count], seed=40, logprobs=5, **kw, **skw)
                assert [g[:2] for g in got] == [tuple(x) for x in plain]
                for b in range(count):
                    assert (got[b][0], got[b][1]) == want[b][:2], (count, b, skw)
                    assert len(got[b][2]) == len(got[b][0])
                    assert _entries_bits(got[b][2]) == _entries_bits(want[b][3]), (count, b, skw)
        for bad in (21, -1):
            with pytest.raises(ValueError):
                batch.generate_batch(prompts[:2], max_new_tokens=2, logprobs=bad)
    finally:
        alone.close()
        batch.close()
