"""GPU: constrained speculative decode through the Gemma host mirror, on SMALL with a context of 32.
host.Gemma.decode_chain under set_token_automaton / set_token_bias: the eager step and the graph replay agree in tokens, count, position and logits bits; every accepted
token is the one-row constrained sampler's token from that row's logits under the state the HOST tracked (q_0 the state word, q_t = step(q_{t-1}, draft t), a forbidden
draft leaving the state); a forbidden draft ends acceptance in front of it; the chain graph re-captures once per bias / automaton key and never for a reset, a replaced
automaton of the same size or a table update.
GemmaModel.generate(speculate_constrained=True) on draft_tokens models: the oracle is a plain model sent the same request -- tokens, finish reason, final state, and for
stochastic requests the tokens of the NEXT request (the generator is where the plain loop leaves it)."""
import numpy as np
import pytest
import torch

import ref_token_automaton as A
from gpu_util import dev_f32, dev_i32
from mila_amd import capi, host
from test_gemma_host_gpu import SMALL, TOKENS

pytestmark = pytest.mark.gpu

MAX_SEQ = 32
SEED = 11
SOFTCAP = 30.0
V = SMALL["vocab_size"]
PROMPT = TOKENS[:7]
F = A.FORBIDDEN
S_TOK = 654
NEVER = [V - 1]
SAMPLING = (0.9, 12, 0.9)


def _mod3(start=0):
    """state k allows the ids = k (mod 3) and goes to k + 1 (mod 3)"""
    nxt = np.full((3, 3), F, dtype=np.uint16)
    for k in range(3):
        nxt[k, k] = (k + 1) % 3
    return host.TokenAutomaton((np.arange(V) % 3).astype(np.uint16), nxt, start=start)


def _one_row(logits_row, table, sampling, r):
    """the one-row constrained sampler on one row of logits: greedy (sampling None) or radix at the draw r"""
    tok, dev, tab = dev_i32(np.array([-1])), dev_f32(logits_row), dev_f32(table)
    if sampling is None:
        capi.sample_argmax_biased(dev, tok, SOFTCAP, None, None, tab, torch.empty(capi.load().mila_cdna4_sample_scratch_bytes(), dtype=torch.uint8, device="cuda:0"))
    else:
        t, k, p = sampling
        capi.sample_radix_biased(dev, tok, SOFTCAP, t, k, p, float(np.float32(r)), None, None, tab,
                                 torch.empty(capi.sample_radix_scratch_bytes(V), dtype=torch.uint8, device="cuda:0"))
    return int(tok.cpu()[0])


def _states(a, q0, drafts):
    q = [q0]
    for d in drafts[1:]:
        q.append(a.step(q[-1], d))      # (a forbidden draft leaves the state)
    return q


# ---- host.Gemma.decode_chain
@pytest.mark.parametrize("sampling", [None, SAMPLING], ids=["greedy", "sampled"])
@pytest.mark.parametrize("policy", ["bf16", "fp4"])
def test_the_constrained_chain_step_eager_and_replayed(policy, sampling):
    models = {m: host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=3) for m in ("fused", "graph")}
    rng = np.random.default_rng(5)
    bias = np.zeros(V, dtype=np.float32)
    bias[rng.permutation(V)[:V // 4]] = -np.inf
    bias[rng.permutation(V)[:50]] = 2.5
    listed = {int(i): float(bias[i]) for i in np.flatnonzero(bias != 0)}
    try:
        for g in models.values():
            g.prefill(PROMPT)
        tok, pos, q = TOKENS[7], len(PROMPT), 0
        partial = forbidden_seen = 0
        for step, (T, with_bias) in enumerate(((4, False), (4, True), (2, True), (3, False))):
            for g in models.values():
                g.set_token_bias(listed if with_bias else None)
            table_of = lambda s: A.mask(_mod3().class_of, _mod3().next, s, bias if with_bias else None)
            draws = rng.uniform(0, 1, T).astype(np.float32)
            # drafts: allowed in their states but (almost surely) not the samples; round by round one more is set to the sample just seen.  In step 0 the second
            # draft is FORBIDDEN in its state at first: acceptance must end in front of it whatever row 1 samples
            drafts = [tok] + [int(3 * rng.integers(1, V // 3 - 1) + (q + t) % 3) for t in range(T - 1)]
            if step == 0:
                drafts[2] += 1
            for rounds in range(T + 1):
                a = _mod3(start=q)
                qs = _states(a, q, drafts)
                out = {}
                for m, g in models.items():
                    g.set_token_automaton(a)      # the same size: the state back to q, row 0 composed for it, no capture
                    out[m] = g.decode_chain(drafts, pos, m, **({} if sampling is None else dict(sampling=sampling, draws=draws)))
                (lf, cf, af, pf), (lg, cg, ag, pg) = out["fused"], out["graph"]
                what = "step %d round %d drafts %s states %s" % (step, rounds, drafts, qs)
                assert (cf, af, pf) == (cg, ag, pg), (what, out["fused"][1:], out["graph"][1:])
                assert np.array_equal(lf.view(np.uint32), lg.view(np.uint32)), "%s: the eager chain step differs from the graph replay" % what
                s = [_one_row(lg[t], table_of(qs[t]), sampling, draws[t]) for t in range(cg)]
                assert ag == s, (what, ag, s)
                assert all(np.isfinite(table_of(qs[t])[s[t]]) for t in range(cg)), what
                assert 1 <= cg <= T and pg == pos + cg, (what, cg, pg)
                assert all(s[t] == drafts[t + 1] for t in range(cg - 1)), (what, s, drafts)
                q_after = a.step(qs[cg - 1], s[cg - 1])
                for m, g in models.items():
                    assert g.token_automaton_state() == q_after, (what, m)
                if cg < T and not a.allowed(qs[cg - 1])[drafts[cg]]:
                    forbidden_seen += 1
                if cg == T:
                    break
                assert s[cg - 1] != drafts[cg], (what, s, drafts)
                partial += 1
                drafts[cg] = s[cg - 1]
            assert cg == T, "T + 1 rounds did not reach a fully accepted run"
            tok, pos, q = ag[-1], pg, q_after
        assert partial > 0 and forbidden_seen > 0
        info = models["graph"].chain_graph_info()
        # captures: T = 4 with the automaton; the bias on; T = 2; T = 3 with the bias off -- never one for a round, a reset or a replaced automaton
        assert info["captures"] == 4, info
        assert models["fused"].chain_graph_info()["captures"] == 0
        # the automaton off: one more capture, and the unconstrained step again
        g = models["graph"]
        g.set_token_automaton(None)
        logits, count, accepted, new_pos = g.decode_chain([tok, 0], pos, "graph")
        assert g.chain_graph_info()["captures"] == 5 and accepted[0] == int(np.argmax(logits[0]))
    finally:
        for g in models.values():
            g.close()


def test_a_bias_table_alone_in_the_chain_step_and_its_updates_capture_nothing():
    g = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=2)
    try:
        g.prefill(PROMPT)
        tok, pos = TOKENS[7], len(PROMPT)
        logits, count, accepted, pos1 = g.decode_chain([tok, 1, 2], pos, "graph")
        top = accepted[0]
        assert g.chain_graph_info()["captures"] == 1
        g.set_token_bias({top: -np.inf})
        table = np.zeros(V, dtype=np.float32)
        table[top] = -np.inf
        l2, c2, a2, p2 = g.decode_chain([tok, 1, 2], pos, "graph")
        assert np.array_equal(l2[0].view(np.uint32), logits[0].view(np.uint32)) and a2[0] == _one_row(l2[0], table, None, 0.0) != top
        assert g.chain_graph_info()["captures"] == 2
        g.set_token_bias({top: -np.inf, a2[0]: -np.inf})      # another table: the same nodes
        table[a2[0]] = -np.inf
        l3, c3, a3, p3 = g.decode_chain([tok, 1, 2], pos, "graph")
        assert a3[0] == _one_row(l3[0], table, None, 0.0) and a3[0] not in (top, a2[0]) and g.chain_graph_info()["captures"] == 2
        lf, cf, af, pf = g.decode_chain([tok, 1, 2], pos, "fused")
        assert (cf, af, pf) == (c3, a3, p3) and np.array_equal(lf.view(np.uint32), l3.view(np.uint32))
    finally:
        g.close()


# ---- GemmaModel.generate(speculate_constrained=True)
class _Pair:
    def __init__(self, policy, k):
        kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED)
        self.plain, self.spec = host.GemmaModel.synthetic(policy, SMALL, **kw), host.GemmaModel.synthetic(policy, SMALL, draft_tokens=k, **kw)

    def both(self, prompt, hint="true", stochastic=False, **req):
        """the request on the plain model, then with the flag on the draft model (hint "true": the plain tokens as the drafter's; None: the prompt lookup): the same
        tokens, finish reason and final state; a stochastic request is followed by an unseeded one on both.  The two models are sent the same requests in the same
        order, so that both reuse the same KV prefix (a prefill of another length has other bits under fp4).  -> (plain result, the speculative loop's counters)"""
        if stochastic:
            req = dict(temperature=0.9, top_k=12, top_p=0.9, **req)
        ref = self.plain.generate(prompt, **req)
        got = self.spec.generate(prompt, draft_hint=ref[0] if hint == "true" else None, speculative_sampling=stochastic, speculate_constrained=True, **req)
        assert got[:2] == ref[:2], (hint, req, got, ref)
        if req.get("automaton") is not None:
            assert got[-1] == ref[-1] == self.plain.last_automaton_state() == self.spec.last_automaton_state(), (req, got[-1], ref[-1])
        stats = self.spec.speculation_stats_forced()
        if stochastic:
            follow = dict(req, seed=None, max_new_tokens=5)
            if "min_tokens" in follow:
                follow["min_tokens"] = min(follow["min_tokens"], 5)
            ref2 = self.plain.generate(prompt, **follow)
            got2 = self.spec.generate(prompt, speculative_sampling=True, speculate_constrained=True, **follow)
            assert got2[:2] == ref2[:2], "the generator state differs after %s: %s != %s" % (req, got2, ref2)
        self.got = got
        return ref, stats

    def close(self):
        self.plain.close()
        self.spec.close()


def _forced_runs(stop_last=False):
    """free, forced, forced, forced, repeating: state 0 allows everything but the three forced tokens, states 1 .. 3 one token each"""
    forced = [40, 500, S_TOK if stop_last else 77]
    class_of = np.zeros(V, dtype=np.uint16)
    for i, t in enumerate(forced):
        class_of[t] = i + 1
    nxt = np.full((4, 4), F, dtype=np.uint16)
    nxt[0, 0] = 1
    for i in range(3):
        nxt[i + 1, i + 1] = (i + 2) % 4
    return host.TokenAutomaton(class_of, nxt), forced


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("policy", ["bf16", "fp4"])
def test_the_constrained_speculative_loop_gives_the_plain_loop_s_tokens(policy, k):
    p = _Pair(policy, k)
    prompt = TOKENS[:6]
    try:
        free = p.plain.generate(prompt, max_new_tokens=14, stop_tokens=NEVER)[0]
        assert p.spec.generate(prompt, max_new_tokens=14, stop_tokens=NEVER)[0] == free
        stop = free[2]      # a stop token the unconstrained greedy run meets at its third token
        constraints = [dict(automaton=_mod3()), dict(logit_bias={free[0]: -4.0, 17: 3.0}, banned_tokens=[free[1], free[3]]),
                       dict(allowed_tokens=sorted(set(free[:6] + [9, 10, 11, 400, 401]))), dict(automaton=_mod3(), banned_tokens=[free[0], 3, 4, 5], logit_bias={7: 2.0})]
        chained = 0
        for stochastic in (False, True):
            for c in constraints:
                for hint in ("true", None):
                    ref, st = p.both(prompt, hint=hint, stochastic=stochastic, max_new_tokens=14, stop_tokens=NEVER, seed=3, **c)
                    assert len(ref[0]) == 14 and st["steps"] >= st["chain_steps"] and st["accepted"] <= st["drafted"], st
                    if hint == "true":
                        assert st["chain_steps"] > 0 and st["accepted"] > 0, (c, st)
                        chained += 1
            for n in (1, 4, 11):
                for hint in ("true", None):
                    ref, st = p.both(prompt, hint=hint, stochastic=stochastic, max_new_tokens=14, stop_tokens=[stop], min_tokens=n, seed=3)
                    assert stop not in ref[0][:n] and (ref[1] == "length" or len(ref[0]) >= n), (n, ref)
                    if hint == "true" and len(ref[0]) > k + 2:
                        assert st["chain_steps"] > 0, (n, st)
        assert chained == 8
        # an unconstrained request afterwards gives the plain model's tokens (no table and no state is left behind), and still speculates
        again = p.plain.generate(prompt, max_new_tokens=14, stop_tokens=NEVER)
        assert p.spec.generate(prompt, max_new_tokens=14, stop_tokens=NEVER, draft_hint=again[0])[:2] == again[:2] and again[1] == "length"
        assert p.spec.speculation_stats()["chain_steps"] > 0 and p.spec.last_automaton_state() is None
    finally:
        p.close()


@pytest.mark.parametrize("k", [2, 3])
def test_forced_runs_are_drafted_for_free_and_always_accepted(k):
    p = _Pair("bf16", k)
    prompt = TOKENS[:6]
    try:
        a, forced = _forced_runs()
        assert a.forced_tokens().tolist() == [-1] + forced
        refs = {}
        for stochastic in (False, True):
            ref, st = p.both(prompt, hint=None, stochastic=stochastic, max_new_tokens=16, stop_tokens=NEVER, seed=3, automaton=a)
            assert ref[0][1:4] == forced and ref[0][5:8] == forced and len(ref[0]) == 16
            assert st["chain_steps"] > 0 and st["forced_accepted"] == st["forced"] > 0, st
            # 15 tokens behind the eager first one, 12 of them forced: at most one step per free token and one per run of k forced ones -- never one per token
            assert st["forced"] >= 6 and st["steps"] <= 9, st
            refs[stochastic] = ref
        # with the flag off: the plain loop
        got = p.spec.generate(prompt, max_new_tokens=16, stop_tokens=NEVER, seed=3, automaton=a)
        assert got == p.plain.generate(prompt, max_new_tokens=16, stop_tokens=NEVER, seed=3, automaton=a) and got[:2] == refs[False][:2]
        assert p.spec.speculation_stats()["chain_steps"] == 0 and p.spec.speculation_stats_forced()["forced"] == 0
        # a forced run that ends in the stop token stops there
        a, forced = _forced_runs(stop_last=True)
        ref, st = p.both(prompt, hint=None, max_new_tokens=16, stop_tokens=[S_TOK], automaton=a)
        assert ref[:2] == (ref[0][:1] + forced[:2], "stop") and ref[-1] == 0, ref
        assert st["forced"] == st["forced_accepted"] == min(k, 3) and st["steps"] == 1, st      # the run is cut at k drafts; its last token is row k's sample
    finally:
        p.close()


def test_log_probabilities_under_the_flag_are_the_plain_loop_s_records():
    p = _Pair("bf16", 3)
    prompt = TOKENS[:6]
    try:
        a, forced = _forced_runs()
        for c in (dict(automaton=a), dict(automaton=_mod3(), banned_tokens=[3, 4, 5])):
            ref, st = p.both(prompt, hint="true", max_new_tokens=10, stop_tokens=NEVER, logprobs=3, **c)
            got = p.got
            assert st["chain_steps"] > 0 and len(got[3]) == len(ref[3]) == 10
            for (lp0, ids0, tlp0), (lp1, ids1, tlp1) in zip(ref[3], got[3]):
                assert np.float32(lp0).view(np.uint32) == np.float32(lp1).view(np.uint32) and np.array_equal(ids0, ids1)
                assert np.array_equal(tlp0.view(np.uint32), tlp1.view(np.uint32))
    finally:
        p.close()
