"""GPU: GemmaModel::generateRequests (host.GemmaModel.generate_requests) -- a batch whose rows each carry their own request.  THE CONTRACT is the oracle: row b gives,
token for token, what generate() gives for request b ALONE on a max_batch = 1 model of the same weights after the same seed -- tokens, finish reason,
log-probability bits and the final automaton state -- whatever the other rows carry.  Every position here lies in one live-length bucket."""
import numpy as np
import pytest

import ref_token_automaton as A
from mila_amd import host
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_rows_gpu import NEW_PROMPT, PROMPTS, SEED

pytestmark = pytest.mark.gpu

V = SMALL["vocab_size"]
F = A.FORBIDDEN
FOUR = [PROMPTS[0], PROMPTS[1], PROMPTS[2], NEW_PROMPT]


def _models(policy="bf16"):
    kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED)
    return host.GemmaModel.synthetic(policy, SMALL, **kw), host.GemmaModel.synthetic(policy, SMALL, max_batch=4, **kw)


def _mod3():
    """state k allows the ids = k (mod 3) and goes to k + 1 (mod 3)"""
    nxt = np.full((3, 3), F, dtype=np.uint16)
    for k in range(3):
        nxt[k, k] = (k + 1) % 3
    return host.TokenAutomaton((np.arange(V) % 3).astype(np.uint16), nxt)


def _halves():
    """two states: state 0 allows the lower half of the vocabulary, state 1 the upper half"""
    class_of = (np.arange(V) >= V // 2).astype(np.uint16)
    return host.TokenAutomaton(class_of, np.array([[1, F], [F, 0]], dtype=np.uint16))


def _alone(model, q, logprobs=None):
    """generate() for one request dict -> what generate_requests reports for its row"""
    kw = {k: v for k, v in q.items() if k != "prompt"}
    kw.setdefault("seed", 0)
    out = model.generate(q["prompt"], logprobs=logprobs, **kw)
    row = (out[0], out[1])
    if logprobs is not None:
        row = row + (out[3],)
    if q.get("automaton") is not None:
        row = row + (out[-1],)
    return row


def _same_row(got, want, with_lp):
    assert got[0] == want[0] and got[1] == want[1], (got[:2], want[:2])
    k = 2
    if with_lp:
        assert len(got[2]) == len(want[2]) == len(got[0])
        for (l0, i0, t0), (l1, i1, t1) in zip(got[2], want[2]):
            assert np.float32(l0).view(np.uint32) == np.float32(l1).view(np.uint32)
            assert np.array_equal(i0, i1) and np.array_equal(np.asarray(t0).view(np.uint32), np.asarray(t1).view(np.uint32))
        k = 3
    assert got[k:] == want[k:], (got[k:], want[k:])


def _mixed(alone):
    """greedy with an automaton; stochastic with a bias and min_tokens; stochastic with penalties and min_p; plain greedy"""
    st = dict(temperature=0.9, top_k=12, top_p=0.9)
    free = alone.generate(FOUR[1], max_new_tokens=8, seed=11, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17], **st)[0]
    return [dict(prompt=FOUR[0], max_new_tokens=7, automaton=_mod3()),
            dict(prompt=FOUR[1], max_new_tokens=8, seed=11, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17], min_tokens=3, stop_tokens=[free[1]], **st),
            dict(prompt=FOUR[2], max_new_tokens=9, seed=23, temperature=1.1, top_k=40, top_p=0.95, min_p=0.02, repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1),
            dict(prompt=FOUR[3], max_new_tokens=6)]


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_a_mixed_batch_gives_each_row_what_generate_gives_it_alone(policy):
    alone, batch = _models(policy)
    try:
        reqs = _mixed(alone)
        want = [_alone(alone, q) for q in reqs]
        got = batch.generate_requests(reqs)
        for b in range(4):
            _same_row(got[b], want[b], False)
        assert isinstance(got[0][-1], int) and len(got[1][0]) >= 3, got      # a final state for the automaton row; min_tokens kept row 1 going
        assert all(t % 3 == i % 3 for i, t in enumerate(got[0][0])), got[0]
        # the same requests permuted over the rows: the permuted results -- no row sees its neighbours
        perm = [2, 0, 3, 1]
        again = batch.generate_requests([reqs[i] for i in perm])
        for b, i in enumerate(perm):
            _same_row(again[b], want[i], False)
        # fewer requests than rows, and one request (a rows step still carries two rows)
        _same_row(batch.generate_requests(reqs[1:2])[0], want[1], False)
        two = batch.generate_requests(reqs[:2])
        _same_row(two[0], want[0], False)
        _same_row(two[1], want[1], False)
    finally:
        alone.close()
        batch.close()


def test_rows_end_at_their_own_stop_sets_and_limits():
    """one row ends at its first token, one at max_new_tokens = 1, the others run on under different stop sets"""
    alone, batch = _models()
    try:
        first = [alone.generate(p, max_new_tokens=5)[0] for p in FOUR]
        reqs = [dict(prompt=FOUR[0], max_new_tokens=6, stop_tokens=[first[0][0]]),
                dict(prompt=FOUR[1], max_new_tokens=1),
                dict(prompt=FOUR[2], max_new_tokens=6, stop_tokens=[first[2][3], 1]),
                dict(prompt=FOUR[3], max_new_tokens=6, stop_tokens=[1], temperature=0.8, top_k=0, top_p=0.9, seed=3)]
        want = [_alone(alone, q) for q in reqs]
        got = batch.generate_requests(reqs)
        for b in range(4):
            _same_row(got[b], want[b], False)
        assert got[0] == ([], "stop") and got[1][1] == "length" and len(got[1][0]) == 1 and got[2][1] == "stop" and len(got[2][0]) <= 3, got
    finally:
        alone.close()
        batch.close()


def test_log_probabilities_carry_the_bits_of_the_row_alone():
    alone, batch = _models()
    try:
        reqs = _mixed(alone)
        want = [_alone(alone, q, logprobs=3) for q in reqs]
        got = batch.generate_requests(reqs, logprobs=3)
        for b in range(4):
            _same_row(got[b], want[b], True)
    finally:
        alone.close()
        batch.close()


def test_parameters_of_one_class_replay_the_captured_graph():
    """the sampler parameters are device words: a second call with other parameters of the same classes captures nothing; a change of class adds one capture"""
    _, batch = _models()
    try:
        a = [dict(prompt=FOUR[0], max_new_tokens=5), dict(prompt=FOUR[1], max_new_tokens=5, temperature=0.9, top_k=12, top_p=0.9, seed=1),
             dict(prompt=FOUR[2], max_new_tokens=5, temperature=0.7, top_k=0, top_p=0.8, seed=2)]
        b = [dict(prompt=FOUR[0], max_new_tokens=5), dict(prompt=FOUR[1], max_new_tokens=5, temperature=1.4, top_k=0, top_p=1.0, min_p=0.1, seed=9),
             dict(prompt=FOUR[2], max_new_tokens=5, temperature=0.5, top_k=3, top_p=0.99, seed=8)]
        batch.generate_requests(a)
        n = batch.rows_graph_info()["captures"]
        assert n >= 1
        batch.generate_requests(b)
        assert batch.rows_graph_info()["captures"] == n, "other parameters of the same classes captured the rows graph again"
        batch.generate_requests([dict(q, temperature=0.9, top_k=5, top_p=0.9) for q in a])      # no greedy row any more: a class fact
        assert batch.rows_graph_info()["captures"] == n + 1
        batch.generate_requests([dict(q, temperature=0.6, top_k=7, top_p=0.8) for q in a])
        assert batch.rows_graph_info()["captures"] == n + 1
        batch.generate_requests([dict(a[0], automaton=_mod3())] + a[1:])                         # a constrained row with an automaton: a class fact
        assert batch.rows_graph_info()["captures"] == n + 2
        batch.generate_requests([dict(a[0], automaton=_halves())] + b[1:])                       # another automaton, other parameters: the same classes
        assert batch.rows_graph_info()["captures"] == n + 2
    finally:
        batch.close()


def test_generate_batch_keeps_its_contract_beside_it():
    alone, batch = _models()
    try:
        kw = dict(max_new_tokens=6, temperature=0.9, top_k=12, top_p=0.9)
        before = batch.generate_batch(FOUR[:3], seed=31, **kw)
        batch.generate_requests(_mixed(alone))
        assert batch.generate_batch(FOUR[:3], seed=31, **kw) == before
        assert tuple(batch.generate_batch(FOUR[1:2], seed=31, **kw)[0]) == tuple(alone.generate(FOUR[1], seed=31, **kw)[:2])
        greedy = batch.generate_batch(FOUR[:3], max_new_tokens=6)
        assert [tuple(g) for g in greedy] == [tuple(alone.generate(p, max_new_tokens=6)[:2]) for p in FOUR[:3]]
        with pytest.raises(ValueError):
            batch.generate_batch(FOUR[:2], max_new_tokens=2, automaton=_mod3())
    finally:
        alone.close()
        batch.close()


def test_refusals_raise_before_anything_is_enqueued():
    alone, batch = _models()
    try:
        ok = [dict(prompt=FOUR[0], max_new_tokens=3), dict(prompt=FOUR[1], max_new_tokens=3, temperature=0.9, top_k=12, top_p=0.9, seed=4)]
        want = batch.generate_requests(ok)
        n = batch.rows_graph_info()["captures"]
        dead = host.TokenAutomaton(np.zeros(V, dtype=np.uint16), np.array([[1], [F]], dtype=np.uint16))      # state 1 allows nothing
        narrow = _halves()
        bad = [[ok[0], dict(ok[1], logprobs=2)],                                     # differing logprobs
               [ok[0], dict(ok[1], speculative_sampling=True)],
               [ok[0], dict(ok[1], speculate_constrained=True)],
               [ok[0], dict(ok[1], draft_hint=[1, 2])],
               [ok[0], dict(ok[1], repetition_penalty=0.0)],                         # a bad row parameter
               [ok[0], dict(ok[1], top_p=0.0)],
               [ok[0], dict(ok[1], temperature=float("nan"))],
               [ok[0], dict(ok[1], prompt=[])],
               [ok[0], dict(ok[1], prompt=[V])],
               ok + ok + ok[:1],                                                     # five requests
               [dict(ok[0], automaton=dead), ok[1]],                                 # a reachable state that allows nothing
               [ok[0], dict(ok[1], automaton=narrow, banned_tokens=list(range(V // 2, V)))],      # ... no token with a finite bias in state 1
               [ok[0], dict(ok[1], automaton=narrow, min_tokens=1)]]
        for reqs in bad:
            with pytest.raises(ValueError):
                batch.generate_requests(reqs)
        with pytest.raises(ValueError, match="row 1"):
            batch.generate_requests([ok[0], dict(ok[1], top_p=0.0)])
        with pytest.raises(ValueError):
            alone.generate_requests(ok)                                              # a one-sequence model
        assert batch.generate_requests(ok) == want and batch.rows_graph_info()["captures"] == n
    finally:
        alone.close()
        batch.close()


def test_the_requests_step_eager_and_replayed_and_what_it_allocates():
    """the low-level surface (host.Gemma.set_rows_requests / set_row_token_bias / set_row_token_automaton): the eager requests step equals the graph replay, every active
    row advances once per step, new parameters of the same classes replay the capture, and what the requests allocated is counted"""
    kw = dict(max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4)
    models = {m: host.Gemma("bf16", SMALL, **kw) for m in ("fused", "graph")}
    fresh = host.Gemma("bf16", SMALL, **kw)
    mem = lambda g: {k: v for k, v in g.memory_stats().items() if k != "scratch_bytes"}
    try:
        base = mem(fresh)
        reqs = [dict(temperature=0.0), dict(temperature=0.9, top_k=12, top_p=0.9), dict(temperature=1.1, top_k=40, top_p=0.95, min_p=0.02, repetition_penalty=1.3, presence_penalty=0.2),
                dict()]
        for g in models.values():
            assert mem(g) == base
            for b, p in enumerate(FOUR):
                g.prefill_row(b, p)
                g.set_active(b, True, token=7 + b)
            g.set_row_token_automaton(0, _mod3())
            g.set_row_token_bias(1, {5: 2.0, 17: float("-inf")})
            g.set_rows_requests(reqs, draws=[0.5] * 4)
        start = [len(p) for p in FOUR]
        rng = np.random.default_rng(3)
        for step in range(6):
            if step == 3:      # other parameters of the same classes: device words, no capture
                for g in models.values():
                    g.set_rows_requests([dict(temperature=-1.0), dict(temperature=0.5, top_k=3, top_p=0.99), dict(temperature=0.7, min_p=0.1, frequency_penalty=0.4), dict()])
            draws = rng.random(4).astype(np.float32)
            out = {m: g.decode_rows(4, max(start) + step, m, greedy=False, sampling=(1.0, 0, 1.0), draws=draws) for m, g in models.items()}
            (_, ft, fp), (_, gt, gp) = out["fused"], out["graph"]
            assert ft.tolist() == gt.tolist() and fp.tolist() == gp.tolist(), (step, ft, gt)
            assert gp.tolist() == [s + step + 1 for s in start], "a row advanced twice or not at all"
            assert int(gt[0]) % 3 == step % 3 and int(gt[1]) != 17, gt
            assert models["graph"].row_token_automaton_state(0) == (step + 1) % 3 and models["graph"].row_token_automaton_state(1) is None
        assert models["graph"].rows_graph_info()["captures"] == 1 and models["fused"].rows_graph_info()["captures"] == 0
        ms = mem(models["graph"])
        assert ms["required"] == ms["actual"] and ms["actual"]["device_state_bytes"] > base["actual"]["device_state_bytes"]
        with pytest.raises(ValueError):
            models["graph"].set_rows_requests([dict(temperature=0.9, top_p=0.0)])
        with pytest.raises(ValueError):
            models["graph"].set_rows_requests([dict()] * 5)
        models["graph"].set_rows_requests(None)      # the shared-parameter step again: one more capture, the parent's node count
        models["graph"].decode_rows(4, max(start) + 6, "graph")
        fresh.decode_rows(4, 0, "graph")
        assert models["graph"].rows_graph_info()["captures"] == 2 and models["graph"].rows_graph_info()["nodes"] == fresh.rows_graph_info()["nodes"]
    finally:
        for g in list(models.values()) + [fresh]:
            g.close()
