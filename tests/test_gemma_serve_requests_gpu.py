"""GPU: GemmaModel::serveRequests (host.GemmaModel.serve_requests) -- a FIFO queue in front of the rows step: more requests than rows, a retired row handed to the next
waiting request, identical prompts admitted together sharing one prefill.  THE CONTRACT is the oracle: request i gives, token for token, what generate() gives for it
ALONE on a max_batch = 1 model of the same weights after its seed -- tokens, finish reason, log-probability bits, final automaton state -- whatever the other requests
are, whichever row it landed in, whenever it was admitted, prefilled or forked.  Every position here lies in one live-length bucket (MAX_SEQ = 64)."""
import pytest

from mila_amd import host
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_row_requests_gpu import FOUR, _mod3, _same_row
from test_gemma_rows_gpu import SEED

pytestmark = pytest.mark.gpu

V = SMALL["vocab_size"]
P15 = FOUR[2]                       # longer than the window of 8: a fork carries a local layer's whole live band
ST = dict(temperature=0.9, top_k=12, top_p=0.9)


@pytest.fixture(scope="module")
def models():
    """(policy, max_batch) -> model, built on first use and shared by the tests of this file (a call leaves nothing behind that the next one reads)"""
    built = {}

    def get(policy, max_batch):
        if (policy, max_batch) not in built:
            kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED)
            if max_batch > 1:
                kw["max_batch"] = max_batch
            built[policy, max_batch] = host.GemmaModel.synthetic(policy, SMALL, **kw)
        return built[policy, max_batch]
    yield get
    for m in built.values():
        m.close()


def _fresh(model, q, logprobs=None):
    """generate() for one request dict on the one-sequence model -> what serve_requests reports for it.  generate() reuses the KV prefix it shares with the run before,
    and re-prefilling the one position behind a reused prefix takes another GEMM form than a whole prompt (with fp8 weights: other bits), so a run on a prompt that
    starts with another token goes first: the oracle prefills the whole prompt, as every admission does."""
    model.generate([V - 1], max_new_tokens=1)
    kw = {k: v for k, v in q.items() if k != "prompt"}
    kw.setdefault("seed", 0)
    out = model.generate(q["prompt"], logprobs=logprobs, **kw)
    assert out[2] == 0, "the oracle reused %d cached positions" % out[2]
    row = (out[0], out[1])
    if logprobs is not None:
        row = row + (out[3],)
    if q.get("automaton") is not None:
        row = row + (out[-1],)
    return row


def _seven(alone):
    """a greedy automaton request; a stochastic one with a bias and min_tokens; a stochastic one with penalties and min-p; plain greedy ones; one with
    max_new_tokens = 1; one ending at its first token; prompt lengths 3, 5, 9 and 15"""
    free = alone.generate(FOUR[1], max_new_tokens=8, seed=11, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17], **ST)[0]
    first = alone.generate(FOUR[3], max_new_tokens=1)[0][0]
    return [dict(prompt=FOUR[0], max_new_tokens=7, automaton=_mod3()),
            dict(prompt=FOUR[1], max_new_tokens=8, seed=11, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17], min_tokens=3, stop_tokens=[free[1]], **ST),
            dict(prompt=P15, max_new_tokens=9, seed=23, temperature=1.1, top_k=40, top_p=0.95, min_p=0.02, repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1),
            dict(prompt=FOUR[3], max_new_tokens=6),
            dict(prompt=FOUR[1], max_new_tokens=1),
            dict(prompt=FOUR[3], max_new_tokens=6, stop_tokens=[first]),
            dict(prompt=P15, max_new_tokens=5)]


def _samples(row):
    """the samples a finished request drew: its tokens, plus the stop token that ended it"""
    return len(row[0]) + (1 if row[1] == "stop" else 0)


def _simulate(R, samples):
    """the admission rule, in Python: FIFO, lowest free row, a request whose first sample ends it frees its row in the same round; a request of s samples holds its
    row for s - 1 steps (the first sample comes with the admission) -> (steps, [(row, admitted_at)] per request)"""
    n, rows, left, placed = len(samples), [None] * R, [0] * R, []
    state = dict(next=0, steps=0)

    def admission_round():
        while True:
            wave = []
            for b in range(R):
                if rows[b] is None and state["next"] < n:
                    rows[b] = state["next"]
                    placed.append((b, state["steps"]))
                    wave.append(b)
                    state["next"] += 1
            if not wave:
                return
            for b in wave:
                left[b] = samples[rows[b]] - 1
                if left[b] <= 0:
                    rows[b] = None

    admission_round()
    while any(r is not None for r in rows):
        state["steps"] += 1
        for b in range(R):
            if rows[b] is not None:
                left[b] -= 1
                if left[b] <= 0:
                    rows[b] = None
        admission_round()
    return state["steps"], placed


def _check_placement(R, got, stats):
    steps, placed = _simulate(R, [_samples(r) for r in got])
    assert stats["steps"] == steps, (stats, steps)
    assert list(zip(stats["rows"], stats["admitted_at"])) == placed, (stats, placed)
    assert sorted(stats["finish_order"]) == list(range(len(got))), stats      # on_finish fired once per request


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_seven_mixed_requests_on_three_rows_each_as_alone_in_any_order(models, policy):
    alone, batch = models(policy, 1), models(policy, 3)
    reqs = _seven(alone)
    want = [_fresh(alone, q) for q in reqs]
    got, stats = batch.serve_requests(reqs)
    assert len(got) == 7
    for i in range(7):
        _same_row(got[i], want[i], False)
    assert got[5][:2] == ([], "stop") and got[4][1] == "length" and len(got[4][0]) == 1, got      # zero tokens; max_new_tokens = 1
    assert isinstance(got[0][-1], int) and len(got[1][0]) >= 3 and all(t % 3 == i % 3 for i, t in enumerate(got[0][0])), got
    assert stats["prefills"] == 7 and stats["forks"] == 0 and stats["prefill_tokens"] == sum(len(q["prompt"]) for q in reqs)
    assert stats["rows"][:3] == [0, 1, 2] and stats["admitted_at"][:3] == [0, 0, 0] and max(stats["admitted_at"]) > 0
    _check_placement(3, got, stats)
    for perm in ([6, 5, 4, 3, 2, 1, 0], [2, 4, 0, 6, 1, 5, 3]):
        again, st = batch.serve_requests([reqs[i] for i in perm])
        for j, i in enumerate(perm):
            _same_row(again[j], want[i], False)
        _check_placement(3, again, st)


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_log_probabilities_carry_the_bits_of_the_request_alone(models, policy):
    alone, batch = models(policy, 1), models(policy, 3)
    reqs = _seven(alone)
    want = [_fresh(alone, q, logprobs=3) for q in reqs]
    got, _ = batch.serve_requests(reqs, logprobs=3)
    for i in range(7):
        _same_row(got[i], want[i], True)
    again, _ = batch.serve_requests(reqs[::-1], logprobs=3)
    for i in range(7):
        _same_row(again[6 - i], want[i], True)


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_identical_prompts_admitted_together_share_one_prefill(models, policy):
    alone, batch = models(policy, 1), models(policy, 4)
    base = dict(prompt=P15, seed=5, repetition_penalty=1.3, max_new_tokens=8, **ST)
    want = [_fresh(alone, dict(base, seed=s)) for s in (5, 6, 7)]
    assert len({tuple(w[0]) for w in want}) > 1, "the three seeds must not agree, or a fork that copied the sampler too would pass"
    got, stats = batch.serve_requests([dict(base, n=3)])
    assert len(got) == 3
    for i in range(3):
        _same_row(got[i], want[i], False)
    assert (stats["prefills"], stats["prefill_tokens"], stats["forks"]) == (1, 15, 2), stats
    assert stats["rows"] == [0, 1, 2] and stats["admitted_at"] == [0, 0, 0]
    # a fourth, different request queued behind them (a greedy one with an automaton: nothing of it is shared), and log-probabilities through a fork
    other = dict(prompt=FOUR[1], max_new_tokens=7, automaton=_mod3())
    got, stats = batch.serve_requests([dict(base, n=3), other])
    for i in range(3):
        _same_row(got[i], want[i], False)
    _same_row(got[3], _fresh(alone, other), False)
    assert (stats["prefills"], stats["prefill_tokens"], stats["forks"]) == (2, 15 + len(FOUR[1]), 2), stats
    want_lp = [_fresh(alone, dict(base, seed=s), logprobs=3) for s in (5, 6, 7)]
    got, _ = batch.serve_requests([dict(base, n=3)], logprobs=3)
    for i in range(3):
        _same_row(got[i], want_lp[i], True)
    # on two rows the third copy arrives after a step: it prefills for itself
    two = models(policy, 2)
    got, stats = two.serve_requests([dict(base, n=3)])
    for i in range(3):
        _same_row(got[i], want[i], False)
    assert (stats["prefills"], stats["prefill_tokens"], stats["forks"]) == (2, 30, 1), stats


def test_the_same_prompt_in_different_rounds_is_prefilled_twice(models):
    alone, batch = models("bf16", 1), models("bf16", 2)
    reqs = [dict(prompt=P15, max_new_tokens=4, seed=3, **ST), dict(prompt=FOUR[0], max_new_tokens=3), dict(prompt=FOUR[1], max_new_tokens=5), dict(prompt=FOUR[3], max_new_tokens=2),
            dict(prompt=FOUR[0], max_new_tokens=4, seed=9, **ST), dict(prompt=P15, max_new_tokens=6, seed=4, **ST)]
    got, stats = batch.serve_requests(reqs)
    for i, q in enumerate(reqs):
        _same_row(got[i], _fresh(alone, q), False)
    assert stats["forks"] == 0 and stats["prefills"] == 6 and stats["prefill_tokens"] == sum(len(q["prompt"]) for q in reqs), stats
    assert stats["admitted_at"][5] > stats["admitted_at"][0] == 0


def test_the_steps_are_those_of_the_admission_rule_and_fewer_than_in_groups(models):
    """arithmetic on lengths, no timing: the rows steps of the call = the Python simulation of the rule on the requests' alone-lengths, and fewer than the same requests
    cost in arrival-order groups of R, each group running as long as its longest member"""
    alone, batch = models("bf16", 1), models("bf16", 2)
    R, lengths = 2, [2, 9, 3, 4, 2, 7, 8, 2]
    prompts = [FOUR[i % 4] for i in range(len(lengths))]
    free = [alone.generate(p, max_new_tokens=n)[0] for p, n in zip(prompts, lengths)]
    never = [t for t in range(V) if all(t not in f for f in free)][:2]      # a stop set the alone runs never produce: every request ends at its max_new_tokens
    reqs = [dict(prompt=p, max_new_tokens=n, stop_tokens=never) for p, n in zip(prompts, lengths)]
    want = [_fresh(alone, q) for q in reqs]
    assert [len(w[0]) for w in want] == lengths and all(w[1] == "length" for w in want)
    got, stats = batch.serve_requests(reqs)
    for i in range(len(reqs)):
        _same_row(got[i], want[i], False)
    steps, placed = _simulate(R, [_samples(w) for w in want])
    assert stats["steps"] == steps and list(zip(stats["rows"], stats["admitted_at"])) == placed, (stats, steps, placed)
    grouped = sum(max(lengths[g:g + R]) for g in range(0, len(lengths), R))
    grouped_steps = sum(max(lengths[g:g + R]) - 1 for g in range(0, len(lengths), R))      # a group's first tokens come with its prefills, as a request's does here
    assert steps < grouped_steps < grouped, (steps, grouped_steps, grouped)


def test_admission_never_captures_within_a_class_and_generate_requests_keeps_its_limit():
    kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED, max_batch=2)
    a, b = host.GemmaModel.synthetic("bf16", SMALL, **kw), host.GemmaModel.synthetic("bf16", SMALL, **kw)
    try:
        plain = [dict(prompt=FOUR[i % 4], max_new_tokens=3 + i % 4) for i in range(7)]
        with pytest.raises(ValueError, match="3 requests for max_batch 2"):
            a.generate_requests(plain[:3])
        a.generate_requests(plain[:2])
        per_call = a.rows_graph_info()["captures"]
        assert per_call >= 1
        got, stats = b.serve_requests(plain)      # five admissions into retired rows, B = 2 throughout, every request greedy and unconstrained
        assert stats["captures"] == per_call == b.rows_graph_info()["captures"], (stats, per_call)
        _, stats = b.serve_requests([dict(q, max_new_tokens=4) for q in plain[::-1]])
        assert stats["captures"] == 0 and b.rows_graph_info()["captures"] == per_call
        _, stats = b.serve_requests(plain[:3] + [dict(plain[3], seed=2, **ST)] + plain[4:])      # a stochastic request enters a row: a class fact
        assert stats["captures"] >= 1
        assert b.generate_requests(plain[:2]) == a.generate_requests(plain[:2]) == got[:2]      # generate_requests beside it, unchanged
    finally:
        a.close()
        b.close()


def test_refusals_name_the_request_and_come_before_anything_is_enqueued(models):
    alone, batch = models("bf16", 1), models("bf16", 2)
    ok = [dict(prompt=FOUR[i % 4], max_new_tokens=3) for i in range(8)]
    want, _ = batch.serve_requests(ok)
    n = batch.rows_graph_info()["captures"]
    with pytest.raises(ValueError, match="request 6: empty prompt"):
        batch.serve_requests(ok[:6] + [dict(ok[6], prompt=[])] + ok[7:])
    for key, value in (("speculative_sampling", True), ("speculate_constrained", True), ("draft_hint", [1, 2])):
        with pytest.raises(ValueError, match="request 4.*speculative"):
            batch.serve_requests(ok[:4] + [dict(ok[4], **{key: value})] + ok[5:])
    with pytest.raises(ValueError, match="request 7.*logprobs"):
        batch.serve_requests(ok[:7] + [dict(ok[7], logprobs=2)])
    with pytest.raises(ValueError, match="request 3.*logprobs"):
        batch.serve_requests(ok[:3] + [dict(ok[3], logprobs=2)] + ok[4:], logprobs=3)
    with pytest.raises(ValueError, match="request 2: unknown keys"):
        batch.serve_requests(ok[:2] + [dict(ok[2], best_of=2)])
    with pytest.raises(ValueError, match="request 5"):
        batch.serve_requests(ok[:5] + [dict(ok[5], top_p=0.0, temperature=0.9, top_k=0)])
    with pytest.raises(ValueError, match="request 1"):
        batch.serve_requests([ok[0], dict(ok[1], prompt=[V])])
    with pytest.raises(ValueError):
        batch.serve_requests([])
    with pytest.raises(ValueError, match="one sequence"):
        alone.serve_requests(ok[:2])
    again, stats = batch.serve_requests(ok)
    assert again == want and stats["captures"] == 0 and batch.rows_graph_info()["captures"] == n
