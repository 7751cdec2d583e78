"""GPU: the prefix cache of GemmaModel::serveRequests (host.GemmaModel.serve_requests_prefix; Mila/PrefixCache.h holds the rule) -- an admission takes the longest prefix
of its prompt that any row holds, live, retired or its own, by one fork of that prefix and prefills the rest; the claims outlive requests and calls.
THE CONTRACT is the oracle: request i, admitted with reuse L from a chain of donors, gives bit for bit what generate() gives for it on a max_batch = 1 model of the same
weights on which the requests of that chain ran before it, in order, generate() itself reusing L positions (a prefilled suffix takes another GEMM form than a whole
prompt -- with fp8 weights: other bits -- so the reuse path is the oracle, and _after asserts the reuse generate() reports).  Every comparison is exact.
_Rule is the admission rule restated in Python -- the queue (FIFO, lowest free row, the identical-prompt rule) and the claims -- driven by the oracle's own results, as
_simulate in tests/test_gemma_serve_requests_gpu.py is driven by the alone-lengths: it says, per request, the row, the admission step, the donor row, the reuse and the
chain.  Prompts are built so that both sides MUST split at L: the request's token at position L differs from what the donor holds there (generate() decodes one step
ahead, so its history may know the donor's last sample, which a row never does: a split inside decoded tokens uses all of the donor's tokens but the last, then a
different one).  Every position lies in one live-length bucket (MAX_SEQ = 64)."""
import pytest

from mila_amd import host
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_row_requests_gpu import FOUR, _mod3, _same_row
from test_gemma_rows_gpu import SEED
from test_gemma_serve_requests_gpu import _samples

pytestmark = pytest.mark.gpu

V = SMALL["vocab_size"]
P15 = FOUR[2]                                    # longer than the window of 8
P20 = P15 + [33, 701, 2, 555, 64]                # past the prefill chunk of 16
ST = dict(temperature=0.9, top_k=12, top_p=0.9)
TIMES = "admission_ms"


@pytest.fixture(scope="module")
def models():
    """(policy, max_batch) -> model, built on first use and shared by the tests of this file; a test that reads claims starts from clear_prefix_cache()"""
    built = {}

    def get(policy, max_batch):
        if (policy, max_batch) not in built:
            kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED)
            if max_batch > 1:
                kw["max_batch"] = max_batch
            built[policy, max_batch] = host.GemmaModel.synthetic(policy, SMALL, **kw)
        m = built[policy, max_batch]
        if max_batch > 1:
            m.clear_prefix_cache()
        return m
    yield get
    for m in built.values():
        m.close()


def _run(model, q, logprobs, want_reuse):
    kw = {k: v for k, v in q.items() if k != "prompt"}
    kw.setdefault("seed", 0)
    out = model.generate(q["prompt"], logprobs=logprobs, **kw)
    assert out[2] == want_reuse, "the oracle reused %d cached positions, the rule says %d (%r)" % (out[2], want_reuse, q["prompt"])
    row = (out[0], out[1])
    if logprobs is not None:
        row = row + (out[3],)
    if q.get("automaton") is not None:
        row = row + (out[-1],)
    return row


def _after(alone, chain, q, L, logprobs=None):
    """generate() for q on the one-sequence model after the requests of its donor chain [(request, its reuse)], in order, reusing L positions itself"""
    alone.generate([V - 1], max_new_tokens=1)
    for d, l in chain:
        _run(alone, d, logprobs, l)
    return _run(alone, q, logprobs, L)


class _Rule:
    """the rows of a serving model as the rule sees them: per row the claim and the (chain, request, reuse) that wrote it.  serve() runs the queue over a list of
    requests and returns, per request, what serve_requests_prefix must report -- the oracle's row, the row it ran in, its admission step, donor row and reuse -- and
    the call's totals"""

    def __init__(self, R, alone, min_prefix=1, logprobs=None):
        self.R, self.alone, self.min_prefix, self.logprobs = R, alone, min_prefix, logprobs
        self.clear()

    def clear(self):
        self.claim = [[] for _ in range(self.R)]
        self.wrote = [None] * self.R

    def _plan(self, row, prompt):
        m = []
        for h in self.claim:
            k = 0
            while k < min(len(h), len(prompt)) and h[k] == prompt[k]:
                k += 1
            m.append(k)
        L = min(max(m), len(prompt) - 1)
        if L < self.min_prefix:
            return -1, 0
        if m[row] >= L:
            return row, L
        return min(s for s in range(self.R) if m[s] >= L), L

    def serve(self, reqs):
        R, n = self.R, len(reqs)
        rows, fresh, left, fed = [None] * R, [None] * R, [0] * R, [0] * R
        out = [None] * n
        tot = dict(steps=0, prefills=0, prefill_tokens=0, forks=0, prefix_forks=0, prefix_in_place=0)
        state = dict(next=0)

        def admission_round():
            while True:
                wave = []
                for b in range(R):
                    if rows[b] is None and state["next"] < n:
                        q = state["next"]
                        state["next"] += 1
                        key = tuple(reqs[q]["prompt"])
                        fork_from = next((s for s in range(R) if rows[s] is not None and fresh[s] == key), None)
                        rows[b], fresh[b] = q, key
                        wave.append((q, b, fork_from))
                if not wave:
                    return
                for q, b, fork_from in wave:      # the cache work, one admission after the other
                    prompt = list(reqs[q]["prompt"])
                    if fork_from is not None:      # the identical-prompt rule: the source row's state, whole
                        chain, _, L = self.wrote[fork_from]
                        tot["forks"] += 1
                        reused, donor = len(prompt), fork_from
                    else:
                        donor, L = self._plan(b, prompt)
                        chain = [] if L == 0 else self.wrote[donor][0] + [self.wrote[donor][1:]]
                        tot["prefills"] += 1
                        tot["prefill_tokens"] += len(prompt) - L
                        if L and donor != b:
                            tot["prefix_forks"] += 1
                        elif L:
                            tot["prefix_in_place"] += 1
                        reused = L
                    want = _after(self.alone, chain, reqs[q], L, self.logprobs)
                    self.claim[b], self.wrote[b] = prompt, (chain, reqs[q], L)
                    out[q] = dict(want=want, row=b, admitted_at=tot["steps"], donor=donor, reused=reused, L=L, chain=chain)
                for q, b, _ in wave:
                    left[b], fed[b] = _samples(out[q]["want"]) - 1, 0
                    if left[b] <= 0:
                        rows[b] = fresh[b] = None

        admission_round()
        while any(r is not None for r in rows):
            tot["steps"] += 1
            for b in range(R):
                fresh[b] = None
                if rows[b] is not None:
                    self.claim[b].append(out[rows[b]]["want"][0][fed[b]])      # the step was fed the sample before its own: never a request's last
                    fed[b] += 1
                    left[b] -= 1
                    if left[b] <= 0:
                        rows[b] = None
            admission_round()
        return out, tot


def _check(rule, model, reqs, logprobs=None):
    """one call against the rule: every row as the oracle's, every stat as the rule's -> (got, stats, expected)"""
    rule.logprobs = logprobs
    want, tot = rule.serve(reqs)
    got, stats = model.serve_requests_prefix(reqs, logprobs=logprobs, min_prefix=rule.min_prefix)
    print("reused", stats["reused_tokens"], "donor", stats["donor_row"], "rows", stats["rows"], "at", stats["admitted_at"], {k: stats[k] for k in tot})
    print("  rule", [w["reused"] for w in want], "donor", [w["donor"] for w in want], "rows", [w["row"] for w in want], "at", [w["admitted_at"] for w in want], tot)
    assert len(got) == len(reqs)
    for i, w in enumerate(want):
        _same_row(got[i], w["want"], logprobs is not None)
    assert stats["reused_tokens"] == [w["reused"] for w in want] and stats["donor_row"] == [w["donor"] for w in want], (stats, want)
    assert stats["rows"] == [w["row"] for w in want] and stats["admitted_at"] == [w["admitted_at"] for w in want], (stats, want)
    assert {k: stats[k] for k in tot} == tot, (stats, tot)
    assert model.prefix_cache_lengths() == [len(h) for h in rule.claim], (model.prefix_cache_lengths(), rule.claim)
    return got, stats, want


def _other(t):
    """a token that is not t"""
    return (t + 7) % (V - 1)


def _tail(donor, L, more=3):
    """a prompt that shares exactly donor[:L] with `donor` (a token list at least L long; beyond its end any token splits)"""
    first = _other(donor[L]) if L < len(donor) else 321
    return donor[:L] + [first] + [(first + 11 * (i + 1)) % (V - 1) for i in range(more)]


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
@pytest.mark.parametrize("L", [1, 7, 8, 9, 15, 16, 17])
def test_two_requests_of_one_wave_share_a_prefix_of_every_kind(models, policy, L):
    """the second forks [0, L) from the first's fresh row and prefills its tail: L = 1; 7, 8, 9 -- a local layer's band (window 8) starts inside, at and before the
    reused prefix; 15 -- the donor's whole prompt; 16, 17 -- a 20-token donor, at the prefill-chunk edge"""
    alone, batch = models(policy, 1), models(policy, 2)
    donor = dict(prompt=P15 if L <= 15 else P20, max_new_tokens=4)
    if L == 15:      # the donor's whole prompt: the request goes on with something else than the donor's first token
        t1 = _after(alone, [], donor, 0)[0][0]
        q = dict(prompt=P15 + [_other(t1), 5, 6], max_new_tokens=5)
    else:
        q = dict(prompt=_tail(donor["prompt"], L), max_new_tokens=5)
    rule = _Rule(2, alone)
    _, stats, want = _check(rule, batch, [donor, q])
    assert stats["reused_tokens"] == [0, L] and stats["donor_row"] == [-1, 0] and stats["admitted_at"] == [0, 0], stats
    assert (stats["prefills"], stats["prefill_tokens"], stats["forks"], stats["prefix_forks"], stats["prefix_in_place"]) == (2, len(donor["prompt"]) + len(q["prompt"]) - L, 0, 1, 0), stats
    assert want[1]["chain"] == [(donor, 0)]


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_the_same_prompt_in_a_later_round_reuses_all_but_its_last_position_in_place_or_by_a_fork(models, policy):
    alone, batch = models(policy, 1), models(policy, 2)
    a = dict(prompt=P15, max_new_tokens=2)
    b = dict(prompt=FOUR[1], max_new_tokens=6)
    again = dict(prompt=P15, max_new_tokens=4, seed=3, **ST)
    rule = _Rule(2, alone)
    _, stats, _ = _check(rule, batch, [a, b, again])      # a retires after one step; `again` enters a's own row: in place, no copy
    assert stats["rows"] == [0, 1, 0] and stats["admitted_at"][2] == 1, stats
    assert stats["reused_tokens"] == [0, 0, 14] and stats["donor_row"] == [-1, -1, 0] and (stats["prefix_forks"], stats["prefix_in_place"]) == (0, 1), stats
    assert stats["prefill_tokens"] == 15 + 9 + 1
    # the donor retires in row 1 while row 0 retires with it: the request enters row 0 -> a fork from a retired row
    three = models(policy, 3)
    rule3 = _Rule(3, alone)
    _, stats, _ = _check(rule3, three, [dict(b, max_new_tokens=2), a, dict(prompt=FOUR[0], max_new_tokens=6), again])
    assert stats["rows"] == [0, 1, 2, 0] and stats["reused_tokens"][3] == 14 and stats["donor_row"][3] == 1 and stats["prefix_forks"] == 1, stats


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_a_split_inside_the_donors_decoded_tokens_from_a_live_and_from_a_retired_donor(models, policy):
    alone, batch = models(policy, 1), models(policy, 2)
    donor = dict(prompt=FOUR[1], max_new_tokens=6)
    free = _after(alone, [], donor, 0)[0]
    assert len(free) == 6
    short = dict(prompt=FOUR[0], max_new_tokens=2)
    # LIVE: `short` retires after step 1, when the donor's row has been fed its first token: the request shares prompt + 1 decoded token with the live, stepped row 0
    q = dict(prompt=FOUR[1] + free[:1] + [_other(free[1]), 9], max_new_tokens=3)
    rule = _Rule(2, alone)
    _, stats, _ = _check(rule, batch, [donor, short, q])
    assert stats["rows"] == [0, 1, 1] and stats["admitted_at"][2] == 1 and stats["reused_tokens"][2] == 10 and stats["donor_row"][2] == 0 and stats["prefix_forks"] == 1, stats
    # RETIRED: all of the donor's tokens but the last, then another one.  The donor is long gone when the request comes; its row was never written since
    rule.clear()
    batch.clear_prefix_cache()
    q = dict(prompt=FOUR[1] + free[:5] + [_other(free[5]), 9], max_new_tokens=3)
    _, stats, _ = _check(rule, batch, [donor, dict(prompt=FOUR[3], max_new_tokens=12), q])      # the request enters the retired donor's own row: in place
    assert stats["rows"] == [0, 1, 0] and stats["admitted_at"][2] == 5 and stats["reused_tokens"][2] == 14 and stats["donor_row"][2] == 0, stats
    assert (stats["prefix_forks"], stats["prefix_in_place"]) == (0, 1), stats
    # ... and from a retired donor in ANOTHER row: a fork of prompt + decoded tokens
    three = models(policy, 3)
    rule3 = _Rule(3, alone)
    _, stats, _ = _check(rule3, three, [dict(short, max_new_tokens=6), donor, dict(prompt=FOUR[3], max_new_tokens=12), q])
    assert stats["rows"] == [0, 1, 2, 0] and stats["reused_tokens"][3] == 14 and stats["donor_row"][3] == 1 and stats["prefix_forks"] == 1, stats


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_identical_prompts_of_one_wave_still_take_one_prefill_and_two_whole_forks(models, policy):
    alone, batch = models(policy, 1), models(policy, 3)
    base = dict(prompt=P15, seed=5, repetition_penalty=1.3, max_new_tokens=8, **ST)
    rule = _Rule(3, alone)
    got, stats, _ = _check(rule, batch, [dict(base, seed=s) for s in (5, 6, 7)])
    assert len({tuple(g[0]) for g in got}) > 1
    assert (stats["prefills"], stats["prefill_tokens"], stats["forks"], stats["prefix_forks"]) == (1, 15, 2, 0), stats
    assert stats["reused_tokens"] == [0, 15, 15] and stats["donor_row"] == [-1, 0, 0], stats
    again, st2 = batch.serve_requests_prefix([dict(base, n=3)])      # the "n" expansion, and now the rows hold the prompt: one in place, then whole forks of it
    want, tot = rule.serve([dict(base, seed=s) for s in (5, 6, 7)])
    for i in range(3):
        _same_row(again[i], want[i]["want"], False)
    assert (st2["prefills"], st2["prefill_tokens"], st2["forks"], st2["prefix_in_place"]) == (1, 1, 2, 1) == (tot["prefills"], tot["prefill_tokens"], tot["forks"], tot["prefix_in_place"]), (st2, tot)


def _stream(alone):
    """seven requests on shared headers: a penalised stochastic one (its token table comes from the WHOLE prompt, reused or not), an automaton, bias + min_tokens,
    and plain ones; headers of 9 and 15 tokens, tails that split from everything before them"""
    h9, h15 = FOUR[1], P15
    free = alone.generate(h9 + [700, 701], max_new_tokens=8, seed=11, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17], **ST)[0]
    return [dict(prompt=h15 + [10, 20], max_new_tokens=5),
            dict(prompt=h9 + [700, 701], max_new_tokens=8, seed=11, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17], min_tokens=3, stop_tokens=[free[1]], **ST),
            dict(prompt=h15 + [10, 21, 22], max_new_tokens=9, seed=23, temperature=1.1, top_k=40, top_p=0.95, min_p=0.02, repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1),
            dict(prompt=h9 + [700, 800], max_new_tokens=7, automaton=_mod3()),
            dict(prompt=h15[:8] + [1, 2, 3], max_new_tokens=1),
            dict(prompt=h9[:4] + [4, 4, 4, 4], max_new_tokens=6),
            dict(prompt=h15 + [10, 20], max_new_tokens=4, seed=2, **ST)]


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_a_mixed_stream_of_seven_requests_on_three_rows_in_two_arrival_orders(models, policy):
    alone, batch = models(policy, 1), models(policy, 3)
    reqs = _stream(alone)
    rule = _Rule(3, alone)
    for order in ([0, 1, 2, 3, 4, 5, 6], [5, 3, 6, 1, 4, 0, 2]):
        rule.clear()
        batch.clear_prefix_cache()
        got, stats, want = _check(rule, batch, [reqs[i] for i in order], logprobs=3)
        assert sum(stats["reused_tokens"]) > 0 and stats["prefix_forks"] > 0, stats
        j = order.index(3)
        assert isinstance(got[j][-1], int) and all(t % 3 == i % 3 for i, t in enumerate(got[j][0])), got[j]
    # log-probabilities off: the same stream once more, on the claims the second order left (everything is a reuse now)
    got, stats, want = _check(rule, batch, reqs)
    assert all(r >= 1 for r in stats["reused_tokens"]), stats


@pytest.mark.parametrize("policy", ["bf16", "fp8"])
def test_claims_survive_a_call_and_end_with_anything_else_that_writes_rows(models, policy):
    alone, batch = models(policy, 1), models(policy, 2)
    first = [dict(prompt=P20, max_new_tokens=3), dict(prompt=FOUR[1], max_new_tokens=5)]
    second = [dict(prompt=_tail(FOUR[1], 6), max_new_tokens=4), dict(prompt=_tail(P20, 17), max_new_tokens=4)]
    rule = _Rule(2, alone)
    _check(rule, batch, first)
    assert batch.prefix_cache_lengths() == [20 + 2, 9 + 4]
    _, stats, _ = _check(rule, batch, second)      # call 2 on call 1's rows: row 0 takes 6 positions from row 1, then row 1 takes 17 from ... row 0's old claim is cut by then
    assert stats["reused_tokens"] == [6, 0] and stats["donor_row"] == [1, -1], stats
    rule.clear()
    batch.clear_prefix_cache()
    _check(rule, batch, first)
    _, stats, _ = _check(rule, batch, second[::-1])      # the other order keeps both: 17 in place, then 6 in place
    assert stats["reused_tokens"] == [17, 6] and stats["donor_row"] == [0, 1] and stats["prefix_in_place"] == 2, stats
    for forget in (lambda: batch.generate(FOUR[0], max_new_tokens=1), batch.clear_prefix_cache, lambda: batch.serve_requests(first[:1]),
                   lambda: batch.generate_requests(first[:1]), lambda: batch.score(P15)):
        rule.clear()
        batch.clear_prefix_cache()
        _check(rule, batch, first)
        assert max(batch.prefix_cache_lengths()) > 0
        forget()
        assert batch.prefix_cache_lengths() == [0, 0]
        rule.clear()
        _, stats, _ = _check(rule, batch, first)
        assert stats["reused_tokens"] == [0, 0] and stats["prefill_tokens"] == 29, stats
    with pytest.raises(ValueError, match="request 1: empty prompt"):      # a failing serving call ends them too
        batch.serve_requests_prefix([first[0], dict(prompt=[])])
    assert batch.prefix_cache_lengths() == [0, 0]


def test_a_prefix_below_min_prefix_is_prefilled_whole(models):
    alone, batch = models("bf16", 1), models("bf16", 2)
    reqs = [dict(prompt=P15, max_new_tokens=3), dict(prompt=_tail(P15, 7), max_new_tokens=3), dict(prompt=_tail(P15, 8, more=4), max_new_tokens=3)]
    rule = _Rule(2, alone, min_prefix=8)
    _, stats, _ = _check(rule, batch, reqs)
    assert stats["reused_tokens"] == [0, 0, 8] and stats["donor_row"][:2] == [-1, -1] and stats["prefill_tokens"] == 15 + 11 + 13 - 8, stats


def test_the_flag_off_is_serve_requests_and_the_flag_on_captures_nothing_within_a_class():
    kw = dict(context=MAX_SEQ, prefill_chunk=16, seed=SEED, max_batch=2)
    a, b = host.GemmaModel.synthetic("bf16", SMALL, **kw), host.GemmaModel.synthetic("bf16", SMALL, **kw)
    try:
        plain = [dict(prompt=(P15 if i % 2 else FOUR[1])[:4 + i] + [i], max_new_tokens=3 + i % 4) for i in range(7)]
        want, st_a = a.serve_requests(plain)
        got, st_b = b.serve_requests_prefix(plain, prefix_cache=False)
        assert got == want and list(st_b) == list(st_a) and {k: v for k, v in st_b.items() if k != TIMES} == {k: v for k, v in st_a.items() if k != TIMES}, (st_a, st_b)
        assert st_b["captures"] == b.rows_graph_info()["captures"] >= 1 and b.prefix_cache_lengths() == [0, 0]
        per_call = st_b["captures"]
        on, st = b.serve_requests_prefix(plain)      # the same class facts: greedy, unconstrained, B = 2 -- forks and suffix prefills are no part of the rows graph
        assert st["captures"] == 0 and b.rows_graph_info()["captures"] == per_call and sum(st["reused_tokens"]) > 0, st
        assert set(st) - set(st_a) == {"reused_tokens", "donor_row", "prefix_forks", "prefix_in_place"}
        _, st = b.serve_requests_prefix([dict(q, max_new_tokens=4) for q in plain[::-1]])
        assert st["captures"] == 0 and b.rows_graph_info()["captures"] == per_call
        assert [g[1] for g in on] == [w[1] for w in want]
    finally:
        a.close()
        b.close()


def test_refusals_come_before_anything_is_enqueued(models):
    alone, batch = models("bf16", 1), models("bf16", 2)
    ok = [dict(prompt=FOUR[i % 4], max_new_tokens=3) for i in range(4)]
    rule = _Rule(2, alone)
    _check(rule, batch, ok)
    held, n = batch.prefix_cache_lengths(), batch.rows_graph_info()["captures"]
    assert max(held) > 0
    for bad in (0, -1):
        with pytest.raises(ValueError, match="min_prefix"):
            batch.serve_requests_prefix(ok, min_prefix=bad)
    assert batch.prefix_cache_lengths() == held and batch.rows_graph_info()["captures"] == n      # refused in front of the model: nothing ran, nothing is forgotten
    with pytest.raises(ValueError, match="one sequence"):
        alone.serve_requests_prefix(ok[:2])
    assert alone.prefix_cache_lengths() == [0]
    _check(rule, batch, ok)


def test_fork_row_prefix_copies_caches_only_and_refuses_before_any_device_work():
    """the transformer's entry under the model: rows 1 and 2 take [0, 9) of row 0 AFTER row 0 has stepped, then prefill their own suffix -- the logits equal those of a
    row that ran the same prefill and the same suffix itself; a row's position word is untouched by the fork alone"""
    import numpy as np
    g = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4)
    one = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED)
    try:
        suffix = [8, 7, 6]
        g.prefill_row(0, P15)
        g.set_active(0, True, token=5)
        g.decode_rows(2, 15, mode="fused")      # row 0 steps: its logits and position move on
        g.set_active(0, False)
        g.prefill_row(3, P15)
        want = g.prefill_row(3, suffix, offset=9)      # the same two pieces in one row, no fork
        g.prefill_row(1, [1, 2])
        g.fork_row_prefix(0, 0b0110, 9)
        with pytest.raises(ValueError, match="beyond row 2's position 0"):      # the fork alone moved no position word: row 2 was never prefilled
            g.fork_row_prefix(2, 0b0001, 1)
        with pytest.raises(ValueError, match="beyond row 1's position 2"):
            g.fork_row_prefix(1, 0b0001, 3)
        for r in (1, 2):
            got = g.prefill_row(r, suffix, offset=9)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), r
        for args, telling in (((0, 0b0001, 4), "other than the source row 0"), ((0, 0, 4), "must name rows"), ((0, 0b10010, 4), "must name rows"), ((4, 0b0010, 4), "source row 4"),
                              ((-1, 0b0010, 4), "source row -1"), ((0, 0b0010, 0), "len 0"), ((0, 0b0010, MAX_SEQ + 1), "len 65"), ((0, 0b0010, 17), "beyond row 0's position 16"),
                              ((2, 0b0010, 13), "beyond row 2's position 12")):
            with pytest.raises(ValueError, match=telling):
                g.fork_row_prefix(*args)
        with pytest.raises(ValueError, match="one sequence"):
            one.fork_row_prefix(0, 0b0010, 1)
        got = g.prefill_row(1, suffix, offset=9)      # the refusals wrote nothing
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        g.close()
        one.close()
