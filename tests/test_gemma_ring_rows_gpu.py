"""GPU: the bounded sliding-window KV cache under batched rows in the Gemma model (GemmaConfig::bounded_local_kv_rows) -- up to four independent sequences per step, each
with its own RING of window + chunk - 1 positions on the sliding-window layers and a flat cache on the global ones.
THE ORACLE is the same sequence alone on a bounded_local_kv one-row model of the same weights, compared as bit patterns: batch invariance of the rows step over enough
steps that every row wraps its ring several times, and above it the contracts of generate_batch, generate_requests, serve_requests and the prefix cache with its
valid-from bound (_RingRule restates Mila/PrefixCache.h, RINGS, in Python; tests/test_gemma_prefix_cache_gpu.py holds the flat rule and the helpers).  The SMALL geometry:
window 8, MAX_SEQ 64 -- every position in one live-length bucket; prefill chunks 4 (capacity 11, no power of two) and 16 (capacity 23)."""
import numpy as np
import pytest

from mila_amd import host
from test_gemma_host_gpu import MAX_SEQ, SMALL
from test_gemma_prefix_cache_gpu import _Rule, _after, _check
from test_gemma_row_requests_gpu import FOUR, _alone, _mod3, _same_row
from test_gemma_rows_gpu import NEW_PROMPT, PROMPTS, SEED, _admit, _same
from test_gemma_serve_requests_gpu import _fresh, _samples

pytestmark = pytest.mark.gpu

V = SMALL["vocab_size"]
W = SMALL["window"]
RING = dict(SMALL, bounded_local_kv=1)      # the one-row oracle's configuration
POLICIES = ["bf16", "fp8", "fp4"]
SERVING = ["bf16", "fp8"]
CHUNKS = [4, 16]
ST = dict(temperature=0.9, top_k=12, top_p=0.9)


def _capacity(chunk):
    return min(MAX_SEQ, W + chunk - 1)


class _Alone:
    """one sequence on a bounded_local_kv one-row model: the chunked prefill, then greedy steps through the fused decode"""

    def __init__(self, policy, chunk, prompt):
        self.g = host.Gemma(policy, RING, max_seq=MAX_SEQ, max_prefill=chunk, seed=SEED)
        self.prefill_logits = self.g.prefill_from(prompt, 0)
        self.pos, self.tok = len(prompt), int(np.argmax(self.prefill_logits))

    def step(self):
        logits = self.g.decode(self.tok, self.pos, "fused")
        self.pos, self.tok = self.pos + 1, int(np.argmax(logits))
        return logits

    def close(self):
        self.g.close()


def _rows_model(policy, chunk, max_batch=4):
    return host.Gemma(policy, SMALL, max_seq=MAX_SEQ, max_prefill=chunk, seed=SEED, max_batch=max_batch, bounded_local_kv_rows=True)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("policy", POLICIES)
def test_ring_rows_equal_the_sequences_alone(policy, chunk):
    """prompts of 3, 9 and 15 tokens in rows 0 .. 2, row 3 inactive, 42 greedy steps (positions up to 57: every row passes the ring's end several times): prefill
    logits, step logits, sampled tokens and positions of every row equal the bounded_local_kv alone runs bit for bit; the eager rows step equals the graph replay"""
    alone = [_Alone(policy, chunk, p) for p in PROMPTS]
    models = {m: _rows_model(policy, chunk) for m in ("fused", "graph")}
    try:
        for g in models.values():
            for b, a in enumerate(alone):
                _admit(g, b, PROMPTS[b], a)      # (asserts the row prefill's logits) row 3 stays inactive: position 0, token 0
        for step in range(42):
            max_pos = max(a.pos for a in alone)
            out = {m: g.decode_rows(4, max_pos, m) for m, g in models.items()}
            want = [a.step() for a in alone]
            for m, (logits, toks, pos) in out.items():
                for b, a in enumerate(alone):
                    assert _same(logits[b], want[b]), "%s step %d: row %d differs from the sequence alone" % (m, step, b)
                    assert int(toks[b]) == a.tok and int(pos[b]) == a.pos, (m, step, b, toks, pos)
                assert int(pos[3]) == 0 and int(toks[3]) == 0, "the inactive row moved"
            assert _same(out["fused"][0], out["graph"][0]), "eager rows step != graph replay at step %d" % step
        assert min(a.pos for a in alone) // _capacity(chunk) >= (4 if chunk == 4 else 1), [a.pos for a in alone]      # every row has passed its ring's end
        assert models["graph"].rows_graph_info()["captures"] == 1 and models["fused"].rows_graph_info()["captures"] == 0
    finally:
        for x in alone + list(models.values()):
            x.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_a_ring_row_retires_and_a_new_prompt_is_admitted_into_it(policy):
    """rows at differing positions; after twelve steps row 1 retires (its position and token stay while rows 0 and 2 go on), is reset and takes a new prompt over its
    old ring; all three rows still equal their alone runs for another twenty steps"""
    alone = [_Alone(policy, 4, p) for p in PROMPTS]
    g = _rows_model(policy, 4)
    try:
        for b, a in enumerate(alone):
            _admit(g, b, PROMPTS[b], a)

        def step(live, what):
            logits, toks, pos = g.decode_rows(3, max(alone[b].pos for b in live), "graph")
            for b in live:
                assert _same(logits[b], alone[b].step()), "%s: row %d differs from the sequence alone" % (what, b)
                assert int(toks[b]) == alone[b].tok and int(pos[b]) == alone[b].pos
            return toks, pos

        for i in range(12):
            step([0, 1, 2], "step %d" % i)
        g.set_active(1, False)
        frozen_pos, frozen_tok = alone[1].pos, alone[1].tok
        for i in range(3):
            toks, pos = step([0, 2], "row 1 retired, step %d" % i)
            assert int(pos[1]) == frozen_pos and int(toks[1]) == frozen_tok, "the retired row moved"
        g.reset_row(1)
        alone[1].close()
        alone[1] = _Alone(policy, 4, NEW_PROMPT)
        _admit(g, 1, NEW_PROMPT, alone[1])
        for i in range(20):
            step([0, 1, 2], "after re-admission, step %d" % i)
        assert g.rows_graph_info()["captures"] == 1
    finally:
        for x in alone + [g]:
            x.close()


def _kv_bytes(rows, chunk):
    """resident KV bytes of `rows` rows from the configuration: 2 (K, V) x NKV x capacity x HS x 2 bytes per layer, the ring's capacity on a sliding-window layer"""
    total = 0
    for i in range(SMALL["num_layers"]):
        glob = (i + 1) % SMALL["sliding_window_pattern"] == 0
        nkv, hs = (SMALL["num_global_kv_heads"], SMALL["global_head_dim"]) if glob else (SMALL["num_kv_heads"], SMALL["head_dim"])
        total += rows * 2 * nkv * (MAX_SEQ if glob else _capacity(chunk)) * hs * 2
    return total


@pytest.mark.parametrize("chunk", CHUNKS)
def test_memory_is_the_rings_and_max_batch_one_is_the_bounded_model(chunk):
    """what the configuration says a built model holds is what it holds; against the flat max_batch = 4 model the state shrinks by exactly the KV difference derived from
    the ring and flat capacities, and nothing else changes; with max_batch = 1 the switch builds the bounded_local_kv model: same bytes, same graph, same logits"""
    ring, flat = _rows_model("bf16", chunk), host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=chunk, seed=SEED, max_batch=4)
    one, plain = _rows_model("bf16", chunk, max_batch=1), host.Gemma("bf16", RING, max_seq=MAX_SEQ, max_prefill=chunk, seed=SEED)
    try:
        sr, sf, s1, sp = ring.memory_stats(), flat.memory_stats(), one.memory_stats(), plain.memory_stats()
        assert sr["required"]["device_state_bytes"] == sr["actual"]["device_state_bytes"]
        assert sr["actual"]["device_parameter_bytes"] == sf["actual"]["device_parameter_bytes"]
        flat_kv = sum(4 * 2 * (SMALL["num_global_kv_heads"] * SMALL["global_head_dim"] if (i + 1) % 6 == 0 else SMALL["num_kv_heads"] * SMALL["head_dim"]) * MAX_SEQ * 2
                      for i in range(SMALL["num_layers"]))
        assert sf["actual"]["device_state_bytes"] - sr["actual"]["device_state_bytes"] == flat_kv - _kv_bytes(4, chunk) > 0, (sf, sr)
        assert s1["actual"] == sp["actual"] and s1["required"] == sp["required"]
        prompt = PROMPTS[2]
        assert _same(plain.prefill_from(prompt, 0), one.prefill_from(prompt, 0))
        tok = 5
        for pos in range(len(prompt), len(prompt) + 2 * _capacity(chunk)):
            a, b = plain.decode(tok, pos, "graph"), one.decode(tok, pos, "graph")
            assert _same(a, b), pos
            tok = int(np.argmax(a))
        assert plain.graph_node_count() == one.graph_node_count() > 0
        with pytest.raises(ValueError, match="the ring needs a rewind rule per row"):      # the plain switch keeps its refusal
            host.Gemma("bf16", RING, max_seq=MAX_SEQ, max_prefill=chunk, seed=SEED, max_batch=2)
    finally:
        for x in (ring, flat, one, plain):
            x.close()


def test_forks_copy_the_live_band_and_the_rewind_rule_holds_per_row():
    """chunk 4: capacity 11, slack 3.  A whole fork behind a 15-token prefill leaves the destination where the prefill would have: both rows step like the sequence
    alone.  Then the rule: the forked row (valid from 15 - 8 + 1) cannot be rewound below its fork length nor donate a shorter prefix; the prefilled row may go back
    by the slack and no further; a donor that has run past the slack refuses its prefix."""
    p = PROMPTS[2]
    alone = _Alone("bf16", 4, p)
    g = _rows_model("bf16", 4)
    try:
        _admit(g, 0, p, alone)
        g.fork_row(0, 0b0110, len(p))
        for b in (1, 2):
            g.set_active(b, True, token=alone.tok)
        for step in range(14):
            logits, toks, pos = g.decode_rows(3, alone.pos, "fused")
            want = alone.step()
            for b in range(3):
                assert _same(logits[b], want) and int(toks[b]) == alone.tok and int(pos[b]) == alone.pos, (step, b)
        at = alone.pos      # 29
        assert g.rewind_row(0, at - 3, at) and not g.rewind_row(0, at - 4, at)      # written - position <= capacity - window
        assert not g.rewind_row(0, at - 3, at + 1)                                   # the same position against one more written
        h = _rows_model("bf16", 4)
        try:
            h.prefill_row(0, p)
            h.fork_row(0, 0b0010, len(p))
            assert h.rewind_row(0, len(p) - 3, len(p)) and not h.rewind_row(1, len(p) - 1, len(p)) and h.rewind_row(1, len(p), len(p))
            with pytest.raises(ValueError, match="no longer holds the band"):
                h.fork_row_prefix(1, 0b0100, len(p) - 1)      # the forked row holds the band [7, 15), and what the rule trusts of it starts at 8
            h.fork_row_prefix(1, 0b0100, len(p))
            h.fork_row_prefix(0, 0b1000, len(p) - 3)          # the prefilled row: inside the slack
            with pytest.raises(ValueError, match="no longer holds the band"):
                h.fork_row_prefix(0, 0b1000, len(p) - 4)
        finally:
            h.close()
        with pytest.raises(ValueError, match="no longer holds the band"):
            g.fork_row_prefix(1, 0b1000, at - 4)
    finally:
        alone.close()
        g.close()


# ---- serving ------------------------------------------------------------------------------------------------------------------------------------------------------
def _serving(policy, chunk, max_batch=4):
    kw = dict(context=MAX_SEQ, prefill_chunk=chunk, seed=SEED)
    return host.GemmaModel.synthetic(policy, RING, **kw), host.GemmaModel.synthetic(policy, SMALL, max_batch=max_batch, bounded_local_kv_rows=True, **kw)


@pytest.mark.parametrize("policy", POLICIES)
def test_generate_batch_gives_generates_tokens_on_rings(policy):
    """greedy generateBatch against generate() per prompt on the one-row ring model: rows of differing lengths, one of them stopped early, 30 new tokens so that the
    rings wrap"""
    alone, batch = _serving(policy, 4)
    try:
        free = [alone.generate(p, max_new_tokens=30)[0] for p in PROMPTS]
        stop = free[0][5]
        want = [alone.generate(p, max_new_tokens=30, stop_tokens=[stop])[:2] for p in PROMPTS]
        got = batch.generate_batch(PROMPTS, max_new_tokens=30, stop_tokens=[stop])
        assert [tuple(g) for g in got] == [tuple(w) for w in want], (got, want)
        assert batch.generate_batch(PROMPTS, max_new_tokens=30, stop_tokens=[stop]) == got      # the same batch again: rows are reset, rings overwritten from 0
    finally:
        alone.close()
        batch.close()


@pytest.mark.parametrize("policy", SERVING)
def test_generate_requests_gives_each_ring_row_what_generate_gives_it_alone(policy):
    """four differing requests -- greedy, stochastic with a seed, biased, a small automaton -- each with the alone model's tokens, finish reason and log-probability bits"""
    alone, batch = _serving(policy, 4)
    try:
        reqs = [dict(prompt=FOUR[3], max_new_tokens=26),
                dict(prompt=FOUR[1], max_new_tokens=28, seed=11, **ST),
                dict(prompt=FOUR[2], max_new_tokens=27, logit_bias={5: 2.0, 900: -3.0}, banned_tokens=[17]),
                dict(prompt=FOUR[0], max_new_tokens=27, automaton=_mod3())]
        want = [_alone(alone, q, logprobs=3) for q in reqs]
        got = batch.generate_requests(reqs, logprobs=3)
        for b in range(4):
            _same_row(got[b], want[b], True)
    finally:
        alone.close()
        batch.close()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("policy", SERVING)
def test_serve_requests_forks_ring_rows_one_prefill_two_forks(policy, chunk):
    """six stochastic requests on four rows, the first with n = 3: its copies share one prefill through the band fork (a 15-token prompt: positions 7 .. 14 of the ring
    layers, all 15 of the global ones).  Row 3 carries a request that outlasts all the others, so every step has four rows and one class: one capture"""
    alone, batch = _serving(policy, chunk)
    try:
        long_free = alone.generate(FOUR[3], max_new_tokens=30, seed=2, **ST)[0]
        never = [t for t in range(V) if t not in long_free][:2]
        head = dict(prompt=FOUR[2], seed=5, max_new_tokens=18, **ST)
        reqs = [dict(head, n=3),
                dict(prompt=FOUR[3], max_new_tokens=30, seed=2, stop_tokens=never, **ST),
                dict(prompt=FOUR[0], max_new_tokens=4, seed=3, **ST),
                dict(prompt=FOUR[1], max_new_tokens=6, seed=4, **ST),
                dict(prompt=NEW_PROMPT, max_new_tokens=3, seed=6, **ST),
                dict(prompt=FOUR[0], max_new_tokens=5, seed=7, **ST)]
        flat = [dict(head, seed=s) for s in (5, 6, 7)] + reqs[1:]
        want = [_fresh(alone, q, logprobs=2) for q in flat]
        assert len(want[3][0]) == 30 and want[3][1] == "length", "the request in row 3 must outlast the others"
        assert len({tuple(w[0]) for w in want[:3]}) > 1, "the three seeds must not agree, or a fork that copied the sampler too would pass"
        got, stats = batch.serve_requests(reqs, logprobs=2)
        assert len(got) == 8
        for i in range(8):
            _same_row(got[i], want[i], True)
        assert stats["forks"] == 2 and stats["prefills"] == 6 and stats["rows"][:4] == [0, 1, 2, 3], stats      # the n = 3 head: one prefill and two forks
        assert stats["captures"] == 1 and batch.rows_graph_info()["captures"] == 1, stats
    finally:
        alone.close()
        batch.close()


def _usable(high, frm, L, cap):
    """Mila/PrefixCache.h, RINGS: a continuation from L reads down to L - window + 1; intact are the positions from max(0, from, high - capacity + 1)"""
    return max(0, L - W + 1) >= max(0, frm, high - cap + 1)


class _RingRule(_Rule):
    """_Rule with the valid-from bound: per row `high` (the furthest length written since the row was last written from 0) and `frm` (what a band fork left)"""

    def __init__(self, R, alone, cap, min_prefix=1, logprobs=None):
        self.cap = cap
        super().__init__(R, alone, min_prefix, logprobs)

    def clear(self):
        super().clear()
        self.high, self.frm = [0] * self.R, [0] * self.R

    def _plan(self, row, prompt):
        m = []
        for s, h in enumerate(self.claim):
            k = 0
            while k < min(len(h), len(prompt)) and h[k] == prompt[k]:
                k += 1
            m.append(k if _usable(self.high[s], self.frm[s], min(k, len(prompt) - 1), self.cap) else 0)
        L = min(max(m), len(prompt) - 1)
        if L < self.min_prefix:
            return -1, 0
        if m[row] >= L:
            return row, L
        return min(s for s in range(self.R) if m[s] >= L), L

    def serve(self, reqs):
        """_Rule.serve with the two accounts kept beside the claims (the queue, the identical-prompt rule and the totals are its own)"""
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
                for q, b, fork_from in wave:
                    prompt = list(reqs[q]["prompt"])
                    if fork_from is not None:
                        chain, _, L = self.wrote[fork_from]
                        tot["forks"] += 1
                        reused, donor = len(prompt), fork_from
                        self.high[b], self.frm[b] = len(prompt), max(0, len(prompt) - W + 1)
                    else:
                        donor, L = self._plan(b, prompt)
                        chain = [] if L == 0 else self.wrote[donor][0] + [self.wrote[donor][1:]]
                        tot["prefills"] += 1
                        tot["prefill_tokens"] += len(prompt) - L
                        if L and donor != b:
                            tot["prefix_forks"] += 1
                            self.high[b], self.frm[b] = len(prompt), max(0, L - W + 1)
                        elif L:
                            tot["prefix_in_place"] += 1
                            self.high[b] = max(self.high[b], len(prompt))
                        else:
                            self.high[b], self.frm[b] = len(prompt), 0
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
                    self.claim[b].append(out[rows[b]]["want"][0][fed[b]])
                    self.high[b] = max(self.high[b], len(self.claim[b]))
                    fed[b] += 1
                    left[b] -= 1
                    if left[b] <= 0:
                        rows[b] = None
            admission_round()
        return out, tot


H12 = FOUR[2][:12]      # a header longer than the window
PREFIX_REQS = [dict(prompt=H12 + [33], max_new_tokens=1),                              # A: row 0, over at its admission: 13 positions written
               dict(prompt=NEW_PROMPT, max_new_tokens=3, seed=21, **ST),               # B: row 1, two steps
               dict(prompt=H12 + [555, 64], max_new_tokens=6),                         # C: row 0 again, in place from A's 12; five steps, 14 + 2 positions written after two
               dict(prompt=H12 + [77, 640, 8], max_new_tokens=4, seed=23, **ST)]       # D: row 1 when B retires after step 2; its donor is row 0, live and written up to 16


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("policy", SERVING)
def test_serve_requests_prefix_reuses_what_the_rings_still_hold(policy, chunk):
    """four requests on two rows that share a 12-token header.  C takes it in place from a row written up to 13 (inside the slack at either chunk).  D's donor has been
    written up to 16: at chunk 16 (capacity 23, slack 15) the header is forked from that row -- its live band [5, 12) and the flat layers' [0, 12) -- and at
    chunk 4 (capacity 11, slack 3) the ring has lost position 5, which a continuation from 12 reads: D prefills whole, as generate() does on the one-row ring model once
    its history has run past it.  The oracle is the prefix cache's own: generate() on the one-row bounded_local_kv model after the donor chain, asserting its reuse"""
    cap = _capacity(chunk)
    # the rule on the CPU, before anything runs: what the workload is built for (given that no request meets a stop token, which the results are checked for below)
    assert _usable(13, 0, 12, cap), "C's donor must lie inside the slack"
    assert _usable(16, 0, 12, cap) == (chunk == 16), "D's donor must lie inside the slack at chunk 16 and past it at chunk 4"
    assert 13 + 2 - 12 <= cap - W and 16 + 2 - 12 <= 23 - W, "generate() decodes ahead: its own history must still be inside the slack where the rows reuse"
    alone, batch = _serving(policy, chunk, max_batch=2)
    try:
        batch.clear_prefix_cache()
        got, stats, want = _check(_RingRule(2, alone, cap), batch, PREFIX_REQS, logprobs=2)
        assert [w["want"][1] for w in want] == ["length"] * 4, "a request met a stop token: the workload no longer says what it was built to say"
        assert stats["rows"] == [0, 1, 0, 1] and stats["admitted_at"] == [0, 0, 0, 2] and stats["reused_tokens"] == [0, 0, 12, 12 if chunk == 16 else 0], stats
        assert stats["donor_row"] == [-1, -1, 0, 0 if chunk == 16 else -1], stats
        assert stats["prefix_in_place"] == 1 and stats["prefix_forks"] == (1 if chunk == 16 else 0), stats
        if chunk == 4:      # the one-row ring model, its history run past row 0's, refuses the same reuse
            alone.generate([V - 1], max_new_tokens=1)
            alone.generate(PREFIX_REQS[0]["prompt"], max_new_tokens=1)
            alone.generate(PREFIX_REQS[2]["prompt"], max_new_tokens=PREFIX_REQS[2]["max_new_tokens"])
            assert alone.generate(PREFIX_REQS[3]["prompt"], max_new_tokens=1)[2] == 0
        batch.clear_prefix_cache()
        assert batch.prefix_cache_lengths() == [0, 0]
    finally:
        alone.close()
        batch.close()
