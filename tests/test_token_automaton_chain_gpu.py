"""GPU: the automaton's chain forms (csrc/sampling.hip: token_automaton_chain_compose_kernel / _chain_step_kernel; include/mila_cdna4.h: the constrained chain step)
against a numpy restatement, bit for bit -- the kernels copy base values and write -inf, so nothing is rounded.  Row t of a chain step was fed tok[t]: its table is that
of q_t, q_0 the state word and q_t = step(q_{t-1}, tok[t]), a forbidden or out-of-range draft leaving the state.  chain_compose writes rows 1 .. T - 1 and the states;
chain_step, behind the accept tail, advances chain_states[count - 1] by tok[0] into the state word and recomposes row 0.
Shapes: one lane (1), above one wave and one workgroup-quarter (65, 257), no multiple of 4 and more than one workgroup (1027: the scalar tail behind 256 vectors),
exactly four workgroups (4096), the grid cap and Gemma's vocabulary (262144)."""
import numpy as np
import pytest
import torch

import ref_token_automaton as A
from gpu_util import dev_f32, dev_i32, dev_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

VOCABS = (1, 65, 257, 1027, 4096, 262144)
ROWS = 4                  # every eff has four rows: the rows >= T must keep their bytes
POISON = 0x7FC0BEEF       # a NaN no table holds


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _poisoned(stride):
    return torch.full((ROWS, stride), POISON, dtype=torch.int32, device="cuda:0").view(torch.float32)


def _strides(V):
    """(an eff stride that allows the 16-byte path, an odd one that forces the scalar walk)"""
    vec = (V + 3) // 4 * 4
    return vec, V + 1 if V % 2 == 0 else V + 2


def _chain_states(class_of, nxt, q0, toks):
    """q_0 .. q_{T-1} of a chain fed toks[0 .. T-1] from the state word q0 (toks[0] is already in q0)"""
    V, q = class_of.size, [q0]
    for t in toks[1:]:
        q.append(A.step(class_of, nxt, q[-1], int(t)) if 0 <= t < V else q[-1])
    return q


def _bases(V, stride, seed):
    """(name, device tensor or None, row -> numpy table or None): none, one shared table, one table per row at the eff stride"""
    shared = A.base_table(V, seed)
    per_row = np.zeros((ROWS, stride), dtype=np.float32)
    for b in range(ROWS):
        per_row[b, :V] = A.base_table(V, seed + 1 + b)
    return [("none", None, lambda b: None), ("shared", dev_f32(shared), lambda b: shared), ("per row", dev_f32(per_row), lambda b: per_row[b, :V])]


def _draft_sets(class_of, nxt, q0, T, rng):
    """drafts tok[1 .. T-1]: all allowed along the way; a forbidden one at each position (where the state there forbids something); an out-of-range id"""
    V = class_of.size

    def pick(q, allowed):
        ids = np.flatnonzero((nxt[q, class_of] != A.FORBIDDEN) == allowed)
        return int(ids[rng.integers(ids.size)]) if ids.size else None

    def walk(bad_at, bad):
        toks, q = [int(rng.integers(V))], q0
        for t in range(1, T):
            d = bad(q) if t == bad_at else pick(q, True)
            if d is None:
                d = pick(q, True) if pick(q, True) is not None else 0
            toks.append(d)
            q = A.step(class_of, nxt, q, d) if 0 <= d < V else q
        return toks

    sets = [("allowed", walk(0, None))]
    for t in range(1, T):
        sets.append(("forbidden at %d" % t, walk(t, lambda q: pick(q, False))))
    sets.append(("out of range at 1", walk(1, lambda q: V)))
    sets.append(("negative at %d" % (T - 1), walk(T - 1, lambda q: -1)))
    return sets


@pytest.mark.parametrize("V", VOCABS)
def test_chain_compose_equals_the_restatement(V):
    rng = np.random.default_rng(V)
    S, Cn = 300, min(7, V)
    class_of, nxt = A.random_automaton(V, S, Cn, seed=V + 1, forbid=0.5)
    cls_dev, nxt_dev = dev_u16(class_of), dev_u16(nxt)
    forbidden_drafts = 0
    for stride in _strides(V):
        bases = _bases(V, stride, seed=V + stride)      # computed once per stride, never written
        for T in (2, 3, 4):
            q0 = int(rng.integers(S))
            for what, toks in _draft_sets(class_of, nxt, q0, T, rng):
                want_q = _chain_states(class_of, nxt, q0, toks)
                forbidden_drafts += sum(a == b for a, b in zip(want_q, want_q[1:]))
                for name, base_dev, base_np in bases:
                    where = "V=%d stride=%d T=%d drafts %s %s base %s" % (V, stride, T, what, toks, name)
                    eff = _poisoned(stride)
                    state_dev, tok_dev = dev_i32(np.array([q0])), dev_i32(np.array(toks + [0] * (ROWS - T)))
                    states_dev = dev_i32(np.full(ROWS, -7))
                    capi.token_automaton_chain_compose(eff, base_dev, cls_dev, nxt_dev, state_dev, tok_dev, states_dev, T)
                    got = _bits(eff)
                    assert (got[0] == POISON).all(), "row 0 was written: " + where
                    assert (got[T:] == POISON).all() and (got[:, V:] == POISON).all(), "a row >= T or the padding of a row was written: " + where
                    for t in range(1, T):
                        assert np.array_equal(got[t, :V], A.mask(class_of, nxt, want_q[t], base_np(t)).view(np.uint32)), "row %d (state %d): %s" % (t, want_q[t], where)
                    assert states_dev.cpu().tolist() == want_q + [-7] * (ROWS - T), "chain_states: " + where
                    assert state_dev.cpu().tolist() == [q0] and tok_dev.cpu().tolist() == toks + [0] * (ROWS - T), "the state word or the tokens were written: " + where
    assert V == 1 or forbidden_drafts > 0, "no draft left its state: the case shows little"


@pytest.mark.parametrize("V", VOCABS)
def test_chain_step_equals_the_restatement_for_every_count(V):
    rng = np.random.default_rng(V + 100)
    S, Cn = 300, min(7, V)
    class_of, nxt = A.random_automaton(V, S, Cn, seed=V + 2, forbid=0.5)
    cls_dev, nxt_dev = dev_u16(class_of), dev_u16(nxt)
    for stride in _strides(V):
        bases = _bases(V, stride, seed=V + stride + 50)
        for T in (2, 3, 4):
            chain = [int(s) for s in rng.integers(0, S, size=T)]      # any states: the kernel reads what chain_compose left, whatever it is
            for count in list(range(1, T + 1)) + [0, T + 1, -3]:
                n = count if 1 <= count <= T else 1      # a count outside 1 .. T is read as 1
                for last in ("allowed", "forbidden", "out of range") if n == count else ("allowed",):
                    q = chain[n - 1]
                    ids = np.flatnonzero((nxt[q, class_of] != A.FORBIDDEN) == (last == "allowed"))
                    tok0 = V if last == "out of range" else int(ids[rng.integers(ids.size)]) if ids.size else 0
                    want = A.step(class_of, nxt, q, tok0) if 0 <= tok0 < V else q
                    for name, base_dev, base_np in bases:
                        where = "V=%d stride=%d T=%d count=%d token %d (%s) base %s" % (V, stride, T, count, tok0, last, name)
                        eff = _poisoned(stride)
                        state_dev, ticket = dev_i32(np.array([S - 1])), dev_i32(np.array([0]))
                        tok_dev, states_dev = dev_i32(np.array([tok0, 1, 2, 3])), dev_i32(np.array(chain + [-7] * (ROWS - T)))
                        result = dev_i32(np.array([count, 11, 12, 13, 14]))
                        capi.token_automaton_chain_step(eff, base_dev, cls_dev, nxt_dev, state_dev, tok_dev, states_dev, result, T, ticket)
                        got = _bits(eff)
                        assert state_dev.cpu().tolist() == [want], "the state word: " + where
                        assert ticket.cpu().tolist() == [0], "a ticket was left: " + where
                        assert np.array_equal(got[0, :V], A.mask(class_of, nxt, want, base_np(0)).view(np.uint32)), "row 0 (state %d): %s" % (want, where)
                        assert (got[1:] == POISON).all() and (got[0, V:] == POISON).all(), "a row behind row 0 was written: " + where
                        assert states_dev.cpu().tolist() == chain + [-7] * (ROWS - T) and result.cpu().tolist() == [count, 11, 12, 13, 14]


def test_a_state_word_outside_the_automaton_is_read_as_state_0():
    V, S = 257, 5
    class_of, nxt = A.random_automaton(V, S, 7, seed=3)
    eff, states_dev = _poisoned(260), dev_i32(np.full(ROWS, -7))
    toks = [0, 5, 9]
    capi.token_automaton_chain_compose(eff, None, dev_u16(class_of), dev_u16(nxt), dev_i32(np.array([S])), dev_i32(np.array(toks + [0])), states_dev, 3)
    want_q = _chain_states(class_of, nxt, 0, toks)
    assert states_dev.cpu().tolist() == want_q + [-7]
    assert np.array_equal(_bits(eff)[2, :V], A.mask(class_of, nxt, want_q[2]).view(np.uint32))


def test_sixteen_chained_replays_follow_the_host_tracked_state():
    """compose, a fake accept tail (count and tok[0] copied in on the device) and chain_step, sixteen times on one stream with no host sync between the launches:
    every chain_states, every table of rows 1 .. 3 and every row 0 is the restatement's for the state the host tracked.  chain_step stores the state word that the
    next compose reads, and 256 workgroups per row walk the tables: a launch that read a word of its neighbour's would write another state's table."""
    V, S, T, steps = 262144, 300, 4, 16
    class_of, nxt = A.random_automaton(V, S, 7, seed=61, forbid=0.3)
    base = A.base_table(V, 62)
    rng = np.random.default_rng(63)
    cls_dev, nxt_dev, base_dev = dev_u16(class_of), dev_u16(nxt), dev_f32(base)
    q0 = 17
    # the whole run on the host first: drafts (a forbidden one in every third step), the accepted count and the last accepted sample
    plan, q = [], q0
    for k in range(steps):
        toks, s = [0], q
        for t in range(1, T):
            ok = (nxt[s, class_of] != A.FORBIDDEN) == (not (k % 3 == 2 and t == 2))
            ids = np.flatnonzero(ok)
            d = int(ids[rng.integers(ids.size)]) if ids.size else int(rng.integers(V))
            toks.append(d)
            s = A.step(class_of, nxt, s, d)
        states = _chain_states(class_of, nxt, q, toks)
        count = 1 + k % T if k % 3 != 2 else 2      # (a forbidden draft at row 2 is never accepted: at most rows 0 and 1)
        ids = np.flatnonzero(nxt[states[count - 1], class_of] != A.FORBIDDEN)
        sample = int(ids[rng.integers(ids.size)])
        q_next = A.step(class_of, nxt, states[count - 1], sample)
        plan.append((toks, states, count, sample, q_next))
        q = q_next
    toks_dev = dev_i32(np.array([p[0] for p in plan]))
    accept_dev = dev_i32(np.array([[p[2], p[3]] for p in plan]))
    eff_log = torch.full((steps, ROWS, V), POISON, dtype=torch.int32, device="cuda:0").view(torch.float32)
    states_log = dev_i32(np.zeros((steps, ROWS)))
    state_dev, ticket = dev_i32(np.array([q0])), dev_i32(np.array([0]))
    tok, result = dev_i32(np.zeros(ROWS)), dev_i32(np.zeros(ROWS + 1))
    torch.cuda.synchronize()
    for k in range(steps):
        tok.copy_(toks_dev[k])
        capi.token_automaton_chain_compose(eff_log[k], base_dev, cls_dev, nxt_dev, state_dev, tok, states_log[k], T)
        result[:1].copy_(accept_dev[k, :1])      # the accept tail: the count and the next input
        tok[:1].copy_(accept_dev[k, 1:])
        capi.token_automaton_chain_step(eff_log[k], base_dev, cls_dev, nxt_dev, state_dev, tok, states_log[k], result, T, ticket)
    got, got_states = _bits(eff_log), states_log.cpu().tolist()
    moved = 0
    for k, (toks, states, count, sample, q_next) in enumerate(plan):
        assert got_states[k] == states, "chain_states of step %d" % k
        for t in range(1, T):
            assert np.array_equal(got[k, t], A.mask(class_of, nxt, states[t], base).view(np.uint32)), "step %d row %d" % (k, t)
        assert np.array_equal(got[k, 0], A.mask(class_of, nxt, q_next, base).view(np.uint32)), "step %d row 0 (state %d)" % (k, q_next)
        moved += q_next != states[0]
    assert moved >= steps // 2, "the state moved in %d of %d steps: the case shows little" % (moved, steps)
    assert state_dev.cpu().tolist() == [plan[-1][4]] and ticket.cpu().tolist() == [0]
