"""GPU: the token automaton kernel (csrc/sampling.hip: token_automaton_kernel; include/mila_cdna4.h: token automaton) against the numpy restatement of
tests/ref_token_automaton.py.  The effective tables are compared as uint32 bits: the kernel copies base values and writes -inf, so nothing is rounded.
Shapes: one lane, below / at / above one wave and one workgroup-quarter (63 .. 65, 255 .. 257), no multiple of 4 (the scalar tail), more than one workgroup per row
(1000 = 250 vectors is one workgroup; 1024 is exactly one; 262144 is 256 workgroups of one vector per lane -- the grid cap, and Gemma's vocabulary)."""
import numpy as np
import pytest
import torch

import ref_token_automaton as A
from gpu_util import dev_f32, dev_i32, dev_u16
from mila_amd import capi
from test_sample_biased_gpu import _membership_settings
from test_sample_filtered_gpu import SENTINEL, _scratch

pytestmark = pytest.mark.gpu

VOCABS = (1, 63, 64, 65, 255, 256, 257, 1000, 1024, 262144)
STATES = (1, 2, 300)
POISON = 0x7FC0BEEF      # a NaN no table holds


def _classes(V):
    return (1, 2, 7) + ((V,) if V <= 1024 else ())


def _automaton(V, S, Cn, seed):
    if Cn == V and V > 7:      # identity classes
        class_of, nxt = A.random_automaton(V, S, Cn, seed)
        return np.arange(V, dtype=np.uint16), nxt
    return A.random_automaton(V, S, min(Cn, 65535), seed)


def _poisoned(rows, V):
    return torch.full((rows, V), POISON, dtype=torch.int32, device="cuda:0").view(torch.float32)


def _bits(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _bases(V, rows, seed):
    """(name, device tensor or None, per-row numpy tables or None)"""
    shared = A.base_table(V, seed)
    per_row = np.stack([A.base_table(V, seed + 1 + b) for b in range(rows)])
    return [("none", None, [None] * rows), ("shared", dev_f32(shared), [shared] * rows), ("per row", dev_f32(per_row), list(per_row))]


def _want(class_of, nxt, states, bases):
    return np.stack([A.mask(class_of, nxt, s, b) for s, b in zip(states, bases)]).view(np.uint32)


@pytest.mark.parametrize("V", VOCABS)
def test_compose_and_step_equal_the_restatement(V):
    rng = np.random.default_rng(V)
    all_bases = {rows: _bases(V, rows, seed=V + rows) for rows in (1, 2, 3, 4)}      # computed once, shared by every automaton below, never written
    for S in STATES:
        for Cn in _classes(V):
            class_of, nxt = _automaton(V, S, Cn, seed=V + 7 * S + Cn)
            cls_dev, nxt_dev = dev_u16(class_of), dev_u16(nxt)
            for rows in (1, 2, 3, 4):
                states = [(5 + 131 * b) % S for b in range(rows)]      # a different state per row wherever S allows
                for name, base_dev, base_np in all_bases[rows]:
                    where = "V=%d S=%d C=%d rows=%d base %s" % (V, S, nxt.shape[1], rows, name)
                    state_dev, ticket = dev_i32(np.array(states)), dev_i32(np.zeros(rows))
                    eff = _poisoned(rows, V)
                    capi.token_automaton_compose(eff, base_dev, cls_dev, nxt_dev, state_dev)
                    assert np.array_equal(_bits(eff), _want(class_of, nxt, states, base_np)), "compose " + where
                    assert state_dev.cpu().tolist() == states, "compose changed a state: " + where
                    # step: even rows get a token their state allows (when there is one), odd rows a forbidden one (when there is one); the last of several rows
                    # is inactive in the first launch, and all rows are active (active_dev NULL) in the second
                    toks = []
                    for b, s in enumerate(states):
                        ok = np.flatnonzero(nxt[s, class_of] != A.FORBIDDEN)
                        no = np.flatnonzero(nxt[s, class_of] == A.FORBIDDEN)
                        pick = ok if (b % 2 == 0 and ok.size) or not no.size else no
                        toks.append(int(pick[rng.integers(pick.size)]))
                    tok_dev = dev_i32(np.array(toks))
                    for active in ([1] * (rows - 1) + [0] if rows > 1 else [1], None):
                        live = [True] * rows if active is None else [bool(a) for a in active]
                        before = state_dev.cpu().tolist()
                        after = [A.step(class_of, nxt, s, t) if on else s for s, t, on in zip(before, toks, live)]
                        eff = _poisoned(rows, V)
                        capi.token_automaton_step(eff, base_dev, cls_dev, nxt_dev, state_dev, tok_dev, ticket, None if active is None else dev_i32(np.array(active)))
                        got, want = _bits(eff), _want(class_of, nxt, after, base_np)
                        for b in range(rows):
                            if live[b]:
                                assert np.array_equal(got[b], want[b]), "step row %d (state %d -> %d, token %d) %s" % (b, before[b], after[b], toks[b], where)
                            else:
                                assert (got[b] == POISON).all(), "an inactive row's table was written: row %d %s" % (b, where)
                        assert state_dev.cpu().tolist() == after, "states after the step: " + where
                        assert ticket.cpu().tolist() == [0] * rows, "a ticket was left: " + where


def test_a_forbidden_token_leaves_the_state_and_recomposes_its_table():
    V, S = 1000, 2
    class_of = (np.arange(V) % 2).astype(np.uint16)
    nxt = np.array([[1, A.FORBIDDEN], [A.FORBIDDEN, 0]], dtype=np.uint16)      # state 0 allows even ids, state 1 odd ids
    base = A.base_table(V, 3)
    cls_dev, nxt_dev, base_dev = dev_u16(class_of), dev_u16(nxt), dev_f32(base)
    state, ticket, eff = dev_i32(np.array([0])), dev_i32(np.array([0])), _poisoned(1, V)
    for tok, want_state in ((3, 0), (4, 1), (6, 1), (V, 1), (-1, 1), (7, 0)):      # forbidden, allowed, forbidden, outside the vocabulary twice, allowed
        eff.view(torch.int32).fill_(POISON)
        capi.token_automaton_step(eff, base_dev, cls_dev, nxt_dev, state, dev_i32(np.array([tok])), ticket)
        assert state.cpu().tolist() == [want_state] and ticket.cpu().tolist() == [0], tok
        assert np.array_equal(_bits(eff)[0], A.mask(class_of, nxt, want_state, base).view(np.uint32)), tok


def test_unaligned_tables_take_the_scalar_walk():
    """an eff / base / class_of that starts off a 16 / 16 / 8 byte boundary, and a row stride that is no multiple of 4"""
    V, S, rows = 1001, 5, 3
    class_of, nxt = A.random_automaton(V, S, 7, seed=9)
    base = np.stack([A.base_table(V, 20 + b) for b in range(rows)])
    cls_buf = dev_u16(np.concatenate([[0], class_of]))
    big = torch.full((rows * V + 1,), POISON, dtype=torch.int32, device="cuda:0").view(torch.float32)
    base_buf = dev_f32(np.concatenate([[0.0], base.reshape(-1)]))
    states = [1, 4, 2]
    state_dev = dev_i32(np.array(states))
    capi.token_automaton_compose(big[1:].view(rows, V), base_buf[1:].view(rows, V), cls_buf[1:], dev_u16(nxt), state_dev)
    assert np.array_equal(_bits(big[1:].view(rows, V)), _want(class_of, nxt, states, list(base)))
    assert int(big.view(torch.int32)[0].cpu()) == POISON


def test_sixty_four_steps_in_a_row_never_read_an_advanced_state():
    """THE STATE HAZARD: every workgroup of a step launch reads the state word and one of them stores the new value; a workgroup that started late must not see it.
    64 launches on one stream with no host sync between them, the token word rewritten between launches by a device-side copy, every launch into its own slice of
    eff: each table must be the restatement's table for that step's state -- a workgroup that read the advanced state would have written the table of the state
    after next into its part of the slice."""
    V, S, rows, steps = 262144, 300, 4, 64
    class_of, nxt = A.random_automaton(V, S, 7, seed=41, forbid=0.25)
    base = A.base_table(V, 42)
    rng = np.random.default_rng(43)
    seq = rng.integers(0, V, size=(steps, rows)).astype(np.int32)
    cls_dev, nxt_dev, base_dev, seq_dev = dev_u16(class_of), dev_u16(nxt), dev_f32(base), dev_i32(seq)
    states = [0, 77, 150, 299]
    state_dev, ticket, tok = dev_i32(np.array(states)), dev_i32(np.zeros(rows)), dev_i32(np.zeros(rows))
    eff = torch.full((steps, rows, V), POISON, dtype=torch.int32, device="cuda:0").view(torch.float32)
    torch.cuda.synchronize()
    for k in range(steps):
        tok.copy_(seq_dev[k])
        capi.token_automaton_step(eff[k], base_dev, cls_dev, nxt_dev, state_dev, tok, ticket)
    got = _bits(eff)
    moved = 0
    for k in range(steps):
        after = [A.step(class_of, nxt, s, int(t)) for s, t in zip(states, seq[k])]
        moved += sum(a != s for a, s in zip(after, states))
        want = _want(class_of, nxt, after, [base] * rows)
        for b in range(rows):
            assert np.array_equal(got[k, b], want[b]), "step %d row %d: state %d -> %d by token %d; %d entries differ" % (
                k, b, states[b], after[b], seq[k, b], int((got[k, b] != want[b]).sum()))
        states = after
    assert moved >= steps * rows // 2, "the state moved in %d of %d steps: the case shows little" % (moved, steps * rows)
    assert state_dev.cpu().tolist() == states and ticket.cpu().tolist() == [0] * rows


def test_the_sampler_on_the_effective_table_returns_only_allowed_tokens():
    """composition with the sampler: sample_radix_biased_fp32 reading eff returns, at 200 draws per truncation setting, a token the state allows -- and the token of
    the same call on a host-built table with the same bits"""
    V, S, state, n_draws = 4097, 7, 3, 200
    rng = np.random.default_rng(5)
    class_of, nxt = A.random_automaton(V, S, 7, seed=6, forbid=0.6)
    base = A.base_table(V, 8)
    logits = dev_f32((rng.standard_normal(V) * 3.0).astype(np.float32))
    eff = _poisoned(1, V)
    capi.token_automaton_compose(eff, dev_f32(base), dev_u16(class_of), dev_u16(nxt), dev_i32(np.array([state])))
    want_table = A.mask(class_of, nxt, state, base)
    assert np.array_equal(_bits(eff)[0], want_table.view(np.uint32))
    host_table = dev_f32(want_table)
    allowed = np.isfinite(want_table)
    n = int(allowed.sum())
    assert 1 < n < V
    draws = [0.0, float(np.nextafter(np.float32(1), np.float32(0)))] + rng.random(n_draws - 2).astype(np.float32).tolist()
    settings = _membership_settings(n)
    out = torch.full((2, len(settings), n_draws), SENTINEL, dtype=torch.int32, device="cuda:0")
    for j, (t, k, p, min_p) in enumerate(settings):
        for i, r in enumerate(draws):
            for w, table in enumerate((eff[0], host_table)):
                capi.sample_radix_biased(logits, out[w, j, i:i + 1], 30.0, t, k, p, r, (min_p, 1.0, 0.0, 0.0), None, table, _scratch(0, V))
    got = out.cpu().numpy()
    assert np.array_equal(got[0], got[1]), "the effective table and a host-built table with the same bits gave different tokens"
    assert ((got[0] >= 0) & (got[0] < V)).all() and allowed[got[0]].all(), "a token the state forbids was sampled"
    assert len(np.unique(got[0])) > 1
