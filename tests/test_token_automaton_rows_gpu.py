"""GPU: the automaton per row (csrc/sampling.hip: token_automaton_rows_kernel; include/mila_cdna4.h: row requests) -- every row of a rows step brings its own image
through a descriptor in device memory.  References: the numpy restatement of tests/ref_token_automaton.py, and the one-row token_automaton_compose / _step run on each
row alone.  Tables are compared as uint32 bits.  Four rows: two different automata with different (S, C), a row with the null descriptor, an inactive row; five steps
with chosen tokens, a forbidden one among them.  Vocab 1003 is no multiple of 4 (all scalar walk with its stride, one workgroup), 4096 takes the 16-byte walk with four
workgroups per row; one case has a row stride that defeats the vector path."""
import numpy as np
import pytest
import torch

import ref_token_automaton as A
from gpu_util import dev_f32, dev_i32, dev_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

POISON = 0x7FC0BEEF      # a NaN no table holds
ROWS = 4
NULL_ROW, INACTIVE_ROW = 2, 3
STEPS = 5


def _poisoned(rows, stride):
    return torch.full((rows, stride), POISON, dtype=torch.int32, device="cuda:0").view(torch.float32)


def _bits(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _images(V):
    """row -> (class_of, next): rows 0 and 1 differ in S and C; row 3 (inactive) has an image of its own; row 2 has none"""
    class_of, nxt = A.random_automaton(V, 5, 3, seed=V + 1, forbid=0.4)
    nxt[:, 0] = A.FORBIDDEN                                   # every state of row 0 forbids class 0 and allows class 1
    nxt[:, 1] = (np.arange(5) + 1) % 5
    return {0: (class_of, nxt), 1: A.random_automaton(V, 300, 11, seed=V + 2, forbid=0.6), INACTIVE_ROW: A.random_automaton(V, 2, 2, seed=V + 3, forbid=0.3)}


def _tokens(images, states, step, rng):
    """one token per row: row 0's third token is forbidden in its state (the state stays), the others are allowed where the state allows any"""
    toks = []
    for b in range(ROWS):
        if b not in images:
            toks.append(int(rng.integers(0, images[0][0].size)))
            continue
        class_of, nxt = images[b]
        ok = np.flatnonzero(nxt[states[b], class_of] != A.FORBIDDEN)
        no = np.flatnonzero(nxt[states[b], class_of] == A.FORBIDDEN)
        pick = no if (b == 0 and step == 2 and no.size) or not ok.size else ok
        toks.append(int(pick[rng.integers(pick.size)]))
    return toks


@pytest.mark.parametrize("V,pad", [(1003, 0), (4096, 0), (4096, 3)])
def test_four_rows_each_with_its_own_image(V, pad):
    stride = V + pad
    rng = np.random.default_rng(V + pad)
    images = _images(V)
    dev_images = {b: (dev_u16(c), dev_u16(n)) for b, (c, n) in images.items()}
    base = np.stack([A.base_table(V, 50 + b) for b in range(ROWS)])
    base_dev = torch.zeros((ROWS, stride), dtype=torch.float32, device="cuda:0")
    base_dev[:, :V] = dev_f32(base)
    desc = torch.zeros(capi.token_automaton_rows_bytes(ROWS), dtype=torch.uint8, device="cuda:0")
    assert desc.numel() == ROWS * 24
    for b in range(ROWS):
        capi.token_automaton_rows_set(desc, b, *(dev_images[b] if b in images else (None, None)))
    start = [3, 171, 123456, 1]      # (row 2's word is never read: no automaton)
    states = list(start)
    state_dev, ticket = dev_i32(np.array(states)), dev_i32(np.zeros(ROWS))
    active = dev_i32(np.array([1, 1, 1, 0]))

    # compose: rows 0, 1 and 3 get the table of their state, row 2 stays as it was
    eff = _poisoned(ROWS, stride)
    capi.token_automaton_rows_compose(eff, base_dev, desc, state_dev, vocab=V)
    got = _bits(eff)
    for b in range(ROWS):
        if b in images:
            assert np.array_equal(got[b, :V], A.mask(*images[b], states[b], base[b]).view(np.uint32)), "compose row %d" % b
        else:
            assert (got[b] == POISON).all(), "compose wrote the row without an automaton"
        assert (got[b, V:] == POISON).all(), "compose wrote the pad of row %d" % b
    assert state_dev.cpu().tolist() == start

    # the one-row entry on each row alone, fed the same tokens
    one_state = {b: dev_i32(np.array([start[b]])) for b in (0, 1)}
    one_ticket = dev_i32(np.zeros(1))
    forbidden_seen = False
    for step in range(STEPS):
        toks = _tokens(images, states, step, rng)
        tok_dev = dev_i32(np.array(toks))
        eff = _poisoned(ROWS, stride)
        capi.token_automaton_rows_step(eff, base_dev, desc, state_dev, tok_dev, ticket, active, vocab=V)
        got = _bits(eff)
        for b in (0, 1):
            class_of, nxt = images[b]
            after = A.step(class_of, nxt, states[b], toks[b])
            forbidden_seen |= b == 0 and step == 2 and after == states[b] and nxt[states[b], class_of[toks[b]]] == A.FORBIDDEN
            states[b] = after
            assert np.array_equal(got[b, :V], A.mask(class_of, nxt, after, base[b]).view(np.uint32)), "step %d row %d" % (step, b)
            assert (got[b, V:] == POISON).all()
            one = _poisoned(1, V)
            capi.token_automaton_step(one[0], dev_f32(base[b]), *dev_images[b], one_state[b], tok_dev[b:b + 1], one_ticket)
            assert np.array_equal(got[b, :V], _bits(one)[0]), "step %d row %d differs from the one-row entry" % (step, b)
            assert one_state[b].cpu().tolist() == [after]
        for b in (NULL_ROW, INACTIVE_ROW):
            assert (got[b] == POISON).all(), "step %d wrote row %d" % (step, b)
        assert state_dev.cpu().tolist() == [states[0], states[1], start[2], start[3]], "step %d" % step
        assert ticket.cpu().tolist() == [0] * ROWS, "a ticket was left at step %d" % step
        assert tok_dev.cpu().tolist() == toks
    assert forbidden_seen, "the forbidden token never came up: the case shows little"


def test_a_descriptor_is_replaced_in_stream_order():
    """a new image for a row between two steps: the first step walks the old image, the second the new one -- no sync between set and step"""
    V = 1003
    old, new = A.random_automaton(V, 4, 3, seed=1), A.random_automaton(V, 9, 5, seed=2)
    keep = [dev_u16(a) for a in (*old, *new)]
    desc = torch.zeros(capi.token_automaton_rows_bytes(1), dtype=torch.uint8, device="cuda:0")
    state, ticket, tok = dev_i32(np.array([2])), dev_i32(np.zeros(1)), dev_i32(np.array([-1]))      # token outside the vocabulary: the state stays
    effs = [_poisoned(1, V), _poisoned(1, V)]
    capi.token_automaton_rows_set(desc, 0, keep[0], keep[1])
    capi.token_automaton_rows_step(effs[0], None, desc, state, tok, ticket)
    capi.token_automaton_rows_set(desc, 0, keep[2], keep[3])
    capi.token_automaton_rows_step(effs[1], None, desc, state, tok, ticket)
    assert np.array_equal(_bits(effs[0])[0], A.mask(*old, 2).view(np.uint32))
    assert np.array_equal(_bits(effs[1])[0], A.mask(*new, 2).view(np.uint32))
    assert state.cpu().tolist() == [2] and ticket.cpu().tolist() == [0]


def test_bad_arguments_are_refused_before_any_launch():
    V = 64
    desc = torch.zeros(capi.token_automaton_rows_bytes(4), dtype=torch.uint8, device="cuda:0")
    cls, nxt = dev_u16(np.zeros(V, dtype=np.uint16)), dev_u16(np.zeros((2, 2), dtype=np.uint16))
    eff, state, ticket, tok = _poisoned(4, V), dev_i32(np.zeros(4)), dev_i32(np.zeros(4)), dev_i32(np.zeros(4))
    assert capi.token_automaton_rows_bytes(0) == 0 and capi.token_automaton_rows_bytes(5) == 0
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_set(desc, 4, cls, nxt)
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_set(desc, -1, cls, nxt)
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_set(desc[1:], 0, cls, nxt)                  # misaligned
    with pytest.raises(capi.InvalidArgument):
        capi.call("token_automaton_rows_set", desc, 0, cls, None, 2, 2, V)     # one of the two pointers
    with pytest.raises(capi.InvalidArgument):
        capi.call("token_automaton_rows_set", desc, 0, cls, nxt, 0, 2, V)      # S = 0
    with pytest.raises(capi.InvalidArgument):
        capi.call("token_automaton_rows_set", desc, 0, cls, nxt, 2, 70000, V)  # C beyond 16 bits
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_step(eff, None, None, state, tok, ticket)
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_step(eff, None, desc, state, None, ticket)
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_step(eff, None, desc, state, tok, None)
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_compose(eff, None, desc, None)
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_compose(_poisoned(5, V), None, desc, state)  # rows = 5
    with pytest.raises(capi.InvalidArgument):
        capi.token_automaton_rows_compose(eff, None, desc, state, vocab=V + 1)  # eff_stride < vocab
    assert (_bits(eff) == POISON).all() and not desc.cpu().numpy().any()
