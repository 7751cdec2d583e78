"""GPU: sample_argmax_chain_accept, the tail of a chain step, on hand-made argmax partials.  Row t was fed tok[t]; a_t = the argmax over row t's partials (ties to the
lowest index); n = the first t in [0, T - 1) with a_t != tok[t + 1], else T - 1.  The kernel writes result = {n + 1, a_0 .. a_n}, tok[0] = a_n, *position += n + 1 and
nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import dev_i32
from mila_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _partials(rows, blocks, rng):
    """rows: per row the token that must win, or (token, tie_with) for a row whose maximum is reached at two indices.  Returns the scratch image (bytes)."""
    nb = capi.load().mila_cdna4_sample_scratch_bytes()
    per = nb // 8
    assert blocks <= per
    img = np.zeros((len(rows), 2, per), dtype=np.float32)
    img[:, 0, :] = np.float32(1e30)                     # slots past `blocks` must never be read: they would win
    img.view(np.int32)[:, 1, :] = 5
    for r, want in enumerate(rows):
        tie = None
        if isinstance(want, tuple):
            want, tie = want
        vals = rng.uniform(-4, 3, blocks).astype(np.float32)
        idx = rng.choice(np.arange(1000, 200000), blocks, replace=False).astype(np.int32)
        slot = int(rng.integers(blocks))
        vals[slot], idx[slot] = 3.5, want
        if tie is not None:                              # the same maximum at a HIGHER index, in an earlier slot: order of arrival must not decide
            other = (slot + 1 + int(rng.integers(blocks - 1))) % blocks
            vals[other], idx[other] = 3.5, tie
            assert tie > want
        img[r, 0, :blocks] = vals
        img.view(np.int32)[r, 1, :blocks] = idx
    return torch.from_numpy(img.view(np.uint8).reshape(-1).copy()).to("cuda:0"), nb


def _run(tok, rows, blocks, position, seed=0):
    T = len(tok)
    rng = np.random.default_rng(seed)
    scratch, nb = _partials(rows, blocks, rng)
    tok_d = dev_i32(np.array(list(tok) + [SENTINEL]))
    res_d = dev_i32(np.full(T + 2, SENTINEL))
    pos_d = dev_i32(np.array([position, SENTINEL]))
    capi.call("sample_argmax_chain_accept", tok_d, res_d, scratch, C.c_size_t(T * nb), blocks, pos_d, T)
    torch.cuda.synchronize()
    return tok_d.cpu().tolist(), res_d.cpu().tolist(), pos_d.cpu().tolist()


def _expect(tok, a):
    T = len(tok)
    n = next((t for t in range(T - 1) if a[t] != tok[t + 1]), T - 1)
    return n, [n + 1] + a[:n + 1]


CASES = [  # name, tok (fed rows), rows (what each row's partials say), expected n
    ("all drafts right, T=4", [11, 21, 31, 41], [21, 31, 41, 51], 3),
    ("all drafts right, T=3", [11, 21, 31], [21, 31, 41], 2),
    ("all drafts right, T=2", [11, 21], [21, 31], 1),
    ("first draft wrong, T=4", [11, 99, 31, 41], [21, 31, 41, 51], 0),
    ("first draft wrong, T=2", [11, 99], [21, 31], 0),
    ("a middle draft wrong, T=4", [11, 21, 99, 41], [21, 31, 41, 51], 1),
    ("the last draft wrong, T=4", [11, 21, 31, 99], [21, 31, 41, 51], 2),
    ("a middle draft wrong, T=3", [11, 21, 99], [21, 31, 41], 1),
    ("a later right draft behind a wrong one does not count", [11, 99, 31, 41], [21, 31, 41, 51], 0),
    ("a tie inside a row goes to the lowest index: the draft verifies", [11, 21, 31], [(21, 500), 31, 41], 2),
    ("a tie inside a row goes to the lowest index: the higher one was drafted", [11, 500, 31], [(21, 500), 31, 41], 0),
    ("token 0 as a draft (padding) that verifies", [11, 0, 0], [0, 0, 7], 2),
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("blocks", [1, 37, 512])
def test_the_accept_rule(case, blocks):
    name, tok, rows, n_want = CASES[case]
    a = [r[0] if isinstance(r, tuple) else r for r in rows]
    n, result = _expect(tok, a)
    assert n == n_want, name
    if blocks == 1 and any(isinstance(r, tuple) for r in rows):
        blocks = 2      # a tie needs two partials
    tok_after, res, pos = _run(tok, rows, blocks, position=100, seed=case)
    T = len(tok)
    assert res[:n + 2] == result, (name, res)
    assert res[n + 2:] == [SENTINEL] * (T - n), (name, res)              # words past a_n, and past the buffer's T + 1 words, are left alone
    assert tok_after == [a[n]] + tok[1:] + [SENTINEL], (name, tok_after)  # tok[0] = the next step's input; the drafts are not touched
    assert pos == [100 + n + 1, SENTINEL], (name, pos)


def test_two_steps_advance_the_same_words():
    """the second step starts from what the first left: tok[0] and the position word"""
    tok, rows = [11, 21, 99], [21, 31, 41]
    rng = np.random.default_rng(3)
    scratch, nb = _partials(rows, 64, rng)
    tok_d, res_d, pos_d = dev_i32(np.array(tok)), dev_i32(np.zeros(4)), dev_i32(np.array([7]))
    capi.call("sample_argmax_chain_accept", tok_d, res_d, scratch, C.c_size_t(3 * nb), 64, pos_d, 3)
    assert res_d.cpu().tolist()[:3] == [2, 21, 31] and tok_d.cpu().tolist() == [31, 21, 99] and pos_d.cpu().tolist() == [9]
    # same partials, drafts now right for them
    tok_d[1:] = torch.tensor([21, 31], dtype=torch.int32, device="cuda:0")
    tok_d[0] = 5
    capi.call("sample_argmax_chain_accept", tok_d, res_d, scratch, C.c_size_t(3 * nb), 64, pos_d, 3)
    assert res_d.cpu().tolist() == [3, 21, 31, 41] and tok_d.cpu().tolist()[0] == 41 and pos_d.cpu().tolist() == [12]
