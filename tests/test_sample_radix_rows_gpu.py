"""GPU: the radix sampler over 1 .. 4 rows in one pipeline (sample_radix_rows_fp32 / _rows_advance_fp32 / _chain_accept_fp32).  The oracle is the one-row entry
sample_radix_fp32 run in the same test on each row alone: row b's token must be ITS token at row b's draw, for every draw and with no exclusions -- integers, so a
token is right or wrong -- whatever the other rows hold."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_util import dev_f32, dev_i32
from mila_amd import capi
from test_sample_chain_accept_gpu import CASES as ACCEPT_CASES
from test_sample_radix_gpu import CASES, DRAWS

pytestmark = pytest.mark.gpu

SENTINEL = -77
# one workgroup, two, a chunk edge (2049 = 8 * 256 + 1, 4097), the full preload (2^18 = kRadixBlocks * 256 * kRadixPre), past the preload and an odd row stride
VOCABS = (65, 257, 2049, 4097, 262144, 300001)
SETTINGS = sorted({c[1:] for c in CASES})           # (softcap, temperature, top_k, top_p): both truncations, top-k only, top-p only, neither


@functools.lru_cache(maxsize=None)
def _scratch(rows, V):
    nb = capi.sample_radix_rows_scratch_bytes(rows, V) if rows else capi.sample_radix_scratch_bytes(V)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device="cuda:0")


def _rows_logits(V, pad=0, fill=0.0):
    """[4, V + pad]: a random row, an all-equal row, a peaked row, another random row; the pad (never to be read) holds `fill`"""
    rng = np.random.default_rng(V)
    lg = np.full((4, V + pad), fill, dtype=np.float32)
    for b in (0, 3):
        lg[b, :V] = (rng.standard_normal(V) * 4.0).astype(np.float32)
        lg[b, rng.integers(0, V, 8)] += 9.0
    lg[1, :V] = 1.5
    lg[2, :V] = (rng.standard_normal(V) * 0.5).astype(np.float32)
    lg[2, (5 * V) // 7] += 60.0
    return lg


def _oracle(dev, V, setting, draws):
    """tokens [rows, len(draws)] of the one-row entry on each row alone; one readback"""
    softcap, t, k, p = setting
    out = torch.full((dev.shape[0], len(draws)), SENTINEL, dtype=torch.int32, device="cuda:0")
    for b in range(dev.shape[0]):
        for i, r in enumerate(draws):
            capi.sample_radix(dev[b, :V], out[b, i:i + 1], softcap, t, k, p, r, _scratch(0, V))
    return out.cpu().numpy()


def _draw_of(j, b):
    return (j + 7 * b) % len(DRAWS)          # call j gives row b this draw: every row meets every draw, the rows of a call different ones


@pytest.mark.parametrize("V", VOCABS)
def test_every_row_has_the_one_row_token_at_every_draw(V):
    lg = _rows_logits(V)
    dev = dev_f32(lg)
    n = len(DRAWS)
    draws = dev_f32(np.array([[DRAWS[_draw_of(j, b)] for b in range(4)] for j in range(n)], dtype=np.float32))
    for setting in SETTINGS:
        softcap, t, k, p = setting
        want = _oracle(dev, V, setting, DRAWS)
        assert (want >= 0).all() and (want < V).all()
        if 0 < k < V:
            assert (want[1] == V - 1).all()                  # all-equal logits under top-k: nothing is strictly above the (k+1)-th largest, no survivor
        if p < 1.0:
            assert (want[2] == (5 * V) // 7).all()           # the peaked row: the nucleus is the peak alone, the sample fixed whatever the draw
        for rows in (1, 2, 3, 4):
            out = torch.full((n, rows + 1), SENTINEL, dtype=torch.int32, device="cuda:0")
            for j in range(n):
                capi.sample_radix_rows(dev[:rows], out[j, :rows], softcap, t, k, p, draws[j, :rows], _scratch(rows, V))
            got = out.cpu().numpy()
            assert (got[:, rows] == SENTINEL).all(), "the word behind token_out was written"
            for b in range(rows):
                exp = np.array([want[b, _draw_of(j, b)] for j in range(n)])
                assert np.array_equal(got[:, b], exp), "V=%d %s rows=%d row %d: %s != one-row %s" % (V, setting, rows, b, got[:, b].tolist(), exp.tolist())


@pytest.mark.parametrize("V", [257, 4097, 300001])
def test_a_row_stride_beyond_the_vocabulary(V):
    """logits_stride > vocab: the pad behind each row would win every maximum if it were read"""
    pad = 13
    dev = dev_f32(_rows_logits(V, pad=pad, fill=1e30))
    plain = dev_f32(_rows_logits(V))
    draws = [0.0, 0.37, 0.81, 0.999999]
    for setting in (CASES[0][1:], CASES[3][1:]):
        softcap, t, k, p = setting
        want = _oracle(plain, V, setting, draws)
        out = dev_i32(np.full(5, SENTINEL))
        capi.sample_radix_rows(dev, out[:4], softcap, t, k, p, dev_f32(np.array(draws)), _scratch(4, V), vocab=V)
        assert out.cpu().tolist() == [int(want[b, b]) for b in range(4)] + [SENTINEL]


@pytest.mark.parametrize("V", [2049, 262144])
def test_a_row_does_not_see_the_other_rows(V):
    """row b's token stays when the other rows' logits and draws are replaced -- once by other numbers, once by a row that holds a NaN"""
    softcap, t, k, p = CASES[0][1:]
    base = _rows_logits(V)
    draws = np.array([0.11, 0.42, 0.63, 0.94], dtype=np.float32)
    out = dev_i32(np.full(4, SENTINEL))
    capi.sample_radix_rows(dev_f32(base), out, softcap, t, k, p, dev_f32(draws), _scratch(4, V))
    first = out.cpu().tolist()
    rng = np.random.default_rng(V + 1)
    for b in range(4):
        for poison in (False, True):
            other = (rng.standard_normal((4, V)) * 3.0).astype(np.float32)
            if poison:
                other[(b + 1) % 4, V // 3] = np.nan
                other[(b + 2) % 4, :] = np.inf
            other[b] = base[b]
            d = rng.uniform(0, 1, 4).astype(np.float32)
            d[b] = draws[b]
            out.fill_(SENTINEL)
            capi.sample_radix_rows(dev_f32(other), out, softcap, t, k, p, dev_f32(d), _scratch(4, V))
            got = out.cpu().tolist()
            assert got[b] == first[b], (b, poison, got, first)
            assert all(0 <= g < V for g in got), got         # a NaN row still ends on a token of the vocabulary


@pytest.mark.parametrize("V,active", [(4097, [1, 0, 1, 1]), (262144, [0, 1, 0, 0]), (65, [1, 1]), (257, [0])])
def test_the_rows_tail_advances_the_active_rows_only(V, active):
    rows = len(active)
    softcap, t, k, p = CASES[0][1:]
    dev = dev_f32(_rows_logits(V)[:rows])
    draws = [0.3, 0.6, 0.05, 0.9][:rows]
    want = _oracle(dev, V, (softcap, t, k, p), draws)
    tok = dev_i32(np.full(rows + 1, SENTINEL))
    pos = dev_i32(np.array([10 * (b + 1) for b in range(rows)] + [SENTINEL]))
    act = dev_i32(np.array(active + [1]))
    for step in (1, 2):                                      # a second call starts from what the first left
        capi.sample_radix_rows_advance(dev, tok[:rows], softcap, t, k, p, dev_f32(np.array(draws)), _scratch(rows, V), pos[:rows], act[:rows])
        assert tok.cpu().tolist() == [int(want[b, b]) if active[b] else SENTINEL for b in range(rows)] + [SENTINEL]
        assert pos.cpu().tolist() == [10 * (b + 1) + (step if active[b] else 0) for b in range(rows)] + [SENTINEL]


# ---- the chain tail: peaked rows, whose sample is fixed whatever the draw (under top-k / top-p nothing else survives), and two-peak rows, where the draw decides
CHAIN_V = 1000
CHAIN_SETTING = (0.0, 1.0, 8, 0.9)


def _chain_logits(rows):
    """row t: a peak at rows[t], or equal peaks at both indices of a tuple"""
    lg = np.zeros((len(rows), CHAIN_V), dtype=np.float32)
    for t, want in enumerate(rows):
        for i in (want if isinstance(want, tuple) else (want,)):
            lg[t, i] = 40.0
    return dev_f32(lg)


def _chain(tok, rows, draws, position):
    T = len(tok)
    tok_d = dev_i32(np.array(list(tok) + [SENTINEL]))
    res_d = dev_i32(np.full(T + 2, SENTINEL))
    pos_d = dev_i32(np.array([position, SENTINEL]))
    capi.sample_radix_chain_accept(tok_d[:T], res_d[:T + 1], _chain_logits(rows), *CHAIN_SETTING, dev_f32(np.array(draws)), _scratch(T, CHAIN_V), pos_d[:1])
    return tok_d.cpu().tolist(), res_d.cpu().tolist(), pos_d.cpu().tolist()


def _check_chain(name, tok, s, got, position=100):
    """s: the samples of the rows.  result = {n + 1, s_0 .. s_n}; tok[0] = s_n; the position word += n + 1; nothing else"""
    T = len(tok)
    n = next((t for t in range(T - 1) if s[t] != tok[t + 1]), T - 1)
    tok_after, res, pos = got
    assert res[:n + 2] == [n + 1] + s[:n + 1], (name, res)
    assert res[n + 2:] == [SENTINEL] * (T - n), (name, res)
    assert tok_after == [s[n]] + list(tok[1:]) + [SENTINEL], (name, tok_after)
    assert pos == [position + n + 1, SENTINEL], (name, pos)
    return n


@pytest.mark.parametrize("case", range(len(ACCEPT_CASES)))
@pytest.mark.parametrize("draw", [0.0, 0.25, 0.999999])
def test_the_accept_rule_on_samples(case, draw):
    """the greedy tail's cases; its tie rows become two equal peaks, where the draw 0.25 samples the lower index (the token the argmax tie rule gave there)"""
    name, tok, rows, n_want = ACCEPT_CASES[case]
    two_peaks = any(isinstance(r, tuple) for r in rows)
    if two_peaks:
        draw = 0.25
    s = [r[0] if isinstance(r, tuple) else r for r in rows]
    draws = [draw] * len(tok)
    # each row's sample is the one-row entry's on that row
    want = _oracle(_chain_logits(rows), CHAIN_V, CHAIN_SETTING, [draw])[:, 0].tolist()
    assert want == s, (name, want)
    assert _check_chain(name, tok, s, _chain(tok, rows, draws, 100)) == n_want, name


@pytest.mark.parametrize("row", [0, 1, 2])
def test_row_t_samples_at_its_own_draw(row):
    """equal logits at a < b on one row: the draw 0.25 samples a, 0.75 samples b.  The draft behind that row is a, so the row's own draw alone decides whether it
    verifies -- the other rows carry the opposite draw"""
    a, b = 21, 500
    tok = [11, 31, 41, 51]
    rows = [31, 41, 51, 61]
    tok[row + 1] = a
    rows[row] = (a, b)
    if row > 0:
        rows[row - 1] = tok[row]
    for mine, sample in ((0.25, a), (0.75, b)):
        draws = [1.0 - mine] * 4
        draws[row] = mine
        s = [r if not isinstance(r, tuple) else sample for r in rows]
        n = _check_chain("row %d draw %g" % (row, mine), tok, s, _chain(tok, rows, draws, 100))
        assert n == (3 if sample == a else row)


def test_two_chain_steps_advance_the_same_words():
    """the second step starts from what the first left: tok[0] and the position word"""
    T, rows = 3, [21, 31, 41]
    logits = _chain_logits(rows)
    draws = dev_f32(np.array([0.5, 0.1, 0.9]))
    tok_d, res_d, pos_d = dev_i32(np.array([11, 21, 99])), dev_i32(np.zeros(4)), dev_i32(np.array([7]))
    capi.sample_radix_chain_accept(tok_d, res_d, logits, *CHAIN_SETTING, draws, _scratch(T, CHAIN_V), pos_d)
    assert res_d.cpu().tolist()[:3] == [2, 21, 31] and tok_d.cpu().tolist() == [31, 21, 99] and pos_d.cpu().tolist() == [9]
    tok_d[1:] = torch.tensor([21, 31], dtype=torch.int32, device="cuda:0")
    tok_d[0] = 5
    capi.sample_radix_chain_accept(tok_d, res_d, logits, *CHAIN_SETTING, draws, _scratch(T, CHAIN_V), pos_d)
    assert res_d.cpu().tolist() == [3, 21, 31, 41] and tok_d.cpu().tolist()[0] == 41 and pos_d.cpu().tolist() == [12]
