"""GPU: row requests at the kernel level (csrc/sampling.hip: radix_requests_* / argmax_requests_*; include/mila_cdna4.h: row requests) -- a rows call whose rows each
sample under their own record in device memory.  The reference is the parent's one-row entry (sample_radix_biased_fp32 / sample_argmax_biased_fp32, which the
float64 tests hold) run on each row alone with that row's parameters, table, bias row and draw: tokens are integers, so a token is right or wrong.  The supports come
from the numpy restatement of tests/ref_sample_support.py.

Vocabularies: 1003 is no multiple of 4 and has fewer workgroups than either cap; 40007 lies above the 128-workgroup cap of the pass launches (32768) and below the
256-workgroup cap of the scale launch; 262144 lies above both (one case)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ref_sample_support as RS
import ref_sampling_filters as F
from gpu_util import dev_f32, dev_i32
from mila_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = -77
SOFTCAP = 30.0
# temperature, top_k, top_p, min_p, repetition, presence, frequency
GREEDY = (0.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0)
TOPK = (0.7, 5, 1.0, 0.0, 1.0, 0.0, 0.0)
TOPP = (1.0, 0, 0.9, 0.0, 1.0, 0.0, 0.0)
FULL = (1.3, 64, 0.95, 0.05, 1.2, 0.3, 0.2)
MIX = (GREEDY, TOPK, TOPP, FULL)
NEAR_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
DRAWS = [0.0, 1.0, NEAR_ONE] + [(i + 0.5) / 64.0 for i in range(64)]


def _penalized(req):
    return req[4] != 1.0 or req[5] != 0.0 or req[6] != 0.0


@functools.lru_cache(maxsize=None)
def _radix_scratch(rows, V):
    nb = capi.sample_radix_rows_scratch_bytes(rows, V) if rows else capi.sample_radix_scratch_bytes(V)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _argmax_scratch(rows):
    return torch.empty(rows * int(capi.load().mila_cdna4_sample_scratch_bytes()), dtype=torch.uint8, device="cuda:0")


def _params(reqs):
    p = torch.zeros(capi.sample_row_params_bytes(4), dtype=torch.uint8, device="cuda:0")
    assert p.numel() == 4 * 32
    for b, (t, k, tp, mp, rep, pres, freq) in enumerate(reqs):
        capi.sample_row_params_set(p, b, t, k, tp, mp, rep, pres, freq)
    return p


@functools.lru_cache(maxsize=None)
def _inputs(V):
    """four rows of logits (rows 2 and 3 flat enough that the nucleus holds many tokens), their tables (prompt flags and counts) and bias rows: row 1's bias holds
    -inf entries, row 2's is zero"""
    logits = np.stack([F.random_logits(V, seed=b) for b in range(4)])
    logits[2:] *= np.float32(0.3)
    tables = np.stack([F.make_table(logits[b], seed=b) for b in range(4)]).view(np.int32)
    rng = np.random.default_rng(V)
    bias = (rng.standard_normal((4, V)) * 0.5).astype(np.float32)
    bias[1, rng.random(V) < 0.3] = -np.inf
    bias[2] = 0.0
    return logits, tables, bias


def _one_row(logits, req, table, bias, r, softcap=SOFTCAP):
    """the one-row entry's token on this row alone: device tensors; the table is given only where the request has a penalty, and is a copy (the entry counts in it)"""
    t, k, tp, mp, rep, pres, freq = req
    V = logits.numel()
    out = dev_i32(np.array([SENTINEL]))
    tab = table.clone() if (table is not None and _penalized(req)) else None
    if t > 0:
        capi.sample_radix_biased(logits, out, softcap, t, k, tp, r, (mp, rep, pres, freq), tab, bias, _radix_scratch(0, V))
    else:
        capi.sample_argmax_biased(logits, out, softcap, (mp, rep, pres, freq), tab, bias, _argmax_scratch(1))
    return int(out.cpu()[0])


def _requests_call(logits, reqs, draws, tables, bias, advance=None, vocab=None, softcap=SOFTCAP):
    """both entries, the greedy one behind the stochastic one, on `rows` rows; returns (tokens, tables after)"""
    rows = logits.shape[0]
    V = logits.shape[1] if vocab is None else vocab
    params = _params(list(reqs) + [GREEDY] * (4 - rows))
    tok = dev_i32(np.full(rows + 1, SENTINEL))
    tab = None if tables is None else tables.clone()
    d = dev_f32(np.array(draws, dtype=np.float32))
    if advance is None:
        capi.sample_radix_requests_rows(logits, tok[:rows], softcap, params, d, tab, bias, _radix_scratch(rows, V), vocab=vocab)
        capi.sample_argmax_requests_rows(logits, tok[:rows], softcap, params, tab, bias, _argmax_scratch(rows), vocab=vocab)
    else:
        pos, act = advance
        capi.sample_radix_requests_rows_advance(logits, tok[:rows], softcap, params, d, tab, bias, _radix_scratch(rows, V), pos, act, vocab=vocab)
        capi.sample_argmax_requests_rows_advance(logits, tok[:rows], softcap, params, tab, bias, _argmax_scratch(rows), pos, act, vocab=vocab)
    got = tok.cpu().tolist()
    assert got[rows] == SENTINEL, "the word behind token_out was written"
    return got[:rows], tab


@functools.lru_cache(maxsize=None)
def _oracle(V, with_bias):
    """want[request index of MIX][draw index] on row b = request index, computed once per vocabulary"""
    logits, tables, bias = _inputs(V)
    lg, tb = dev_f32(logits), dev_i32(tables)
    bs = dev_f32(bias) if with_bias else None
    want = np.zeros((4, len(DRAWS)), dtype=np.int64)
    for b, req in enumerate(MIX):
        for j, r in enumerate(DRAWS if req[0] > 0 else DRAWS[:1]):
            want[b, j] = _one_row(lg[b], req, tb[b], None if bs is None else bs[b], r)
        if req[0] <= 0:
            want[b, :] = want[b, 0]
    return want


def _draw_of(j, b):
    return (j + 17 * b) % len(DRAWS)


@pytest.mark.parametrize("V,row_counts,perms", [(1003, (1, 2, 3, 4), ((0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2))), (40007, (4, 3), ((0, 1, 2, 3), (2, 0, 3, 1))),
                                               (262144, (4,), ((0, 1, 2, 3),))])
def test_every_row_has_its_one_row_token_at_every_draw(V, row_counts, perms):
    """four different requests in one call, with per-row tables and bias rows; the same requests permuted over the rows give the permuted tokens"""
    logits, tables, bias = _inputs(V)
    want = _oracle(V, True)
    assert len(np.unique(want[1])) > 1 and len(np.unique(want[3])) > 1, "the draws decide nothing: the case shows little"
    for perm in perms:
        for rows in row_counts:
            who = list(perm[:rows])
            lg, tb, bs = dev_f32(logits[who]), dev_i32(tables[who]), dev_f32(bias[who])
            reqs = [MIX[i] for i in who]
            for j in range(len(DRAWS)):
                got, tab = _requests_call(lg, reqs, [DRAWS[_draw_of(j, b)] for b in range(rows)], tb, bs)
                exp = [int(want[i, _draw_of(j, b)]) for b, i in enumerate(who)]
                assert got == exp, "V=%d perm %s rows=%d draws #%d: %s != one-row %s" % (V, perm, rows, j, got, exp)
                if j % 16 == 0:      # the tables: exactly one count, at the token of the penalized row
                    diff = (tab.cpu().numpy() - tables[who]).astype(np.int64)
                    for b, i in enumerate(who):
                        hit = np.flatnonzero(diff[b])
                        assert hit.tolist() == ([got[b]] if _penalized(MIX[i]) else []) and diff[b].sum() == (1 if _penalized(MIX[i]) else 0), (b, hit)


@pytest.mark.parametrize("V", [1003, 40007])
def test_a_row_keeps_its_token_beside_rows_of_nan(V):
    """each of the four requests in row 0, the other rows' logits NaN (their records the other three requests)"""
    logits, tables, bias = _inputs(V)
    want = _oracle(V, False)
    for i in range(4):
        who = [i] + [x for x in range(4) if x != i]
        lg = logits[who].copy()
        lg[1:] = np.nan
        lg_dev, tb = dev_f32(lg), dev_i32(tables[who])
        for j in range(0, len(DRAWS), 1 if V == 1003 else 6):
            got, _ = _requests_call(lg_dev, [MIX[x] for x in who], [DRAWS[j], 0.3, 0.6, 0.9], tb, None)
            assert got[0] == want[i, j], (V, i, j, got)
            assert all(0 <= g < V for g in got), got


def test_every_stochastic_token_lies_in_the_exact_support():
    """no softcap and power-of-two temperatures: x = l / t is exact, so ref_sample_support's top-k set is exact; the logits are designed so that the nucleus and min-p
    cuts are far from flipping (asserted: a margin of 1e-5 of the total, forty times the device's error -- expf within a few ulps, 1e-7 relative, and the 2^-22 of the
    fixed-point truncation)"""
    V = 1003
    reqs = ((0.5, 5, 1.0, 0.0, 1.0, 0.0, 0.0), (1.0, 0, 0.9, 0.0, 1.0, 0.0, 0.0), (2.0, 64, 0.95, 0.05, 1.25, 0.5, 0.25), (1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0))
    logits, tables, _ = _inputs(V)
    sup = []
    for b, (t, k, p, mp, rep, pres, freq) in enumerate(reqs):
        x3 = F.adjusted_logits(logits[b], tables[b], 0.0, rep, pres, freq) if _penalized(reqs[b]) else logits[b]
        s = RS.support(x3, 0.0, t, k, p, mp)
        assert s.m_nucleus > 1e-5 and s.m_minp > 1e-5, (b, s.m_nucleus, s.m_minp)
        sup.append(s)
    assert len(sup[0].set) == 5 and 1 < len(sup[2].set) <= 64 and len(sup[3].set) == V
    params = _params(reqs)
    lg, tb = dev_f32(logits), dev_i32(tables)
    seen = [set() for _ in reqs]
    for j in range(len(DRAWS)):
        tok = dev_i32(np.full(4, SENTINEL))
        capi.sample_radix_requests_rows(lg, tok, 0.0, params, dev_f32(np.array([DRAWS[_draw_of(j, b)] for b in range(4)])), tb.clone(), None, _radix_scratch(4, V))
        for b, g in enumerate(tok.cpu().tolist()):
            assert g in sup[b].set, "row %d sampled %d outside its support at draw %g" % (b, g, DRAWS[_draw_of(j, b)])
            seen[b].add(g)
    assert all(len(s) > 1 for s in seen), "the draws decide nothing: the case shows little"
    ends = dev_i32(np.full(4, SENTINEL))      # the end draws: the first survivor at 0, the last at 1
    for r, pick in ((0.0, lambda s: int(s.tokens[0])), (1.0, lambda s: s.last())):
        capi.sample_radix_requests_rows(lg, ends, 0.0, params, dev_f32(np.full(4, r)), tb.clone(), None, _radix_scratch(4, V))
        assert ends.cpu().tolist() == [pick(s) for s in sup], r


def test_duplicated_maxima_and_values_equal_across_a_digit_edge():
    """greedy: the lowest id among equal maxima, with and without a bias.  Stochastic: two values on the two sides of a radix digit edge (keys ... 0x3FF | ... 0x400,
    the last bin of one second-pass digit and the first of the next) and a tie group at the top-k boundary, against the one-row entry at every draw"""
    V = 1003
    rng = np.random.default_rng(7)
    lg = np.minimum((rng.standard_normal((4, V)) * 2.0).astype(np.float32), np.float32(4.0))
    top = np.float32(11.0)
    lg[0, [17, 400, 999]] = top                                   # greedy, no bias: ties to 17
    lg[1, [900, 23, 512]] = top                                   # greedy with a bias row of zeros but -inf at 23: ties to 512
    # keys 0xC0A003FF | 0xC0A00400 (about 5.0): neighbours in value, the last bin of one second-pass digit and the first of the next.  No softcap, a bias row of zeros
    # and t = 1: the scaled values are the logits, and the four are the largest of rows 2 and 3
    lo, hi = RS.float_of(np.array([0xC0A003FF, 0xC0A00400], dtype=np.uint32))
    assert 4.0 < lo < hi < top
    for b in (2, 3):
        lg[b, [5, 800]] = lo
        lg[b, [300, 301]] = hi
    bias = np.zeros((4, V), dtype=np.float32)
    bias[1, 23] = -np.inf
    reqs = (GREEDY, GREEDY, (1.0, 2, 1.0, 0.0, 1.0, 0.0, 0.0), (1.0, 3, 0.9, 0.0, 1.0, 0.0, 0.0))
    lg_dev, bs_dev = dev_f32(lg), dev_f32(bias)
    seen = [set(), set()]
    for j, r in enumerate(DRAWS):
        got, _ = _requests_call(lg_dev, reqs, [r] * 4, None, bs_dev, softcap=0.0)
        assert got[0] == 17 and got[1] == 512, got
        for b in (2, 3):
            assert got[b] == _one_row(lg_dev[b], reqs[b], None, bs_dev[b], r, softcap=0.0), (b, r, got)
            seen[b - 2].add(got[b])
    # top-k 2: strictly above the third largest (the lower pair's value) -- the upper pair; top-k 3: strictly above the fourth largest -- the upper pair again
    assert seen[0] == {300, 301} and seen[1] == {300, 301}, seen
    got, _ = _requests_call(lg_dev[:1], reqs[:1], [0.5], None, None)      # no bias at all: sample_argmax_fp32 on the logits as they are
    assert got == [17]


def test_a_bias_row_that_allows_exactly_one_token():
    V = 1003
    logits, tables, _ = _inputs(V)
    bias = np.zeros((4, V), dtype=np.float32)
    bias[0] = -np.inf
    bias[0, 777] = -3.0
    bias[1] = -np.inf
    bias[1, 4] = 0.0
    bias[2, ::2] = -np.inf
    bias[3, 1::2] = -np.inf
    reqs = (FULL, GREEDY, TOPP, TOPK)
    lg, tb, bs = dev_f32(logits), dev_i32(tables), dev_f32(bias)
    for r in DRAWS:
        got, _ = _requests_call(lg, reqs, [r] * 4, tb, bs)
        assert got[0] == 777 and got[1] == 4 and got[2] % 2 == 1 and got[3] % 2 == 0, (r, got)
        for b in (2, 3):
            assert got[b] == _one_row(lg[b], reqs[b], tb[b], bs[b], r), (b, r)


@pytest.mark.parametrize("V,active", [(1003, [1, 0, 1, 1]), (40007, [0, 1, 1, 0]), (1003, [1, 1]), (1003, [0])])
def test_the_two_tails_advance_each_active_row_once_and_leave_the_others(V, active):
    """inactive rows: token, position and table words bit-identical before and after; an active penalized row's table gains exactly one count, at its token"""
    rows = len(active)
    logits, tables, bias = _inputs(V)
    reqs = (FULL, GREEDY, (0.0, 0, 1.0, 0.0, 1.5, 0.2, 0.1), TOPK)[:rows]      # stochastic penalized, greedy, greedy penalized, stochastic
    lg, tb, bs = dev_f32(logits[:rows]), dev_i32(tables[:rows]), dev_f32(bias[:rows])
    draws = [0.3, 0.6, 0.05, 0.9][:rows]
    want = [_one_row(lg[b], reqs[b], tb[b], bs[b], draws[b]) for b in range(rows)]
    pos = dev_i32(np.array([10 * (b + 1) for b in range(rows)] + [SENTINEL]))
    act = dev_i32(np.array(active + [1]))
    got, tab = _requests_call(lg, reqs, draws, tb, bs, advance=(pos[:rows], act[:rows]))
    assert got == [want[b] if active[b] else SENTINEL for b in range(rows)]
    assert pos.cpu().tolist() == [10 * (b + 1) + (1 if active[b] else 0) for b in range(rows)] + [SENTINEL]
    diff = (tab.cpu().numpy() - tables[:rows]).astype(np.int64)
    for b in range(rows):
        counted = active[b] and _penalized(reqs[b])
        assert np.flatnonzero(diff[b]).tolist() == ([want[b]] if counted else []) and diff[b].sum() == (1 if counted else 0), b


def test_a_batch_of_one_class_leaves_the_other_entrys_rows_alone():
    """all rows stochastic: the greedy entry writes nothing; all rows greedy: the stochastic entry writes nothing"""
    V = 1003
    logits, tables, _ = _inputs(V)
    lg, tb = dev_f32(logits), dev_i32(tables)
    tok, pos, act = dev_i32(np.full(4, SENTINEL)), dev_i32(np.arange(4)), dev_i32(np.ones(4))
    tab = tb.clone()
    capi.sample_argmax_requests_rows_advance(lg, tok, SOFTCAP, _params((TOPK, TOPP, FULL, TOPK)), tab, None, _argmax_scratch(4), pos, act)
    capi.sample_radix_requests_rows_advance(lg, tok, SOFTCAP, _params((GREEDY,) * 4), dev_f32(np.full(4, 0.5)), tab, None, _radix_scratch(4, V), pos, act)
    assert tok.cpu().tolist() == [SENTINEL] * 4 and pos.cpu().tolist() == [0, 1, 2, 3] and torch.equal(tab, tb)


def test_new_parameters_for_a_row_take_effect_in_stream_order():
    """the record is device memory: a setter between two calls changes what the second samples, with no sync and the same launch arguments"""
    V = 1003
    logits, _, _ = _inputs(V)
    lg = dev_f32(logits[:1])
    params = _params((TOPK,))
    a, b = dev_i32(np.array([SENTINEL])), dev_i32(np.array([SENTINEL]))
    d = dev_f32(np.array([0.77]))
    capi.sample_radix_requests_rows(lg, a, SOFTCAP, params, d, None, None, _radix_scratch(1, V))
    capi.sample_row_params_set(params, 0, *TOPP)
    capi.sample_radix_requests_rows(lg, b, SOFTCAP, params, d, None, None, _radix_scratch(1, V))
    assert int(a.cpu()[0]) == _one_row(lg[0], TOPK, None, None, 0.77) and int(b.cpu()[0]) == _one_row(lg[0], TOPP, None, None, 0.77)


def test_bad_arguments_are_refused_before_any_launch():
    V = 1003
    lib = capi.load()
    logits, tables, _ = _inputs(V)
    lg, tb = dev_f32(logits), dev_i32(tables)
    tok, pos, act, d = dev_i32(np.full(4, SENTINEL)), dev_i32(np.zeros(4)), dev_i32(np.ones(4)), dev_f32(np.zeros(4))
    params = torch.zeros(128, dtype=torch.uint8, device="cuda:0")
    good = dict(temperature=1.0, top_k=5, top_p=0.9)
    for bad in (dict(temperature=float("nan")), dict(temperature=float("inf")), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(min_p=1.0),
                dict(min_p=-0.1), dict(top_k=-1), dict(top_p=0.0), dict(top_p=float("nan")), dict(presence_penalty=float("inf")), dict(frequency_penalty=float("nan"))):
        with pytest.raises(capi.InvalidArgument):
            capi.sample_row_params_set(params, 0, **{**good, **bad})
    for row in (-1, 4):
        with pytest.raises(capi.InvalidArgument):
            capi.sample_row_params_set(params, row, **good)
    with pytest.raises(capi.InvalidArgument):
        capi.sample_row_params_set(params[2:], 0, **good)
    with pytest.raises(capi.InvalidArgument):
        capi.call("sample_row_params_set", params, 0, None)
    assert not params.cpu().numpy().any(), "a refused setter wrote the record"
    assert capi.sample_row_params_bytes(0) == 0 and capi.sample_row_params_bytes(5) == 0

    rs, as_ = _radix_scratch(4, V), _argmax_scratch(4)
    z = C.c_size_t

    def radix(rows=4, scratch=rs, nbytes=None, stride=V, vocab=V, params_=params, draws=d, adv=False, table_stride=V):
        args = [capi._ptr(lg), z(stride), capi._ptr(tok), rows, vocab, C.c_float(SOFTCAP), capi._ptr(params_), capi._ptr(draws), capi._ptr(tb), z(table_stride), None, z(0),
                capi._ptr(scratch), z(scratch.numel() if nbytes is None else nbytes)]
        if adv:
            return lib.mila_cdna4_sample_radix_requests_rows_advance_fp32(*args, capi._ptr(pos), None, None)      # active_dev missing
        return lib.mila_cdna4_sample_radix_requests_rows_fp32(*args, None)

    def argmax(rows=4, scratch=as_, nbytes=None, stride=V, vocab=V):
        return lib.mila_cdna4_sample_argmax_requests_rows_fp32(capi._ptr(lg), z(stride), capi._ptr(tok), rows, vocab, C.c_float(SOFTCAP), capi._ptr(params), capi._ptr(tb), z(V),
                                                               None, z(0), capi._ptr(scratch), z(scratch.numel() if nbytes is None else nbytes), None)

    for fn in (radix, argmax):
        assert fn(rows=0) == capi.MILA_E_INVALID_ARGUMENT and fn(rows=5) == capi.MILA_E_INVALID_ARGUMENT
        assert fn(vocab=0) == capi.MILA_E_INVALID_ARGUMENT and fn(stride=V - 1) == capi.MILA_E_INVALID_ARGUMENT
        assert fn(nbytes=1024) == capi.MILA_E_SCRATCH_TOO_SMALL
    assert radix(scratch=torch.empty(rs.numel() + 8, dtype=torch.uint8, device="cuda:0")[4:], nbytes=rs.numel()) == capi.MILA_E_INVALID_ARGUMENT      # misaligned scratch
    assert argmax(scratch=torch.empty(as_.numel() + 8, dtype=torch.uint8, device="cuda:0")[1:], nbytes=as_.numel()) == capi.MILA_E_INVALID_ARGUMENT
    assert radix(adv=True) == capi.MILA_E_INVALID_ARGUMENT and radix(table_stride=V - 1) == capi.MILA_E_INVALID_ARGUMENT
    assert tok.cpu().tolist() == [SENTINEL] * 4 and pos.cpu().tolist() == [0] * 4 and torch.equal(tb, dev_i32(tables))
