"""GPU: token log-probabilities (token_logprobs_rows_fp32 / token_logprobs_publish_fp32, csrc/logprobs.hip) against float64 on the same fp32 logits, the order of the
top-n ids, and the bitwise properties: row invariance, untouched rows and sentinels, run-to-run determinism, the published record.

Bars (absolute, on a log-probability): softcap 0 -- z is exact; expf / logf at a few ulp, a fixed-order sum of up to 2^18 terms (about 18 * 2^-24 relative) and one
rounding of z - m at a magnitude <= 64: about 1e-5 in all, the bar is 5e-5.  Softcap 30 adds the device tanhf's error on z_tok and on the sum, about
30 * 4 ulp * 2 = 1.4e-5 if tanhf is within 4 ulp: the bar is 1e-4.  The measured maxima are printed (-s) and recorded in profiles/r10_token_logprobs.md."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import dev_f32, dev_i32
from mila_amd import capi
from test_sample_radix_rows_gpu import VOCABS, _rows_logits

pytestmark = pytest.mark.gpu

BAR = {0.0: 5e-5, 30.0: 1e-4}
TOP_NS = (0, 1, 5, 20)
SENT_I = -77
SENT_F = -777.25
PEAK_ROW, EQUAL_ROW = 2, 1


def _scratch(rows, V, n):
    nb = capi.token_logprobs_scratch_bytes(rows, V, n)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device="cuda:0")


def _gapped_logits(V):
    """[4, V]: quiet noise below 21 planted values 30, 29, .. 10 at distinct places (another set per row): the top 21 stay well apart under a softcap of 30"""
    rng = np.random.default_rng(V + 17)
    lg = (rng.standard_normal((4, V)) * 0.5).astype(np.float32)
    for b in range(4):
        where = rng.choice(V, 21, replace=False)
        lg[b, where] = (30.0 - np.arange(21)).astype(np.float32)
    return lg


@functools.lru_cache(maxsize=None)
def _case(V, softcap, gapped=False):
    """the logits [4, V] (numpy and device) and their float64 reference: log-probabilities [4, V] and the ids in top-n order [4, 21]"""
    lg = _gapped_logits(V) if gapped else _rows_logits(V)
    x = lg.astype(np.float64)
    z = softcap * np.tanh(x / softcap) if softcap > 0 else x
    m = z.max(axis=1, keepdims=True)
    ref = (z - m) - np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    k = min(V, 21)
    order = np.stack([np.lexsort((np.arange(V), -z[b]))[:k] for b in range(4)])      # by -z, then by index
    return lg, dev_f32(lg), ref, order, z


def _tokens(V):
    return np.array([V // 2, V // 3, (5 * V) // 7, V - 1], dtype=np.int32)          # row 2: the peak of _rows_logits


def _run(dev, V, softcap, n, tokens, rows=4, active=None, count=None, vocab=None):
    """one call; returns (logprob [rows], ids [rows, n], logprobs [rows, n]) and checks the sentinel words behind every output"""
    lp = torch.full((rows + 1,), SENT_F, dtype=torch.float32, device="cuda:0")
    ids = torch.full((rows * n + 1,), SENT_I, dtype=torch.int32, device="cuda:0")
    tlp = torch.full((rows * n + 1,), SENT_F, dtype=torch.float32, device="cuda:0")
    capi.token_logprobs_rows(dev[:rows], dev_i32(tokens[:rows]), softcap, n, lp[:rows], ids[:rows * n] if n else None, tlp[:rows * n] if n else None,
                             _scratch(rows, V, n), active_dev=None if active is None else dev_i32(active), count_dev=None if count is None else dev_i32([count]), vocab=vocab)
    lp, ids, tlp = lp.cpu().numpy(), ids.cpu().numpy(), tlp.cpu().numpy()
    assert lp[rows] == SENT_F and ids[rows * n] == SENT_I and tlp[rows * n] == SENT_F, "a word behind an output was written"
    return lp[:rows], ids[:rows * n].reshape(rows, n), tlp[:rows * n].reshape(rows, n)


@functools.lru_cache(maxsize=None)
def _outputs(V, softcap, n, gapped=False):
    _, dev, _, _, _ = _case(V, softcap, gapped)
    return _run(dev, V, softcap, n, _tokens(V))


@pytest.mark.parametrize("softcap", [0.0, 30.0])
@pytest.mark.parametrize("V", VOCABS)
def test_against_float64(V, softcap):
    worst = 0.0
    for gapped in (False, True):
        _, _, ref, order, _ = _case(V, softcap, gapped)
        tok = _tokens(V)
        for n in TOP_NS:
            lp, ids, tlp = _outputs(V, softcap, n, gapped)
            err = np.abs(lp.astype(np.float64) - ref[np.arange(4), tok]).max()
            if n:
                assert (ids >= 0).all() and (ids < V).all()
                err = max(err, np.abs(tlp.astype(np.float64) - np.take_along_axis(ref, ids.astype(np.int64), axis=1)).max())
            worst = max(worst, err)
    print("token_logprobs V=%d softcap=%g: max |logprob - float64| = %.3e (bar %g)" % (V, softcap, worst, BAR[softcap]))
    assert worst <= BAR[softcap], (V, softcap, worst)


@pytest.mark.parametrize("V", VOCABS)
def test_ids_are_exact_without_a_softcap(V):
    _, _, ref, order, _ = _case(V, 0.0)
    peak = (5 * V) // 7
    for n in TOP_NS[1:]:
        lp, ids, tlp = _outputs(V, 0.0, n)
        assert np.array_equal(ids, order[:, :n]), (V, n, ids.tolist(), order[:, :n].tolist())       # placed ties included
        assert ids[EQUAL_ROW].tolist() == list(range(n))
        assert np.abs(tlp[EQUAL_ROW].astype(np.float64) + np.log(V)).max() <= BAR[0.0]
        assert abs(float(lp[EQUAL_ROW]) + np.log(V)) <= BAR[0.0]
        assert ids[PEAK_ROW, 0] == peak and tlp[PEAK_ROW, 0] > -1e-3
    lp0, _, _ = _outputs(V, 0.0, 0)
    assert lp0[PEAK_ROW] > -1e-3                           # _tokens' row 2 is the peak


@pytest.mark.parametrize("V", VOCABS)
def test_ids_under_a_softcap_on_rows_with_a_gap(V):
    _, _, _, order, z = _case(V, 30.0, True)
    for b in range(4):
        top = z[b, order[b]]
        assert (top[:-1] - top[1:] >= 1e-3).all(), "the test's own rows: the top 21 must be 1e-3 apart"
    for n in TOP_NS[1:]:
        _, ids, _ = _outputs(V, 30.0, n, True)
        assert np.array_equal(ids, order[:, :n]), (V, n)


@pytest.mark.parametrize("V", VOCABS)
def test_the_first_id_is_the_greedy_samplers_token(V):
    for gapped in (False, True):
        _, dev, _, _, _ = _case(V, 0.0, gapped)
        tok = torch.full((4,), SENT_I, dtype=torch.int32, device="cuda:0")
        scratch = torch.empty(int(capi.load().mila_cdna4_sample_scratch_bytes()), dtype=torch.uint8, device="cuda:0")
        for b in range(4):
            capi.call("sample_argmax_fp32", dev[b], tok[b:b + 1], V, scratch, capi.C.c_size_t(scratch.numel()))
        greedy = tok.cpu().numpy()
        for n in TOP_NS[1:]:
            _, ids, _ = _outputs(V, 0.0, n, gapped)
            assert np.array_equal(ids[:, 0], greedy), (V, n, ids[:, 0].tolist(), greedy.tolist())


@pytest.mark.parametrize("softcap", [0.0, 30.0])
@pytest.mark.parametrize("V", VOCABS)
def test_a_listed_token_has_the_bits_of_its_list_entry(V, softcap):
    _, dev, _, _, _ = _case(V, softcap)
    for n in TOP_NS[1:]:
        _, ids, tlp = _outputs(V, softcap, n)
        pick = [min(b, n - 1) for b in range(4)]                                     # row b asks for its entry b (the last one when the list is shorter)
        lp, ids2, tlp2 = _run(dev, V, softcap, n, np.array([ids[b, pick[b]] for b in range(4)], dtype=np.int32))
        assert np.array_equal(ids2, ids) and np.array_equal(tlp2.view(np.uint32), tlp.view(np.uint32))
        assert [int(v) for v in lp.view(np.uint32)] == [int(tlp[b, pick[b]].view(np.uint32)) for b in range(4)], (V, softcap, n)


@pytest.mark.parametrize("V", [65, 4097, 300001])
def test_a_token_at_minus_infinity_reports_minus_infinity(V):
    lg = _rows_logits(V).copy()
    tok = _tokens(V)
    tok[PEAK_ROW] = V // 5                                                           # not the peak
    for b in range(4):
        lg[b, tok[b]] = -np.inf
    for n in (0, 5):
        lp, ids, tlp = _run(dev_f32(lg), V, 0.0, n, tok)
        assert np.isneginf(lp).all(), lp
        if n:
            assert np.isfinite(tlp).all() and not (ids == tok[:, None]).any()


def _bits(out):
    return [a.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist() for a in out]


@pytest.mark.parametrize("n", [0, 5, 20])
@pytest.mark.parametrize("V", VOCABS)
def test_row_invariance_and_untouched_rows(V, n):
    """a row stride with a 13-float pad that would win every maximum if it were read; rows = 1 .. 4 against the one-row call on each row alone, bit for bit"""
    pad, softcap = 13, 30.0
    dev = dev_f32(_rows_logits(V, pad=pad, fill=1e30))
    tok = _tokens(V)
    alone = [_run(dev[b:b + 1], V, softcap, n, tok[b:b + 1], rows=1, vocab=V) for b in range(4)]
    for rows in (1, 2, 3, 4):
        got = _run(dev, V, softcap, n, tok, rows=rows, vocab=V)
        again = _run(dev, V, softcap, n, tok, rows=rows, vocab=V)
        assert _bits(got) == _bits(again), "two runs differ"
        for b in range(rows):
            assert _bits([a[b] for a in got]) == _bits([a[0] for a in alone[b]]), (V, n, rows, b)
    full = _run(dev, V, softcap, n, tok, vocab=V)
    assert _bits(full) == _bits(_outputs(V, softcap, n)), "the pad behind a row was read"
    # inactive rows, and rows from *count_dev on, keep their sentinels; the others are what they are without the words
    for active in ([1, 0, 1, 1], [0, 0, 0, 1], [0, 0, 0, 0]):
        got = _run(dev, V, softcap, n, tok, active=active, vocab=V)
        for b in range(4):
            if active[b]:
                assert _bits([a[b] for a in got]) == _bits([a[b] for a in full]), (active, b)
            else:
                assert got[0][b] == SENT_F and (got[1][b] == SENT_I).all() and (got[2][b] == SENT_F).all(), (active, b)
    for count in (0, 1, 3, 4):
        got = _run(dev, V, softcap, n, tok, count=count, vocab=V)
        for b in range(4):
            if b < count:
                assert _bits([a[b] for a in got]) == _bits([a[b] for a in full]), (count, b)
            else:
                assert got[0][b] == SENT_F and (got[1][b] == SENT_I).all() and (got[2][b] == SENT_F).all(), (count, b)


@pytest.mark.parametrize("seq", [6, (1 << 32) + 5])
@pytest.mark.parametrize("V", [257, 262144])
def test_publish_writes_one_record_into_its_slot(V, seq):
    words, ring_size, softcap = capi.token_logprobs_record_words(), 4, 30.0
    _, dev, _, _, _ = _case(V, softcap)
    tok = _tokens(V)
    seq_dev = torch.tensor([seq], dtype=torch.int64, device="cuda:0")
    for n in TOP_NS:
        for b in (0, PEAK_ROW):
            lp, ids, tlp = _outputs(V, softcap, n)
            ring = torch.full((ring_size * words + 1,), SENT_I, dtype=torch.int32, device="cuda:0")
            capi.token_logprobs_publish(dev[b], dev_i32(tok[b:b + 1]), softcap, n, seq_dev, ring, _scratch(1, V, n), ring_size=ring_size)
            got = ring.cpu().numpy()
            slot = seq % ring_size
            rec = got[slot * words:(slot + 1) * words]
            assert int(rec[0].view(np.uint32)) == seq & 0xffffffff and rec[1] == tok[b] and rec[3] == n
            assert int(rec[2].view(np.uint32)) == int(lp[b].view(np.uint32))
            assert rec[4:4 + n].tolist() == ids[b].tolist()
            assert rec[24:24 + n].view(np.uint32).tolist() == tlp[b].view(np.uint32).tolist()
            assert (rec[4 + n:24] == SENT_I).all() and (rec[24 + n:] == SENT_I).all()
            rest = np.delete(got, np.arange(slot * words, (slot + 1) * words))
            assert (rest == SENT_I).all(), "a neighbouring slot was written"
