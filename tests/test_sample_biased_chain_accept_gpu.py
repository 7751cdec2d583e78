"""GPU: the chain tails with a bias (include/mila_cdna4.h: the constrained chain step) -- sample_radix_biased_chain_accept_fp32 and
sample_argmax_biased_chain_accept_fp32.  Integer outputs: a token is right or wrong.  The oracle is the one-row biased entry on each row alone (row t's logits, row t's
table, for radix the draw draws[t]); the acceptance rule is restated here.  Every accept length 0 .. T - 1 is reached by editing the drafts to the samples just seen.
Vocabularies: one workgroup (65), a chunk edge (4097), the full preload and Gemma's vocabulary (262144)."""
import numpy as np
import pytest
import torch

from gpu_util import dev_f32, dev_i32
from mila_amd import capi
from test_sample_filtered_gpu import SENTINEL, _greedy_scratch, _scratch
from test_sample_radix_rows_gpu import _rows_logits

pytestmark = pytest.mark.gpu

VOCABS = (65, 4097, 262144)
SETTING = (30.0, 0.8, 40, 0.95)      # softcap, temperature, top_k, top_p: both truncations on
NEG_INF = np.float32(-np.inf)
POSITION = 100


def _tables(V, rows=4):
    """[rows, V] bias tables: finite values of both signs, a third of the entries -inf, another pattern per row"""
    rng = np.random.default_rng(V + 5)
    b = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    b[rng.random((rows, V)) < 0.33] = NEG_INF
    return b


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _one_row_samples(kind, dev, tables_dev, shared, draws, V):
    """row t's token from the one-row biased entry: row t's logits, row t's table (shared: table 0), the draw draws[t]"""
    out = torch.full((dev.shape[0],), SENTINEL, dtype=torch.int32, device="cuda:0")
    for t in range(dev.shape[0]):
        table = tables_dev[0 if shared else t]
        if kind == "radix":
            capi.sample_radix_biased(dev[t], out[t:t + 1], *SETTING, draws[t], None, None, table, _scratch(0, V))
        else:
            capi.sample_argmax_biased(dev[t], out[t:t + 1], SETTING[0], None, None, table, _greedy_scratch())
    return out.cpu().tolist()


def _chain(kind, tok, dev, bias_dev, draws, V, bias_stride=None):
    T = len(tok)
    tok_d, res_d, pos_d = dev_i32(np.array(list(tok) + [SENTINEL])), dev_i32(np.full(T + 2, SENTINEL)), dev_i32(np.array([POSITION, SENTINEL]))
    if kind == "radix":
        capi.sample_radix_biased_chain_accept(tok_d[:T], res_d[:T + 1], dev[:T], *SETTING, dev_f32(np.array(draws[:T], dtype=np.float32)), bias_dev, _scratch(T, V), pos_d[:1],
                                              bias_stride=bias_stride)
    else:
        capi.sample_argmax_biased_chain_accept(tok_d[:T], res_d[:T + 1], dev[:T], SETTING[0], bias_dev, _greedy_scratch(4), pos_d[:1], bias_stride=bias_stride)
    return tok_d.cpu().tolist(), res_d.cpu().tolist(), pos_d.cpu().tolist()


def _check(where, tok, s, got):
    """s: the samples of the rows.  result = {n + 1, s_0 .. s_n}; tok[0] = s_n; the position word += n + 1; nothing else"""
    T = len(tok)
    n = next((t for t in range(T - 1) if s[t] != tok[t + 1]), T - 1)
    tok_after, res, pos = got
    assert res[:n + 2] == [n + 1] + s[:n + 1], (where, res, s)
    assert res[n + 2:] == [SENTINEL] * (T - n), (where, res)
    assert tok_after == [s[n]] + list(tok[1:]) + [SENTINEL], (where, tok_after)
    assert pos == [POSITION + n + 1, SENTINEL], (where, pos)
    return n


@pytest.mark.parametrize("kind", ["greedy", "radix"])
@pytest.mark.parametrize("V", VOCABS)
def test_every_row_samples_as_the_one_row_biased_entry_and_every_accept_length_is_reached(V, kind):
    lg, tables = _rows_logits(V), _tables(V)
    dev, tables_dev = dev_f32(lg), dev_f32(tables)
    logits_before, tables_before = _bits(dev), _bits(tables_dev)
    draws = [0.03, 0.41, 0.77, 0.9990234]
    differ = 0
    for shared in (False, True):
        s = _one_row_samples(kind, dev, tables_dev, shared, draws, V)
        for t, tk in enumerate(s):
            assert 0 <= tk < V and np.isfinite(tables[0 if shared else t, tk]), "the one-row entry returned a forbidden token"
        plain = _one_row_samples(kind, dev, dev_f32(np.zeros((1, V), dtype=np.float32)), True, draws, V)
        differ += sum(a != b for a, b in zip(s, plain))
        bias_dev = tables_dev[0] if shared else tables_dev
        for T in (2, 3, 4):
            for n_right in range(T):      # the first n_right drafts are the samples just seen, the others are not
                tok = [7] + [s[t] if t < n_right else (s[t] + 1) % V for t in range(T - 1)]
                where = "V=%d %s T=%d %s tables, %d correct drafts" % (V, kind, T, "shared" if shared else "per-row", n_right)
                assert _check(where, tok, s[:T], _chain(kind, tok, dev, bias_dev, draws, V)) == min(n_right, T - 1), where
        # a shared table is also one given with stride 0 through a [rows, V] tensor
        tok = [7] + s[:2]
        if shared:
            assert _check("stride 0", tok, s[:3], _chain(kind, tok, dev, tables_dev, draws, V, bias_stride=0)) == 2
    assert differ >= 2, "the bias moved %d samples: the case shows little" % differ
    assert np.array_equal(_bits(dev), logits_before) and np.array_equal(_bits(tables_dev), tables_before), "logits or bias were written"


@pytest.mark.parametrize("V", VOCABS)
def test_a_null_bias_is_the_unbiased_chain_entry(V):
    dev = dev_f32(_rows_logits(V))
    draws = [0.2, 0.6, 0.05, 0.85]
    s = []
    for t in range(4):      # the unbiased one-row samples: the drafts that are all accepted
        out = dev_i32(np.array([SENTINEL]))
        capi.sample_radix(dev[t], out, *SETTING, draws[t], _scratch(0, V))
        s.append(int(out.cpu()[0]))
    for T in (2, 3, 4):
        for tok in ([7] + [(x + 1) % V for x in s[:T - 1]], [7] + s[:T - 1]):
            tok_d, res_d, pos_d = dev_i32(np.array(tok + [SENTINEL])), dev_i32(np.full(T + 2, SENTINEL)), dev_i32(np.array([POSITION, SENTINEL]))
            capi.sample_radix_chain_accept(tok_d[:T], res_d[:T + 1], dev[:T], *SETTING, dev_f32(np.array(draws[:T], dtype=np.float32)), _scratch(T, V), pos_d[:1])
            want = (tok_d.cpu().tolist(), res_d.cpu().tolist(), pos_d.cpu().tolist())
            assert want[1][0] == (T if tok[1:] == s[:T - 1] else 1), "the unbiased chain entry accepted %d of %s" % (want[1][0], tok)
            assert _chain("radix", tok, dev, None, draws, V) == want, (V, T)
    with pytest.raises(Exception):      # the greedy chain from the logits needs a table: refused, nothing launched
        _chain("greedy", [7, 1], dev, None, draws, V)


@pytest.mark.parametrize("kind", ["greedy", "radix"])
@pytest.mark.parametrize("V", VOCABS)
def test_a_row_with_one_finite_entry_returns_it_at_every_draw(V, kind):
    """the forced token of an automaton state: whatever the logits and the draw, the one atom of the masked distribution"""
    lg = _rows_logits(V)
    dev = dev_f32(lg)
    only = [int(np.argmin(lg[0, :V])), V - 1, 0, (5 * V) // 7 - 1]      # the least likely token of row 0, both ends, the neighbour of row 2's peak
    tables = np.full((4, V), NEG_INF, dtype=np.float32)
    for t, i in enumerate(only):
        tables[t, i] = np.float32(-2.5)
    tables_dev = dev_f32(tables)
    for r in (0.0, 0.5, 1.0):
        for T in (2, 3, 4):
            tok = [7] + only[:T - 1]      # the forced drafts: all accepted
            got = _chain(kind, tok, dev, tables_dev, [r] * 4, V)
            assert _check("V=%d %s T=%d r=%g" % (V, kind, T, r), tok, only[:T], got) == T - 1
