"""GPU: the filtered sampler entries of the C ABI (include/mila_cdna4.h: sampling filters) -- repetition / presence / frequency penalties from the token table,
min-p, the penalized greedy sampler, the table update and the table maintenance.  Integer outputs: a token is right or wrong.  Without a softcap the adjusted logit
is restated bit for bit on the host (tests/ref_sampling_filters.py), so the filtered entry must return, at EVERY draw, what the unfiltered entry returns on the
host-adjusted logits; with a softcap (tanhf differs by ulps between host and device) decisive draws are held to the NumPy oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ref_sampling_filters as R
from gpu_util import dev_f32, dev_i32
from mila_amd import capi
from test_sample_radix_gpu import CASES, DRAWS
from test_sample_radix_rows_gpu import VOCABS, _rows_logits

pytestmark = pytest.mark.gpu

SENTINEL = -77
FLT_MAX = np.finfo(np.float32).max
assert VOCABS == (65, 257, 2049, 4097, 262144, 300001)


@functools.lru_cache(maxsize=None)
def _scratch(rows, V):
    nb = capi.sample_radix_rows_scratch_bytes(rows, V) if rows else capi.sample_radix_scratch_bytes(V)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _greedy_scratch(rows=1):
    return torch.empty(rows * int(capi.load().mila_cdna4_sample_scratch_bytes()), dtype=torch.uint8, device="cuda:0")


def _guarded(words):
    """int32 words with a sentinel behind them"""
    return np.concatenate([np.asarray(words, dtype=np.int32).reshape(-1), np.array([SENTINEL], dtype=np.int32)])


def _plain(dev, setting, draws):
    """tokens of sample_radix_fp32 on `dev` at every draw; one readback"""
    softcap, t, k, p = setting
    out = torch.full((len(draws),), SENTINEL, dtype=torch.int32, device="cuda:0")
    for i, r in enumerate(draws):
        capi.sample_radix(dev, out[i:i + 1], softcap, t, k, p, r, _scratch(0, dev.numel()))
    return out.cpu().tolist()


def _filtered(dev, setting, draws, filters, table_np):
    """tokens of sample_radix_filtered_fp32 at every draw, each from a fresh copy of the table (None: no table); one readback"""
    softcap, t, k, p = setting
    out = torch.full((len(draws),), SENTINEL, dtype=torch.int32, device="cuda:0")
    fresh = None if table_np is None else dev_i32(table_np)
    for i, r in enumerate(draws):
        table = None if fresh is None else fresh.clone()
        capi.sample_radix_filtered(dev, out[i:i + 1], softcap, t, k, p, r, filters, table, _scratch(0, dev.numel()))
    return out.cpu().tolist()


# ---- 1. exact identity without a softcap
@pytest.mark.parametrize("V", VOCABS)
def test_penalties_equal_the_unfiltered_sampler_on_host_adjusted_logits(V):
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    lg = R.random_logits(V)
    table = R.make_table(lg)
    dev = dev_f32(lg)
    unpenalized = _plain(dev, setting, DRAWS)
    for pen in R.PENALTIES:
        filters = (0.0,) + pen
        x3 = R.adjusted_logits(lg, table, 0.0, *pen)
        want = _plain(dev_f32(x3), setting, DRAWS)
        got = _filtered(dev, setting, DRAWS, filters, table)
        assert got == want, "V=%d %s: %s != unfiltered on x3 %s" % (V, pen, got, want)
        changed = sum(a != b for a, b in zip(got, unpenalized))
        print("V=%d %s: the penalties change %d of %d tokens" % (V, pen, changed, len(DRAWS)))
        if V >= 257:
            assert changed >= 1, "the penalties changed no token: the case shows nothing"


@pytest.mark.parametrize("V", VOCABS)
def test_penalized_greedy_equals_the_argmax_of_host_adjusted_logits(V):
    lg = R.greedy_logits(V)                                         # a tie for the place behind the top
    table = R.make_table(lg)
    dev = dev_f32(lg)
    out = torch.full((2 * len(R.GREEDY_PENALTIES) + 1,), SENTINEL, dtype=torch.int32, device="cuda:0")
    capi.call("sample_argmax_fp32", dev, out[0:1], V, _greedy_scratch(), C.c_size_t(_greedy_scratch().numel()))
    for j, pen in enumerate(R.GREEDY_PENALTIES):
        x3 = R.adjusted_logits(lg, table, 0.0, *pen)
        capi.call("sample_argmax_fp32", dev_f32(x3), out[1 + 2 * j:2 + 2 * j], V, _greedy_scratch(), C.c_size_t(_greedy_scratch().numel()))
        capi.sample_argmax_filtered(dev, out[2 + 2 * j:3 + 2 * j], 0.0, (0.0,) + pen, dev_i32(table), _greedy_scratch())
    got = out.cpu().tolist()
    moved = False
    for j, pen in enumerate(R.GREEDY_PENALTIES):
        assert got[2 + 2 * j] == got[1 + 2 * j] == R.argmax_filtered(lg, 0.0, (0.0,) + pen, table), (V, pen, got)
        moved |= got[2 + 2 * j] != got[0]
    if V >= 257:
        assert moved, "no penalty moved the greedy token: the case shows nothing"


def test_penalized_greedy_ties_go_to_the_lower_id_and_the_softcap_comes_first():
    V = 3000
    lg = np.full(V, -1.0, dtype=np.float32)
    lg[[700, 1900, 2500]] = [200.0, 100.0, 100.0]                   # under softcap 30 all three saturate near 30; 700 stays the largest
    table = np.zeros(V, dtype=np.int32)
    table[700] = 2                                                  # generated twice: presence 0.5 takes it below the other two, which tie
    out = dev_i32(np.full(3, SENTINEL))
    capi.sample_argmax_filtered(dev_f32(lg), out[0:1], 30.0, (0.0, 1.0, 0.5, 0.0), dev_i32(table), _greedy_scratch())
    capi.sample_argmax_filtered(dev_f32(lg), out[1:2], 0.0, (0.0, 1.0, 0.5, 0.0), dev_i32(table), _greedy_scratch())     # no softcap: 199.5 still wins
    capi.sample_argmax_filtered(dev_f32(lg), out[2:3], 30.0, (0.0, 1.0, 0.5, 0.0), None, _greedy_scratch())            # no table: no penalty
    assert out.cpu().tolist() == [1900, 700, 700]


# ---- 2. with the softcap: decisive draws against the NumPy oracle
def _sweep(lg, setting, filters, table, floor=12):
    softcap, t, k, p = setting
    d = R.Distribution(lg, softcap, t, k, p, filters, table)
    base = R.Distribution(lg, softcap, t, k, p)
    got = _filtered(dev_f32(lg), setting, DRAWS, filters, table)
    decisive = differ = 0
    for r, g in zip(DRAWS, got):
        tok, m = d.draw(r)
        if d.decisive(m):
            assert g == tok, "r=%g: %d != oracle %d (margins %s)" % (r, g, tok, m)
            decisive += 1
            differ += tok != base.draw(r)[0]
    print("V=%d %s filters %s: %d of %d draws decisive, %d of them differ from the unfiltered token" % (lg.size, setting, filters, decisive, len(DRAWS), differ))
    assert decisive >= floor, "too few decisive draws (%d)" % decisive
    return decisive, differ


@pytest.mark.parametrize("case", [(262144, 30.0, 0.8, 64, 0.95), (2049, 30.0, 0.8, 64, 0.95)])
def test_penalties_behind_the_softcap_match_the_oracle_on_decisive_draws(case):
    assert case in CASES
    V, setting = case[0], case[1:]
    lg = R.random_logits(V)
    table = R.make_table(lg)
    differ = [_sweep(lg, setting, (0.0,) + pen, table)[1] for pen in R.PENALTIES]
    assert min(differ) >= 1, "a penalty triple moved no decisive token: %s" % differ
    assert sum(differ) >= 6, "the penalties moved only %s decisive tokens" % differ


# ---- 3. min-p
def _minp_inputs(V):
    lg = R.random_logits(V, seed=5)
    return lg


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("min_p", [0.05, 0.3])
def test_min_p_without_a_nucleus_equals_the_unfiltered_sampler_on_masked_logits(V, min_p):
    """top_p = 1: the survivors of min-p are those of the unfiltered sampler on logits whose failing entries are -FLT_MAX (their e underflows to 0; the maximum, and so
    every other e, is unchanged), at every draw"""
    filters = (min_p, 1.0, 0.0, 0.0)
    for setting in ((0.0, 1.0, 0, 1.0), (0.0, 1.5, 0, 1.0)):
        softcap, t, k, p = setting
        lg = _minp_inputs(V)
        d = R.Distribution(lg, softcap, t, k, p, filters)
        assert d.m_minp > 1e-4, "a survivor sits on the min-p threshold (ratio within %g of 1)" % d.m_minp
        pre = R.Distribution(lg, softcap, t, k, p)
        assert 0 < (d.e > 0).sum() < (pre.e > 0).sum(), "min-p drops nothing here"
        masked = np.where(d.e == 0, -FLT_MAX, lg).astype(np.float32)
        want = _plain(dev_f32(masked), setting, DRAWS)
        got = _filtered(dev_f32(lg), setting, DRAWS, filters, None)
        assert got == want, "V=%d min_p=%g %s: %s != %s" % (V, min_p, setting, got, want)
        assert all((d.e > 0)[g] for g in got)


@pytest.mark.parametrize("V,min_p", [(262144, 0.05), (262144, 0.3), (2049, 0.05), (4097, 0.3)])
def test_min_p_behind_a_nucleus_matches_the_oracle_on_decisive_draws(V, min_p):
    lg = _minp_inputs(V)
    setting = (0.0, 1.2, 0, 0.9)
    filters = (min_p, 1.0, 0.0, 0.0)
    d = R.Distribution(lg, *setting, filters)
    assert d.m_minp > 1e-4
    _sweep(lg, setting, filters, None)


@pytest.mark.parametrize("V", VOCABS)
def test_any_min_p_leaves_the_peak_of_a_peaked_row(V):
    lg = _rows_logits(V)[2]
    for min_p in (1e-6, 0.05, 0.9):
        got = _filtered(dev_f32(lg), (0.0, 1.0, 0, 1.0), DRAWS, (min_p, 1.0, 0.0, 0.0), None)
        assert got == [(5 * V) // 7] * len(DRAWS), (V, min_p, got)


# ---- 4. the table update and the table maintenance
@pytest.mark.parametrize("V", [65, 4097, 300001])
def test_the_sample_is_counted_in_the_table_and_nothing_else_is_written(V):
    t, k, p = R.IDENTITY_SETTINGS[V]
    lg = R.random_logits(V)
    table = R.make_table(lg)
    dev = dev_f32(lg)
    filters = (0.0, 1.15, 0.5, 0.25)
    for greedy in (False, True):
        buf = dev_i32(_guarded(table))
        tok = dev_i32(np.full(2, SENTINEL))
        if greedy:
            capi.sample_argmax_filtered(dev, tok[0:1], 0.0, filters, buf[:V], _greedy_scratch())
        else:
            capi.sample_radix_filtered(dev, tok[0:1], 0.0, t, k, p, 0.37, filters, buf[:V], _scratch(0, V))
        s, behind = tok.cpu().tolist()
        assert 0 <= s < V and behind == SENTINEL
        after = buf.cpu().numpy()
        want = _guarded(table)
        R.count_token(want, s)
        assert np.array_equal(after, want), "exactly table[%d] goes up by one" % s
        assert (after[s] < 0) == (table[s] < 0)                     # bit 31 is untouched
    # without a table nothing is written but the token
    tok = dev_i32(np.full(2, SENTINEL))
    capi.sample_radix_filtered(dev, tok[0:1], 0.0, t, k, p, 0.37, (0.05, 1.15, 0.5, 0.25), None, _scratch(0, V))
    assert tok.cpu().tolist()[1] == SENTINEL and 0 <= tok.cpu().tolist()[0] < V


@pytest.mark.parametrize("V", [65, 262144])
def test_mark_prompt_sets_exactly_the_flags_of_the_listed_ids(V):
    rng = np.random.default_rng(V)
    ids = np.concatenate([[0, V - 1, 7, 7, 7, V - 1], rng.integers(0, V, 700), [0]]).astype(np.int32)
    tables = dev_i32(np.full((3, V), SENTINEL))
    capi.token_table_clear(tables, 1)
    capi.token_table_mark_prompt(tables, dev_i32(ids), 1)
    got = tables.cpu().numpy()
    want = np.zeros(V, dtype=np.uint32)
    want[ids] = R.FLAG
    assert np.array_equal(got[1].view(np.uint32), want)
    assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all(), "a neighbouring row was written"
    # ids outside the vocabulary are skipped; n = 0 is a no-op
    capi.token_table_clear(tables, 2)
    capi.token_table_mark_prompt(tables, dev_i32(np.array([-1, V, 3, 2 ** 31 - 1])), 2)
    capi.token_table_mark_prompt(tables, dev_i32(np.array([5])), 2, n=0)
    got = tables.cpu().numpy()
    assert np.flatnonzero(got[2]).tolist() == [3] and (got[0] == SENTINEL).all()
    assert capi.token_table_bytes(V) == 4 * V


# ---- 5. rows
def _draw_of(j, b):
    return (j + 7 * b) % len(DRAWS)


@pytest.mark.parametrize("V", VOCABS)
def test_every_row_has_the_one_row_filtered_token_and_table(V):
    """row b's token and table are the one-row filtered entry's on row b alone at row b's draw, whatever the other rows hold"""
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    filters = (0.05, 1.15, 0.5, 0.25)
    lg = _rows_logits(V)
    tables = np.stack([R.make_table(lg[b], seed=b) for b in range(4)])
    dev = dev_f32(lg)
    draws_used = DRAWS[::3]
    n = len(draws_used)
    want = np.array([_filtered(dev[b], setting, DRAWS, filters, tables[b]) for b in range(4)])
    assert (want >= 0).all() and (want < V).all()
    for rows in (1, 2, 3, 4):
        for j in range(n):
            tb = dev_i32(_guarded(tables[:rows]))
            out = dev_i32(np.full(rows + 1, SENTINEL))
            draws = dev_f32(np.array([DRAWS[_draw_of(3 * j, b)] for b in range(rows)]))
            capi.sample_radix_filtered_rows(dev[:rows], out[:rows], *setting, draws, filters, tb[:rows * V].view(rows, V), _scratch(rows, V))
            got, after = out.cpu().tolist(), tb.cpu().numpy()
            exp = [int(want[b, _draw_of(3 * j, b)]) for b in range(rows)]
            assert got == exp + [SENTINEL], "V=%d rows=%d call %d: %s != one-row %s" % (V, rows, j, got, exp)
            exp_tb = tables[:rows].copy()
            for b in range(rows):
                R.count_token(exp_tb[b], exp[b])
            assert np.array_equal(after[:-1].reshape(rows, V), exp_tb) and after[-1] == SENTINEL


@pytest.mark.parametrize("V,active", [(4097, [1, 0, 1, 1]), (262144, [0, 1, 0, 0]), (65, [1, 1]), (257, [0])])
@pytest.mark.parametrize("greedy", [False, True])
def test_the_rows_advance_tails_leave_an_inactive_row_alone(V, active, greedy):
    rows = len(active)
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    filters = (0.0, 1.3, 0.6, 0.4)
    lg = _rows_logits(V)[:rows]
    tables = np.stack([R.make_table(lg[b], seed=b) for b in range(rows)])
    dev = dev_f32(lg)
    draws = [0.3, 0.6, 0.05, 0.9][:rows]
    if greedy:
        want = [R.argmax_filtered(lg[b], 0.0, filters, tables[b]) for b in range(rows)]
    else:
        want = [_filtered(dev[b], setting, [draws[b]], filters, tables[b])[0] for b in range(rows)]
    tb = dev_i32(_guarded(tables))
    tok = dev_i32(np.full(rows + 1, SENTINEL))
    pos = dev_i32(np.array([10 * (b + 1) for b in range(rows)] + [SENTINEL]))
    act = dev_i32(np.array(active + [1]))
    if greedy:
        capi.sample_argmax_filtered_rows_advance(dev, tok[:rows], 0.0, filters, tb[:rows * V].view(rows, V), _greedy_scratch(rows), pos[:rows], act[:rows])
    else:
        capi.sample_radix_filtered_rows_advance(dev, tok[:rows], *setting, dev_f32(np.array(draws)), filters, tb[:rows * V].view(rows, V), _scratch(rows, V), pos[:rows], act[:rows])
    assert tok.cpu().tolist() == [want[b] if active[b] else SENTINEL for b in range(rows)] + [SENTINEL]
    assert pos.cpu().tolist() == [10 * (b + 1) + (1 if active[b] else 0) for b in range(rows)] + [SENTINEL]
    exp_tb = tables.copy()
    for b in range(rows):
        if active[b]:
            R.count_token(exp_tb[b], want[b])
    after = tb.cpu().numpy()
    assert np.array_equal(after[:-1].reshape(rows, V), exp_tb) and after[-1] == SENTINEL


# ---- 6. the advance forms
@pytest.mark.parametrize("greedy", [False, True])
def test_three_chained_advance_calls_equal_three_eager_filtered_calls(greedy):
    V = 2049
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    filters = (0.0, 1.3, 2.0, 1.0) if greedy else (0.05, 1.15, 0.5, 0.25)      # (greedy: strong enough that each count moves the next argmax)
    lg = R.random_logits(V)
    table0 = R.make_table(lg)
    dev = dev_f32(lg)
    rs = [0.37, 0.81, 0.12]
    # eager: three filtered calls on one table, which carries the counts from call to call
    eager_tb = dev_i32(table0)
    eager = dev_i32(np.full(3, SENTINEL))
    for i, r in enumerate(rs):
        if greedy:
            capi.sample_argmax_filtered(dev, eager[i:i + 1], 0.0, filters, eager_tb, _greedy_scratch())
        else:
            capi.sample_radix_filtered(dev, eager[i:i + 1], *setting, r, filters, eager_tb, _scratch(0, V))
    want = eager.cpu().tolist()
    host_tb = table0.copy()
    for s in want:
        R.count_token(host_tb, s)
    assert np.array_equal(eager_tb.cpu().numpy(), host_tb)
    if greedy:
        assert len(set(want)) > 1, "the counts of the first tokens must move the later ones"
    ILLEGAL = 2.0
    tb = dev_i32(table0)
    tok, pos = dev_i32(np.array([SENTINEL, SENTINEL])), dev_i32(np.array([41]))
    seq = torch.tensor([6], dtype=torch.int64, device="cuda:0")
    ring = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    draws = torch.full((8,), ILLEGAL, dtype=torch.float32, device="cuda:0")
    for i, r in enumerate(rs):
        draws[(7 + i) % 8] = r                                     # sample number 7 + i reads slot (7 + i) % 8
    for i in range(3):
        if greedy:
            capi.sample_argmax_filtered_advance(dev, tok[0:1], 0.0, filters, tb, _greedy_scratch(), pos, seq, ring)
        else:
            capi.sample_radix_filtered_advance(dev, tok[0:1], *setting, draws, filters, tb, _scratch(0, V), pos, seq, ring)
        assert tok.cpu().tolist() == [want[i], SENTINEL] and int(pos.cpu()[0]) == 42 + i and int(seq.item()) == 7 + i
        assert int(ring[(7 + i) % 8].item()) == ((7 + i) << 32) | want[i]
    assert int(ring[2:7].abs().sum().item()) == 0
    assert np.array_equal(tb.cpu().numpy(), host_tb)


# ---- 7. neutral filters
@pytest.mark.parametrize("V", VOCABS)
def test_neutral_filters_without_a_table_are_the_unfiltered_entries(V):
    lg = _rows_logits(V)
    dev = dev_f32(lg)
    for setting in ((30.0, 0.8, 64, 0.95), (0.0, 1.0, 0, 1.0)):
        for filters in (None, R.NEUTRAL):
            assert _filtered(dev[0], setting, DRAWS, filters, None) == _plain(dev[0], setting, DRAWS)
        out = dev_i32(np.full((2, 5), SENTINEL))
        draws = dev_f32(np.array([0.11, 0.42, 0.63, 0.94]))
        capi.sample_radix_rows(dev, out[0, :4], *setting, draws, _scratch(4, V))
        capi.sample_radix_filtered_rows(dev, out[1, :4], *setting, draws, R.NEUTRAL, None, _scratch(4, V))
        got = out.cpu().tolist()
        assert got[0] == got[1] and got[0][4] == SENTINEL
    # an all-zero table under neutral penalties: the same tokens again (x3 has the bits of x0), and the table counts them
    zero = np.zeros(V, dtype=np.int32)
    assert _filtered(dev[0], (30.0, 0.8, 64, 0.95), DRAWS, R.NEUTRAL, zero) == _plain(dev[0], (30.0, 0.8, 64, 0.95), DRAWS)
    out = dev_i32(np.full(3, SENTINEL))
    capi.call("sample_argmax_fp32", dev[0], out[0:1], V, _greedy_scratch(), C.c_size_t(_greedy_scratch().numel()))
    capi.sample_argmax_filtered(dev[0], out[1:2], 30.0, R.NEUTRAL, None, _greedy_scratch())
    capi.sample_argmax_filtered(dev[0], out[2:3], 0.0, (0.3, 1.0, 0.0, 0.0), None, _greedy_scratch())     # min_p alone does not change a greedy request
    got = out.cpu().tolist()
    assert got[0] == got[1] == got[2] == int(np.argmax(lg[0]))


# ---- 8. refusals
def test_refusals():
    V = 257
    dev, tok, tb = dev_f32(R.random_logits(V)), dev_i32(np.array([SENTINEL])), dev_i32(np.zeros(V))
    before = tb.clone()
    for bad in ((0.0, 0.0, 0.0, 0.0), (0.0, -2.0, 0.0, 0.0), (0.0, float("nan"), 0.0, 0.0), (0.0, 1.0, float("inf"), 0.0), (0.0, 1.0, 0.0, float("nan")),
                (1.0, 1.0, 0.0, 0.0), (-0.01, 1.0, 0.0, 0.0), (float("nan"), 1.0, 0.0, 0.0)):
        with pytest.raises(capi.InvalidArgument):
            capi.sample_radix_filtered(dev, tok, 0.0, 1.0, 0, 1.0, 0.5, bad, tb, _scratch(0, V))
        with pytest.raises(capi.InvalidArgument):
            capi.sample_argmax_filtered(dev, tok, 0.0, bad, tb, _greedy_scratch())
        with pytest.raises(capi.InvalidArgument):
            capi.sample_radix_filtered_rows(dev.view(1, V), tok, 0.0, 1.0, 0, 1.0, dev_f32(np.array([0.5])), bad, tb.view(1, V), _scratch(1, V))
    with pytest.raises(capi.InvalidArgument):
        capi.sample_radix_filtered(dev, tok, 0.0, 0.0, 0, 1.0, 0.5, R.NEUTRAL, tb, _scratch(0, V))                    # temperature <= 0: the greedy entry
    with pytest.raises(capi.MilaError):
        capi.sample_argmax_filtered(dev, tok, 0.0, R.NEUTRAL, tb, _greedy_scratch()[:16])                             # scratch too small
    assert tok.cpu().tolist() == [SENTINEL] and torch.equal(tb, before), "a refused call touched the device"


# ---- the host mirror's sampling op (Operations.h: RocmSamplingOp + RocmTokenTable through host.Sampler)
def test_the_sampling_op_routes_to_the_filtered_entries():
    from mila_amd import host
    V = 2049
    t, k, p = R.IDENTITY_SETTINGS[V]
    lg = R.random_logits(V)
    prompt = np.argsort(-lg)[:6].astype(np.int32)                   # the six largest logits are "in the prompt"
    s = host.Sampler(V, softcap=0.0)
    try:
        s.set_logits(lg)
        table = np.zeros(V, dtype=np.int32)
        table[prompt] = -2 ** 31
        filters = dict(min_p=0.05, repetition_penalty=1.3, presence_penalty=2.0, frequency_penalty=1.0)
        f4 = host._filters(**filters)
        s.set_token_table(prompt)
        assert np.array_equal(s.token_table().view(np.int32), table)
        got = []
        for r, enq in ((0.37, False), (0.81, True), (0.12, False)):
            want = _filtered(dev_f32(lg), (0.0, t, k, p), [r], f4, table)[0]
            tok = (s.sample_enqueued if enq else s.sample)(t, k, p, r, **filters)
            assert tok == want, (r, tok, want)
            R.count_token(table, tok)
            assert np.array_equal(s.token_table().view(np.int32), table), "the op's table does not count the token"
            got.append(tok)
        greedy = s.sample(0.0, 0, 1.0, 0.5, repetition_penalty=1.3, presence_penalty=2.0, frequency_penalty=1.0)
        assert greedy == R.argmax_filtered(lg, 0.0, (0.0, 1.3, 2.0, 1.0), table)
        assert s.sample(0.0, 0, 1.0, 0.5, min_p=0.3) == int(np.argmax(lg))                       # min_p alone: the plain greedy token, no table needed
        assert 0 <= s.sample(t, k, p, 0.37) < V                                                   # neutral: the op's own (search) pipeline, as before
        with pytest.raises(ValueError):
            s.sample(t, k, p, 0.5, repetition_penalty=0.0)
    finally:
        s.close()
    fresh = host.Sampler(V)
    try:
        fresh.set_logits(lg)
        with pytest.raises(ValueError):
            fresh.sample(t, k, p, 0.5, presence_penalty=1.0)                                      # penalties without a token table
        assert 0 <= fresh.sample(t, k, p, 0.5, min_p=0.05) < V                                    # min_p needs none
    finally:
        fresh.close()
