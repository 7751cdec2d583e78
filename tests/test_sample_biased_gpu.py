"""GPU: the biased sampler entries of the C ABI (include/mila_cdna4.h: logit bias) -- an fp32 bias table added to the capped logit ahead of the penalties: logit bias,
banned tokens, a closed answer set.  Integer outputs: a token is right or wrong.  Without a softcap the adjusted logit is restated bit for bit on the host
(tests/ref_logit_bias.py), so a biased entry must return, at EVERY draw, what the unfiltered entry returns on the host-adjusted logits; that a forbidden token is never
returned is checked on its own, against nothing but the list."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_logit_bias as B
import ref_sampling_filters as R
from gpu_util import dev_f32, dev_i32
from mila_amd import capi
from test_sample_filtered_gpu import SENTINEL, _filtered, _greedy_scratch, _guarded, _plain, _scratch
from test_sample_radix_gpu import DRAWS
from test_sample_radix_rows_gpu import VOCABS, _rows_logits

pytestmark = pytest.mark.gpu

assert VOCABS == (65, 257, 2049, 4097, 262144, 300001)
NEG_INF = float("-inf")


def _biased(dev, setting, draws, filters, table_np, bias_dev):
    """tokens of sample_radix_biased_fp32 at every draw, each from a fresh copy of the table (None: no table); one readback"""
    softcap, t, k, p = setting
    out = torch.full((len(draws),), SENTINEL, dtype=torch.int32, device="cuda:0")
    fresh = None if table_np is None else dev_i32(table_np)
    for i, r in enumerate(draws):
        table = None if fresh is None else fresh.clone()
        capi.sample_radix_biased(dev, out[i:i + 1], softcap, t, k, p, r, filters, table, bias_dev, _scratch(0, dev.numel()))
    return out.cpu().tolist()


def _argmax_plain(dev):
    out = dev_i32(np.array([SENTINEL]))
    capi.call("sample_argmax_fp32", dev, out, int(dev.numel()), _greedy_scratch(), C.c_size_t(_greedy_scratch().numel()))
    return int(out.cpu()[0])


# ---- 1. exact identity without a softcap
@pytest.mark.parametrize("V", VOCABS)
def test_bias_equals_the_unfiltered_sampler_on_host_adjusted_logits(V):
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    lg = R.random_logits(V)
    table = R.make_table(lg)
    dev = dev_f32(lg)
    unbiased = _plain(dev, setting, DRAWS)
    for name, bias in B.patterns(lg).items():
        bias_dev = dev_f32(bias)
        for pen in [None] + R.PENALTIES:
            x3 = B.adjusted_logits(lg, bias) if pen is None else B.adjusted_logits(lg, bias, table, *pen)
            want = _plain(dev_f32(x3), setting, DRAWS)
            got = _biased(dev, setting, DRAWS, None if pen is None else (0.0,) + pen, None if pen is None else table, bias_dev)
            assert got == want, "V=%d %s %s: %s != unfiltered on x3 %s" % (V, name, pen, got, want)
            assert all(np.isfinite(bias[g]) for g in got)
            if pen is None:
                changed = sum(a != b for a, b in zip(got, unbiased))
                print("V=%d %s: the bias changes %d of %d tokens" % (V, name, changed, len(DRAWS)))
                if V >= 257:
                    assert changed >= 1, "the bias pattern changed no token: the case shows nothing"


# ---- 2. membership: a token outside the allow-list is never returned
EDGE_DRAWS = [0.0, 2.0 ** -24, float(np.nextafter(np.float32(1), np.float32(0)))] + DRAWS


def _membership_settings(n):
    """(temperature, top_k, top_p, min_p): no truncation, top_k below and above the list size, a nucleus, min-p"""
    return [(1.0, 0, 1.0, 0.0), (1.0, max(1, n - 1), 1.0, 0.0), (1.0, n + 24, 1.0, 0.0), (1.0, 0, 0.9, 0.0), (1.0, 0, 1.0, 0.1)]


@pytest.mark.parametrize("V,vectors", [(4097, 32), (262144, 4)])
@pytest.mark.parametrize("n", [3, 40])
def test_every_token_is_in_the_allow_list(V, vectors, n):
    out = torch.full((vectors, len(_membership_settings(n)), len(EDGE_DRAWS)), SENTINEL, dtype=torch.int32, device="cuda:0")
    lists = []
    for s in range(vectors):
        lg = R.random_logits(V, seed=100 + s)
        bias, ids = B.allow_bias(lg, n, seed=s)
        assert V - 1 not in ids and len(ids) == n
        lists.append(set(ids))
        dev, bias_dev = dev_f32(lg), dev_f32(bias)
        for j, (t, k, p, min_p) in enumerate(_membership_settings(n)):
            for i, r in enumerate(EDGE_DRAWS):
                capi.sample_radix_biased(dev, out[s, j, i:i + 1], 30.0, t, k, p, r, (min_p, 1.0, 0.0, 0.0), None, bias_dev, _scratch(0, V))
    got = out.cpu().numpy()
    for s in range(vectors):
        bad = [(j, EDGE_DRAWS[i], int(got[s, j, i])) for j in range(got.shape[1]) for i in range(got.shape[2]) if int(got[s, j, i]) not in lists[s]]
        assert not bad, "V=%d list of %d, vector %d: (setting, draw, token) outside the list: %s" % (V, n, s, bad[:8])


def test_the_fallback_of_a_biased_call_is_the_last_entry_with_mass():
    """r = 1 is legal in the one-row entry: the target is the whole mass, summed chunk by chunk, while the walk sums in index order.  With equal masses both sums are
    exact and the walk ends on the last listed token; with irregular masses they may differ in the last bits either way, and whichever way they fall the token is one
    of the list -- vocab - 1, the unbiased sampler's fallback, never"""
    V = 4097
    for n in (3, 7, 11, 40):
        ids = sorted(int(i) for i in np.random.default_rng(n).choice(V - 1, size=n, replace=False))
        bias = np.full(V, -np.inf, dtype=np.float32)
        bias[ids] = 0.0
        draws = [1.0, EDGE_DRAWS[2]]
        got = _biased(dev_f32(np.full(V, 0.1, dtype=np.float32)), (0.0, 0.7, 0, 1.0), draws, None, None, dev_f32(bias))
        assert got[0] == ids[-1] and got[1] in ids, (n, got, ids)
        for seed in range(8):
            got = _biased(dev_f32((R.random_logits(V, seed=seed) * 0.25).astype(np.float32)), (0.0, 0.7, 0, 1.0), draws, None, None, dev_f32(bias))
            assert got[0] in ids and got[1] in ids, (n, seed, got, ids)


# ---- 3. greedy
@pytest.mark.parametrize("V", VOCABS)
def test_biased_greedy_equals_the_argmax_of_host_adjusted_logits(V):
    lg = R.greedy_logits(V)
    table = R.make_table(lg)
    dev = dev_f32(lg)
    plain = _argmax_plain(dev)
    moved = False
    for name, bias in B.patterns(lg).items():
        for pen in [None] + R.GREEDY_PENALTIES:
            x3 = B.adjusted_logits(lg, bias) if pen is None else B.adjusted_logits(lg, bias, table, *pen)
            want = int(np.argmax(x3))                                   # (numpy: the first of equal maxima, the lower id)
            out = dev_i32(np.full(2, SENTINEL))
            capi.sample_argmax_biased(dev, out[0:1], 0.0, None if pen is None else (0.0,) + pen, None if pen is None else dev_i32(table), dev_f32(bias), _greedy_scratch())
            assert out.cpu().tolist() == [want, SENTINEL], (V, name, pen)
            assert _argmax_plain(dev_f32(x3)) == want
            moved |= want != plain
    if V >= 257:
        assert moved


def test_biased_greedy_ties_bans_and_the_softcap_comes_first():
    V = 3000
    lg = np.full(V, -1.0, dtype=np.float32)
    lg[[700, 1900, 2500]] = [5.0, 4.0, 4.0]
    zero = np.zeros(V, dtype=np.float32)

    def greedy(logits, softcap, bias):
        out = dev_i32(np.array([SENTINEL]))
        capi.sample_argmax_biased(dev_f32(logits), out, softcap, None, None, dev_f32(bias), _greedy_scratch())
        return int(out.cpu()[0])

    assert greedy(lg, 0.0, zero) == 700
    ban = zero.copy()
    ban[700] = -np.inf
    assert greedy(lg, 0.0, ban) == 1900                               # the ban on the top token yields the second; the tie behind it goes to the lower id
    tie = zero.copy()
    tie[[1900, 2500]] = 1.0
    assert greedy(lg, 0.0, tie) == 700                                # 5 == 4 + 1: a three-way tie, the lowest id
    tie[700] = -0.5
    assert greedy(lg, 0.0, tie) == 1900
    # the cap comes BEFORE the bias: 200 and 100 both saturate near 30 (30 * tanh(100 / 30) = 29.92, 30 * tanh(200 / 30) = 29.9999), so a bias of +1 on the smaller
    # one wins by 0.92; were the bias added first (201 vs 101 -> both near 30, order kept) token 700 would win.  Without a softcap 200 stays far ahead.
    big = np.full(V, -1.0, dtype=np.float32)
    big[[700, 1900]] = [200.0, 100.0]
    plus = zero.copy()
    plus[1900] = 1.0
    assert greedy(big, 30.0, plus) == 1900
    assert greedy(big, 0.0, plus) == 700


# ---- 4. rows
def _draw_of(j, b):
    return (j + 7 * b) % len(DRAWS)


@pytest.mark.parametrize("V", VOCABS)
def test_every_row_has_the_one_row_biased_token(V):
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    filters = (0.05, 1.15, 0.5, 0.25)
    lg = _rows_logits(V)
    tables = np.stack([R.make_table(lg[b], seed=b) for b in range(4)])
    pats = [B.sparse_bias(lg[0], 0), B.ban_bias(lg[1]), B.allow_bias(lg[2], 3)[0], B.sparse_bias(lg[3], 3)]
    biases = np.stack(pats)
    dev = dev_f32(lg)
    per_row = dev_f32(biases)
    shared = dev_f32(pats[0])
    want_own = np.array([_biased(dev[b], setting, DRAWS, filters, tables[b], per_row[b]) for b in range(4)])
    want_shared = np.array([_biased(dev[b], setting, DRAWS, filters, tables[b], shared) for b in range(4)])
    assert (want_own != want_shared).any()
    for rows in (1, 2, 3, 4):
        for j in range(0, len(DRAWS), 5):
            draws = dev_f32(np.array([DRAWS[_draw_of(j, b)] for b in range(rows)]))
            for bias_dev, want in ((per_row[:rows], want_own), (shared, want_shared)):
                tb = dev_i32(_guarded(tables[:rows]))
                out = dev_i32(np.full(rows + 1, SENTINEL))
                capi.sample_radix_biased_rows(dev[:rows], out[:rows], *setting, draws, filters, tb[:rows * V].view(rows, V), bias_dev, _scratch(rows, V))
                exp = [int(want[b, _draw_of(j, b)]) for b in range(rows)]
                assert out.cpu().tolist() == exp + [SENTINEL], "V=%d rows=%d call %d stride %s" % (V, rows, j, "vocab" if bias_dev.dim() == 2 else "0")
                exp_tb = tables[:rows].copy()
                for b in range(rows):
                    R.count_token(exp_tb[b], exp[b])
                after = tb.cpu().numpy()
                assert np.array_equal(after[:-1].reshape(rows, V), exp_tb) and after[-1] == SENTINEL


@pytest.mark.parametrize("V,active", [(4097, [1, 0, 1, 1]), (65, [1, 1]), (262144, [0, 1, 0, 0])])
@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("with_table", [False, True])
def test_the_biased_rows_advance_tails(V, active, greedy, with_table):
    rows = len(active)
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    filters = (0.0, 1.3, 0.6, 0.4) if with_table else None
    lg = _rows_logits(V)[:rows]
    tables = np.stack([R.make_table(lg[b], seed=b) for b in range(rows)])
    biases = np.stack([B.ban_bias(lg[b]) if b % 2 else B.sparse_bias(lg[b], b) for b in range(rows)])
    dev, bias_dev = dev_f32(lg), dev_f32(biases)
    draws = [0.3, 0.6, 0.05, 0.9][:rows]
    if greedy:
        want = [int(np.argmax(B.adjusted_logits(lg[b], biases[b], tables[b], *filters[1:]) if with_table else B.adjusted_logits(lg[b], biases[b]))) for b in range(rows)]
    else:
        want = [_biased(dev[b], setting, [draws[b]], filters, tables[b] if with_table else None, bias_dev[b])[0] for b in range(rows)]
    tb = dev_i32(_guarded(tables))
    tbv = tb[:rows * V].view(rows, V) if with_table else None
    tok = dev_i32(np.full(rows + 1, SENTINEL))
    pos = dev_i32(np.array([10 * (b + 1) for b in range(rows)] + [SENTINEL]))
    act = dev_i32(np.array(active + [1]))
    if greedy:
        capi.sample_argmax_biased_rows_advance(dev, tok[:rows], 0.0, filters, tbv, bias_dev, _greedy_scratch(rows), pos[:rows], act[:rows])
    else:
        capi.sample_radix_biased_rows_advance(dev, tok[:rows], *setting, dev_f32(np.array(draws)), filters, tbv, bias_dev, _scratch(rows, V), pos[:rows], act[:rows])
    assert tok.cpu().tolist() == [want[b] if active[b] else SENTINEL for b in range(rows)] + [SENTINEL]
    assert pos.cpu().tolist() == [10 * (b + 1) + (1 if active[b] else 0) for b in range(rows)] + [SENTINEL]
    exp_tb = tables.copy()
    if with_table:
        for b in range(rows):
            if active[b]:
                R.count_token(exp_tb[b], want[b])
    after = tb.cpu().numpy()
    assert np.array_equal(after[:-1].reshape(rows, V), exp_tb) and after[-1] == SENTINEL


@pytest.mark.parametrize("greedy", [False, True])
def test_three_chained_biased_advance_calls_and_an_update_between_them(greedy):
    """the advance forms read the table each call: an entry changed between two calls (stream order) holds from the next call on"""
    V = 2049
    t, k, p = R.IDENTITY_SETTINGS[V]
    setting = (0.0, t, k, p)
    lg = R.random_logits(V)
    bias = B.sparse_bias(lg)
    dev = dev_f32(lg)
    rs = [0.37, 0.81, 0.12]
    # eager: the same three calls; before the third the token of the first call is banned
    def run(call):
        bias_dev = dev_f32(bias)
        got = []
        for i, r in enumerate(rs):
            if i == 2:
                capi.token_bias_set(bias_dev, dev_i32(np.array([got[0]])), dev_f32(np.array([-np.inf])))
            got.append(call(bias_dev, i, r))
        return got
    one = dev_i32(np.array([SENTINEL]))

    def eager(bias_dev, i, r):
        if greedy:
            capi.sample_argmax_biased(dev, one, 0.0, None, None, bias_dev, _greedy_scratch())
        else:
            capi.sample_radix_biased(dev, one, *setting, r, None, None, bias_dev, _scratch(0, V))
        return int(one.cpu()[0])
    want = run(eager)
    assert want[2] != want[0]
    tok, pos = dev_i32(np.array([SENTINEL, SENTINEL])), dev_i32(np.array([41]))
    seq = torch.tensor([6], dtype=torch.int64, device="cuda:0")
    ring = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    draws = torch.full((8,), 2.0, dtype=torch.float32, device="cuda:0")
    for i, r in enumerate(rs):
        draws[(7 + i) % 8] = r

    def advance(bias_dev, i, r):
        if greedy:
            capi.sample_argmax_biased_advance(dev, tok[0:1], 0.0, None, None, bias_dev, _greedy_scratch(), pos, seq, ring)
        else:
            capi.sample_radix_biased_advance(dev, tok[0:1], *setting, draws, None, None, bias_dev, _scratch(0, V), pos, seq, ring)
        got = tok.cpu().tolist()
        assert got[1] == SENTINEL and int(pos.cpu()[0]) == 42 + i and int(seq.item()) == 7 + i
        assert int(ring[(7 + i) % 8].item()) == ((7 + i) << 32) | got[0]
        return got[0]
    assert run(advance) == want


# ---- 5. bias = NULL
@pytest.mark.parametrize("V", [65, 4097, 262144])
def test_a_null_bias_is_the_filtered_entry(V):
    t, k, p = R.IDENTITY_SETTINGS[V]
    lg = _rows_logits(V)
    dev = dev_f32(lg)
    tables = np.stack([R.make_table(lg[b], seed=b) for b in range(4)])
    filters = (0.05, 1.15, 0.5, 0.25)
    for setting in ((30.0, 0.8, 64, 0.95), (0.0, t, k, p)):
        for table in (None, tables[0]):
            assert _biased(dev[0], setting, DRAWS[::4], filters, table, None) == _filtered(dev[0], setting, DRAWS[::4], filters, table)
        out = dev_i32(np.full((2, 5), SENTINEL))
        tb = dev_i32(np.stack([tables, tables]))
        draws = dev_f32(np.array([0.11, 0.42, 0.63, 0.94]))
        capi.sample_radix_filtered_rows(dev, out[0, :4], *setting, draws, filters, tb[0], _scratch(4, V))
        capi.sample_radix_biased_rows(dev, out[1, :4], *setting, draws, filters, tb[1], None, _scratch(4, V))
        got = out.cpu().tolist()
        assert got[0] == got[1] and got[0][4] == SENTINEL
        assert torch.equal(tb[0], tb[1]) and not torch.equal(tb[0], dev_i32(tables)), "the table update of the two entries differs"
    out = dev_i32(np.full(4, SENTINEL))
    tb = dev_i32(np.stack([tables[0], tables[0]]))
    capi.sample_argmax_filtered(dev[0], out[0:1], 30.0, filters, tb[0], _greedy_scratch())
    capi.sample_argmax_biased(dev[0], out[1:2], 30.0, filters, tb[1], None, _greedy_scratch())
    capi.sample_argmax_biased(dev[0], out[2:3], 30.0, None, None, None, _greedy_scratch())      # no table, no bias: the plain greedy sampler
    got = out.cpu().tolist()
    assert got[0] == got[1] and got[2] == int(np.argmax(lg[0])) and got[3] == SENTINEL and torch.equal(tb[0], tb[1])


# ---- 6. side effects
@pytest.mark.parametrize("V", [65, 4097, 300001])
def test_the_logits_and_the_bias_are_not_written_and_the_table_counts_the_token(V):
    t, k, p = R.IDENTITY_SETTINGS[V]
    lg = R.random_logits(V)
    table = R.make_table(lg)
    bias = B.sparse_bias(lg)
    bias[[1, V - 2]] = -np.inf
    for greedy in (False, True):
        dev = dev_f32(_guarded(lg.view(np.int32)).view(np.float32))
        bias_dev = dev_f32(_guarded(bias.view(np.int32)).view(np.float32))
        buf = dev_i32(_guarded(table))
        tok = dev_i32(np.full(2, SENTINEL))
        if greedy:
            capi.sample_argmax_biased(dev[:V], tok[0:1], 30.0, (0.0, 1.15, 0.5, 0.25), buf[:V], bias_dev[:V], _greedy_scratch())
        else:
            capi.sample_radix_biased(dev[:V], tok[0:1], 30.0, t, k, p, 0.37, (0.0, 1.15, 0.5, 0.25), buf[:V], bias_dev[:V], _scratch(0, V))
        s, behind = tok.cpu().tolist()
        assert 0 <= s < V and behind == SENTINEL and np.isfinite(bias[s])
        assert np.array_equal(dev.cpu().numpy().view(np.int32), _guarded(lg.view(np.int32))), "the logits were written"
        assert np.array_equal(bias_dev.cpu().numpy().view(np.int32), _guarded(bias.view(np.int32))), "the bias table was written"
        want = _guarded(table)
        R.count_token(want, s)
        assert np.array_equal(buf.cpu().numpy(), want), "exactly table[%d] goes up by one" % s


# ---- 7. maintenance
@pytest.mark.parametrize("V", [65, 4097, 262144])
def test_fill_and_set_equal_numpy(V):
    rng = np.random.default_rng(V)
    MARK = np.float32(-77.5)
    tables = dev_f32(np.full(3 * V + 1, MARK, dtype=np.float32))
    view = tables[:3 * V].view(3, V)
    want = np.full((3, V), MARK, dtype=np.float32)
    for value in (0.0, NEG_INF, 2.5):
        capi.token_bias_fill(view, value, row=1)
        want[1] = value
        ids = rng.choice(V, size=min(V, 700), replace=False).astype(np.int32)
        vals = (rng.standard_normal(ids.size) * 5).astype(np.float32)
        vals[::7] = -np.inf
        capi.token_bias_set(view, dev_i32(ids), dev_f32(vals), row=1)
        want[1, ids] = vals
        got = tables.cpu().numpy()
        assert np.array_equal(got[:3 * V].reshape(3, V).view(np.int32), want.view(np.int32)), "row 1 differs, or a neighbouring row was written"
        assert got[-1] == MARK
    # ids outside the vocabulary are skipped; n = 0 is a no-op
    capi.token_bias_fill(view, 0.0, row=2)
    capi.token_bias_set(view, dev_i32(np.array([-1, V, 3, 2 ** 31 - 1])), dev_f32(np.array([1.0, 2.0, 3.0, 4.0])), row=2)
    capi.token_bias_set(view, dev_i32(np.array([5])), dev_f32(np.array([9.0])), row=2, n=0)
    got = tables.cpu().numpy()
    assert np.flatnonzero(got[2 * V:3 * V]).tolist() == [3] and got[2 * V + 3] == 3.0 and got[-1] == MARK
    assert np.array_equal(got[:2 * V].view(np.int32), want[:2].reshape(-1).view(np.int32))
    assert capi.token_bias_bytes(V) == 4 * V


def test_refusals_touch_nothing():
    V = 257
    dev, tok = dev_f32(R.random_logits(V)), dev_i32(np.array([SENTINEL]))
    bias = dev_f32(np.zeros((2, V), dtype=np.float32))
    before = bias.clone()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(capi.InvalidArgument):
            capi.token_bias_fill(bias, bad)
    with pytest.raises(capi.InvalidArgument):
        capi.token_bias_set(bias, dev_i32(np.array([1])), dev_f32(np.array([1.0])), n=-1)
    with pytest.raises(capi.InvalidArgument):
        capi.sample_radix_biased_rows(dev_f32(np.zeros((2, V), dtype=np.float32)), dev_i32(np.full(2, SENTINEL)), 0.0, 1.0, 0, 1.0, dev_f32(np.array([0.5, 0.5])), None, None,
                                      bias, _scratch(2, V), bias_stride=V - 1)
    with pytest.raises(capi.InvalidArgument):
        capi.sample_radix_biased(dev, tok, 0.0, 0.0, 0, 1.0, 0.5, None, None, bias[0], _scratch(0, V))     # temperature <= 0: the greedy entry
    assert tok.cpu().tolist() == [SENTINEL] and torch.equal(bias, before)
