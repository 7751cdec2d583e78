"""GPU: the SUPPORT of the stochastic samplers -- which tokens can be returned at all -- against tests/ref_sample_support.py, at the inputs where a digit-selection
kernel goes wrong.  The logits are built by bit pattern (top-k: the k-th and the (k+1)-th largest keys placed in a chosen digit, bin, sign region, tie group or crowd)
or from a handful of levels (nucleus, min-p) so that the reference decides every draw: nothing is skipped.  tests/test_sample_support_cpu.py shows the committed
oracle alone inside every assertion made here.  Each case: every returned token is in the reference set, the set of returned tokens EQUALS the reference set, and the
midpoint of a survivor's CDF bracket returns that survivor -- through the radix pipeline (sample_radix_*) and the 16-ary search pipeline (sample_stochastic_fp32).

The table of top-k cases is ref_sample_support.TOPK_CASES (name = where the two keys first differ, sign region, ties, the bin radix_pick must find, crowd; then V, k):

    d0 (bits 31..21): pos / pos k5 / pos far / neg / neg wide / cross sign (k 5 and 1); the bin of the threshold's first digit: 7 (last of thread 0), 8 (first of
        thread 1), 4 and 2043 (the lowest and highest a finite value reaches: bins 0..3 and 2044..2047 of the first pass hold only infinities and NaNs)
    d1 (only bits 20..10): pos, neg, t = 0.5; bins 0, 7, 8, 2046, 2047 (positive) and 0, 8 (negative)
    d2 (only bits 9..0): 1 ulp apart (pos, neg, k 1 / 5 / 64); bins 0, 3, 4, 1022, 1023; the carry 0x3FF -> 0x000 into the second and into the first digit; t = 2
    +0.0 above -0.0 and -0.0 at the lower index (k 1 and 5): equal as floats, so the group goes and k - 1 survive (none at k = 1: vocab - 1)
    ties: a group straddling the cut (k 1, 5, 64), a group inside, every key equal
    crowd: 3 000+ non-survivors in the threshold's own second digit (k 1, 5, 64, with a straddling tie); 2 048 survivors of 4 097 above it; 262 144 and 300 001

Calls: the whole file makes 10 318 sampler calls (printed per test) and runs in about four seconds -- the case of 2 048 survivors runs its 2 304 draws four to a call through
sample_radix_rows_fp32 and a quarter of them through the one-row entries, and the fallback test runs every entry on the first FALLBACK_FULL vectors of a size and the
radix, rows and search entries on the others."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import ref_sample_support as S
from gpu_util import dev_f32, dev_i32, dev_u16
from mila_amd import capi
from test_sample_filtered_gpu import SENTINEL, _scratch
from test_sample_radix_gpu import _scratch as _search_scratch

pytestmark = pytest.mark.gpu

CALLS = [0]
NEUTRAL = (1.0, 0.0, 0.0)                      # repetition, presence, frequency: a table then changes no logit


def _out(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")


def _radix(dev, t, k, p, draws, out, min_p=0.0, bf16=False):
    """sample_radix_fp32 / _bf16 (min_p > 0: sample_radix_filtered_fp32 without a table) at every draw, into out[i]"""
    V = int(dev.numel())
    for i, r in enumerate(draws):
        if min_p > 0:
            capi.sample_radix_filtered(dev, out[i:i + 1], 0.0, t, k, p, float(r), (min_p,) + NEUTRAL, None, _scratch(0, V))
        else:
            capi.sample_radix(dev, out[i:i + 1], 0.0, t, k, p, float(r), _scratch(0, V), bf16=bf16)
    CALLS[0] += len(draws)


def _search(dev, t, k, p, draws, out):
    V = int(dev.numel())
    scratch, nb = _search_scratch(V, False)
    for i, r in enumerate(draws):
        capi.call("sample_stochastic_fp32", dev, out[i:i + 1], V, 0.0, float(t), int(k), float(p), float(r), scratch, C.c_size_t(nb))
    CALLS[0] += len(draws)


def _rows(dev4, t, k, p, draws, out):
    """four draws to a call: row b of dev4 [4, V] at draws[4j + b] (sample_radix_rows_fp32); len(draws) a multiple of four"""
    V = int(dev4.shape[1])
    d = dev_f32(np.asarray(draws, dtype=np.float32))
    for j in range(0, len(draws), 4):
        capi.sample_radix_rows(dev4, out[j:j + 4], 0.0, t, k, p, d[j:j + 4], _scratch(4, V))
    CALLS[0] += len(draws) // 4


def _hold(sup, n_mid, tokens, what):
    """the three assertions of a case on the tokens of [midpoints of all survivors in index order] + [grid]"""
    tokens = [int(v) for v in tokens]
    if not sup.tokens.size:
        assert set(tokens) == {sup.V - 1}, "%s: nothing has mass, yet a token other than vocab - 1: %s" % (what, sorted(set(tokens))[:8])
        return
    outside = sorted(set(tokens) - sup.set)
    assert not outside, "%s: tokens outside the reference support: %s" % (what, outside[:8])
    wrong = [(int(sup.tokens[i]), tokens[i]) for i in range(n_mid) if tokens[i] != int(sup.tokens[i])]
    assert not wrong, "%s: (survivor, token at the midpoint of its bracket): %s" % (what, wrong[:8])
    assert set(tokens) == sup.set, "%s: %d survivors were never returned" % (what, len(sup.set - set(tokens)))


# ---- part 2: exact top-k
@pytest.mark.parametrize("case", [c for c in S.TOPK_CASES if not c["exact"]], ids=lambda c: c["name"])
def test_top_k_support_is_exact(case):
    c = case
    lg = S.topk_logits(c)
    sup = S.support(lg, 0.0, c["t"], c["k"], 1.0)
    mid, grid = S.topk_draws(sup, c["k"])
    draws = np.concatenate([mid, grid])
    dev, out = dev_f32(lg), _out(2 * draws.size)
    _radix(dev, c["t"], c["k"], 1.0, draws, out[:draws.size])
    _search(dev, c["t"], c["k"], 1.0, draws, out[draws.size:])
    got = out.cpu().numpy()
    _hold(sup, mid.size, got[:draws.size], "radix")
    _hold(sup, mid.size, got[draws.size:], "search")
    print("%s: %d survivors, %d draws per pipeline; %d calls so far" % (c["name"], sup.tokens.size, draws.size, CALLS[0]))


def test_top_k_support_with_the_crowd_above_the_cut():
    """2 048 survivors of 4 097, every mass exactly 1.0 (ref_sample_support: exact): all 2 048 midpoints and the grid through the rows entry, four draws to a call;
    through the two one-row entries the midpoints of the 128 survivors nearest the cut (the lowest values: the first a wrong threshold loses), of every 16th survivor
    in index order (a key let in by mistake moves every bracket behind it by one) and a quarter of the grid"""
    c = S.TOPK_BY_NAME["crowd above"]
    lg = S.topk_logits(c)
    sup = S.support(lg, 0.0, c["t"], c["k"], 1.0)
    mid, grid = S.topk_draws(sup, c["k"])
    draws = np.concatenate([mid, grid])
    assert draws.size % 4 == 0
    dev4 = dev_f32(np.tile(lg, (4, 1)))
    pick = sorted(set(np.argsort(lg[sup.tokens], kind="stable")[:128].tolist()) | set(range(0, mid.size, 16)))
    sub = np.concatenate([mid[pick], grid[::4]])
    out = _out(draws.size + 2 * sub.size)
    _rows(dev4, c["t"], c["k"], 1.0, draws, out[:draws.size])
    _radix(dev4[0], c["t"], c["k"], 1.0, sub, out[draws.size:draws.size + sub.size])
    _search(dev4[0], c["t"], c["k"], 1.0, sub, out[draws.size + sub.size:])
    got = out.cpu().numpy()
    _hold(sup, mid.size, got[:draws.size], "rows")
    for name, tok in (("radix", got[draws.size:draws.size + sub.size]), ("search", got[draws.size + sub.size:])):
        assert set(int(v) for v in tok) <= sup.set, "%s: a token outside the reference support" % name
        assert [int(v) for v in tok[:len(pick)]] == [int(sup.tokens[i]) for i in pick], "%s: a midpoint draw does not return its survivor" % name
    print("crowd above: %d + 2 x %d draws; %d calls so far" % (draws.size, sub.size, CALLS[0]))


def test_four_top_k_classes_as_the_rows_of_one_call():
    cases = [S.TOPK_BY_NAME[n] for n in S.ROWS_SUBSET]
    lgs = [S.topk_logits(c) for c in cases]
    sups = [S.support(lg, 0.0, 1.0, 5, 1.0) for lg in lgs]
    per_row = [np.concatenate(S.topk_draws(s, 5)) for s in sups]
    n = max(d.size for d in per_row)
    n += -n % 4
    draws = np.full((n, 4), 0.5, dtype=np.float32)                  # a row with fewer survivors repeats the draw 0.5 behind its own
    for b, d in enumerate(per_row):
        draws[:d.size, b] = d
    dev4, dd = dev_f32(np.stack(lgs)), dev_f32(draws)
    out = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
    for j in range(n):
        capi.sample_radix_rows(dev4, out[j], 0.0, 1.0, 5, 1.0, dd[j], _scratch(4, 4097))
    CALLS[0] += n
    got = out.cpu().numpy()
    assert len({s.tokens.size for s in sups}) > 1
    for b, s in enumerate(sups):
        _hold(s, s.tokens.size, got[:, b], "row %d (%s)" % (b, cases[b]["name"]))


@pytest.mark.parametrize("case", S.BF16_CASES, ids=lambda c: c["name"])
def test_top_k_support_on_bf16_logits(case):
    c = case
    lg = S.topk_logits(c)
    sup = S.support(lg, 0.0, 1.0, c["k"], 1.0)
    mid, grid = S.topk_draws(sup, c["k"])
    draws = np.concatenate([mid, grid])
    out = _out(draws.size)
    _radix(dev_u16(orc.to_bf16_bits(lg)), 1.0, c["k"], 1.0, draws, out, bf16=True)
    _hold(sup, mid.size, out.cpu().numpy(), "radix bf16")


# ---- part 3: nucleus and min-p
@pytest.mark.parametrize("case", S.NUCLEUS_CASES, ids=lambda c: "%s V=%d" % (c["name"], c["V"]))
def test_nucleus_and_min_p_support(case):
    c = case
    lg = S.nucleus_logits(c)
    sup = S.support(lg, 0.0, 1.0, c["k"], c["p"], c["min_p"])
    mid = sup.midpoints()
    draws = np.concatenate([mid, S.NUCLEUS_GRID])
    dev, out = dev_f32(lg), _out(2 * draws.size)
    _radix(dev, 1.0, c["k"], c["p"], draws, out[:draws.size], min_p=c["min_p"])
    if c["min_p"] == 0:
        _search(dev, 1.0, c["k"], c["p"], draws, out[draws.size:])      # (the search pipeline has no min-p)
    got = out.cpu().numpy()
    _hold(sup, mid.size, got[:draws.size], "radix")
    if c["min_p"] == 0:
        _hold(sup, mid.size, got[draws.size:], "search")
    print("%s: %d survivors; %d calls so far" % (c["name"], sup.tokens.size, CALLS[0]))


# ---- part 5: the fallback of the inverse-CDF walk
def _fallback_entries(V, lg, setting, full, run):
    """every entry at the four draws of ref_sample_support.FALLBACK_DRAWS; run(entry, bf16, draws_taken, call): call(out) writes one token per draw taken"""
    k, p, min_p = setting
    D = S.FALLBACK_DRAWS
    dev4 = dev_f32(np.tile(lg, (4, 1)))
    dev = dev4[0]
    dd = dev_f32(np.array(D, dtype=np.float32))
    ones = dev_i32(np.ones(4))
    flt = (min_p,) + NEUTRAL

    def advance(fn, *mid):
        """four calls of a one-row advance entry: the sequence number starts at 3, so call i draws slot (4 + i) % 4 = i"""
        pos, seq = dev_i32(np.array([7])), torch.tensor([3], dtype=torch.int64, device="cuda:0")
        return lambda out: [fn(dev, out[i:i + 1], 0.0, 1.0, k, p, dd, *mid, _scratch(0, V), pos, seq, None) for i in range(4)]

    if min_p == 0:
        take = D if full else D[:1]
        run("radix", False, take, lambda out: _radix(dev, 1.0, k, p, take, out))
        run("rows", False, D, lambda out: capi.sample_radix_rows(dev4, out, 0.0, 1.0, k, p, dd, _scratch(4, V)))
        take = D if full else D[:2]
        run("search", False, take, lambda out: _search(dev, 1.0, k, p, take, out))
    elif not full:
        run("filtered_rows", False, D, lambda out: capi.sample_radix_filtered_rows(dev4, out, 0.0, 1.0, k, p, dd, flt, None, _scratch(4, V)))
    if not full:
        return
    if min_p == 0:
        devb = dev_u16(orc.to_bf16_bits(lg))
        run("radix_bf16", True, D, lambda out: _radix(devb, 1.0, k, p, D, out, bf16=True))
        run("advance", False, D, advance(capi.sample_radix_advance))
        run("rows_advance", False, D, lambda out: capi.sample_radix_rows_advance(dev4, out, 0.0, 1.0, k, p, dd, _scratch(4, V), dev_i32(np.zeros(4)), ones))
        rows_tok = _out(4)
        capi.sample_radix_rows(dev4, rows_tok, 0.0, 1.0, k, p, dd, _scratch(4, V))
        tok = _out(4)
        tok[1:] = rows_tok[:3]                                  # the drafts are the samples themselves (a device copy): all four are accepted and reported

        def chain(out):
            res = _out(5)
            capi.sample_radix_chain_accept(tok, res, dev4, 0.0, 1.0, k, p, dd, _scratch(4, V), dev_i32(np.array([7])))
            out.copy_(res[1:])
        run("chain_accept", False, D, chain)
    for with_table in (False, True):
        tag = "+table" if with_table else ""
        one = (lambda: dev_i32(np.zeros(V))) if with_table else (lambda: None)
        four = (lambda: dev_i32(np.zeros((4, V)))) if with_table else (lambda: None)
        run("filtered" + tag, False, D, lambda out: [capi.sample_radix_filtered(dev, out[i:i + 1], 0.0, 1.0, k, p, D[i], flt, one(), _scratch(0, V)) for i in range(4)])
        run("filtered_advance" + tag, False, D, advance(capi.sample_radix_filtered_advance, flt, one()))
        run("filtered_rows" + tag, False, D, lambda out: capi.sample_radix_filtered_rows(dev4, out, 0.0, 1.0, k, p, dd, flt, four(), _scratch(4, V)))
        run("filtered_rows_advance" + tag, False, D,
            lambda out: capi.sample_radix_filtered_rows_advance(dev4, out, 0.0, 1.0, k, p, dd, flt, four(), _scratch(4, V), dev_i32(np.zeros(4)), ones))


ONE_ROW_CALLS = {"radix": None, "search": None, "radix_bf16": None}          # counted by their helpers; the others below by their draws


@pytest.mark.parametrize("V,vectors", S.FALLBACK_VECTORS)
def test_a_token_with_zero_mass_is_never_returned(V, vectors):
    """Gaussian logits with the last eighth of the vocabulary at -30 (no mass after any of the four truncations) and draws at and next to 1, where the walk's running
    sum (index order) can end below r * total (chunk order).  Every entry returns a token of the reference support -- the walk's fallback is the last entry with mass,
    never vocab - 1 --, at r = 1 under top-k alone (an exact support) it is the LAST survivor, and the two pipelines agree.  The cuts of a Gaussian vector are not
    designed, so a token within FALLBACK_SLACK of the mass at the nucleus / min-p cut may be in or out (Support.near); the masked tail is far outside either way.
    While the unbiased walks still fell back to vocab - 1, 424 of the 3 944 (vector, setting, draw, entry) combinations here returned it: 44 of 1 548 at V = 4 097,
    127 of 1 548 at 65 537 and 253 of 848 at 262 144, at r = 1 and at the two draws next below it, through every entry."""
    records, slots = [], 0
    out = _out(vectors * 4 * 80)
    for seed in range(vectors):
        lg = S.fallback_logits(V, seed)
        lgb = orc.from_bf16_bits(orc.to_bf16_bits(lg))
        for setting in S.fallback_settings(V):
            k, p, min_p = setting
            sups = {False: S.support(lg, 0.0, 1.0, k, p, min_p, slack=S.FALLBACK_SLACK)}

            def run(entry, bf16, draws, call):
                nonlocal slots
                if bf16 and True not in sups:
                    sups[True] = S.support(lgb, 0.0, 1.0, k, p, min_p, slack=S.FALLBACK_SLACK)
                call(out[slots:slots + len(draws)])
                if entry not in ONE_ROW_CALLS:
                    CALLS[0] += 1 if "rows" in entry or entry == "chain_accept" else len(draws)
                records.append((slots, entry, seed, setting, list(draws), sups[bf16]))
                slots += len(draws)
            _fallback_entries(V, lg, setting, seed < S.FALLBACK_FULL, run)
    got = out.cpu().numpy()
    bad, combos, by = [], 0, {}
    for at, entry, seed, setting, draws, sup in records:
        assert V - 1 not in sup.set and V - 1 not in sup.near
        for i, r in enumerate(draws):
            tok = int(got[at + i])
            combos += 1
            by[(seed, setting, r, entry)] = tok
            if tok not in sup.set and tok not in sup.near:
                bad.append((seed, setting, r, entry, tok))
            elif r == 1.0 and setting[1] >= 1.0 and setting[2] == 0 and tok != sup.last():
                bad.append((seed, setting, r, entry, tok, "not the last survivor", sup.last()))
    for (seed, setting, r, entry), tok in by.items():
        radix = by.get((seed, setting, r, "radix"), tok)
        if entry == "search" and tok != radix:
            bad.append((seed, setting, r, "radix != search", radix, tok))
    print("V=%d: %d of %d (vector, setting, draw, entry) combinations fail; %d calls so far" % (V, len(bad), combos, CALLS[0]))
    assert not bad, "V=%d: %d of %d combinations (seed, (k, p, min_p), draw, entry, token): %s" % (V, len(bad), combos, bad[:6])
