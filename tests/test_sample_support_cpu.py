"""CPU: the inputs of tests/test_sample_support_gpu.py are shown here to keep the REFERENCE alone inside the conditions the GPU test relies on.  For every case the
committed oracle (oracle/mila_oracle.c: orc_sample_stochastic) returns a token of ref_sample_support.support(...) at every draw the GPU test uses and, at the midpoint
of every survivor's bracket, that survivor; the designed margins hold -- every bracket is at least 1e-3 of the total and every nucleus margin at least 1e-2 -- so no
GPU draw needs to be skipped.  A case that misses a margin fails HERE."""
import numpy as np
import pytest

import orc
import ref_sample_support as S

MIN_BRACKET, MIN_NUCLEUS, MIN_MINP = 1e-3, 1e-2, 1e-2


def _oracle_agrees(lg, t, k, p, sup, draws_mid, draws_grid):
    for i, r in enumerate(draws_mid):
        tok = orc.sample_stochastic(lg, 0.0, t, k, p, float(r))[0]
        assert tok == int(sup.tokens[i]), "midpoint %g of survivor %d: the oracle returns %d" % (r, sup.tokens[i], tok)
    for r in draws_grid:
        tok = orc.sample_stochastic(lg, 0.0, t, k, p, float(r))[0]
        assert tok in sup.set if sup.set else tok == sup.V - 1, "draw %g: the oracle's token %d is outside the reference support" % (r, tok)


def test_the_table_of_top_k_cases():
    assert len(S.TOPK_CASES) <= 60 and len(S.TOPK_BY_NAME) == len(S.TOPK_CASES)
    assert {c["k"] for c in S.TOPK_CASES} >= {1, 5, 64} and {c["V"] for c in S.TOPK_CASES} == {65, 4097, 262144, 300001}
    rows = [S.TOPK_BY_NAME[n] for n in S.ROWS_SUBSET]
    assert len(rows) == 4 and all((c["V"], c["k"], c["t"]) == (4097, 5, 1.0) for c in rows)
    # the key map is the kernels': monotone but for the two zeros, and its own inverse
    x = np.array([-np.inf, -3.0e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], dtype=np.float32)
    keys = S.key_of(x)
    assert np.all(np.diff(keys.astype(np.int64)) > 0) and int(keys[4]) == S.MINUS_ZERO and int(keys[5]) == S.PLUS_ZERO
    assert np.array_equal(S.float_of(keys).view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("case", S.TOPK_CASES + S.BF16_CASES, ids=lambda c: c["name"])
def test_top_k_case(case):
    c = case
    lg = S.topk_logits(c)
    V, k = c["V"], c["k"]
    assert lg.size == V and np.isfinite(lg).all()
    sup = S.support(lg, 0.0, c["t"], k, 1.0)
    # the case is what its row of the table says: the (k+1)-th and the k-th largest keys, the ties, the crowd
    keys = np.sort(S.key_of((lg / np.float32(c["t"])).astype(np.float32)))[::-1]
    assert int(keys[k]) == c["k1"] and int(keys[k - 1]) == c["kk"]
    want = {"none": k, "inside": k, "straddle": max(0, k - 2), "all": 0}[c["ties"]]
    if c["kk"] == S.PLUS_ZERO and c["k1"] == S.MINUS_ZERO:
        want = k - 1                                           # the two zeros are one tie group
        zeros = np.flatnonzero(lg == 0)
        assert zeros.size == 2 and bool(np.signbit(lg[zeros[0]])) == c["swap"]
    assert sup.tokens.size == want
    if c["ties"] == "inside":
        assert np.unique(lg[sup.tokens]).size == k - 1
    if c["crowd"]:
        assert int(((keys[k + 1:] >> 10) == (c["k1"] >> 10)).sum()) >= min(c["crowd"], 3000) or c["exact"]
    if c["exact"]:
        # the one case with brackets below 1e-3 (1 / 2048): every survivor's fp32 mass is exactly 1.0 and every sum an integer, so there is nothing to round
        x = lg[sup.tokens].astype(np.float64)
        assert k == 2048 and sup.tokens.size == k and (x.max() - x.min()) < 2.0 ** -50
        assert np.array_equal(np.exp((lg[sup.tokens] - lg.max()).astype(np.float32)), np.ones(k, dtype=np.float32))
        assert np.array_equal(sup.midpoints().astype(np.float64) * k, np.arange(k) + 0.5)
        assert int((keys[:k] >> 10 == (c["kk"] >> 10)).sum()) < k, "the survivors do not cross a second-digit boundary"
    elif sup.tokens.size:
        assert sup.min_bracket() >= MIN_BRACKET
        spread = lg[sup.tokens].astype(np.float64)
        if not c.get("bf16"):                                  # (bf16 holds eight bits: its survivors are a few percent apart, the brackets still far above 1e-3)
            assert np.exp(spread.min() / c["t"] - spread.max() / c["t"]) > 0.99, "the survivors' masses are not near equal"
    mid, grid = S.topk_draws(sup, k)
    assert mid.size == sup.tokens.size and grid.size == min(4 * k, 256)
    _oracle_agrees(lg, c["t"], k, 1.0, sup, mid, grid)


@pytest.mark.parametrize("case", S.NUCLEUS_CASES, ids=lambda c: "%s V=%d" % (c["name"], c["V"]))
def test_nucleus_case(case):
    c = case
    lg = S.nucleus_logits(c)
    sup = S.support(lg, 0.0, 1.0, c["k"], c["p"], c["min_p"])
    levels = [v for v, _ in c["levels"]][:c["keeps"]]
    assert sorted(set(float(v) for v in lg[sup.tokens]), reverse=True) == [float(np.float32(v)) for v in levels], "the design keeps other levels than the reference"
    assert sup.min_bracket() >= MIN_BRACKET
    if c["p"] < 1.0:
        assert sup.m_nucleus >= MIN_NUCLEUS
        for f in S._fractions(c["V"], c["levels"]):
            assert c["k"] or abs(c["p"] - f) >= MIN_NUCLEUS, "p within 1e-2 of a cumulative level sum"
    if c["min_p"] > 0:
        assert sup.m_minp >= MIN_MINP
    else:
        _oracle_agrees(lg, 1.0, c["k"], c["p"], sup, sup.midpoints(), S.NUCLEUS_GRID)      # (the C oracle has no min-p: those cases rest on the margins above)


@pytest.mark.parametrize("V,vectors", S.FALLBACK_VECTORS)
def test_fallback_vectors(V, vectors):
    """vocab - 1 (and the whole masked tail) is outside the support, slack included, in every setting; the oracle's token at every draw is inside it, and at r = 1 it is
    the last survivor"""
    for seed in range(vectors):
        lg = S.fallback_logits(V, seed)
        for b16 in (False, True):
            x = orc.from_bf16_bits(orc.to_bf16_bits(lg)) if b16 else lg
            for k, p, min_p in S.fallback_settings(V):
                sup = S.support(x, 0.0, 1.0, k, p, min_p, slack=S.FALLBACK_SLACK)
                outer = sup.set | sup.near
                assert sup.tokens.size >= 8 and max(outer) < V - V // 8, "a masked token is in the support"
                if min_p > 0 or (b16 and seed >= 4) or (V > 4097 and seed >= 4):
                    continue                                   # (the C oracle has no min-p; a sort of the whole vector per draw: the first vectors of the large sizes)
                for r in S.FALLBACK_DRAWS:
                    tok = orc.sample_stochastic(x, 0.0, 1.0, k, p, r)[0]
                    assert tok in outer, (V, seed, b16, (k, p), r, tok)
                    if r == 1.0 and p >= 1.0:
                        assert tok == sup.last()
