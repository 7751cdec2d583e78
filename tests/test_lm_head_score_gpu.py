"""GPU: prompt log-probabilities from the scoring lm_head (lm_head_score_bf16, csrc/lm_head_score.hip) against float64 on the CPU, and its bitwise properties: the tie
rule, target == argmax, determinism, row invariance.

Bar on every log-probability: BAR[softcap] + 2 * delta.  BAR is test_token_logprobs_gpu.py's (derived there for EXACT z: expf / logf at a few ulp, a fixed-order sum
of up to 2^18 terms, tanhf at a few ulp under a softcap of 30).  Here z carries the GEMM's accumulation error: a chain of K fp32 additions is off by at most
delta = K * 2^-23 * max_i sum_k |x_k W_ik| (K roundings of half an ulp 2^-24 each, on partial sums bounded by sum |x w|, with a factor 2 for the products' own alignment
inside the matrix instruction); softcap and log-sum-exp are 1-Lipschitz in the max norm, so z_t and log S each move by at most delta.  A derived bound, not a
measurement: the measured maxima are printed (-s) and recorded in profiles/r12_prompt_logprobs.md.

fmt 1 (an e4m3 table) is held to float64 of "sum the exact e4m3 values, THEN multiply by the channel's scale" -- matvec_f32out's arithmetic.  Against the prefill
GEMM's "w = bf16(decode * scale), then sum" the bar need NOT hold (each weight moves by up to 2^-9 relative before the sum): the difference is printed, not asserted.

Shapes, with S the slab size: rows 1, 5, 128, 129, 200 (a ragged row block, a second block); vocab 1000 and 2 S + 37 (a ragged tile; three slabs, the last ragged); K 64, 72, 512
(one K-tile, a ragged one, several) -- the ragged K of an e4m3 table is 80, since the entry refuses K % 16 != 0 there; 262144 (the workload's 256 slabs of 8 tiles and its
index width) and 40000 (slabs of two tiles, the last with one) at 3 rows."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import bf16_bits_to_f32, dev_i32, dev_u16, empty_u8, f32_to_bf16_bits
from mila_amd import capi

pytestmark = pytest.mark.gpu

BAR = {0.0: 5e-5, 30.0: 1e-4}
SENT_F, SENT_I = -777.25, -77
ROWS = (1, 5, 128, 129, 200)
S_SMALL = capi.lm_head_score_slab(1000)                 # 128: one tile per slab below 32768 entries
VOCABS = (1000, 2 * S_SMALL + 37)
KS = (64, 72, 512)                                       # one K-tile, a ragged K-tile, several


def _k(K, fmt):
    """the ragged K-tile of an e4m3 table: the entry takes whole 16-byte segments only (K % 16 == 0 with fmt 1), so 72 becomes 80"""
    return 80 if (K == 72 and fmt == 1) else K


def _e4m3_table():
    b = np.arange(256)
    ex, man = (b >> 3) & 15, b & 7
    mag = np.where(ex == 0, man * 2.0 ** -9, (1 + man / 8.0) * 2.0 ** (ex.astype(np.float64) - 7))
    mag = np.where((ex == 15) & (man == 7), np.nan, mag)
    return np.where(b & 0x80, -mag, mag)


E4M3 = _e4m3_table()


def _special_targets(V):
    S = capi.lm_head_score_slab(V)
    t = [0, V - 1, 127, 128, S - 1, S, 2 * S - 1, 2 * S, -1, V // 3, V, -5]
    return [v for v in t if v <= V]                        # V itself and -5: outside the vocabulary -> NaN


class Case:
    """x [rows, K] and W [V, K] (bf16 values), the device copies, and the float64 reference of every row: log-probabilities [rows, V], z, and delta [rows]"""

    def __init__(self, V, K, fmt, softcap, rows=200, seed=0, W_edit=None, x_edit=None):
        rng = np.random.default_rng(seed + 7 * V + K)
        xb = f32_to_bf16_bits(rng.standard_normal((rows, K)).astype(np.float32))
        Wb = f32_to_bf16_bits((rng.standard_normal((V, K)) * (2.0 / np.sqrt(K))).astype(np.float32))
        if x_edit is not None:
            x_edit(xb)
        if W_edit is not None:
            W_edit(Wb)
        self.V, self.K, self.fmt, self.softcap, self.rows = V, K, fmt, softcap, rows
        self.x_dev = dev_u16(xb)
        x = bf16_bits_to_f32(xb).astype(np.float64)
        if fmt == 0:
            self.W_dev, self.s_dev = dev_u16(Wb), None
            w, sc = bf16_bits_to_f32(Wb).astype(np.float64), np.ones(V)
        else:
            self.W_dev = empty_u8(V, K)
            self.s_dev = torch.empty(V, dtype=torch.float32, device="cuda:0")
            capi.call("quantize_fp8_per_channel", self.W_dev, self.s_dev, dev_u16(Wb), V, K)          # the project's own quantizer
            torch.cuda.synchronize()
            q, sc = self.W_dev.cpu().numpy(), self.s_dev.cpu().numpy().astype(np.float64)
            w = E4M3[q]
            assert np.isfinite(w).all()
            wq = bf16_bits_to_f32(f32_to_bf16_bits((w * sc[:, None]).astype(np.float32))).astype(np.float64)
            self.y_gemm_order = x @ wq.T                                                             # bf16(decode * scale), then sum: NOT this entry's contract
        y = (x @ w.T) * sc[None, :]                                                                  # sum, then scale
        self.delta = K * 2.0 ** -23 * ((np.abs(x) @ np.abs(w).T) * np.abs(sc)[None, :]).max(axis=1)
        self.z = self._cap(y)
        self.ref = self._logsoftmax(self.z)
        st = _special_targets(V)
        self.targets = np.array([st[r % len(st)] for r in range(rows)], dtype=np.int32)
        self.t_dev = dev_i32(self.targets)

    def _cap(self, y):
        return self.softcap * np.tanh(y / self.softcap) if self.softcap > 0 else y

    @staticmethod
    def _logsoftmax(z):
        m = z.max(axis=1, keepdims=True)
        return (z - m) - np.log(np.exp(z - m).sum(axis=1, keepdims=True))

    def run(self, first=0, rows=None, argmax=True, targets_dev=None, x_dev=None):
        rows = self.rows - first if rows is None else rows
        lp = torch.full((rows + 1,), SENT_F, dtype=torch.float32, device="cuda:0")
        am = torch.full((rows + 1,), SENT_I, dtype=torch.int32, device="cuda:0")
        alp = torch.full((rows + 1,), SENT_F, dtype=torch.float32, device="cuda:0")
        x = (self.x_dev if x_dev is None else x_dev)[first:first + rows]
        t = (self.t_dev if targets_dev is None else targets_dev)[first:first + rows]
        capi.lm_head_score(x, self.W_dev, self.s_dev, t, self.softcap, lp[:rows], am[:rows] if argmax else None, alp[:rows] if argmax else None)
        torch.cuda.synchronize()
        lp, am, alp = lp.cpu().numpy(), am.cpu().numpy(), alp.cpu().numpy()
        assert lp[rows] == SENT_F and am[rows] == SENT_I and alp[rows] == SENT_F, "a word behind an output was written"
        if not argmax:
            assert (am == SENT_I).all() and (alp == SENT_F).all()
        return lp[:rows], am[:rows], alp[:rows]

    def check(self, out, first=0):
        """the three outputs of rows first .. against float64; returns the worst |logprob - float64|"""
        lp, am, alp = out
        n = lp.size
        rows = np.arange(first, first + n)
        t = self.targets[rows]
        inside = (t >= 0) & (t < self.V)
        assert np.isnan(lp[~inside]).all(), "a target outside the vocabulary must report NaN"
        bar = BAR[self.softcap] + 2 * self.delta[rows]
        err = np.abs(lp[inside].astype(np.float64) - self.ref[rows[inside], t[inside]])
        assert (err <= bar[inside]).all(), ("logprob", float(err.max()), float(bar[inside].min()))
        assert ((am >= 0) & (am < self.V)).all()
        aerr = np.abs(alp.astype(np.float64) - self.ref[rows, am])
        assert (aerr <= bar).all(), ("argmax_logprob", float(aerr.max()), float(bar.min()))
        top2 = np.partition(self.z[rows], self.V - 2, axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 2 * self.delta[rows]
        assert np.array_equal(am[clear], self.z[rows].argmax(axis=1)[clear]), "argmax differs on a row whose float64 top two are more than 2 delta apart"
        hit = inside & (t == am)
        assert np.array_equal(lp[hit].view(np.uint32), alp[hit].view(np.uint32)), "target == argmax must carry the argmax entry's bits"
        return float(max(err.max() if err.size else 0.0, aerr.max()))


@functools.lru_cache(maxsize=4)
def _case(V, K, fmt, softcap):
    return Case(V, K, fmt, softcap)


def _bits(out):
    return [a.view(np.uint32).tolist() for a in out]


@pytest.mark.parametrize("softcap", [0.0, 30.0])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VOCABS)
def test_against_float64(V, K, fmt, softcap):
    K = _k(K, fmt)
    c = _case(V, K, fmt, softcap)
    worst = 0.0
    for rows in ROWS:
        out = c.run(0, rows)
        worst = max(worst, c.check(out))
        if rows == 200:
            assert _bits(out) == _bits(c.run(0, rows)), "two runs differ"
            lp_only = c.run(0, rows, argmax=False)[0]
            assert lp_only.view(np.uint32).tolist() == out[0].view(np.uint32).tolist()
    line = "lm_head_score V=%d K=%d fmt=%d softcap=%g: max |logprob - float64| = %.3e (bar %g + 2 delta, delta <= %.2e)" % (V, K, fmt, softcap, worst, BAR[softcap], c.delta.max())
    if fmt == 1:
        alt = Case._logsoftmax(c._cap(c.y_gemm_order))
        line += "; float64 of the GEMM order differs from the contract's by up to %.2e" % np.abs(alt - c.ref).max()
    print(line)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("V", [262144, 40000])
def test_the_workloads_vocabulary_and_a_ragged_last_slab(V, fmt):
    """262144: the workload's slab count (256 slabs of 8 tiles) and index width.  40000: 313 tiles in slabs of two, the last slab with one tile"""
    c = Case(V, 64, fmt, 30.0, rows=3)
    S = capi.lm_head_score_slab(V)
    assert S == (1024 if V == 262144 else 256)
    for targets in ([0, V - 1, S], [S - 1, 2 * S - 1, V - S], [V - 129, -1, V // 2 + 1]):
        c.targets = np.array(targets, dtype=np.int32)
        c.t_dev = dev_i32(c.targets)
        out = c.run()
        worst = c.check(out)
        assert _bits(out) == _bits(c.run())
    print("lm_head_score V=%d K=64 fmt=%d rows=3: max |logprob - float64| = %.3e" % (V, fmt, worst))


@pytest.mark.parametrize("softcap", [0.0, 30.0])
@pytest.mark.parametrize("fmt", [0, 1])
def test_ties_go_to_the_lower_index_and_a_peak_is_certain(fmt, softcap):
    """every x row has a 8 in column 0; table rows with a 4 there and zeros elsewhere score 32, far above the rest.  Duplicates of such a row have equal z bit for bit:
    in two tiles of one slab, in two slabs -- the lower index wins.  One such row alone is a peak."""
    V, K = 40000, 64
    S = capi.lm_head_score_slab(V)
    assert S == 256
    four, eight = 0x4080, 0x4100                        # bf16 bits of 4.0 and 8.0

    def x_edit(xb):
        xb[:, 0] = eight

    for dups in ((10 + 128, 10), (300, 10), (V - 1, 3 * S + 5, 3 * S + 5 + 128), (777,)):
        def W_edit(Wb):
            for i in dups:
                Wb[i, :] = 0
                Wb[i, 0] = four
        c = Case(V, K, fmt, softcap, rows=5, W_edit=W_edit, x_edit=x_edit)
        c.targets = np.array([min(dups), max(dups), 0, min(dups), -1], dtype=np.int32)
        c.t_dev = dev_i32(c.targets)
        lp, am, alp = c.run()
        assert am.tolist() == [min(dups)] * 5, (dups, am.tolist())
        assert lp[0].view(np.uint32) == alp[0].view(np.uint32) and lp[3].view(np.uint32) == alp[3].view(np.uint32)
        assert lp[1].view(np.uint32) == alp[1].view(np.uint32), "a duplicate of the best row has its z, bit for bit"
        bar = BAR[softcap] + 2 * c.delta
        assert (np.abs(alp.astype(np.float64) - c.ref[np.arange(5), am]) <= bar).all()
        if len(dups) == 1:
            assert (alp > -1e-3).all() and lp[0] > -1e-3, alp


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("V,K", [(VOCABS[1], 72), (1000, 512)])
def test_row_invariance(V, K, fmt):
    """each row alone (rows = 1) against the same row inside calls of 5, 129 and 200 rows at different offsets, bit for bit; also from an x whose rows are a pad apart"""
    K = _k(K, fmt)
    c = _case(V, K, fmt, 30.0)
    alone = [c.run(r, 1) for r in range(c.rows)]
    for first, rows in ((0, 5), (77, 5), (3, 129), (71, 129), (0, 200)):
        got = c.run(first, rows)
        for j in range(rows):
            assert _bits([a[j:j + 1] for a in got]) == _bits(alone[first + j]), (first, rows, j)
    wide = torch.full((c.rows, K + 24), 0x7f80, dtype=torch.int16, device="cuda:0")                     # the pad is +inf: it must never be read
    wide[:, :K] = c.x_dev
    got = c.run(0, 200, x_dev=wide[:, :K])
    assert _bits(got) == _bits(c.run(0, 200))
