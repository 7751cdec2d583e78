"""A plain reference of the stochastic sampler's SUPPORT -- the set of tokens that survive top-k, the nucleus and min-p -- and of each survivor's CDF bracket, in numpy
with integers and float64 only, and the designed inputs of tests/test_sample_support_cpu.py and tests/test_sample_support_gpu.py.

The semantics are those of oracle/mila_oracle.c: orc_sample_stochastic (and of tests/ref_sampling_filters.py for min-p):
    x = (softcap > 0 ? softcap * tanh(l / softcap) : l) / t
    top-k keeps x > the (k+1)-th largest x, compared as FLOATS: a tie group is all-in or all-out, and -0.0 == +0.0
    e = exp(x - max x) over the survivors; the nucleus keeps tie groups, highest first, until their mass EXCEEDS p * total
    min-p then drops e < min_p
    token(r) = the first index with e > 0 and cumulative >= r * total; vocab - 1 when nothing has mass

Exactness.  With softcap = 0 and t a power of two x = l / t is exact in fp32 and in float64 alike, so the top-k set is exact: no margin, no skipped draw.  The nucleus and
min-p compare masses the device holds in fp32 (and 2^-40 fixed point): `Support.m_nucleus` and `Support.m_minp` say how far the cut is from flipping, and the inputs
below are DESIGNED so that it is far (tests/test_sample_support_cpu.py asserts the margins)."""
import numpy as np

INF = 1e30


# ---- the order-preserving key of csrc/sampling.hip (ordered_key) and its inverse: inputs are written as keys -------------------------------------------------------
def key_of(x):
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def float_of(key):
    k = np.ascontiguousarray(key, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


KEY_LOWEST = 0x00800000          # key of -FLT_MAX: every key below it is -inf or a NaN
PLUS_ZERO, MINUS_ZERO = 0x80000000, 0x7FFFFFFF


class Support:
    """tokens: the survivors in token-index order; lo / hi: their CDF brackets as fractions of the surviving mass (float64); total: that mass relative to e(max) = 1"""

    def __init__(self, V, tokens, mass, m_nucleus, m_minp, near):
        self.V = V
        self.tokens = tokens
        self.set = set(int(i) for i in tokens)
        self.mass = mass
        self.total = float(mass.sum())
        cum = np.cumsum(mass)
        self.hi = cum / self.total if tokens.size else cum
        self.lo = self.hi - (mass / self.total if tokens.size else mass)
        self.m_nucleus, self.m_minp = m_nucleus, m_minp
        self.near = near          # tokens outside the support that a mass error of `slack` (support(..., slack=)) at the nucleus or min-p cut would let in

    def midpoints(self):
        return ((self.lo + self.hi) * 0.5).astype(np.float32)

    def min_bracket(self):
        return float((self.hi - self.lo).min()) if self.tokens.size else INF

    def last(self):
        """what the samplers return at r = 1: the last survivor; vocab - 1 when there is none"""
        return int(self.tokens[-1]) if self.tokens.size else self.V - 1


def support(logits, softcap, t, k, p, min_p=0.0, slack=0.0):
    x = np.ascontiguousarray(logits, dtype=np.float32).astype(np.float64)
    V = x.size
    if softcap > 0:
        x = float(softcap) * np.tanh(x / float(softcap))
    x = x / float(np.float32(t))
    keep = np.ones(V, dtype=bool)
    if 0 < k < V:
        keep = x > np.sort(x)[::-1][k]                       # strictly above the (k+1)-th largest; float compare: +0 == -0
    e = np.where(keep, np.exp(x - x.max()), 0.0)
    total = float(e.sum())
    near = np.zeros(V, dtype=bool)
    m_nucleus = m_minp = INF
    if p < 1.0 and keep.any():
        vals, counts = np.unique(x[keep], return_counts=True)
        vals, counts = vals[::-1], counts[::-1]              # descending: one entry per tie group
        after = np.cumsum(np.exp(vals - x.max()) * counts)
        before = after - np.exp(vals - x.max()) * counts
        target = float(np.float32(p)) * total
        g = int(np.nonzero(after > target)[0][0]) if (after > target).any() else vals.size - 1
        m_nucleus = min(abs(after[g] - target), abs(target - before[g])) / total
        near |= keep & (x < vals[g]) & (x >= vals[np.nonzero(before <= target + slack * total)[0][-1]])
        keep &= x >= vals[g]
        e = np.where(keep, e, 0.0)
    if min_p > 0.0 and keep.any():
        mp = float(np.float32(min_p))
        m_minp = float(np.abs(e[keep] / mp - 1.0).min())
        near |= keep & (e < mp) & (e >= mp * (1.0 - slack))
        keep &= e >= mp
        e = np.where(keep, e, 0.0)
    tokens = np.flatnonzero(keep)
    return Support(V, tokens, e[tokens], m_nucleus, m_minp, set(int(i) for i in np.flatnonzero(near & ~keep)))


# ---- part 2: top-k cases, written as keys --------------------------------------------------------------------------------------------------------------------------
# A case names the key of the (k+1)-th largest value (`k1`, the threshold the digit selection must find) and the key of the k-th largest (`kk`, the lowest survivor).
# The other survivors are distinct keys within 8000 ulps above kk (a relative 1e-3: near-equal masses, brackets about 1 / k); a few near misses lie within 8000 ulps
# below k1; the rest of the vocabulary is drawn from the keys between -FLT_MAX and k1.  Digits: d0 = key >> 21, d1 = (key >> 10) & 2047, d2 = key & 1023; radix_pick
# gives thread t the bins [8t, 8t + 8) of the first two passes and [4t, 4t + 4) of the last.
POS, NEG = 0xBF800000, 0x40400000            # keys of +1.0 and of about -1.5 with d1 = d2 = 0


def _k(base, d1=0, d2=0):
    return base | (d1 << 10) | d2


def T(name, V, k, k1, kk, ties="none", crowd=0, t=1.0, swap=False, exact=False):
    return dict(name=name, V=V, k=k, k1=k1, kk=kk, ties=ties, crowd=crowd, t=t, swap=swap, exact=exact)


# exact=True (the crowd ABOVE the boundary, 2 048 survivors of 4 097): brackets of 1 / 2048 are below the 1e-3 the other cases keep, so the case is built to need no
# margin at all -- every survivor lies within 2^-57 of the maximum (values near 2^-45), so its fp32 mass expf(x - max) is exactly 1.0, every partial sum is an integer
# below 2^24 and the midpoint (i + 0.5) / 2048 times the total 2048 is exact: the device's arithmetic has no rounding to be decisive about.
TINY = 0xA9000000                             # key of 2^-45

TOPK_CASES = [
    # where kk and k1 first differ | sign region | ties | the bin of k1's digit in the pass that separates them | crowd | k | V
    T("d0 pos", 65, 1, _k(POS, 5, 77), _k(POS + (3 << 21), 9, 1)),
    T("d0 pos k5", 4097, 5, _k(POS, 5, 77), _k(POS + (1 << 21), 0, 0)),
    T("d0 pos far", 4097, 5, _k(POS, 300, 77), _k(POS + (2 << 21), 1, 1)),
    T("d0 neg", 65, 5, _k(NEG, 5, 77), _k(NEG + (2 << 21), 5, 77)),
    T("d0 neg wide", 4097, 5, _k(NEG, 0, 0), _k(NEG + (1 << 21), 0, 0)),
    T("d0 cross sign", 65, 5, 0x4A7FFFFF, 0xB5800000),                                      # -2^-20 below +2^-20
    T("d0 cross sign k1", 4097, 1, 0x4A7FFFFF, 0xB5800000),
    T("d0 bin 7 of thread 0", 65, 5, (7 << 21) | 12345, POS),                               # k1 about -2e38: the last bin thread 0 owns in pass 0
    T("d0 bin 8, first of thread 1", 4097, 5, (8 << 21) | 12345, POS),
    T("d0 bin 4, the lowest finite", 65, 1, KEY_LOWEST + 5, NEG),                           # bins 0 .. 3 and 2044 .. 2047 of pass 0 hold only infinities and NaNs
    T("d0 bin 2043, the highest finite", 65, 1, 0xFF600000, 0xFF600000 + 900, t=0.5),       # ... so the highest is met with both keys in it (about 3e38: a d2 case)
    T("d1 pos", 65, 5, _k(POS, 100, 5), _k(POS, 101, 5)),
    T("d1 pos bin 0", 4097, 1, _k(POS, 0, 0), _k(POS, 1, 0)),
    T("d1 pos bin 7", 4097, 5, _k(POS, 7, 1023), _k(POS, 8, 0)),
    T("d1 pos bin 8", 65, 5, _k(POS, 8, 3), _k(POS, 9, 3)),
    T("d1 pos bin 2047", 4097, 5, _k(POS - (1 << 21), 2047, 9), _k(POS, 0, 9)),             # (then the carry reaches d0: a d0 case whose k1 digit is the last bin of pass 1)
    T("d1 pos bin 2046", 4097, 5, _k(POS, 2046, 9), _k(POS, 2047, 9)),
    T("d1 neg", 4097, 5, _k(NEG, 100, 5), _k(NEG, 1000, 5)),
    T("d1 neg bin 0", 65, 1, _k(NEG, 0, 1), _k(NEG, 3, 0)),
    T("d1 neg bin 8", 4097, 5, _k(NEG, 8, 0), _k(NEG, 9, 0)),
    T("d1 neg half t", 65, 5, _k(NEG, 7, 5), _k(NEG, 8, 5), t=0.5),
    T("d2 pos 1 ulp", 65, 5, _k(POS, 100, 5), _k(POS, 100, 6)),
    T("d2 pos 1 ulp k1", 4097, 1, _k(POS, 100, 500), _k(POS, 100, 501)),
    T("d2 pos bin 0", 4097, 5, _k(POS, 100, 0), _k(POS, 100, 1)),
    T("d2 pos bin 3", 65, 1, _k(POS, 100, 3), _k(POS, 100, 4)),
    T("d2 pos bin 4", 4097, 5, _k(POS, 100, 4), _k(POS, 100, 700)),
    T("d2 pos bin 1023 carry", 65, 5, _k(POS, 100, 1023), _k(POS, 101, 0)),                 # low ten bits 0x3FF against 0x000 of the digit above
    T("d2 pos bin 1023 carry k64", 4097, 64, _k(POS, 2047, 1023), _k(POS + (1 << 21), 0, 0)),
    T("d2 pos bin 1022", 4097, 5, _k(POS, 7, 1022), _k(POS, 7, 1023)),
    T("d2 neg 1 ulp", 4097, 5, _k(NEG, 100, 5), _k(NEG, 100, 6)),
    T("d2 neg 1 ulp k64", 65, 64, _k(NEG, 8, 0), _k(NEG, 8, 1)),
    T("d2 neg bin 3", 65, 1, _k(NEG, 0, 3), _k(NEG, 0, 4)),
    T("d2 neg carry", 4097, 1, _k(NEG, 7, 1023), _k(NEG, 8, 0)),
    T("d2 neg double t", 65, 5, _k(NEG, 100, 4), _k(NEG, 100, 9), t=2.0),
    T("+0 above -0", 65, 1, MINUS_ZERO, PLUS_ZERO),                                         # 1 ulp apart as keys, a carry through every digit, EQUAL as floats:
    T("+0 above -0 k5", 4097, 5, MINUS_ZERO, PLUS_ZERO),                                    # the two zeros go together and fewer than k survive
    T("-0 before +0", 65, 1, MINUS_ZERO, PLUS_ZERO, swap=True),                             # the same with -0.0 at the lower index
    T("-0 before +0 k5", 4097, 5, MINUS_ZERO, PLUS_ZERO, swap=True),
    T("tie straddles d0", 65, 5, _k(POS, 5, 77), _k(POS, 5, 77), ties="straddle"),
    T("tie straddles k1", 4097, 1, _k(NEG, 100, 5), _k(NEG, 100, 5), ties="straddle"),
    T("tie straddles k64", 4097, 64, _k(POS, 2047, 1023), _k(POS, 2047, 1023), ties="straddle"),
    T("tie inside d1", 65, 5, _k(POS, 100, 5), _k(POS, 101, 5), ties="inside"),
    T("tie inside d2 neg", 4097, 5, _k(NEG, 100, 5), _k(NEG, 100, 6), ties="inside"),
    T("all equal", 4097, 5, _k(POS, 100, 5), _k(POS, 100, 5), ties="all"),
    T("crowd below d2", 4097, 5, _k(POS, 100, 600), _k(POS, 100, 601), crowd=3000),
    T("crowd below d2 bin 1022 neg", 4097, 64, _k(NEG, 8, 1022), _k(NEG, 8, 1023), crowd=3000),
    T("crowd below d2 k1", 4097, 1, _k(POS, 7, 512), _k(POS, 7, 515), crowd=3500),
    T("crowd below tie straddles", 4097, 5, _k(POS, 100, 600), _k(POS, 100, 600), ties="straddle", crowd=3000),
    T("crowd above", 4097, 2048, _k(TINY, 100, 599), _k(TINY, 100, 600), crowd=1000, exact=True),
    T("crowd below 2^18", 262144, 5, _k(POS, 100, 600), _k(POS, 100, 601), crowd=200000),
    T("crowd below 300001", 300001, 5, _k(NEG, 2047, 900), _k(NEG, 2047, 901), crowd=250000),
]
TOPK_BY_NAME = {c["name"]: c for c in TOPK_CASES}
ROWS_SUBSET = ["d0 bin 8, first of thread 1", "d1 neg", "d2 pos bin 1022", "crowd below tie straddles"]     # one call of four rows (one k, one V), a class per row


# the classes bf16 logits can hold: the low 16 bits of the VALUE are zero, so the keys differ in the first digit or in the upper five bits of the second.  A case is
# written with the upper 16 bits of its keys; a negative value's key ends in 0xFFFF, a positive one's in 0x0000 (bf16_key).
def bf16_key(hi):
    return (hi << 16) | (0xFFFF if hi < 0x8000 else 0)


def T16(name, V, k, k1hi, kkhi, ties="none", swap=False):
    return dict(T(name, V, k, bf16_key(k1hi), bf16_key(kkhi), ties=ties, swap=swap), bf16=True)


BF16_CASES = [
    T16("bf16 d0 pos", 65, 5, 0xBF80, 0xBFC0),
    T16("bf16 d0 neg", 4097, 5, 0x4040, 0x4080),
    T16("bf16 d0 cross sign", 65, 1, 0x4A7F, 0xB580),
    T16("bf16 d1 pos 1 ulp", 4097, 5, 0xBF81, 0xBF82),
    T16("bf16 d1 pos 1 ulp k64", 4097, 64, 0xBF81, 0xBF82),
    T16("bf16 d1 neg 1 ulp", 65, 5, 0x4041, 0x4042),
    T16("bf16 d1 bin 0", 4097, 1, 0xBF80, 0xBF81),
    T16("bf16 d1 carry into d0", 4097, 5, 0xBF9F, 0xBFA0),
    T16("bf16 +0 above -0", 65, 1, 0x7FFF, 0x8000),
    T16("bf16 -0 before +0 k5", 4097, 5, 0x7FFF, 0x8000, swap=True),
    T16("bf16 tie straddles", 4097, 5, 0xBF85, 0xBF85, ties="straddle"),
]
assert bf16_key(0x7FFF) == MINUS_ZERO and bf16_key(0x8000) == PLUS_ZERO


def topk_logits(c):
    """the logits of a top-k case (fp32; bf16 values where the case says so) -- x = logits / t is exact, t being a power of two"""
    V, k, k1, kk = c["V"], c["k"], c["k1"], c["kk"]
    rng = np.random.default_rng(sum(map(ord, c["name"])) * 7919 + V)
    b16 = c.get("bf16", False)
    g = 1 << 16 if b16 else 1                                              # the step between two neighbouring keys
    span = max(8, 2 * k) if b16 else 8000                                  # the survivors lie within `span` steps above kk, the near misses as far below k1
    keys = []
    if c["ties"] == "all":
        keys = [k1] * V
    else:
        if c["exact"]:
            surv = [kk + j for j in range(k)]                              # 2 048 distinct keys in a row: they cross a d1 boundary
        else:
            n = k - 1
            if c["ties"] == "straddle":
                n = max(0, k - 2)                                          # the group takes the last two places (one when k = 1) inside the top k, and goes
            base = 0xBA800000 if kk == PLUS_ZERO else kk                   # the survivors above +0.0: normal values near 2^-10
            offs = rng.choice(np.arange(1, span + 1), size=n, replace=False).tolist()
            surv = [base + o * g for o in offs]
            if c["ties"] == "inside" and n >= 2:
                surv[1] = surv[0]                                          # a tie group wholly inside: still k survivors
            if c["ties"] == "straddle":
                surv += [k1] * (k - n)                                     # the group's members inside the top k (kk == k1) ...
            else:
                surv.append(kk)
        keys += surv
        keys += [k1] * (2 if c["ties"] == "straddle" else 1)               # ... and outside it (the (k+1)-th largest)
        lo = max(KEY_LOWEST | (g - 1), k1 - span * g)
        if k1 - g >= lo:
            keys += (k1 - g * rng.integers(1, (k1 - lo) // g + 1, size=min(6, V - len(keys)))).tolist()      # near misses
        if c["crowd"]:
            first = k1 & ~1023                                             # the keys that share k1's first two digits and lie below it
            assert k1 - first >= 500, "no room for a crowd below k1 in its own second digit"
            keys += rng.integers(first, k1, size=c["crowd"]).tolist()
        rest = V - len(keys)
        assert rest >= 0
        if b16:
            keys += [bf16_key(int(h)) for h in rng.integers((KEY_LOWEST >> 16) + 1, k1 >> 16, size=rest)]
        else:
            keys += rng.integers(KEY_LOWEST, k1, size=rest).tolist()
    keys = np.array(keys, dtype=np.uint32)
    perm = rng.permutation(V)
    out = np.empty(V, dtype=np.uint32)
    out[perm] = keys
    x = float_of(out)
    if c["k1"] == MINUS_ZERO and c["kk"] == PLUS_ZERO:
        ip, im = int(np.flatnonzero(out == PLUS_ZERO)[0]), int(np.flatnonzero(out == MINUS_ZERO)[0])
        if (im < ip) != c["swap"]:
            x[ip], x[im] = x[im], x[ip]
    lg = (x * np.float32(c["t"])).astype(np.float32)
    assert np.array_equal((lg / np.float32(c["t"])).astype(np.float32).view(np.uint32), x.view(np.uint32)), "logits / t is not exact"
    assert not b16 or not (lg.view(np.uint32) & np.uint32(0xFFFF)).any(), "a bf16 case holds a value bf16 cannot"
    return lg


def topk_draws(sup, k):
    """(midpoints of every survivor's bracket, a uniform grid of 4k draws -- 256 at the most, the case of 2 048 survivors)"""
    n = min(4 * k, 256)
    return sup.midpoints(), ((np.arange(n) + 0.5) / n).astype(np.float32)


# ---- part 3: nucleus and min-p cases, designed from levels ---------------------------------------------------------------------------------------------------------
def level_logits(V, levels, seed):
    """levels: [(logit, count)], the last count None = the rest of the vocabulary; scattered over the indices by a seeded permutation"""
    vals = []
    for v, n in levels:
        vals += [v] * (V - len(vals) if n is None else n)
    assert len(vals) == V
    out = np.empty(V, dtype=np.float32)
    out[np.random.default_rng(seed).permutation(V)] = np.array(vals, dtype=np.float32)
    return out


def _below(v, ulps):
    return float(float_of(np.array([key_of(np.float32(v))[0] - ulps], dtype=np.uint32))[0])


def N(name, V, levels, k, p, min_p=0.0, keeps=None):
    return dict(name=name, V=V, levels=levels, k=k, p=p, min_p=min_p, keeps=keeps)


def _fractions(V, levels):
    """cumulative mass fractions of the levels, from the top"""
    counts = [V - sum(m for _, m in levels if m is not None) if n is None else n for _, n in levels]
    mass = np.array([np.exp(v - levels[0][0]) * n for (v, _), n in zip(levels, counts)])
    return np.cumsum(mass) / mass.sum()


def nucleus_cases():
    """p is placed from the cumulative fractions f of the levels, 1.25e-2 or more from each; `keeps`: how many LEVELS (from the top) survive -- the design, which the CPU
    test holds support() to"""
    out = []
    for V in (65, 4097):
        base = [(0.0, 1), (-1.0, 8), (-2.0, 24 if V == 65 else 64), (-8.0, None)]
        f = _fractions(V, base)               # V = 65: .139 .548 .9985 1; V = 4097: .0717 .2826 .9033 1
        out += [N("the top token alone", V, base, 0, f[0] / 2, keeps=1),
                N("just short of a level sum", V, base, 0, f[1] - 0.015, keeps=2),
                N("just past a level sum: the next level enters whole", V, base, 0, f[1] + 0.015, keeps=3),
                N("the cut inside a level", V, base, 0, (f[1] + f[2]) / 2, keeps=3),
                N("only the lowest level goes", V, base, 0, f[2] - 0.0125, keeps=3)]
        # the boundary probability shares one / two digits of bits(e) with its neighbour level: x differs by 2^-11 / 2^-21 in relative terms
        for ulps, tag in ((1 << 12, "2^-11"), (4, "2^-21")):
            lv = [(0.0, 1), (-1.0, 8), (_below(-1.0, ulps), 8), (-8.0, None)]
            g = _fractions(V, lv)
            out += [N("levels %s apart, the lower one out" % tag, V, lv, 0, g[1] - 0.015, keeps=2),
                    N("levels %s apart, both in" % tag, V, lv, 0, g[1] + 0.015, keeps=3)]
        # e = exp(-30) = 2^-43.3: fixed-point mass 0 in radix_fixed, never in a nucleus with p < 1 (its whole level holds under 1e-11 of the mass: out by the oracle too)
        out.append(N("a level with mass below 2^-40", V, [(0.0, 1), (-1.0, 8), (-2.0, 16), (-30.0, None)], 0, 0.98, keeps=3))
        # top-k removes a tie group the nucleus would have kept: k = 20 cuts INSIDE the third level (9 tokens above it), so the level goes; p = 0.9 of what is left keeps
        # both levels (of the whole vector it would have reached into the third)
        out.append(N("top-k takes a level first", V, base, 20, 0.9, keeps=2))
        out.append(N("top-k, then a nucleus of the top token", V, base, 20, 0.2, keeps=1))
        out.append(N("min-p alone", V, base, 0, 1.0, min_p=0.2, keeps=2))                   # e = 1 and 0.368 stay; 0.135 and 3e-4 go
        out.append(N("min-p after a nucleus", V, base, 0, f[2] - 0.0125, min_p=0.2, keeps=2))
        out.append(N("min-p keeps what the nucleus kept", V, base, 0, f[1] - 0.015, min_p=0.05, keeps=2))
    for c in out:
        c["p"] = float(np.float32(round(float(c["p"]), 4)))
    return out


NUCLEUS_CASES = nucleus_cases()
NUCLEUS_GRID = ((np.arange(16) + 0.5) / 16).astype(np.float32)      # beside the midpoints of every survivor


def nucleus_logits(c):
    return level_logits(c["V"], c["levels"], seed=c["V"] + len(c["name"]))


# ---- part 5: the fallback of the inverse-CDF walk ------------------------------------------------------------------------------------------------------------------
FALLBACK_VECTORS = [(4097, 32), (65537, 32), (262144, 4)]
FALLBACK_FULL = 4          # the first vectors of a size go through every entry at every draw; the others through the radix, rows and search entries
ONE = np.float32(1.0)
FALLBACK_DRAWS = [1.0, float(np.nextafter(ONE, np.float32(0))), float(ONE - np.float32(2.0 ** -23)), float(ONE - np.float32(2.0 ** -20))]
FALLBACK_SLACK = 1e-4      # the cuts of a Gaussian vector are not designed: a token within this much mass of the nucleus / min-p cut may be in or out (Support.near)


def fallback_logits(V, seed):
    lg = np.random.default_rng(7000 + 131 * seed + V).standard_normal(V).astype(np.float32)
    lg[V - V // 8:] = -30.0
    return lg


def fallback_settings(V):
    """(top_k, top_p, min_p)"""
    return [(0, 0.9, 0.0), (V // 4, 1.0, 0.0), (0, 1.0, 0.05), (64, 0.95, 0.0)]
