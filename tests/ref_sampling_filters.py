"""NumPy restatements of the sampling filters (include/mila_cdna4.h: sampling filters) for the CPU and GPU tests: the adjusted logit in the fp32 operation order the
kernels pin, and the filtered stochastic sampler (the semantics stated at mila_amd/csrc/sampling.hip: "Stochastic sampler", plus min-p) with float64 sums and the
margins that say how far each of its decisions is from flipping."""
import numpy as np

FLAG = np.uint32(0x80000000)
COUNT_MASK = np.uint32(0x7fffffff)
NEUTRAL = (0.0, 1.0, 0.0, 0.0)              # (min_p, repetition_penalty, presence_penalty, frequency_penalty)
# the penalty triples (repetition, presence, frequency) of the exact-identity tests
PENALTIES = [(1.3, 0.0, 0.0), (1.0, 0.6, 0.4), (1.15, 0.5, 0.25)]
# ... of the greedy identity test: one more, strong enough to move the argmax at every vocabulary >= 257
GREEDY_PENALTIES = PENALTIES + [(2.0, 3.0, 1.0)]
# (temperature, top_k, top_p) per vocabulary for the exact-identity tests: chosen so that the table of make_table() changes at least one of the 25 draws' tokens at
# every vocabulary >= 257 (tests/test_sampling_filters_cpu.py asserts it from the oracle, before any GPU is involved)
IDENTITY_SETTINGS = {65: (1.0, 8, 0.9), 257: (1.0, 0, 0.95), 2049: (0.8, 64, 0.95), 4097: (0.7, 2048, 0.97), 262144: (0.8, 64, 0.95), 300001: (0.9, 200, 0.9)}


class Mt19937_64:
    """std::mt19937_64(seed) + std::uniform_real_distribution<float>(0, 1) in libstdc++'s arithmetic (generate_canonical<float, 24> takes ONE 64-bit output: the
    value rounded to float over 2^64, clipped below 1): the draws of GemmaModel's sampler, one per sample in the order of the samples"""
    M64 = (1 << 64) - 1

    def __init__(self, seed):
        mt = [int(seed) & self.M64]
        for i in range(1, 312):
            mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & self.M64)
        self.mt, self.i = mt, 312

    def raw(self):
        mt = self.mt
        if self.i >= 312:
            for i in range(312):
                x = (mt[i] & 0xFFFFFFFF80000000) | (mt[(i + 1) % 312] & 0x7FFFFFFF)
                mt[i] = mt[(i + 156) % 312] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
            self.i = 0
        x = mt[self.i]
        self.i += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEE000000000
        x ^= x >> 43
        return x & self.M64

    def uniform(self):
        u = np.array([self.raw()], dtype=np.uint64).astype(np.float32)[0] / np.float32(18446744073709551616.0)
        return min(u, np.nextafter(np.float32(1), np.float32(0)))


def random_logits(V, seed=0):
    """a few strong candidates over noise, like real logits (the generator of tests/test_sample_radix_gpu.py)"""
    rng = np.random.default_rng(V + seed)
    lg = (rng.standard_normal(V) * 4.0).astype(np.float32)
    lg[rng.integers(0, V, 8)] += 9.0
    return lg


def greedy_logits(V):
    """random_logits with a tie for the place behind the top: when a penalty takes the top away, the lower id must win"""
    lg = random_logits(V)
    lg[(3 * V) // 5] = lg[int(np.argsort(-lg, kind="stable")[1])]
    return lg


def capped(logits, softcap):
    """x0: the soft-capped logits in fp32 (numpy's tanh: ulps from the device's tanhf, so with a softcap only decisive draws are compared)"""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    if softcap > 0:
        c = np.float32(softcap)
        x = (c * np.tanh(x / c)).astype(np.float32)
    return x


def adjusted_logits(logits, table, softcap, rep, pres, freq):
    """x3 of every logit: fp32 throughout, every operation rounded on its own, inv_rep = 1.0f / rep divided once"""
    x0 = capped(logits, softcap)
    w = np.ascontiguousarray(table).view(np.uint32)
    rep, pres, freq = np.float32(rep), np.float32(pres), np.float32(freq)
    inv_rep = np.float32(1.0) / rep
    c = w & COUNT_MASK
    x1 = np.where(w != 0, np.where(x0 > 0, x0 * inv_rep, x0 * rep), x0).astype(np.float32)
    x2 = (x1 - (freq * c.astype(np.float32)).astype(np.float32)).astype(np.float32)
    return np.where(c > 0, (x2 - pres).astype(np.float32), x2).astype(np.float32)


def make_table(logits, seed=0):
    """the table of the kernel tests: the sixteen largest logits marked, alternating the prompt flag and the counts 1 .. 4, plus 200 random prompt flags and 48 random
    counts (drawn with replacement: fewer distinct words at a small vocabulary)"""
    lg = np.asarray(logits)
    V = lg.size
    rng = np.random.default_rng(1000 + seed + V)
    w = np.zeros(V, dtype=np.uint32)
    top = np.argsort(-lg, kind="stable")[:min(16, V)]
    for j, i in enumerate(top):
        w[i] = FLAG if j % 2 == 0 else np.uint32(1 + (j // 2) % 4)
    w[rng.integers(0, V, 200)] |= FLAG
    for i in rng.integers(0, V, 48):
        w[i] += np.uint32(rng.integers(1, 5))
    return w.view(np.int32)


def count_token(table, s):
    """what a sampler's tail does to the table after choosing s"""
    w = table.view(np.uint32)
    w[s] += np.uint32(1)


class Distribution:
    """the filtered distribution of one logits vector: e (fp32, the masked probabilities relative to the maximum) and the margins of the three cuts"""

    def __init__(self, logits, softcap, temperature, top_k, top_p, filters=NEUTRAL, table=None):
        min_p, rep, pres, freq = filters
        V = np.asarray(logits).size
        x3 = capped(logits, softcap) if table is None else adjusted_logits(logits, table, softcap, rep, pres, freq)
        x = (x3 / np.float32(temperature)).astype(np.float32)
        self.x = x
        self.m_topk = self.m_nucleus = self.m_minp = 1e30
        mx = x.max()
        keep = np.ones(V, dtype=bool)
        if 0 < top_k < V:
            xs = np.sort(x)[::-1]
            kthr, ak = xs[top_k], float(xs[top_k - 1])
            self.m_topk = (ak - float(kthr)) / max(abs(ak), 1e-30)
            keep = x > kthr                                    # strictly above the (k+1)-th largest
        e = np.where(keep, np.exp((x - mx).astype(np.float32)), np.float32(0)).astype(np.float32)
        total = float(e.astype(np.float64).sum())
        if top_p < 1.0:
            vals, counts = np.unique(e[e > 0], return_counts=True)
            vals, counts = vals[::-1], counts[::-1]            # descending; a tie group enters as a whole
            mass = np.cumsum(vals.astype(np.float64) * counts)
            target = float(np.float32(top_p)) * total
            hit = np.nonzero(mass > target)[0]
            if hit.size:
                g = hit[0]
                before = mass[g - 1] if g else 0.0
                self.m_nucleus = min(abs(mass[g] - target), abs(target - before)) / total
                e = np.where(e < vals[g], np.float32(0), e)
        if min_p > 0.0:
            alive = e[e > 0].astype(np.float64)
            if alive.size:
                self.m_minp = float(np.abs(alive / float(np.float32(min_p)) - 1.0).min())
            e = np.where(e < np.float32(min_p), np.float32(0), e)
        self.e = e
        self.cum = np.cumsum(e.astype(np.float64))
        self.total = float(self.cum[-1])

    def draw(self, r):
        """(token, margins[3]): the first index with e > 0 and cumulative >= r * total, vocab - 1 otherwise; margins as orc.sample_stochastic reports them"""
        target = float(np.float32(r)) * self.total
        cand = np.nonzero((self.e > 0) & (self.cum >= target))[0]
        m2 = 1e30
        tok = self.e.size - 1
        if cand.size:
            tok = int(cand[0])
            m2 = min(abs(self.cum[tok] - target), abs(target - (self.cum[tok] - float(self.e[tok])))) / self.total
        return tok, np.array([self.m_topk, self.m_nucleus, m2])

    def decisive(self, margins):
        """the rule of tests/test_sample_radix_gpu.py: the top-k cut is no near tie and the CDF bracket of the token is not within 2e-3 of the total of flipping"""
        return margins[0] > 1e-6 and margins[2] > 2e-3


def sample_filtered(logits, softcap, temperature, top_k, top_p, r, filters=NEUTRAL, table=None):
    """(token, margins[3], min-p margin) of one draw"""
    d = Distribution(logits, softcap, temperature, top_k, top_p, filters, table)
    tok, m = d.draw(r)
    return tok, m, d.m_minp


def argmax_filtered(logits, softcap, filters, table):
    """the penalized greedy token: argmax(x3), ties to the lower id"""
    return int(np.argmax(adjusted_logits(logits, table, softcap, *filters[1:])))
