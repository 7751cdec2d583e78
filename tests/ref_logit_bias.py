"""The float32 restatement of the biased adjusted logit (include/mila_cdna4.h: logit bias) and the bias patterns of the kernel tests.  xb = x0 + bias is one fp32
addition; the penalties then act on xb in the place of x0 (tests/ref_sampling_filters.py: adjusted_logits).  Bit-exact only WITHOUT a softcap, as that oracle is
(numpy's tanh is ulps from the device's tanhf)."""
import numpy as np

import ref_sampling_filters as R

NEG_INF = np.float32(-np.inf)


def biased_logits(logits, bias):
    """xb without a softcap: lg + bias in float32"""
    return (np.ascontiguousarray(logits, dtype=np.float32) + np.ascontiguousarray(bias, dtype=np.float32)).astype(np.float32)


def adjusted_logits(logits, bias, table=None, rep=1.0, pres=0.0, freq=0.0):
    """x3 of every logit without a softcap: the bias first, then the penalties of `table` (None: none)"""
    xb = biased_logits(logits, bias)
    if table is None:
        return xb
    with np.errstate(invalid="ignore"):
        return R.adjusted_logits(xb, table, 0.0, rep, pres, freq)


def sparse_bias(logits, seed=0):
    """finite values of both signs on about an eighth of the ids, the six largest logits among them (pushed down and up by turns)"""
    lg = np.asarray(logits)
    V = lg.size
    rng = np.random.default_rng(7000 + seed + V)
    b = np.zeros(V, dtype=np.float32)
    ids = rng.choice(V, size=max(4, V // 8), replace=False)
    b[ids] = (rng.standard_normal(ids.size) * 3.0).astype(np.float32)
    top = np.argsort(-lg, kind="stable")[:6]
    b[top] = np.array([-7.5, 5.25, -3.0, 6.5, -1.25, 4.0], dtype=np.float32)[:top.size]
    return b


def ban_bias(logits):
    """token 0, token vocab - 1 and the unbiased argmax are forbidden"""
    lg = np.asarray(logits)
    b = np.zeros(lg.size, dtype=np.float32)
    b[[0, lg.size - 1, int(np.argmax(lg))]] = NEG_INF
    return b


def allow_bias(logits, n=3, seed=0):
    """a closed answer set of n tokens that holds neither the argmax nor vocab - 1: ranks 1 and 2 of the logits and n - 2 random ids"""
    lg = np.asarray(logits)
    V = lg.size
    order = np.argsort(-lg, kind="stable")
    rng = np.random.default_rng(9000 + seed + V)
    pool = [int(i) for i in rng.permutation(V - 1) if i != order[0]]      # (V - 1 is never drawn)
    ids = []
    for i in [int(order[1]), int(order[2])] + pool:
        if i != V - 1 and i not in ids:
            ids.append(i)
        if len(ids) == n:
            break
    b = np.full(V, NEG_INF, dtype=np.float32)
    b[ids] = 0.0
    return b, sorted(ids)


def patterns(logits):
    """name -> bias table of the three patterns of the identity test"""
    return {"sparse": sparse_bias(logits), "ban": ban_bias(logits), "allow3": allow_bias(logits, 3)[0]}
