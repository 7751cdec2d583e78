"""Inputs, float64 expectations and assertions for the row-kernel table (tests/row_kernel_classes.py), shared by tests/test_row_kernel_classes_cpu.py (the oracle, an
fp32 emulation and omitted-chunk mutants against the assertions) and tests/test_row_kernel_classes_gpu.py (the kernels against the same assertions).

An implementation under test is a function (case, inputs) -> outputs; `check(case, inputs, outputs)` is the one assertion every implementation meets.  Outputs are a
dict: bf16 tensors as uint16 bit patterns, fp32 tensors as float32.  Slices are laid out as the entries take them, [outer, dim] or [outer, dim, inner]; `as_slices`
turns either into [slices, dim].  The bars are those of tests/test_ops_gpu.py, unchanged."""
import numpy as np

import orc
import row_kernel_classes as tbl
from gpu_util import assert_bf16_close, bf16_bits_to_f32, f32_to_bf16_bits


def bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def as_slices(X, inner):
    """[outer, dim, inner] -> [outer * inner, dim] (slice o * inner + j), a copy; [outer, dim] as it is"""
    if inner == 1:
        return X
    return np.ascontiguousarray(np.swapaxes(X, 1, 2)).reshape(-1, X.shape[1])


def from_slices(S, inner):
    if inner == 1:
        return S
    return np.ascontiguousarray(np.swapaxes(S.reshape(-1, inner, S.shape[1]), 1, 2))


def weighted_elements(case, s0, s1):
    """(element index, sign) of the weighted element of slices s0 .. s1 - 1: position P[s % len(P)], slot s % unit, the sign alternating"""
    P = np.asarray(tbl.positions(case), dtype=np.int64)
    s = np.arange(s0, s1)
    return P[s % len(P)] * case.unit + s % case.unit, np.where(s % 2 == 0, 1.0, -1.0).astype(np.float32)


def block_ranges(case, max_elements=1 << 24):
    """slice ranges [s0, s1) that cover a case in blocks of at most max_elements (whole `outer` rows): the CPU tests walk the large cases block by block"""
    n = tbl.outer_of(case) * case.inner
    step = max(case.inner, (max_elements // case.dim) // case.inner * case.inner)
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def _background(case, s0, s1, scale, shift, rounded=True):
    """[s1 - s0, dim]: slice s takes row s % 8 of eight drawn rows (a large case does not draw 10^8 normals)"""
    rng = np.random.default_rng(case.dim * 131 + case.inner)
    base = (rng.standard_normal((8, case.dim)) * scale + shift).astype(np.float32)
    if rounded:
        base = bf(base)
    return base[np.arange(s0, s1) % 8]


def build_inputs(case, s0=0, s1=None):
    """the inputs of slices s0 .. s1 - 1 of a case (default: all of them, tbl.outer_of(case) * inner) as a dict; X in the entry's layout"""
    n = tbl.outer_of(case) * case.inner
    s1 = n if s1 is None else s1
    assert s0 % case.inner == 0 and s1 % case.inner == 0
    rng = np.random.default_rng(case.dim + 7 * case.inner)
    fp32 = case.op.endswith("fp32")
    rnd = (lambda v: np.asarray(v, dtype=np.float32)) if fp32 else bf
    e, sign = weighted_elements(case, s0, s1)
    rows = np.arange(s1 - s0)
    inp = dict(s0=s0, s1=s1, e=e)
    if case.op.startswith("softmax"):
        S = _background(case, s0, s1, 1.0, 0.0, rounded=not fp32)
        S[rows, e] = float(case.mode[1:])
        inp["X"] = from_slices(S, case.inner)
        return inp
    if case.op.startswith("fused_tail_norm"):
        where, scale, nxt = case.mode.split("_")
        A = _background(case, s0, s1, tbl.BACKGROUND, 0.0)
        RES = bf(np.roll(A, 3, axis=1) * 0.5)
        (A if where == "A" else RES)[rows, e] = tbl.SPIKE * sign
        # RES mode: the normalised a has unit scale whatever A's is, so post_w carries the background's 2^-6 and the weighted element of RES keeps 3/4 of the second sum
        pw = bf((1 + 0.1 * rng.uniform(-1, 1, case.dim)) * (1.0 if where == "A" else tbl.BACKGROUND))
        nw = bf(1 + 0.1 * rng.uniform(-1, 1, case.dim))
        inp.update(A=A, RES=RES, pw=pw, nw=nw if nxt == "next" else None, post_scale=1.0 if scale == "s1" else 0.75, eps=1e-6)
        return inp
    S = _background(case, s0, s1, tbl.BACKGROUND, 0.25 if case.op.startswith("layernorm") else 0.0, rounded=not fp32)
    S[rows, e] = tbl.SPIKE * sign
    inp["X"] = from_slices(S, case.inner)
    if case.op.startswith("rmsnorm"):
        m = case.mode
        inp.update(w=rnd(1 + 0.1 * rng.uniform(-1, 1, case.dim)) if m != "noweight" else None, b=rnd(0.05 * rng.uniform(-1, 1, case.dim)) if m == "bias" else None,
                   eps=1e-6 if m == "gemma" else 1e-5, off=1.0 if m == "unit_offset" else 0.0)
    elif case.op.startswith("layernorm"):
        inp.update(w=rnd(0.5 + 0.1 * rng.uniform(-1, 1, case.dim)), b=rnd(0.05 * rng.uniform(-1, 1, case.dim)) if case.mode == "bias" else None, eps=1e-5)
    return inp


def weight_share(case, inp):
    """per slice: the share of the reduction (sum of squares; of squared deviations for LayerNorm; 1.0 where the unit holds the absmax) the weighted unit holds"""
    key = "X" if "X" in inp else ("A" if case.mode.startswith("A") else "RES")
    S = as_slices(inp[key], case.inner).astype(np.float64)
    if case.op.startswith("layernorm"):
        S = S - S.mean(axis=1, keepdims=True)
    rows = np.arange(S.shape[0])
    u0 = inp["e"] // case.unit * case.unit
    if case.op.startswith("quantize"):
        m = np.abs(S).max(axis=1)
        return np.where(np.abs(S[rows, inp["e"]]) == m, 1.0, 0.0)
    q = S * S
    inside = sum(q[rows, u0 + k] for k in range(case.unit))
    return inside / q.sum(axis=1)


# ---- expectations: the float64 oracle -----------------------------------------------------------------------------------------------------------------------------
def expect(case, inp):
    op = case.op
    if op.startswith("rmsnorm"):
        y, r = orc.rmsnorm(inp["X"], inp["w"], inp["b"], eps=inp["eps"], w_offset=inp["off"], inner=case.inner, return_rstd=True)
        return dict(Y=y, rstd=r)
    if op.startswith("layernorm"):
        y, m, r = orc.cpu_layernorm(inp["X"], inp["w"], inp["b"], inp["eps"], return_stats=True)
        return dict(Y=y, mean=m, rstd=r)
    if op.startswith("softmax"):
        return dict(Y=orc.cpu_softmax(inp["X"], 1))
    if op.startswith("quantize"):
        q, s = orc.quantize_act_fp8_per_token(inp["X"])
        return dict(Q=q, scales=s)
    raise KeyError(op)


def oracle_as_outputs(case, inp):
    """the oracle's own outputs in the outputs' formats: what a perfect kernel returns"""
    ex = expect(case, inp)
    if case.op.endswith("bf16") and not case.op.startswith("quantize"):
        ex["Y"] = f32_to_bf16_bits(ex["Y"])
        if case.op.startswith("rmsnorm"):
            ex["rstd"] = f32_to_bf16_bits(ex["rstd"])
    return ex


# ---- the one assertion --------------------------------------------------------------------------------------------------------------------------------------------
def assert_bf16(got_bits, expected, atol, what):
    """gpu_util.assert_bf16_close(got, expected, 1, atol) over every element.  An element whose bits are RNE(expected), and finite, meets that bar by definition; only the
    others are handed on (a 10^8-element output is not widened to float64 to find that it is equal)."""
    got = np.asarray(got_bits, dtype=np.uint16).reshape(-1)
    exp = np.asarray(expected, dtype=np.float32).reshape(-1)
    assert got.size == exp.size, (got.size, exp.size)
    rest = np.flatnonzero((got != f32_to_bf16_bits(exp)) | ((got & 0x7f80) == 0x7f80))
    if rest.size:
        assert_bf16_close(got[rest], exp[rest], 1, atol, "%s (%d of %d elements differ from RNE(expected); the first at %d)" % (what, rest.size, got.size, int(rest[0])))


def assert_close(got, expected, atol, rtol, what):
    """numpy.testing.assert_allclose's bar, |got - expected| <= atol + rtol |expected| on every element (a NaN or an infinity fails), without its report of every
    mismatch: the CPU tests fail this on purpose, slice by slice"""
    got, expected = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(expected, dtype=np.float64).reshape(-1)
    assert got.size == expected.size, (what, got.size, expected.size)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - expected) <= atol + rtol * np.abs(expected))
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError("%s: %d of %d elements outside atol %g rtol %g; the first at %d: got %r expected %r" % (what, int(bad.sum()), bad.size, atol, rtol, i, got[i], expected[i]))


def check(case, inp, out, ex=None):
    """every output element of a case against the oracle at the project's bars (tests/test_ops_gpu.py: test_rmsnorm_rows, test_rmsnorm_fp32_row,
    test_layernorm_bf16_and_fp32, test_softmax; the quantizer bit-exact).  ex: expect(case, inp) where the caller has it already."""
    ex = expect(case, inp) if ex is None else ex
    op, what = case.op, case.name
    if op == "rmsnorm_bf16":
        assert_bf16(out["Y"], ex["Y"], 1e-30, what)
        assert_bf16(out["rstd"], ex["rstd"], 0, what + " rstd")
    elif op == "rmsnorm_fp32":
        got = np.asarray(out["Y"], dtype=np.float32).reshape(ex["Y"].shape)
        assert np.isfinite(got).all(), what
        assert np.abs(got - ex["Y"]).max() <= 4e-6 * max(1.0, float(np.abs(ex["Y"]).max())), what
        r = np.asarray(out["rstd"], dtype=np.float32).reshape(-1)
        assert np.isfinite(r).all() and np.abs(r - ex["rstd"].reshape(-1)).max() <= 4e-7 * float(np.abs(ex["rstd"]).max()), what + " rstd"
    elif op == "layernorm_bf16":
        assert_bf16(out["Y"], ex["Y"], 1e-6, what)
        assert_close(out["mean"], ex["mean"], 1e-5, 1e-7, what + " mean")            # (assert_allclose's default rtol beside the atol, as test_layernorm_bf16_and_fp32 has it)
        assert_close(out["rstd"], ex["rstd"], 0, 1e-5, what + " rstd")
    elif op == "layernorm_fp32":
        assert_close(out["Y"], ex["Y"], 1e-4, 0, what)
        assert_close(out["mean"], ex["mean"], 1e-5, 1e-7, what + " mean")            # (assert_allclose's default rtol beside the atol, as test_layernorm_bf16_and_fp32 has it)
        assert_close(out["rstd"], ex["rstd"], 0, 1e-5, what + " rstd")
    elif op == "softmax_fp32":
        got = np.asarray(out["Y"], dtype=np.float32).reshape(ex["Y"].shape)
        assert_close(got, ex["Y"], 2e-7, 1e-5, what)
        assert_close(got.astype(np.float64).sum(axis=1), np.ones(got.shape[:1] + got.shape[2:]), 1e-5, 1e-7, what + " sums to 1")
    elif op == "softmax_bf16":
        assert_bf16(out["Y"], ex["Y"], 1e-30, what)
    elif op == "quantize_fp8_per_token":
        assert np.array_equal(np.asarray(out["scales"], dtype=np.float32).view(np.uint32), ex["scales"].view(np.uint32)), what + ": scales differ"
        assert np.array_equal(np.asarray(out["Q"], dtype=np.uint8).reshape(ex["Q"].shape), ex["Q"]), what + ": e4m3 bytes differ"
    else:
        raise KeyError(op)


# ---- models in numpy: an fp32 emulation of a correct kernel, and float64 / fp32 mutants that leave the weighted unit out of one reduction ------------------------------
def _ordered_sum(v, T):
    """sum over axis 1 of [S, dim] in dtype T in a plain lane-then-group order: the 8 elements of a chunk, the 64 chunks of a group, the groups"""
    S, dim = v.shape
    pad = (-dim) % 512
    v = np.concatenate([v.astype(T), np.zeros((S, pad), dtype=T)], axis=1) if pad else v.astype(T)
    v = v.reshape(S, -1, 64, 8)
    return v.sum(axis=3, dtype=T).sum(axis=2, dtype=T).sum(axis=1, dtype=T)


def _mask(case, inp, S):
    """[S, dim] of 1, with 0 over the weighted unit of each slice"""
    keep = np.ones(S.shape, dtype=S.dtype)
    rows = np.arange(S.shape[0])
    u0 = inp["e"] // case.unit * case.unit
    for k in range(case.unit):
        keep[rows, u0 + k] = 0
    return keep


def model(case, inp, T=np.float32, omit=None):
    """the case's operation in numpy in dtype T.  omit = "sum" | "mean" | "max": that reduction leaves out the weighted unit of every slice (the sum of squares, of squared
    deviations or of exponentials; LayerNorm's mean; softmax's max or the quantizer's absmax) -- the kernel that loses a chunk.  Returns outputs in the outputs' formats."""
    op, dim = case.op, case.dim
    one = T(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if op.startswith("quantize"):
            X = inp["X"]
            if omit is None:
                q, s = orc.quantize_act_fp8_per_token(X)
            else:
                assert omit == "max"
                q, s = orc.quantize_act_fp8_per_token(X * _mask(case, inp, X))
            return dict(Q=q, scales=s)
        S = as_slices(inp["X"], case.inner).astype(T)
        keep = _mask(case, inp, S) if omit else None
        if op.startswith("rmsnorm"):
            assert omit in (None, "sum")
            q = S * S
            ss = _ordered_sum(q * keep if omit else q, T)
            rstd = one / np.sqrt(ss / T(dim) + T(inp["eps"]))
            Y = S * rstd[:, None]
            if inp["w"] is not None:
                Y = Y * (inp["w"].astype(T) + T(inp["off"]))
            if inp["b"] is not None:
                Y = Y + inp["b"].astype(T)
            out = dict(Y=from_slices(Y, case.inner), rstd=rstd)
            if op.endswith("bf16"):
                return dict(Y=f32_to_bf16_bits(out["Y"].astype(np.float32)), rstd=f32_to_bf16_bits(rstd.astype(np.float32)))
            return dict(Y=out["Y"].astype(np.float32), rstd=rstd.astype(np.float32))
        if op.startswith("layernorm"):
            assert omit in (None, "sum", "mean")
            mean = _ordered_sum(S * keep if omit == "mean" else S, T) / T(dim)
            d = S - mean[:, None]
            q = d * d
            var = _ordered_sum(q * keep if omit == "sum" else q, T) / T(dim)
            rstd = one / np.sqrt(var + T(inp["eps"]))
            Y = rstd[:, None] * d * inp["w"].astype(T)
            if inp["b"] is not None:
                Y = Y + inp["b"].astype(T)
            Y = Y.astype(np.float32)
            return dict(Y=f32_to_bf16_bits(Y) if op.endswith("bf16") else Y, mean=mean.astype(np.float32), rstd=rstd.astype(np.float32))
        if op.startswith("softmax"):
            assert omit in (None, "sum", "max")
            m = np.where(keep > 0, S, -np.inf).max(axis=1) if omit == "max" else S.max(axis=1)
            ex = np.exp(S - m[:, None])
            s = _ordered_sum(ex * keep if omit == "sum" else ex, T)
            Y = from_slices((ex * (one / s)[:, None]).astype(np.float32), case.inner)
            return dict(Y=f32_to_bf16_bits(Y) if op.endswith("bf16") else Y)
    raise KeyError(op)


def reductions(case):
    """the reductions of a case's operation a mutant can leave a chunk out of, with the dtype the mutant is modelled in.  A max that misses softmax's weighted element
    shows only through the overflow of exp in fp32 (in float64 the result is the same function), so that mutant is an fp32 model, at the height 120 the table has for it."""
    op = case.op
    if op.startswith("rmsnorm"):
        return [("sum", np.float64)]
    if op.startswith("layernorm"):
        return [("sum", np.float64), ("mean", np.float64)]
    if op.startswith("softmax"):
        return [("sum", np.float64)] + ([("max", np.float32)] if case.mode == "h120" else [])
    if op.startswith("quantize"):
        return [("max", np.float64)]
    return []


def failing_slices(case, inp, out, ex=None):
    """the slices on which `out` misses check(): the check, slice by slice"""
    bad = []
    n = inp["s1"] - inp["s0"]
    ex = expect(case, inp) if ex is None else ex

    def part_of(d, i):
        o = i // case.inner
        return {k: (v[o:o + 1] if k in ("Y", "Q") else np.asarray(v).reshape(-1)[i:i + case.inner]) for k, v in d.items()}
    for i in range(0, n, case.inner):
        o = i // case.inner
        sub = dict(inp, X=inp["X"][o:o + 1], e=inp["e"][i:i + case.inner], s0=inp["s0"] + i, s1=inp["s0"] + i + case.inner)
        try:
            check(case, sub, part_of(out, i), part_of(ex, i))
        except AssertionError:
            bad.append(i)
    return bad


# ---- the sandwich tail in float64, for the CPU test of its weighted rows ------------------------------------------------------------------------------------------------
def tail_model(case, inp, omit=None):
    """r = bf16(bf16(res + bf16(rmsnorm(a; post_w))) * post_scale), xn = bf16(rmsnorm(r; next_w)) with float64 reductions; omit = 1 | 2: that reduction leaves out the
    weighted chunk.  Returns (r bits, xn bits or None)."""
    A, RES = inp["A"].astype(np.float64), inp["RES"].astype(np.float64)
    keep = _mask(case, inp, A)
    qa = A * A
    rstd_a = 1.0 / np.sqrt((qa * keep if omit == 1 else qa).sum(axis=1) / case.dim + inp["eps"])
    an = bf((A * rstd_a[:, None] * inp["pw"].astype(np.float64)).astype(np.float32)).astype(np.float64)
    r = bf((RES + an).astype(np.float32))
    if inp["post_scale"] != 1.0:
        r = bf(r * np.float32(inp["post_scale"]))
    if inp["nw"] is None:
        return f32_to_bf16_bits(r), None
    r64 = r.astype(np.float64)
    qr = r64 * r64
    rstd_r = 1.0 / np.sqrt((qr * keep if omit == 2 else qr).sum(axis=1) / case.dim + inp["eps"])
    return f32_to_bf16_bits(r), f32_to_bf16_bits((r64 * rstd_r[:, None] * inp["nw"].astype(np.float64)).astype(np.float32))


# ---- q/k/v post-processing: weighted head rows ----------------------------------------------------------------------------------------------------------------------
def qkv_inputs(qc):
    """packed [T, NH HS | NKV HS | NKV HS] rows (no v block when kv_shared): head row r = t * heads + h of each stream weights chunk r % (HS / 8), slot r % 8"""
    rng = np.random.default_rng(qc.HS * 17 + qc.NH)
    HS, n = qc.HS, qc.HS // 8
    streams = []
    for heads in (qc.NH, qc.NKV) + (() if qc.kv_shared else (qc.NKV,)):
        S = bf(rng.standard_normal((qc.T * heads, HS)) * tbl.BACKGROUND)
        r = np.arange(qc.T * heads)
        S[r, (r % n) * 8 + r % 8] = tbl.SPIKE * np.where(r % 2 == 0, 1.0, -1.0)
        streams.append(S.reshape(qc.T, heads * HS))
    packed = np.ascontiguousarray(np.concatenate(streams, axis=1))
    qw, kw, vw = (bf(1 + 0.1 * rng.uniform(-1, 1, HS)) for _ in range(3))
    return packed, qw, kw, vw


# ---- RoPE beyond the grid cap: pairs drawn by angle ---------------------------------------------------------------------------------------------------------------------
def rope_inputs(rng, cos, sin, T, H, HS, pos_offset):
    """[1, T, H, HS] bf16 values whose rotated pairs stay at least 0.1 rad off both axes.  The rotation y0 = x0 c - x1 s, y1 = x0 s + x1 c in fp32 carries an error of
    about 2^-23 (|x0 c| + |x1 s|); where the rotated pair lands within 2^-14 of an axis, that is more than the one bf16 ulp of the small output the bar of
    test_rope_cache_and_rotation allows.  Among the 8.4 M outputs of this case's shape i.i.d. Gaussian inputs put a few hundred pairs there (measured: 7 outputs at 2
    ulp, every one of magnitude below 2^-13 of its operands), among the 2 560 of that test none.  The case is here for the indexing of the loop's second trip, so it draws the
    OUTPUT angle phi = k pi / 2 + U(0.1, pi / 2 - 0.1) and a radius in +-[0.5, 2], and rotates back with the device's own cache: |y| >= 0.1 r on every output."""
    half = HS // 2
    c = np.asarray(cos, dtype=np.float64)[pos_offset:pos_offset + T, None, :]
    s = np.asarray(sin, dtype=np.float64)[pos_offset:pos_offset + T, None, :]
    phi = rng.integers(4, size=(T, H, half)) * (np.pi / 2) + rng.uniform(0.1, np.pi / 2 - 0.1, (T, H, half))
    r = rng.uniform(0.5, 2.0, (T, H, half))
    y0, y1 = r * np.cos(phi), r * np.sin(phi)
    X = np.concatenate([y0 * c + y1 * s, y1 * c - y0 * s], axis=2)
    return bf(X.astype(np.float32)).reshape(1, T, H, HS)
