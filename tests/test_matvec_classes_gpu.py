"""GPU: the decode Linear's weight stream (csrc/matvec_body.h, matvec.hip, matvec_rows.hip) at every case of tests/matvec_classes.py.

The exact leg: operands on which every partial sum and every output is exactly representable (one nonzero weight per 64-chunk group of a row, integer x, power-of-two
scales, prologues whose normed row is known exactly), so the bar is BIT EQUALITY with the float64 reference on y, res_out and the fp32 logits, with the poisoned padding
and the row past the batch untouched, and every workgroup's argmax partial the maximum (lowest column on ties) over the columns its waves own.  A chunk, a step, a scale
or a row taken from the wrong place changes an output (tests/test_matvec_classes_cpu.py shows it on a model of the stream).

The float64 leg: dense Gaussian operands, every entry form x format in the default launch shape at 1 and 3 rows; the operands of the stage under test are the bf16 bits
it receives (from the unfused entries on the device, themselves held to float64 at 1 ulp).  bf16 outputs: 1 bf16 ulp of RNE(float64) or 2^-17 sum |x w| of that element;
fp32 outputs: 2^-23 (S U EPC / 2 + 6) sum |x w|.  -s prints the worst measured ratio per case."""
import ctypes as C

import numpy as np
import pytest
import torch

import matvec_classes as mc
import test_matvec_rows_gpu as t
from gpu_util import assert_gemm_close, bits, dev_f32, dev_u16, dev_u8, empty_f32, empty_u16, f32_to_bf16_bits, bf16_bits_to_f32, host
from mila_amd import capi

pytestmark = pytest.mark.gpu

PAD = mc.PAD
FMT_FORM = [(fmt, f) for fmt in range(3) for f in mc.FORM_NAMES + ("combine",)]


def _rows_buf(vals, stride):
    """test_matvec_rows_gpu._rows_in with the rows given: [rows + 1, stride] bf16, the padding and the extra row poisoned"""
    rows, K = vals.shape
    buf = np.full((rows + 1, stride), t.POISON16, dtype=np.uint16)
    buf[:rows, :K] = mc.bf16_bits(vals)
    return dev_u16(buf)


def _dev_weights(c, o):
    W = mc.encode_weights(c, o.Wi)
    s = mc.scales_of(c, o.w)
    return (dev_u16(W) if c.fmt == 0 else dev_u8(W)), (dev_f32(s) if s is not None else None)


def _check_f32(Y, rows, N, want, what):
    got = host(Y)
    for b in range(rows):
        assert np.array_equal(got[b, :N].view(np.uint32), want[b].astype(np.float32).view(np.uint32)), "%s: fp32 row %d differs from the reference" % (what, b)
        assert np.isnan(got[b, N:]).all(), "%s: row %d wrote past its width" % (what, b)
    assert np.isnan(got[rows]).all(), "%s: the row past the batch was written" % what
    return got


def _check_partials(c, g, logits, scratch, nb, blocks, what):
    """every workgroup's (value, column) partial of every row: the maximum over the columns its waves own (row groups rg with rg % (16 blocks) // 16 == block), the lowest
    column on ties, from the DEVICE logits"""
    assert blocks == g.blocks, (what, blocks, g.blocks)
    raw = host(scratch)
    col = np.arange(c.N)
    owner = ((col // g.R) % g.total_waves) // mc.WAVES
    P = nb // 8
    for b in range(c.rows):
        v = raw[b * nb:(b + 1) * nb].view(np.float32)[:blocks]
        i = raw[b * nb:(b + 1) * nb].view(np.int32)[P:P + blocks]
        for k in range(blocks):
            mine = col[owner == k]
            top = logits[b, mine].max()
            assert v[k] == top and i[k] == mine[logits[b, mine] == top][0], "%s: partial of workgroup %d, row %d: (%r, %d)" % (what, k, b, v[k], i[k])
    assert (raw[c.rows * nb:] == 0x5A).all(), "%s: partials written past the last row's scratch" % what
    tied = sum(int((logits[b] == logits[b].max()).sum() > 1) for b in range(c.rows))
    return tied


def _run_exact(c):
    f, g, o = mc.FORM[c.form], mc.geometry(c), mc.operands(c)
    W, s = _dev_weights(c, o)
    rows, K, N = c.rows, c.K, c.N
    what = c.name
    if c.entry == "combine":
        y = empty_u16(2, N + PAD)
        capi.call("matvec_attn_combine", y, dev_f32(mc.combine_partials(c, o.X)), 3, K // c.hs, c.hs, W, s, c.fmt, N, c.group)
        t._check_rows_u16(y, 1, N, mc.bf16_bits(o.y), what)
        return
    p = mc.prologue_inputs(c, o.X) if f.pro else None
    xs, ys, rs, ros = K + 24, N + PAD, K + 16, K + 8
    X = _rows_buf(p.x if f.pro else o.X.astype(np.float64), xs)
    Y = empty_f32(rows + 1, ys) if f.f32 else empty_u16(rows + 1, ys)
    bias = dev_u16(mc.bf16_bits(o.bias)) if f.bias else None
    kw = dict(W=W, scales=s if s is not None else 0, norm_w=0, post_w=0, res=0, res_out=0, post_scale=1.0, eps=mc.EPS, fmt=c.fmt, K=K, N=N, group=c.group or 128,
              geglu=int(f.geglu), f32_out=int(f.f32))
    RO = None
    if f.pro:
        kw["norm_w"] = dev_u16(mc.bf16_bits(p.norm_w))
    if f.pro == 2:
        RO = empty_u16(rows + 1, ros)
        kw.update(post_w=dev_u16(mc.bf16_bits(p.post_w)), res=_rows_buf(p.res, rs), res_out=RO, post_scale=c.ps)
    nb = capi.load().mila_cdna4_sample_scratch_bytes()
    scratch, blocks = None, C.c_int(0)
    a = t._fused_args(y=Y, x=X, **kw)
    if f.argmax:
        scratch = torch.full(((rows + 1) * nb,), 0x5A, dtype=torch.uint8, device="cuda")
        a.argmax_scratch, a.argmax_scratch_bytes, a.argmax_blocks = scratch.data_ptr(), rows * nb, C.pointer(blocks)
    if c.entry == "rows":
        t._run_rows(t._rows_args(a, rows, xs, ys, rs, ros, bias=bias))
    elif f.pro:
        t._run_one(a)
    elif f.f32:
        capi.call("matvec_f32out", Y, X, W, s, c.fmt, K, N, c.group)
    else:
        t._plain_one(c.fmt, Y, X, W, s, bias, K, N, c.group)
    if RO is not None:
        t._check_rows_u16(RO, rows, K, mc.bf16_bits(p.res_out), what + " res_out")
    if f.f32:
        got = _check_f32(Y, rows, N, o.y, what)
        if f.argmax:
            return _check_partials(c, g, got[:, :N], scratch, nb, blocks.value, what)
    else:
        t._check_rows_u16(Y, rows, N, mc.bf16_bits(o.y), what)


@pytest.mark.parametrize("fmt,form", FMT_FORM)
def test_the_stream_is_exact_on_integer_rows(fmt, form):
    cases = [c for c in mc.CASES if c.fmt == fmt and c.form == form]
    assert cases
    tied = 0
    try:
        for c in cases:
            capi.tune_reset()
            for k, v in mc.tunings(c).items():
                capi.tune(k, v)
            try:
                tied += _run_exact(c) or 0
            except capi.MilaError as e:
                raise AssertionError("%s: %s" % (c.name, e)) from e
    finally:
        capi.tune_reset()
    if form == "tail_f32_argmax":
        kinds = {(c.entry, mc.geometry(c).R, c.rows) for c in cases}
        assert {("one", 1, 1), ("one", 2, 1), ("one", 4, 1), ("rows", 1, 2), ("rows", 1, 3), ("rows", 1, 4)} <= kinds and tied >= len(cases)
    print("%d cases" % len(cases))


# ---- the float64 leg -------------------------------------------------------------------------------------------------------------------------------------------------
def _vals(bits16):
    return bf16_bits_to_f32(bits16).astype(np.float64)


def _ulp1(got_bits, exact, what):
    """bf16 bits within 1 ulp of RNE(exact), every element (the unfused row kernels: one rounding of an fp32 value)"""
    got_bits, exact = np.asarray(got_bits).reshape(1, -1), np.asarray(exact, dtype=np.float64).reshape(1, -1)
    assert_gemm_close(got_bits, exact, np.zeros_like(exact), 1, what)


def _dev_quantized(fmt, q, s):
    return (dev_u16(q) if fmt == 0 else dev_u8(q)), (dev_f32(s) if s is not None else None)


def _rmsnorm_dev(xb, wb, rows, K):
    y = empty_u16(rows, K)
    capi.call("rmsnorm_bf16", y, None, xb, wb, None, rows, 1, K, mc.EPS, 0.0)
    return y


_rms64 = mc.rms64


def _hold(form, fmt, got, exact, mag, geo, stats_out, what):
    """an output [rows, N] against its float64 expectation and sum |x w|: the bars of this file's docstring"""
    if got.dtype == np.float32:
        err = np.abs(got.astype(np.float64) - exact)
        bound = mc.f32_bound(geo.S, geo.U, geo.epc, mag)
        ratio = float((err[mag > 0] / bound[mag > 0]).max())
        stats_out.append(("f32", ratio))
        assert np.isfinite(got).all() and (err <= bound).all(), "%s: fp32 output off by %.3g of its bound" % (what, ratio)
    else:
        st = {}
        assert_gemm_close(got, exact, mag, 1, what, atol_global=np.inf, stats=st)
        stats_out.append(("bf16 slack used", st["worst_ratio"] / mc.SLACK))
        stats_out.append(("bf16 worst ulp", float(st["worst_ulp"])))


def _run_dense(fmt, form, K, N, rows, stats):
    f = mc.FORM[form]
    group = 128
    d = mc.dense_case(fmt, form, K, N, rows)            # the draws the CPU test holds to the condition on the slack
    xv, Wd = d["x"], d["Wd"]
    W, s = _dev_quantized(fmt, d["q"], d["s"])
    c = mc.Case("dense", "one" if rows == 1 else "rows", form, fmt, group if fmt == 2 else 0, 0, 0, K, N, rows, False, 0, 0.75, 0)
    geo = mc.geometry(c)
    what = "dense %s f%d K %d N %d rows %d" % (form, fmt, K, N, rows)
    xs, ys, rs, ros = K + 24, N + PAD, K + 16, K + 8
    X = _rows_buf(xv, xs)
    xd = X[:rows, :K].contiguous()
    kw = dict(W=W, scales=s if s is not None else 0, norm_w=0, post_w=0, res=0, res_out=0, post_scale=1.0, eps=mc.EPS, fmt=fmt, K=K, N=N, group=group, geglu=int(f.geglu),
              f32_out=int(f.f32))
    bias_v, bias = None, None
    stage = xv                                   # the float64 values of the bf16 bits the stream receives
    RO = None
    if f.bias:
        bias_v = d["bias"]
        bias = dev_u16(mc.bf16_bits(bias_v))
    if f.pro:
        nwv = d["norm_w"]
        nw = dev_u16(mc.bf16_bits(nwv))
        kw["norm_w"] = nw
        src, srcv = xd, xv
        if f.pro == 2:
            pwv, resv = d["post_w"], d["res"]
            pw, R = dev_u16(mc.bf16_bits(pwv)), _rows_buf(resv, rs)
            a_ = _rmsnorm_dev(xd, pw, rows, K)
            _ulp1(bits(a_), _rms64(xv, pwv), what + ": rmsnorm(x, post_w)")
            r_ = empty_u16(rows, K)
            capi.call("residual_bf16", r_, R[:rows, :K].contiguous(), a_, C.c_int64(rows * K))
            _ulp1(bits(r_), resv + _vals(bits(a_)), what + ": residual")
            before = _vals(bits(r_))
            capi.call("scale_bf16", r_, r_, C.c_int64(rows * K), 0.75)
            _ulp1(bits(r_), before * 0.75, what + ": scale")
            RO = empty_u16(rows + 1, ros)
            kw.update(post_w=pw, res=R, res_out=RO, post_scale=0.75)
            src, srcv = r_, _vals(bits(r_))
        h_ = _rmsnorm_dev(src, nw, rows, K)
        _ulp1(bits(h_), _rms64(srcv, nwv), what + ": rmsnorm(., norm_w)")
        stage = _vals(bits(h_))
    exact = stage @ Wd.T + (bias_v[None, :] if bias_v is not None else 0.0)
    mag = np.abs(stage) @ np.abs(Wd).T

    def launch(kw, Y, n_out):
        a = t._fused_args(y=Y, x=X, **dict(kw, N=n_out))
        if rows > 1:
            t._run_rows(t._rows_args(a, rows, xs, Y.shape[1], rs, ros, bias=bias))
        elif f.pro:
            t._run_one(a)                        # (row 0 of X, of R and of RO)
        elif f.f32:
            capi.call("matvec_f32out", Y, xd, W, s, fmt, K, n_out, group)
        else:
            t._plain_one(fmt, Y, xd, W, s, bias, K, n_out, group)
        return host(Y) if Y.dtype == torch.float32 else bits(Y)

    if f.geglu:
        # gate / up: the non-GeGLU form of the same prologue over the 2 N rows, held to float64 here; y: 1 bf16 ulp of gelu(g) u on those bits, or 1e-6 |u|
        GU = empty_u16(rows + 1, 2 * N + PAD)
        gu = launch(dict(kw, geglu=0), GU, 2 * N)[:rows, :2 * N]
        _hold(form, fmt, gu, exact, mag, geo, stats, what + " gate/up")
        gv, uv = _vals(gu[:, :N]), _vals(gu[:, N:])
        Y = empty_u16(rows + 1, ys)
        got = launch(kw, Y, N)
        want = mc.gelu64(gv) * uv
        gotv = _vals(got[:rows, :N])
        ulp = np.abs(t_ordered(got[:rows, :N]) - t_ordered(f32_to_bf16_bits(want.astype(np.float32))))
        assert (np.isfinite(gotv) & ((ulp <= 1) | (np.abs(gotv - want) <= 1e-6 * np.abs(uv)))).all(), "%s: GeGLU output: worst %d ulp" % (what, int(ulp.max()))
        stats.append(("geglu_ulp", float(ulp.max())))
    else:
        Y = empty_f32(rows + 1, ys) if f.f32 else empty_u16(rows + 1, ys)
        got = launch(kw, Y, N)
        _hold(form, fmt, got[:rows, :N], exact, mag, geo, stats, what)
    assert (np.isnan(got[:rows, N:]).all() and np.isnan(got[rows]).all()) if f.f32 else ((got[:rows, N:] == t.POISON16).all() and (got[rows] == t.POISON16).all()), what
    zero = (np.abs(Wd).sum(1) == 0)[:N] if not f.geglu else np.zeros(N, dtype=bool)
    if zero.any() and not f.bias:
        assert (got[:rows, :N][:, zero] == 0).all(), what + ": the all-zero column"
    if RO is not None:
        assert np.array_equal(bits(RO)[:rows, :K], bits(src)), what + ": res_out differs from the unfused chain"
        assert (bits(RO)[:rows, K:] == t.POISON16).all() and (bits(RO)[rows] == t.POISON16).all()


def t_ordered(b16):
    b = np.asarray(b16, dtype=np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7fff), b)


def _run_dense_combine(fmt, HS, NH, splits, stats):
    K, N = NH * HS, mc.DENSE_COMBINE_N
    part, Wv = mc.dense_combine_case(fmt, HS, NH, splits)                              # one split empty
    P = dev_f32(part)
    what = "dense combine f%d HS %d NH %d splits %d" % (fmt, HS, NH, splits)
    # the merged row the stream receives.  No entry runs the attention combine kernel on hand-written partials, so the row comes from THIS entry's own prologue in front
    # of a bf16 identity matrix (y = x, exactly) and is held to the float64 merge here
    xm = empty_u16(K)
    capi.call("matvec_attn_combine", xm, P, splits, NH, HS, dev_u16(mc.bf16_bits(np.eye(K))), None, 0, K, 0)
    _ulp1(bits(xm), mc.merge64(part, HS), what + ": the merge")
    stage = _vals(bits(xm))[None, :]
    q, sc, Wd = mc.quantized64(fmt, Wv)
    W, s = _dev_quantized(fmt, q, sc)
    Y = empty_u16(2, N + PAD)
    capi.call("matvec_attn_combine", Y, P, splits, NH, HS, W, s, fmt, N, 128)
    got = bits(Y)
    c = mc.Case("dense", "combine", "combine", fmt, 128 if fmt == 2 else 0, 1, mc.COMBINE_U[fmt], K, N, 1, False, 0, 1.0, HS)
    _hold("combine", fmt, got[:1, :N], stage @ Wd.T, np.abs(stage) @ np.abs(Wd).T, mc.geometry(c), stats, what)
    assert (got[0, N:] == t.POISON16).all() and (got[1] == t.POISON16).all(), what


@pytest.mark.parametrize("fmt,form", FMT_FORM)
def test_the_stream_against_float64_on_dense_rows(fmt, form):
    stats = []
    if form == "combine":
        for HS, NH, splits in mc.DENSE_COMBINE:
            _run_dense_combine(fmt, HS, NH, splits, stats)
    else:
        for K, N in mc.DENSE_SHAPES:
            for rows in mc.DENSE_ROWS:
                _run_dense(fmt, form, K, N, rows, stats)
    worst = {}
    for k, v in stats:
        worst[k] = max(worst.get(k, 0.0), v)
    print("f%d %s: worst measured / bar: %s" % (fmt, form, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
