"""GPU: the multi-row decode Linear (csrc/matvec_rows.hip) is BATCH INVARIANT -- every output row of a 2 .. 4 row launch is bit-equal to the one-row entry
(matvec_* / matvec_f32out / fused_norm_matvec) called on that row alone.  Rows hold different data, row strides exceed the widths, outputs are handed in as NaN patterns
with one more row than the launch has, which must stay untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gpu_util import bits, dev_f32, dev_i32, dev_u16, dev_u8, empty_f32, empty_u16, host
from mila_amd import capi

pytestmark = pytest.mark.gpu

POISON16 = 0x7fc0
EPS = 1e-6


def _bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def _d(x):
    return dev_u16(orc.to_bf16_bits(x))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_W = {}


def _weights(N, K, fmt, G=128):
    """device weights of a shape and format, made once per process"""
    key = (N, K, fmt, G)
    if key not in _W:
        rng = np.random.default_rng(N * 7 + K + fmt)
        Wb = orc.to_bf16_bits((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
        if fmt == 0:
            _W[key] = (dev_u16(Wb), None)
        elif fmt == 1:
            q, s = orc.quantize_fp8_per_channel(Wb)
            _W[key] = (dev_u8(q), dev_f32(s))
        else:
            q, s = orc.quantize_fp4_per_group(Wb, G)
            _W[key] = (dev_u8(q), dev_f32(s))
    return _W[key]


def _rows_in(rng, rows, K, stride, scale=1.0):
    """[rows + 1, stride] bf16: every row different (and differently scaled), the padding and the extra row poisoned"""
    buf = np.full((rows + 1, stride), POISON16, dtype=np.uint16)
    for b in range(rows):
        buf[b, :K] = orc.to_bf16_bits(_bf(rng.standard_normal(K) * scale * (1 + b)))
    return dev_u16(buf)


def _fused_args(**kw):
    a = capi.fused_matvec_args()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return a


def _rows_args(a, rows, x_stride, y_stride, res_stride=0, res_out_stride=0, bias=None):
    r = capi.matvec_rows_args()
    r.a = a
    r.bias = bias.data_ptr() if bias is not None else None
    r.rows = rows
    r.x_stride, r.y_stride, r.res_stride, r.res_out_stride = x_stride, y_stride, res_stride, res_out_stride
    return r


def _run_rows(r):
    capi.check(capi.load().mila_cdna4_matvec_rows(C.byref(r), _stream()))


def _run_one(a):
    capi.check(capi.load().mila_cdna4_fused_norm_matvec(C.byref(a), _stream()))


def _plain_one(fmt, y, x, W, s, bias, K, N, G=128):
    if fmt == 0:
        capi.call("matvec_bf16", y, x, W, bias, K, N)
    elif fmt == 1:
        capi.call("matvec_bf16_qfp8", y, x, W, s, bias, K, N)
    else:
        capi.call("matvec_bf16_qfp4", y, x, W, s, bias, K, N, G)


def _check_rows_u16(Y, rows, N, ref_rows, what):
    got = bits(Y)
    for b in range(rows):
        assert np.array_equal(got[b, :N], ref_rows[b]), "%s: row %d differs from the one-row entry" % (what, b)
        assert (got[b, N:] == POISON16).all(), "%s: row %d wrote past its width" % (what, b)
    assert (got[rows] == POISON16).all(), "%s: the row past the batch was written" % what


@pytest.mark.parametrize("rows", [2, 3, 4])
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("K,N", [(256, 40), (4096, 129), (8192, 64), (15360, 96)])
def test_plain_rows_equal_the_one_row_entries(K, N, fmt, rows):
    """(256, 40): one partial step, mostly clamped chunks; (4096, 129): a ragged last group of waves; (8192, 64): the largest K with one x chunk per thread;
    (15360, 96): two x chunks per thread and the LDS maximum at four rows.  With a bias, as the plain entries take one."""
    rng = np.random.default_rng(K + N + 10 * fmt + rows)
    W, s = _weights(N, K, fmt)
    xs, ys = K + 24, N + 9
    X = _rows_in(rng, rows, K, xs)
    bias = _d(_bf(rng.standard_normal(N)))
    ref = []
    for b in range(rows):
        y = empty_u16(N)
        _plain_one(fmt, y, X[b, :K].clone(), W, s, bias, K, N)
        ref.append(bits(y))
    Y = empty_u16(rows + 1, ys)
    a = _fused_args(y=Y, x=X, W=W, scales=s if s is not None else 0, norm_w=0, post_w=0, res=0, res_out=0, post_scale=1.0, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=0,
                    f32_out=0)
    _run_rows(_rows_args(a, rows, xs, ys, bias=bias))
    _check_rows_u16(Y, rows, N, ref, "plain fmt %d K %d N %d" % (fmt, K, N))
    plan = capi.matvec_rows_plan(fmt, K, N, rows=rows)
    assert plan["U"] == capi.matvec_rows_plan(fmt, K, N, rows=1)["U"] and plan["xc"] == (1 if K <= 8192 else 2)


@pytest.mark.parametrize("rows", [2, 3, 4])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_norm_prologue_rows_equal_fused_norm_matvec(fmt, rows):
    K, N = 3840, 520
    rng = np.random.default_rng(fmt + rows)
    W, s = _weights(N, K, fmt)
    nw = _d(_bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    xs, ys = K + 8, N + 3
    X = _rows_in(rng, rows, K, xs, 2.0)
    kw = dict(W=W, scales=s if s is not None else 0, norm_w=nw, post_w=0, res=0, res_out=0, post_scale=1.0, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=0, f32_out=0)
    ref = []
    for b in range(rows):
        y = empty_u16(N)
        _run_one(_fused_args(y=y, x=X[b, :K].clone(), **kw))
        ref.append(bits(y))
    Y = empty_u16(rows + 1, ys)
    _run_rows(_rows_args(_fused_args(y=Y, x=X, **kw), rows, xs, ys))
    _check_rows_u16(Y, rows, N, ref, "norm prologue fmt %d" % fmt)


@pytest.mark.parametrize("rows", [2, 3, 4])
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("post_scale", [1.0, 0.75])
def test_sandwich_tail_geglu_rows_equal_fused_norm_matvec(post_scale, fmt, rows):
    """the post-attention tail + pre-FFN norm + fc_gate_up + GeGLU launch of the decode layer: y and the residual stream res_out, row by row"""
    K, N = 3840, 260
    rng = np.random.default_rng(fmt + 3 * rows + 100)
    W, s = _weights(2 * N, K, fmt)
    nw, pw = _d(_bf(1 + 0.1 * rng.uniform(-1, 1, K))), _d(_bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    xs, rs, ros, ys = K + 8, K + 16, K + 24, N + 5
    X, R = _rows_in(rng, rows, K, xs), _rows_in(rng, rows, K, rs)
    kw = dict(W=W, scales=s if s is not None else 0, norm_w=nw, post_w=pw, post_scale=post_scale, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=1, f32_out=0)
    ref_y, ref_r = [], []
    for b in range(rows):
        y, ro = empty_u16(N), empty_u16(K)
        _run_one(_fused_args(y=y, x=X[b, :K].clone(), res=R[b, :K].clone(), res_out=ro, **kw))
        ref_y.append(bits(y))
        ref_r.append(bits(ro))
    Y, RO = empty_u16(rows + 1, ys), empty_u16(rows + 1, ros)
    _run_rows(_rows_args(_fused_args(y=Y, x=X, res=R, res_out=RO, **kw), rows, xs, ys, rs, ros))
    _check_rows_u16(Y, rows, N, ref_y, "geglu fmt %d" % fmt)
    _check_rows_u16(RO, rows, K, ref_r, "res_out fmt %d" % fmt)


@pytest.mark.parametrize("rows", [2, 3, 4])
@pytest.mark.parametrize("fmt,N", [(0, 5000), (1, 300)])
def test_f32_rows_keep_the_samplers_first_stage_per_row(fmt, N, rows):
    """fp32 logits + per-row argmax partials: the logits are the one-row entry's bits, and sample_argmax_rows_final_advance picks, per ACTIVE row, the token
    sample_argmax_fp32 picks from that row's logits -- with duplicated weight rows, so every row's maximum is an exact tie across waves and workgroups that must go to
    the lowest index.  An inactive row keeps its token and its position."""
    lib = capi.load()
    K = 256
    rng = np.random.default_rng(N + rows)
    W, s = _weights(N, K, fmt)
    W, s = W.clone(), (s.clone() if s is not None else None)
    nw = _d(_bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    xs, ys = K + 8, N + 7
    X = _rows_in(rng, rows, K, xs)
    nb = lib.mila_cdna4_sample_scratch_bytes()
    kw = dict(W=W, scales=s if s is not None else 0, norm_w=nw, post_w=0, res=0, res_out=0, post_scale=1.0, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=0, f32_out=1)

    def one_row(b):
        y = empty_f32(N)
        _run_one(_fused_args(y=y, x=X[b, :K].clone(), **kw))
        return host(y)

    # every row's winner is copied over three other weight rows: exact ties in every row of the batch (the copies of another row's winner tie among themselves too)
    for b in range(rows):
        win = int(np.argmax(one_row(b)))
        dup = [(win + 17 * (b + 1)) % N, (win * 3 + 1 + b) % N, N - 1 - b]
        W[dup] = W[win].clone()
        if s is not None:
            s[dup] = s[win].clone()
    ref = [one_row(b) for b in range(rows)]
    want = []
    for b in range(rows):
        tied = np.flatnonzero(ref[b] == ref[b].max())
        assert tied.size >= 2, "the tie was not constructed"
        want.append(int(tied[0]))
    # the reference sampler on each row's logits
    scratch1 = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for b in range(rows):
        tok = dev_i32(np.array([-1]))
        capi.call("sample_argmax_fp32", dev_f32(ref[b]), tok, N, scratch1, C.c_size_t(nb))
        assert int(host(tok)[0]) == want[b]

    Y = empty_f32(rows + 1, ys)
    scratch = torch.full(((rows + 1) * nb,), 0x5A, dtype=torch.uint8, device="cuda")
    blocks = C.c_int(0)
    a = _fused_args(y=Y, x=X, **kw)
    a.argmax_scratch, a.argmax_scratch_bytes, a.argmax_blocks = scratch.data_ptr(), rows * nb, C.pointer(blocks)
    _run_rows(_rows_args(a, rows, xs, ys))
    got = host(Y)
    for b in range(rows):
        assert np.array_equal(got[b, :N].view(np.uint32), ref[b].view(np.uint32)), "logits of row %d differ from the one-row entry" % b
        assert np.isnan(got[b, N:]).all()
    assert np.isnan(got[rows]).all(), "the row past the batch was written"
    assert 0 < blocks.value <= nb // 8
    assert bool((scratch[rows * nb:] == 0x5A).all()), "partials written past the last row's scratch"
    # the last row is inactive: its token and position stay
    active = np.ones(rows, dtype=np.int32)
    active[rows - 1] = 0
    tok, pos = dev_i32(np.full(rows + 1, -7)), dev_i32(np.arange(rows + 1) * 10 + 3)
    capi.call("sample_argmax_rows_final_advance", tok, scratch, C.c_size_t(rows * nb), blocks.value, pos, dev_i32(active), rows)
    t, p = host(tok), host(pos)
    for b in range(rows - 1):
        assert int(t[b]) == want[b] and int(p[b]) == 10 * b + 4, (b, t, p, want)
    assert int(t[rows - 1]) == -7 and int(p[rows - 1]) == 10 * (rows - 1) + 3, "an inactive row moved"
    assert int(t[rows]) == -7 and int(p[rows]) == 10 * rows + 3, "the row past the batch moved"
    # all rows active; and the position bump alone
    capi.call("sample_argmax_rows_final_advance", tok, scratch, C.c_size_t(rows * nb), blocks.value, pos, dev_i32(np.ones(rows, dtype=np.int32)), rows)
    assert [int(v) for v in host(tok)[:rows]] == want
    before = host(pos).copy()
    capi.call("advance_positions_rows", pos, dev_i32(active), rows)
    assert np.array_equal(host(pos), before + np.concatenate([active, [0]]))


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("max_wg", [1, 3])
def test_rows_on_a_small_grid_walk_every_tail_of_the_streaming_loop(max_wg, fmt):
    """N = 200 columns (and fewer) on 1 / 3 workgroups of 16 waves: a wave's pipeline steps are its columns x the steps per column S.  K = 256 is S = 1 in every format,
    so 200 / 100 / 40 / 17 / 5 columns give waves with >= 4, 3, 2, 1 and 0 steps -- every peeled tail of the two-buffer loop; K = 4096 / 6144 are S = 2 / 3 at the
    formats' default chunks in flight (one column per wave: 2 and 3 steps, the refill of the third).  Then U = 1, 2, 4 through matvec.chunks_in_flight, the one-row kernel
    under the same setting being the reference."""
    N, rows = 200, 3
    try:
        capi.tune("matvec.max_workgroups", max_wg)
        cases = [(0, 256, n) for n in (200, 100, 40, 17, 5)] + [(0, 4096, 40), (0, 6144, 40), (0, 6144, 200)] + [(U, 4096, 40) for U in (1, 2, 4)]
        for U, K, n in cases:
            if U:
                capi.tune("matvec.chunks_in_flight", U)
            rng = np.random.default_rng(K + n + fmt)
            W, s = _weights(N, K, fmt)
            xs, ys = K + 8, N + 1
            X = _rows_in(rng, rows, K, xs)
            ref = []
            for b in range(rows):
                y = empty_u16(n)
                _plain_one(fmt, y, X[b, :K].clone(), W, s, None, K, n)
                ref.append(bits(y))
            Y = empty_u16(rows + 1, ys)
            a = _fused_args(y=Y, x=X, W=W, scales=s if s is not None else 0, norm_w=0, post_w=0, res=0, res_out=0, post_scale=1.0, eps=EPS, fmt=fmt, K=K, N=n, group=128,
                            geglu=0, f32_out=0)
            _run_rows(_rows_args(a, rows, xs, ys))
            _check_rows_u16(Y, rows, n, ref, "grid %d U %d K %d n %d fmt %d" % (max_wg, U, K, n, fmt))
            assert capi.matvec_rows_plan(fmt, K, n, rows=rows)["workgroups"] <= max_wg
    finally:
        capi.tune_reset()


def test_what_does_not_fit_is_refused():
    W, s = _weights(40, 256, 0)
    X, Y = _rows_in(np.random.default_rng(0), 4, 256, 256), empty_u16(5, 40)
    kw = dict(y=Y, x=X, W=W, scales=0, norm_w=0, post_w=0, res=0, res_out=0, post_scale=1.0, eps=EPS, fmt=0, K=256, N=40, group=128, geglu=0, f32_out=0)
    lib = capi.load()
    for rows in (1, 5):
        r = _rows_args(_fused_args(**kw), rows, 256, 40)
        assert lib.mila_cdna4_matvec_rows(C.byref(r), _stream()) == capi.MILA_E_UNSUPPORTED
    r = _rows_args(_fused_args(**kw), 2, 128, 40)      # rows would overlap
    assert lib.mila_cdna4_matvec_rows(C.byref(r), _stream()) == capi.MILA_E_INVALID_ARGUMENT
    assert (bits(Y) == POISON16).all()


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("R", [2, 4])
def test_output_columns_per_wave_step_do_not_enter_a_columns_arithmetic(R, fmt):
    """the model's tall Linears (fc_gate_up, the lm_head) run the ONE-ROW kernel with 2 or 4 output columns per wave step, the rows kernel always with one: a column's
    bits must not depend on it.  The one-row reference under matvec.rows_per_wave = 2 / 4 (GeGLU: at most 2) against the rows kernel, plain and sandwich tail + GeGLU
    forms, at a column count that is no multiple of R"""
    rows, K = 4, 3840
    rng = np.random.default_rng(R + 10 * fmt)
    try:
        capi.tune("matvec.rows_per_wave", R)
        assert capi.matvec_rows_plan(fmt, K, 523, rows=1)["R"] == R and capi.matvec_rows_plan(fmt, K, 523, rows=rows)["R"] == 1
        # plain
        N = 523
        W, s = _weights(N, K, fmt)
        xs, ys = K + 8, N + 1
        X = _rows_in(rng, rows, K, xs)
        ref = []
        for b in range(rows):
            y = empty_u16(N)
            _plain_one(fmt, y, X[b, :K].clone(), W, s, None, K, N)
            ref.append(bits(y))
        Y = empty_u16(rows + 1, ys)
        a = _fused_args(y=Y, x=X, W=W, scales=s if s is not None else 0, norm_w=0, post_w=0, res=0, res_out=0, post_scale=1.0, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=0,
                        f32_out=0)
        _run_rows(_rows_args(a, rows, xs, ys))
        _check_rows_u16(Y, rows, N, ref, "plain, one-row R %d fmt %d" % (R, fmt))
        # sandwich tail + GeGLU (the fc_gate_up launch)
        N = 261
        W, s = _weights(2 * N, K, fmt)
        nw, pw = _d(_bf(1 + 0.1 * rng.uniform(-1, 1, K))), _d(_bf(1 + 0.1 * rng.uniform(-1, 1, K)))
        Rr = _rows_in(rng, rows, K, xs)
        kw = dict(W=W, scales=s if s is not None else 0, norm_w=nw, post_w=pw, post_scale=0.75, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=1, f32_out=0)
        ref = []
        for b in range(rows):
            y, ro = empty_u16(N), empty_u16(K)
            _run_one(_fused_args(y=y, x=X[b, :K].clone(), res=Rr[b, :K].clone(), res_out=ro, **kw))
            ref.append(bits(y))
        Y, RO = empty_u16(rows + 1, N + 3), empty_u16(rows + 1, K)
        _run_rows(_rows_args(_fused_args(y=Y, x=X, res=Rr, res_out=RO, **kw), rows, xs, N + 3, xs, K))
        _check_rows_u16(Y, rows, N, ref, "geglu, one-row R %d fmt %d" % (R, fmt))
    finally:
        capi.tune_reset()
