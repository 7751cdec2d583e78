"""The row kernels at every kernel form and tail class (tests/row_kernel_classes.py), on rows that carry their reduction's weight in one position: the base kernels
(RMSNorm, LayerNorm, softmax, per-token FP8 quantization) against the float64 oracle at the bars of tests/test_ops_gpu.py, every output element, through the one
assertion tests/test_row_kernel_classes_cpu.py proves sensitive (ref_row_kernels.check); the fused forms (sandwich tail, q/k/v post-processing, the norm prologues of the
decode Linear) bit for bit against the chains of those base kernels, as tests/test_fused_gpu.py builds them; and one case per capped-grid kernel beyond the cap, where
the grid-stride loop makes its second trip.  Output buffers come poisoned from gpu_util.empty_*."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import ref_row_kernels as ref
import row_kernel_classes as tbl
from gpu_util import bits, dev_f32, dev_i32, dev_u16, dev_u8, empty_f32, empty_u16, empty_u8, host
from mila_amd import capi

pytestmark = pytest.mark.gpu

BASE = [c for c in tbl.CASES if not c.op.startswith("fused_tail_norm")]
TAIL = [c for c in tbl.CASES if c.op.startswith("fused_tail_norm")]
EPS = 1e-6


def _d(x):
    return None if x is None else dev_u16(orc.to_bf16_bits(x))


def _f(x):
    return None if x is None else dev_f32(x)


def _run(case, inp):
    """the case's entry on the GPU -> outputs in ref.check's formats"""
    X = inp["X"]
    outer, dim, inner, op = X.shape[0], case.dim, case.inner, case.op
    if op == "rmsnorm_bf16":
        Y, rstd = empty_u16(*X.shape), empty_u16(outer * inner)
        capi.call(op, Y, rstd, _d(X), _d(inp["w"]), _d(inp["b"]), outer, inner, dim, inp["eps"], inp["off"])
        return dict(Y=bits(Y), rstd=bits(rstd))
    if op == "rmsnorm_fp32":
        Y, rstd = empty_f32(*X.shape), empty_f32(outer * inner)
        capi.call(op, Y, rstd, _f(X), _f(inp["w"]), _f(inp["b"]), outer, inner, dim, inp["eps"], inp["off"])
        return dict(Y=host(Y), rstd=host(rstd))
    if op == "layernorm_bf16":
        Y, mean, rstd = empty_u16(*X.shape), empty_f32(outer), empty_f32(outer)
        capi.call(op, Y, mean, rstd, _d(X), _d(inp["w"]), _d(inp["b"]), outer, dim, inp["eps"])
        return dict(Y=bits(Y), mean=host(mean), rstd=host(rstd))
    if op == "layernorm_fp32":
        Y, mean, rstd = empty_f32(*X.shape), empty_f32(outer), empty_f32(outer)
        capi.call(op, Y, mean, rstd, _f(X), _f(inp["w"]), _f(inp["b"]), outer, dim, inp["eps"])
        return dict(Y=host(Y), mean=host(mean), rstd=host(rstd))
    if op == "softmax_fp32":
        Y = empty_f32(*X.shape)
        capi.call(op, Y, _f(X), outer, dim, inner)
        return dict(Y=host(Y))
    if op == "softmax_bf16":
        Y = empty_u16(*X.shape)
        capi.call(op, Y, _d(X), outer, dim, inner)
        return dict(Y=bits(Y))
    if op == "quantize_fp8_per_token":
        Q, s = empty_u8(outer, dim), empty_f32(outer)
        capi.call(op, Q, s, _d(X), outer, dim)
        return dict(Q=host(Q), scales=host(s))
    raise KeyError(op)


@pytest.mark.parametrize("case", BASE, ids=[c.name for c in BASE])
def test_base_kernel_against_float64_on_weighted_rows(case):
    inp = ref.build_inputs(case)
    assert inp["X"].shape[0] == tbl.outer_of(case)
    ref.check(case, inp, _run(case, inp))


@pytest.mark.parametrize("K", sorted({c.dim for c in BASE if c.op == "quantize_fp8_per_token"}))
def test_quantizer_zero_row_and_absmax_at_powers_of_two(K):
    """an all-zero row (the 1e-12 floor of the scale) and rows whose absmax is 448 * 2^k, k = -20 .. 20 step 4: the scale is an exact power of two and x / scale exact"""
    ks = list(range(-20, 21, 4))
    rng = np.random.default_rng(K)
    X = ref.bf(rng.standard_normal((1 + len(ks), K)))
    X[0] = 0.0
    for i, k in enumerate(ks):
        row = X[1 + i]
        row *= np.float32(2.0 ** k)                                      # (exact: a power of two)
        row[np.abs(row) > 448.0 * 2.0 ** k] = 0.0
        row[(K - 8 + i) % K if i % 2 else (i * 8) % K] = (-1) ** i * 448.0 * 2.0 ** k
    Q, s = empty_u8(*X.shape), empty_f32(X.shape[0])
    capi.call("quantize_fp8_per_token", Q, s, _d(X), X.shape[0], K)
    eq, es = orc.quantize_act_fp8_per_token(X)
    assert np.array_equal(host(s).view(np.uint32), es.view(np.uint32))
    assert np.array_equal(host(Q), eq)
    assert host(s)[0] == np.float32(1e-12) / np.float32(448.0) and not host(Q)[0].any()
    assert np.array_equal(host(s)[1:], np.float32(2.0) ** np.asarray(ks, dtype=np.float32))


@pytest.mark.parametrize("case", TAIL, ids=[c.name for c in TAIL])
def test_tail_norm_equals_the_chain_on_weighted_rows(case):
    """fused_tail_norm[_quant]_bf16 == rmsnorm + residual (+ scale) + rmsnorm (+ quantize_fp8_per_token), bit for bit; every kernel of the chain is in the table at this dim"""
    inp = ref.build_inputs(case)
    T, D, ps = inp["A"].shape[0], case.dim, inp["post_scale"]
    a, res, pw, nw = _d(inp["A"]), _d(inp["RES"]), _d(inp["pw"]), _d(inp["nw"])
    an, r0, x0 = empty_u16(T, D), empty_u16(T, D), empty_u16(T, D)
    capi.call("rmsnorm_bf16", an, None, a, pw, None, T, 1, D, EPS, 0.0)
    capi.call("residual_bf16", r0, res, an, C.c_int64(T * D))
    if ps != 1.0:
        capi.call("scale_bf16", r0, r0, C.c_int64(T * D), ps)
    if nw is not None:
        capi.call("rmsnorm_bf16", x0, None, r0, nw, None, T, 1, D, EPS, 0.0)
    r1, x1 = empty_u16(T, D), empty_u16(T, D)
    if case.op == "fused_tail_norm_bf16":
        capi.call(case.op, r1, x1 if nw is not None else None, a, res, pw, nw, T, D, ps, EPS)
    else:
        q0, s0, q1, s1 = empty_u8(T, D), empty_f32(T), empty_u8(T, D), empty_f32(T)
        capi.call("quantize_fp8_per_token", q0, s0, x0, T, D)
        capi.call(case.op, r1, x1, q1, s1, a, res, pw, nw, T, D, ps, EPS)
        assert np.array_equal(host(s0).view(np.uint32), host(s1).view(np.uint32)), "per-token scales differ"
        assert np.array_equal(host(q0), host(q1)), "e4m3 rows differ"
    assert np.array_equal(bits(r0), bits(r1)), "residual stream differs"
    if nw is not None:
        assert np.array_equal(bits(x0), bits(x1)), "normed output differs"
    assert np.isfinite(orc.from_bf16_bits(bits(r1))).all()


# ---- q/k/v post-processing ----------------------------------------------------------------------------------------------------------------------------------------
def _gather(Kc, rows):
    """bf16 cache rows [1, NKV, cap, HS] at `rows` -> kv_write_fp8's source layout [1, T, NKV * HS]"""
    return Kc[0][:, torch.as_tensor(rows, device="cuda"), :].permute(1, 0, 2).contiguous()


@pytest.mark.parametrize("qc", tbl.QKV_CASES, ids=[q.name for q in tbl.QKV_CASES])
def test_qkv_post_equals_the_unfused_chain_on_weighted_head_rows(qc):
    HS, NH, NKV, T = qc.HS, qc.NH, qc.NKV, qc.T
    cap, pos0 = T + 1, 3                                       # positions 3 .. T + 2 on a ring of T + 1 rows: the chunk wraps
    max_seq = pos0 + T + 1
    packed, qw, kw, vw = ref.qkv_inputs(qc)
    qd, kd = NH * HS, NKV * HS
    width = packed.shape[1]
    assert width == qd + kd + (0 if qc.kv_shared else kd)
    cos, sin = empty_f32(max_seq, HS // 2), empty_f32(max_seq, HS // 2)
    capi.call("rope_build_cache", cos, sin, max_seq, HS, 1e4, qc.rot)
    P, dqw, dkw, dvw = _d(packed), _d(qw), _d(kw), (None if qc.kv_shared else _d(vw))
    # the unfused chain: split3 + q_norm + k_norm + v_norm + rope + kv_write
    q0, k0, v0 = empty_u16(T, qd), empty_u16(T, kd), empty_u16(T, kd)
    capi.call("split3_bf16", q0, k0, None if qc.kv_shared else v0, P, T, qd, kd, 0 if qc.kv_shared else kd)
    qn, kn, vn = empty_u16(T, qd), empty_u16(T, kd), empty_u16(T, kd)
    capi.call("rmsnorm_bf16", qn, None, q0, dqw, None, T * NH, 1, HS, EPS, 0.0)
    capi.call("rmsnorm_bf16", kn, None, k0, dkw, None, T * NKV, 1, HS, EPS, 0.0)
    capi.call("rmsnorm_bf16", vn, None, k0 if qc.kv_shared else v0, dvw, None, T * NKV, 1, HS, EPS, 0.0)
    capi.call("rope_forward_bf16", qn, kn, qn, kn, cos, sin, 1, T, NH, NKV, HS, pos0, max_seq)
    K0 = torch.zeros((1, NKV, cap, HS), dtype=torch.int16, device="cuda")
    V0 = torch.zeros_like(K0)
    capi.call("kv_write_bf16", K0, V0, kn, vn, 1, T, NKV, HS, pos0, cap)
    base_ptr = P.data_ptr()
    kptr = C.c_void_p(base_ptr + 2 * qd)
    vptr = kptr if qc.kv_shared else C.c_void_p(base_ptr + 2 * (qd + kd))
    rows = [(pos0 + t) % cap for t in range(T)]
    pos_dev = dev_i32([pos0])
    q1 = empty_u16(T, qd)
    qs, qv = empty_u16(NH, HS), empty_u16(NH, HS)              # the single-token entries: token 0 at pos0
    if not qc.fp8:
        K1, V1 = torch.zeros_like(K0), torch.zeros_like(K0)
        capi.call("fused_qkv_post_prefill", q1, K1, V1, P, kptr, vptr, C.c_int64(width), dqw, dkw, dvw, cos, sin, T, NH, NKV, HS, pos0, cap, EPS)
        assert np.array_equal(bits(K1), bits(K0)), "K cache differs"
        assert np.array_equal(bits(V1), bits(V0)), "V cache differs"
        for entry, where, qo in (("fused_qkv_post", pos0, qs), ("fused_qkv_post_devpos", pos_dev, qv)):
            Ks_, Vs_ = torch.zeros_like(K0), torch.zeros_like(K0)
            capi.call(entry, qo, Ks_, Vs_, P, kptr, vptr, dqw, dkw, dvw, cos, sin, NH, NKV, HS, where, cap, EPS)
            for got, full in ((Ks_, K0), (Vs_, V0)):
                e = np.zeros_like(bits(full))
                e[:, :, rows[0]] = bits(full)[:, :, rows[0]]
                assert np.array_equal(bits(got), e), entry + ": cache row differs"
    else:
        def caches():
            return [empty_u8(NKV, cap, HS), empty_u8(NKV, cap, HS), empty_f32(NKV, cap), empty_f32(NKV, cap)]

        def same(got, exp, what):
            for name, g, e in zip(("K8", "V8", "Ks", "Vs"), got, exp):
                g, e = host(g), host(e)
                assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, e.view(np.uint32) if e.dtype == np.float32 else e), "%s: %s differs" % (what, name)
        exp, got = caches(), caches()
        capi.call("kv_write_fp8", *exp, _gather(K0, rows), _gather(V0, rows), 1, T, NKV, HS, pos0, cap)
        capi.call("fused_qkv_post_kvfp8_prefill", q1, *got, P, kptr, vptr, C.c_int64(width), dqw, dkw, dvw, cos, sin, T, NH, NKV, HS, pos0, cap, EPS)
        same(got, exp, "prefill")
        exp1 = caches()
        capi.call("kv_write_fp8", *exp1, _gather(K0, rows[:1]), _gather(V0, rows[:1]), 1, 1, NKV, HS, pos0, cap)
        for entry, where, qo in (("fused_qkv_post_kvfp8", pos0, qs), ("fused_qkv_post_kvfp8_devpos", pos_dev, qv)):
            got1 = caches()
            capi.call(entry, qo, *got1, P, kptr, vptr, dqw, dkw, dvw, cos, sin, NH, NKV, HS, where, cap, EPS)
            same(got1, exp1, entry)
    assert np.array_equal(bits(q1), bits(qn)), "q differs"
    assert np.array_equal(bits(qs).reshape(-1), bits(qn)[0]) and np.array_equal(bits(qv).reshape(-1), bits(qn)[0]), "single-token q differs"
    # q_out against the float64 oracle: norm -> bf16 -> rotation with the device's cache
    q = packed[:, :qd].reshape(T * NH, HS)
    qe = orc.rope_rotate(ref.bf(orc.rmsnorm(q, qw, None, eps=EPS)).reshape(1, T, NH, HS), host(cos), host(sin), pos0)
    ref.assert_bf16(bits(q1), qe, 1e-30, qc.name + " q_out vs float64")


# ---- the norm and sandwich prologues of the decode Linear ----------------------------------------------------------------------------------------------------------
def _weights(rng, N, K, fmt):
    Wb = orc.to_bf16_bits((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
    if fmt == 0:
        return dev_u16(Wb), None
    q, s = orc.quantize_fp8_per_channel(Wb) if fmt == 1 else orc.quantize_fp4_per_group(Wb, 128)
    return dev_u8(q), dev_f32(s)


def _matvec(fmt, y, x, W, s, K, N):
    if fmt == 0:
        capi.call("matvec_bf16", y, x, W, None, K, N)
    elif fmt == 1:
        capi.call("matvec_bf16_qfp8", y, x, W, s, None, K, N)
    else:
        capi.call("matvec_bf16_qfp4", y, x, W, s, None, K, N, 128)


def _fused(**kw):
    a = capi.fused_matvec_args()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    capi.check(capi.load().mila_cdna4_fused_norm_matvec(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("geglu", [0, 1])
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("K", tbl.MATVEC_K)
def test_norm_matvec_prologues_equal_the_unfused_chain_on_weighted_rows(K, fmt, geglu):
    """fused_norm_matvec, PRO 1 (x <- rmsnorm(x)) and PRO 2 (the sandwich tail, with res and res_out), one launch per position class, against rmsnorm (+ residual +
    scale + rmsnorm) + matvec (+ geglu), bit for bit, res_out included"""
    rng = np.random.default_rng(K + fmt)
    N = tbl.MATVEC_N
    rows = 2 * N if geglu else N
    W, s = _weights(rng, rows, K, fmt)
    nw = _d(ref.bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    pw = _d(ref.bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    sc = s if s is not None else 0
    for i, c in enumerate(tbl.matvec_positions(K)):
        xb = ref.bf(rng.standard_normal(K) * tbl.BACKGROUND)
        rb = ref.bf(rng.standard_normal(K) * tbl.BACKGROUND)
        xb[c * 8 + c % 8] = rb[c * 8 + c % 8] = tbl.SPIKE * (-1) ** i
        x, res = _d(xb), _d(rb)
        for post_scale in (None, 1.0, 0.75):                     # None: PRO 1
            h, gu, y0 = empty_u16(K), empty_u16(rows), empty_u16(N)
            if post_scale is None:
                capi.call("rmsnorm_bf16", h, None, x, nw, None, 1, 1, K, EPS, 0.0)
            else:
                a_, r_ = empty_u16(K), empty_u16(K)
                capi.call("rmsnorm_bf16", a_, None, x, pw, None, 1, 1, K, EPS, 0.0)
                capi.call("residual_bf16", r_, res, a_, C.c_int64(K))
                if post_scale != 1.0:
                    capi.call("scale_bf16", r_, r_, C.c_int64(K), post_scale)
                capi.call("rmsnorm_bf16", h, None, r_, nw, None, 1, 1, K, EPS, 0.0)
            _matvec(fmt, gu, h, W, s, K, rows)
            if geglu:
                capi.call("geglu_bf16", y0, gu, 1, N)
            else:
                y0 = gu
            y1, r1 = empty_u16(N), empty_u16(K)
            what = "K=%d fmt=%d geglu=%d chunk %d post_scale %r" % (K, fmt, geglu, c, post_scale)
            if post_scale is None:
                _fused(y=y1, x=x, W=W, scales=sc, norm_w=nw, post_w=0, res=0, res_out=0, post_scale=1.0, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=geglu)
            else:
                _fused(y=y1, x=x, W=W, scales=sc, norm_w=nw, post_w=pw, res=res, res_out=r1, post_scale=post_scale, eps=EPS, fmt=fmt, K=K, N=N, group=128, geglu=geglu)
                assert np.array_equal(bits(r_), bits(r1)), what + ": residual stream differs"
            assert np.array_equal(bits(y0), bits(y1)), what + ": output differs"
            assert np.isfinite(orc.from_bf16_bits(bits(y1))).all(), what


# ---- beyond the grid cap: the second trip of the grid-stride loops -------------------------------------------------------------------------------------------------
def test_elementwise_vector_kernels_beyond_the_grid_cap():
    n = tbl.N_VEC8
    rng = np.random.default_rng(n)
    X = ref.bf(rng.standard_normal(n) * 3)
    Z = ref.bf(rng.standard_normal(n))
    dX, dZ = _d(X), _d(Z)
    Y = empty_u16(n)
    capi.call("gelu_bf16", Y, dX, C.c_int64(n))
    ref.assert_bf16(bits(Y), orc.cpu_gelu(X), 1e-6, "gelu_bf16")                       # the bar of test_gelu_residual_scale
    Y = empty_u16(n)
    capi.call("residual_bf16", Y, dX, dZ, C.c_int64(n))
    assert np.array_equal(bits(Y), orc.to_bf16_bits(X + Z))
    Y = empty_u16(n)
    sc = float(np.sqrt(np.float32(3840.0)))
    capi.call("scale_bf16", Y, dX, C.c_int64(n), sc)
    assert np.array_equal(bits(Y), orc.to_bf16_bits(X * np.float32(sc)))


def test_elementwise_fp32_kernels_beyond_the_grid_cap():
    n = tbl.N_ELEM
    rng = np.random.default_rng(n)
    X = (rng.standard_normal(n) * 3).astype(np.float32)
    Z = rng.standard_normal(n).astype(np.float32)
    Yf = empty_f32(n)
    capi.call("gelu_fp32", Yf, dev_f32(X), C.c_int64(n))
    ref.assert_close(host(Yf), orc.cpu_gelu(X), 1e-6, 1e-5, "gelu_fp32")
    Yf = empty_f32(n)
    capi.call("residual_fp32", Yf, dev_f32(X), dev_f32(Z), C.c_int64(n))
    assert np.array_equal(host(Yf), orc.cpu_residual(X, Z))
    Xw = X * 100
    y = empty_u16(n)
    capi.call("convert_f32_to_bf16", y, dev_f32(Xw), C.c_int64(n))
    assert np.array_equal(bits(y), orc.to_bf16_bits(Xw))
    z = empty_f32(n)
    capi.call("convert_bf16_to_f32", z, y, C.c_int64(n))
    assert np.array_equal(host(z), orc.round_bf16(Xw))


def test_geglu_and_split3_beyond_the_grid_cap():
    tokens, half = tbl.GEGLU_BEYOND
    rng = np.random.default_rng(half)
    X = ref.bf(rng.standard_normal((tokens, 2 * half)) * 2)
    dX = _d(X)
    Y = empty_u16(tokens, half)
    capi.call("geglu_bf16", Y, dX, tokens, half)
    ref.assert_bf16(bits(Y), orc.geglu(X), 1e-5, "geglu")                              # the bar of test_geglu
    rows, na, nb, nc = tbl.SPLIT3_BEYOND
    assert (rows, na + nb + nc) == X.shape
    a, b, c = empty_u16(rows, na), empty_u16(rows, nb), empty_u16(rows, nc)
    capi.call("split3_bf16", a, b, c, dX, rows, na, nb, nc)
    Xb = orc.to_bf16_bits(X)
    assert np.array_equal(bits(a), Xb[:, :na]) and np.array_equal(bits(b), Xb[:, na:na + nb]) and np.array_equal(bits(c), Xb[:, na + nb:])


@pytest.mark.parametrize("form,HS,T,NH", tbl.ROPE_BEYOND, ids=[r[0] for r in tbl.ROPE_BEYOND])
def test_rope_beyond_the_grid_cap(form, HS, T, NH):
    NKV, off = 1, 7
    max_seq = T + off
    cos, sin = empty_f32(max_seq, HS // 2), empty_f32(max_seq, HS // 2)
    capi.call("rope_build_cache", cos, sin, max_seq, HS, 1e4, 0)
    rng = np.random.default_rng(HS)
    Q = ref.rope_inputs(rng, host(cos), host(sin), T, NH, HS, off)
    K = ref.rope_inputs(rng, host(cos), host(sin), T, NKV, HS, off)
    Qo, Ko = empty_u16(1, T, NH, HS), empty_u16(1, T, NKV, HS)
    capi.call("rope_forward_bf16", Qo, Ko, _d(Q), _d(K), cos, sin, 1, T, NH, NKV, HS, off, max_seq)
    ref.assert_bf16(bits(Qo), orc.rope_rotate(Q, host(cos), host(sin), off), 1e-30, "rope q")      # the bar of test_rope_cache_and_rotation
    ref.assert_bf16(bits(Ko), orc.rope_rotate(K, host(cos), host(sin), off), 1e-30, "rope k")
