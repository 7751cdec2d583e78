"""GPU: every decode-step kernel whose signature leads with plain (preloaded) arguments, run once with EVERY parameter at a distinctive non-default value, at the smallest
shapes that reach every argument -- a launcher that hands a leading argument to the wrong slot, or a kernel that rebuilds its parameter block wrongly, fails here against
the oracles the other GPU tests use (orc.linear_* / orc.rmsnorm in float64, orc.gqa_attention, the unfused chain of entry points bit for bit).

fp4 runs at group 64: the entry points take 64 or 128 only (a group of 32 is refused as an invalid argument), and 128 is the default everywhere else."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gpu_util import assert_bf16_close, bits, dev_f32, dev_i32, dev_u16, dev_u8, empty_f32, empty_u16, host
from mila_amd import capi

pytestmark = pytest.mark.gpu

K, N = 512, 48


def _bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def _d(x):
    return dev_u16(orc.to_bf16_bits(x))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _slack(x, Wf):
    return float(2.0 ** -17 * (np.abs(x).astype(np.float64) @ np.abs(Wf).astype(np.float64).T).max())


def _weights(rng, rows, fmt, G=64):
    """(device weights, device scales, oracle Linear x -> y in float64, dequantized weights)"""
    Wb = orc.to_bf16_bits((rng.standard_normal((rows, K)) / np.sqrt(K)).astype(np.float32))
    if fmt == 0:
        return dev_u16(Wb), None, (lambda x, b=None: orc.linear_bf16w(x[None], Wb, b)[0]), orc.from_bf16_bits(Wb)
    if fmt == 1:
        q, s = orc.quantize_fp8_per_channel(Wb)
        return dev_u8(q), dev_f32(s), (lambda x, b=None: orc.linear_fp8w(x[None], q, s, b)[0]), orc.dequant_fp8(q, s)
    q, s = orc.quantize_fp4_per_group(Wb, G)
    return dev_u8(q), dev_f32(s), (lambda x, b=None: orc.linear_fp4w(x[None], q, s, G, b)[0]), orc.dequant_fp4(q, s, G)


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_plain_matvec_with_bias(fmt):
    rng = np.random.default_rng(fmt)
    W, s, lin, Wf = _weights(rng, N, fmt)
    x = _bf(rng.uniform(-1, 1, K))
    bb = orc.to_bf16_bits(rng.uniform(-0.5, 0.5, N).astype(np.float32))
    y = empty_u16(N)
    if fmt == 0:
        capi.call("matvec_bf16", y, _d(x), W, dev_u16(bb), K, N)
    elif fmt == 1:
        capi.call("matvec_bf16_qfp8", y, _d(x), W, s, dev_u16(bb), K, N)
    else:
        capi.call("matvec_bf16_qfp4", y, _d(x), W, s, dev_u16(bb), K, N, 64)
    assert_bf16_close(bits(y), lin(x, bb), 1, _slack(x, Wf), "matvec fmt %d" % fmt)


def _fused(**kw):
    a = capi.fused_matvec_args()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return a


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("geglu", [0, 1])
def test_sandwich_tail_matvec_reads_every_prologue_operand(fmt, geglu):
    """PRO 2 (x, post_w, res, res_out, post_scale, eps, norm_w all distinct) in front of the plain and the GeGLU epilogue, against the float64 oracle of the chain
    a = post_norm(x); r = bf16((res + a) * post_scale); h = pre_norm(r); y = W h"""
    rng = np.random.default_rng(10 + fmt + geglu)
    rows = 2 * N if geglu else N
    W, s, lin, Wf = _weights(rng, rows, fmt)
    x, res = _bf(rng.standard_normal(K) * 3), _bf(rng.standard_normal(K))
    pw, nw = _bf(1 + 0.3 * rng.uniform(-1, 1, K)), _bf(0.5 + 0.3 * rng.uniform(-1, 1, K))
    eps, post_scale = 1e-3, 0.75
    y, r_out = empty_u16(N), empty_u16(K)
    a = _fused(y=y, x=_d(x), W=W, scales=s if s is not None else 0, norm_w=_d(nw), post_w=_d(pw), res=_d(res), res_out=r_out, post_scale=post_scale, eps=eps,
               fmt=fmt, K=K, N=N, group=64, geglu=geglu)
    capi.check(capi.load().mila_cdna4_fused_norm_matvec(C.byref(a), _stream()))
    # the unfused chain of entry points, bit for bit (test_fused_gpu.py holds the same identity at the model's shapes) ...
    a_, r_, h_, gu, y0 = empty_u16(K), empty_u16(K), empty_u16(K), empty_u16(rows), empty_u16(N)
    capi.call("rmsnorm_bf16", a_, None, _d(x), _d(pw), None, 1, 1, K, eps, 0.0)
    capi.call("residual_bf16", r_, _d(res), a_, C.c_int64(K))
    capi.call("scale_bf16", r_, r_, C.c_int64(K), post_scale)
    capi.call("rmsnorm_bf16", h_, None, r_, _d(nw), None, 1, 1, K, eps, 0.0)
    if fmt == 0:
        capi.call("matvec_bf16", gu, h_, W, None, K, rows)
    elif fmt == 1:
        capi.call("matvec_bf16_qfp8", gu, h_, W, s, None, K, rows)
    else:
        capi.call("matvec_bf16_qfp4", gu, h_, W, s, None, K, rows, 64)
    if geglu:
        capi.call("geglu_bf16", y0, gu, 1, N)
    else:
        y0 = gu
    assert np.array_equal(bits(r_out), bits(r_)), "residual stream"
    assert np.array_equal(bits(y), bits(y0)), "output"
    # ... and its last step against the float64 oracle on the chain's own h
    if not geglu:
        h = orc.from_bf16_bits(bits(h_))
        assert_bf16_close(bits(y), lin(h), 1, _slack(h, Wf), "sandwich matvec fmt %d" % fmt)


@pytest.mark.parametrize("fmt", [0, 2])
def test_lm_head_form_writes_logits_and_the_samplers_partials(fmt):
    """f32_out with the argmax epilogue (amax_v / amax_i in the tail) behind the RMSNorm prologue: logits against the float64 oracle, the token the partials give
    against the argmax of those logits"""
    rng = np.random.default_rng(20 + fmt)
    lib = capi.load()
    W, s, lin, Wf = _weights(rng, N, fmt)
    x, nw = _bf(rng.standard_normal(K) * 2), _bf(1 + 0.3 * rng.uniform(-1, 1, K))
    eps = 1e-3
    logits = empty_f32(N)
    nb = lib.mila_cdna4_sample_scratch_bytes()
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    blocks = C.c_int(0)
    a = _fused(y=logits, x=_d(x), W=W, scales=s if s is not None else 0, norm_w=_d(nw), post_w=0, res=0, res_out=0, post_scale=1.0, eps=eps, fmt=fmt, K=K, N=N, group=64,
               geglu=0, f32_out=1)
    a.argmax_scratch = scratch.data_ptr(); a.argmax_scratch_bytes = nb; a.argmax_blocks = C.pointer(blocks)
    capi.check(lib.mila_cdna4_fused_norm_matvec(C.byref(a), _stream()))
    h = _bf(orc.rmsnorm(x[None], nw, None, eps=eps))[0]
    exp = np.asarray(lin(h), dtype=np.float64)
    lg = host(logits)
    assert np.all(np.abs(lg - exp) <= 1e-3 * np.abs(exp) + _slack(h, Wf)), float(np.abs(lg - exp).max())
    assert blocks.value == (N + 15) // 16      # one row per wave, 16 waves per workgroup
    tok, pos = dev_i32(np.array([-1])), dev_i32(np.array([9]))
    seq = torch.tensor([2], dtype=torch.int64, device="cuda")
    ring = torch.zeros(4, dtype=torch.int64, device="cuda")
    capi.call("sample_argmax_final_advance", tok, scratch, C.c_size_t(nb), blocks.value, pos, seq, ring, 4)
    assert int(host(tok)[0]) == int(np.argmax(lg)) and int(host(pos)[0]) == 10


# ---- attention: window 8 in a 16-row ring, position on the device, two batch rows ------------------------------------------------------------------------------
B, NH, NKV, WINDOW, CAP, POS, SCALE = 2, 4, 2, 8, 16, 37, 0.3


def _history(rng, HS):
    hk = _bf(rng.uniform(-1, 1, (B, POS + 1, NKV, HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (B, POS + 1, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, 1, NH, HS)))
    return hk, hv, q


def _scratch(HS):
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(B, NH, HS)
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), C.c_size_t(nbytes)


@pytest.mark.parametrize("HS", [64, 256])
def test_decode_attention_with_the_position_on_the_device(HS):
    rng = np.random.default_rng(HS)
    hk, hv, q = _history(rng, HS)
    Kc = torch.full((B, NKV, CAP, HS), 0x7fc0, dtype=torch.int16, device="cuda")
    Vc = Kc.clone()
    for s0 in range(0, POS + 1, 7):
        e0 = min(POS + 1, s0 + 7)
        capi.call("kv_write_bf16", Kc, Vc, _d(hk[:, s0:e0]), _d(hv[:, s0:e0]), B, e0 - s0, NKV, HS, s0, CAP)
    scratch, nbytes = _scratch(HS)
    Y = empty_u16(B, NH * HS)
    pd = dev_i32(np.array([POS]))
    capi.call("attn_decode_bf16_devpos", Y, _d(q), Kc, Vc, scratch, nbytes, B, NH, NKV, HS, CAP, pd, POS + 1, WINDOW, SCALE)
    exp = orc.gqa_attention(q, hk, hv, POS, WINDOW, SCALE)[:, 0]
    assert_bf16_close(bits(Y), exp, 1, 2e-3, "devpos decode HS %d" % HS)


@pytest.mark.parametrize("HS", [64, 256])
def test_fused_decode_attention_with_a_packed_batch_stride(HS):
    """the one-launch form (q_raw / k_raw / v_raw, norm weights, RoPE rows, eps in the tail; q_raw, K, V, pos_dev leading) on rows of a packed projection whose stride is
    not NH * HS: the per-row fused_qkv_post + the batched decode, bit for bit, and the float64 oracle through that chain's q"""
    rng = np.random.default_rng(HS + 1)
    hk, hv, _ = _history(rng, HS)
    max_seq, eps = 64, 1e-3
    packed = NH * HS + 2 * NKV * HS + 24
    rows = _bf(rng.standard_normal((B, packed)))
    rows_d = _d(rows)
    k_off, v_off = NH * HS, NH * HS + NKV * HS
    qw, kw, vw = (_d(_bf(1 + 0.3 * rng.uniform(-1, 1, HS))) for _ in range(3))
    cos, sin = empty_f32(max_seq, HS // 2), empty_f32(max_seq, HS // 2)
    capi.call("rope_build_cache", cos, sin, max_seq, HS, 1e4, 0)
    Kc0 = torch.full((B, NKV, CAP, HS), 0x7fc0, dtype=torch.int16, device="cuda")
    Vc0 = Kc0.clone()
    for s0 in range(0, POS, 7):
        e0 = min(POS, s0 + 7)
        capi.call("kv_write_bf16", Kc0, Vc0, _d(hk[:, s0:e0]), _d(hv[:, s0:e0]), B, e0 - s0, NKV, HS, s0, CAP)
    scratch, nbytes = _scratch(HS)
    K0, V0, q0, y0 = Kc0.clone(), Vc0.clone(), empty_u16(B, NH * HS), empty_u16(B, NH * HS)
    for b in range(B):
        capi.call("fused_qkv_post", q0[b], K0[b], V0[b], rows_d[b, 0:], rows_d[b, k_off:], rows_d[b, v_off:], qw, kw, vw, cos, sin, NH, NKV, HS, POS, CAP, eps)
    capi.call("attn_decode_bf16", y0, q0, K0, V0, scratch, nbytes, B, NH, NKV, HS, CAP, POS + 1, WINDOW, SCALE)
    K1, V1, y1 = Kc0.clone(), Vc0.clone(), empty_u16(B, NH * HS)
    pd = dev_i32(np.array([POS]))
    capi.call("fused_attn_decode_batch_bf16", y1, K1, V1, rows_d[0, 0:], rows_d[0, k_off:], rows_d[0, v_off:], C.c_int64(packed), qw, kw, vw, cos, sin,
              scratch, nbytes, B, NH, NKV, HS, CAP, 0, pd, WINDOW, SCALE, eps)
    assert np.array_equal(bits(K1), bits(K0)) and np.array_equal(bits(V1), bits(V0)), "cache rows differ"
    assert np.array_equal(bits(y1), bits(y0)), "attention output differs"
    kr, vr = orc.from_bf16_bits(bits(K0)), orc.from_bf16_bits(bits(V0))
    hk2, hv2 = hk.copy(), hv.copy()
    hk2[:, POS], hv2[:, POS] = kr[:, :, POS % CAP], vr[:, :, POS % CAP]
    exp = orc.gqa_attention(orc.from_bf16_bits(bits(q0)).reshape(B, 1, NH, HS), hk2, hv2, POS, WINDOW, SCALE)[:, 0]
    assert_bf16_close(bits(y1), exp, 1, 2e-3, "fused decode HS %d" % HS)


def test_decode_attention_with_more_than_one_split():
    """a band long enough for the plan to split it: the partials (scratch, splits in the leading block) and the combine launch"""
    HS, cap, length, window = 256, 1100, 1000, 0
    plan = capi.attn_decode_plan(B, NH, NKV, HS, cap, window, length)
    assert plan["splits"] > 1, plan
    rng = np.random.default_rng(3)
    hk = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (B, length, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, 1, NH, HS)))
    Kc = torch.full((B, NKV, cap, HS), 0x7fc0, dtype=torch.int16, device="cuda")
    Vc = Kc.clone()
    capi.call("kv_write_bf16", Kc, Vc, _d(hk), _d(hv), B, length, NKV, HS, 0, cap)
    scratch, nbytes = _scratch(HS)
    Y = empty_u16(B, NH * HS)
    pd = dev_i32(np.array([length - 1]))
    capi.call("attn_decode_bf16_devpos", Y, _d(q), Kc, Vc, scratch, nbytes, B, NH, NKV, HS, cap, pd, length, window, SCALE)
    assert_bf16_close(bits(Y), orc.gqa_attention(q, hk, hv, length - 1, window, SCALE)[:, 0], 1, 2e-3, "split decode")


@pytest.mark.parametrize("HS", [64, 256])
def test_fp8_cache_append_and_decode_with_the_position_on_the_device(HS):
    """kv_write_fp8 (chunks, host position) fills the ring up to POS - 1, its device-position form appends the token at *pos, the device-position decode reads the band:
    bytes and scales against orc.quantize_fp8_per_channel, the output against the oracle on the dequantized history"""
    rng = np.random.default_rng(HS + 2)
    hk, hv, q = _history(rng, HS)

    def quant(x):
        qb, sc = orc.quantize_fp8_per_channel(orc.to_bf16_bits(x).reshape(-1, HS))
        return qb.reshape(x.shape), sc.reshape(x.shape[:-1]), orc.round_bf16(orc.dequant_fp8(qb, sc)).reshape(x.shape)
    K8 = torch.full((B, NKV, CAP, HS), 0x7F, dtype=torch.uint8, device="cuda")
    V8 = K8.clone()
    Ks = torch.full((B, NKV, CAP), float("nan"), dtype=torch.float32, device="cuda")
    Vs = Ks.clone()
    for s0 in range(0, POS, 7):
        e0 = min(POS, s0 + 7)
        capi.call("kv_write_fp8", K8, V8, Ks, Vs, _d(hk[:, s0:e0]), _d(hv[:, s0:e0]), B, e0 - s0, NKV, HS, s0, CAP)
    pd = dev_i32(np.array([POS]))
    capi.call("kv_write_fp8_devpos", K8, V8, Ks, Vs, _d(hk[:, POS:POS + 1]), _d(hv[:, POS:POS + 1]), B, NKV, HS, pd, CAP)
    qk, sk, dk = quant(hk)
    qv, sv, dv = quant(hv)
    for t in range(POS + 1 - CAP, POS + 1):
        assert np.array_equal(host(K8)[:, :, t % CAP], qk[:, t]) and np.array_equal(host(V8)[:, :, t % CAP], qv[:, t]), t
        assert np.array_equal(host(Ks)[:, :, t % CAP], sk[:, t]) and np.array_equal(host(Vs)[:, :, t % CAP], sv[:, t]), t
    scratch, nbytes = _scratch(HS)
    Y = empty_u16(B, NH * HS)
    capi.call("attn_decode_kvfp8_devpos", Y, _d(q), K8, V8, Ks, Vs, scratch, nbytes, B, NH, NKV, HS, CAP, pd, POS + 1, WINDOW, SCALE)
    assert_bf16_close(bits(Y), orc.gqa_attention(q, dk, dv, POS, WINDOW, SCALE)[:, 0], 1, 2e-3, "fp8-cache devpos decode HS %d" % HS)
