"""GPU parity: Linear hot path (decode matvec x3 formats, quantize-on-load, prefill GEMM) against the
CPU oracle, through the C ABI.  Reference scenarios: Tests/Dnn/Components/Linear/Linear.Cuda.cpp.

Bars: integer outputs (fp8 bytes, fp4 nibbles, scales) bit-exact; bf16 outputs within 1 bf16 ulp of
the float64 oracle fed the identical bf16-rounded operands (or within an absolute slack of
2^-17 * sum|x||w| when heavy cancellation makes the result tiny); fp32 logits within 1e-3 relative
(north star).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import ref_matmul
from gpu_util import (assert_bf16_close, bits, dev_f32, dev_u16, dev_u8, empty_f32, empty_u16, empty_u8,
                      host, rel_err, sample_rows)
from mila_amd import capi

pytestmark = pytest.mark.gpu


def _weights(rng, N, K, kind):
    if kind == "closed_form":   # Linear.Cuda.cpp:70-75
        o = np.arange(N)[:, None]
        i = np.arange(K)[None, :]
        W = (np.float32(0.1) * (((o * 13 + i * 7) % 17).astype(np.float32) - 8.0) / 17.0).astype(np.float32)
    else:
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    return orc.to_bf16_bits(W)


def _slack(x, Wf):
    return float(2.0 ** -17 * (np.abs(x).astype(np.float64) @ np.abs(Wf).astype(np.float64).T).max())


def test_hardware_fp8_fp4_converts_match_the_reference_luts():
    """v_cvt_scalef32_pk_bf16_{fp8,fp4} with scale 1.0 == the reference decode tables, every byte,
    every byte position (OPS/Linear/Kernels/MatVec/CudaMatVecBias.Bf16.cu:20-25; Linear.Cuda.cpp:929)."""
    o8, o4 = empty_f32(4 * 256), empty_f32(4 * 512)
    capi.call("selftest_decode", o8, o4)
    o8, o4 = host(o8).reshape(4, 256), host(o4).reshape(4, 512)
    lut8 = orc.E4M3_LUT
    for pos in range(4):
        fin = ~np.isnan(lut8)
        assert np.array_equal(o8[pos][fin], lut8[fin]), "fp8 byte position %d" % pos
        assert np.all(np.isnan(o8[pos][~fin]))
        exp = np.empty(512, np.float32)
        exp[0::2] = orc.E2M1_LUT[np.arange(256) & 0xf]       # low nibble = even column
        exp[1::2] = orc.E2M1_LUT[np.arange(256) >> 4]
        assert np.array_equal(o4[pos], exp), "fp4 byte position %d" % pos


@pytest.mark.parametrize("K,N", [(3840, 256), (64, 32), (4096, 77), (15360, 48), (8, 1), (8192, 130)])
@pytest.mark.parametrize("kind", ["random", "closed_form"])
@pytest.mark.parametrize("bias", [False, True])
def test_matvec_bf16(K, N, kind, bias):
    rng = np.random.default_rng(K * 7 + N)
    Wb = _weights(rng, N, K, kind)
    x = orc.round_bf16(rng.uniform(-1, 1, K).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    y = empty_u16(N)
    capi.call("matvec_bf16", y, dev_u16(orc.to_bf16_bits(x)), dev_u16(Wb), dev_u16(bb) if bias else None, K, N)
    exp = orc.linear_bf16w(x[None], Wb, bb)[0]
    assert_bf16_close(bits(y), exp, 1, _slack(x, orc.from_bf16_bits(Wb)), "matvec_bf16")


@pytest.mark.parametrize("K,N", [(3840, 256), (64, 32), (4096, 77), (15360, 48), (16, 3)])
@pytest.mark.parametrize("bias", [False, True])
def test_matvec_fp8(K, N, bias):
    rng = np.random.default_rng(K * 3 + N)
    q, s = orc.quantize_fp8_per_channel(_weights(rng, N, K, "random"))
    x = orc.round_bf16(rng.uniform(-1, 1, K).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    y = empty_u16(N)
    capi.call("matvec_bf16_qfp8", y, dev_u16(orc.to_bf16_bits(x)), dev_u8(q), dev_f32(s), dev_u16(bb) if bias else None, K, N)
    exp = orc.linear_fp8w(x[None], q, s, bb)[0]
    assert_bf16_close(bits(y), exp, 1, _slack(x, orc.dequant_fp8(q, s)), "matvec_fp8")


@pytest.mark.parametrize("K,N,G", [(3840, 256, 128), (128, 32, 128), (4096, 77, 64), (15360, 48, 128), (64, 5, 64),
                                   (8192, 40, 128)])
@pytest.mark.parametrize("bias", [False, True])
def test_matvec_fp4(K, N, G, bias):
    rng = np.random.default_rng(K * 5 + N)
    q, s = orc.quantize_fp4_per_group(_weights(rng, N, K, "random"), G)
    x = orc.round_bf16(rng.uniform(-1, 1, K).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    y = empty_u16(N)
    capi.call("matvec_bf16_qfp4", y, dev_u16(orc.to_bf16_bits(x)), dev_u8(q), dev_f32(s), dev_u16(bb) if bias else None, K, N, G)
    exp = orc.linear_fp4w(x[None], q, s, G, bb)[0]
    assert_bf16_close(bits(y), exp, 1, _slack(x, orc.dequant_fp4(q, s, G)), "matvec_fp4")


@pytest.mark.parametrize("R,U", [(1, 1), (1, 4), (2, 1), (2, 2), (2, 4), (4, 1), (4, 2)])
def test_matvec_every_launch_shape_gives_the_same_answer(R, U):
    """rows-per-wave / unroll variants and a tiny grid (grid-stride path) are all parity-checked."""
    rng = np.random.default_rng(R * 10 + U)
    K, N, G = 3840, 203, 128
    Wb = _weights(rng, N, K, "random")
    q8, s8 = orc.quantize_fp8_per_channel(Wb)
    q4, s4 = orc.quantize_fp4_per_group(Wb, G)
    x = orc.round_bf16(rng.uniform(-1, 1, K).astype(np.float32))
    xd = dev_u16(orc.to_bf16_bits(x))
    lib = capi.load()
    try:
        capi.tune("matvec.rows_per_wave", R)
        capi.tune("matvec.chunks_in_flight", U)
        capi.tune("matvec.max_workgroups", 3)
        y = empty_u16(N)
        capi.call("matvec_bf16", y, xd, dev_u16(Wb), None, K, N)
        assert_bf16_close(bits(y), orc.linear_bf16w(x[None], Wb)[0], 1, 1e-5, "bf16 R%d U%d" % (R, U))
        capi.call("matvec_bf16_qfp8", y, xd, dev_u8(q8), dev_f32(s8), None, K, N)
        assert_bf16_close(bits(y), orc.linear_fp8w(x[None], q8, s8)[0], 1, 1e-5, "fp8 R%d U%d" % (R, U))
        capi.call("matvec_bf16_qfp4", y, xd, dev_u8(q4), dev_f32(s4), None, K, N, G)
        assert_bf16_close(bits(y), orc.linear_fp4w(x[None], q4, s4, G)[0], 1, 1e-5, "fp4 R%d U%d" % (R, U))
    finally:
        capi.tune_reset()


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_fp32_logits_within_1e3_relative(fmt):
    """North-star bar: lm_head logits in fp32 within 1e-3 relative of the reference arithmetic."""
    rng = np.random.default_rng(fmt)
    K, N, G = 3840, 4096, 128
    Wb = _weights(rng, N, K, "random")
    x = orc.round_bf16(rng.uniform(-1, 1, K).astype(np.float32))
    y = empty_f32(N)
    xd = dev_u16(orc.to_bf16_bits(x))
    if fmt == 0:
        capi.call("matvec_f32out", y, xd, dev_u16(Wb), None, 0, K, N, 0)
        exp = orc.linear_bf16w(x[None], Wb)[0]
    elif fmt == 1:
        q, s = orc.quantize_fp8_per_channel(Wb)
        capi.call("matvec_f32out", y, xd, dev_u8(q), dev_f32(s), 1, K, N, 0)
        exp = orc.linear_fp8w(x[None], q, s)[0]
    else:
        q, s = orc.quantize_fp4_per_group(Wb, G)
        capi.call("matvec_f32out", y, xd, dev_u8(q), dev_f32(s), 2, K, N, G)
        exp = orc.linear_fp4w(x[None], q, s, G)[0]
    assert rel_err(host(y), exp) < 1e-5        # measured margin; the stated bar is 1e-3
    assert rel_err(host(y), exp) < 1e-3


@pytest.mark.parametrize("K,N", [(3840, 262144), (15360, 3840), (3840, 30720)])
def test_matvec_full_size_exact_integer_property(K, N):
    """BASELINE.json sizes (lm_head, fc_down, fc_gate_up): small-integer operands make every
    partial sum exact in fp32, so the result must equal the exact integer dot product -- a
    size-independent, bit-exact check of the indexing over the whole weight matrix."""
    g = torch.Generator(device="cuda").manual_seed(K + N)
    Wi = torch.randint(-2, 3, (N, K), device="cuda", generator=g, dtype=torch.int32)
    xi = torch.randint(-1, 2, (K,), device="cuda", generator=g, dtype=torch.int32)
    exact = (Wi.to(torch.float32) @ xi.to(torch.float32))          # |sum| <= 2*15360 < 2^24: exact
    W = Wi.to(torch.bfloat16).view(torch.int16).contiguous()
    x = xi.to(torch.bfloat16).view(torch.int16).contiguous()
    y = empty_f32(N)
    capi.call("matvec_f32out", y, x, W, None, 0, K, N, 0)
    assert torch.equal(y, exact)
    # fp8: the same integers are exactly representable in E4M3; per-channel scale 0.5 is exact too
    W8 = Wi.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    s = torch.full((N,), 0.5, device="cuda")
    capi.call("matvec_f32out", y, x, W8, s, 1, K, N, 0)
    assert torch.equal(y, exact * 0.5)
    # fp4: nibbles for {-2,-1,0,1,2} are {0xC,0xA,0,2,4}; group scale 2.0
    lut = torch.tensor([0xC, 0xA, 0x0, 0x2, 0x4], device="cuda", dtype=torch.uint8)
    nib = lut[(Wi + 2).long()]
    W4 = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    s4 = torch.full((N, K // 128), 2.0, device="cuda")
    capi.call("matvec_f32out", y, x, W4, s4, 2, K, N, 128)
    assert torch.equal(y, exact * 2.0)


# ---- quantize-on-load: bit-exact ----------------------------------------------------------------------
def _quant_inputs(rng, N, K):
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    W[1] = 0.0                                   # all-zero channel -> scale 1
    W[2, : K // 2] *= 1e-3                       # tiny values -> fp8 subnormals
    W[3] *= 1e4                                  # large magnitudes
    W[4, 5] = -0.0
    W[5, :] = np.linspace(-1, 1, K)              # ties / breakpoints sweep
    return orc.to_bf16_bits(W)


@pytest.mark.parametrize("N,K", [(32, 64), (64, 3840), (16, 15360), (7, 4096)])
def test_quantize_fp8_per_channel_bit_exact(N, K):
    Wb = _quant_inputs(np.random.default_rng(N + K), N, K)
    q, s = empty_u8(N, K), empty_f32(N)
    capi.call("quantize_fp8_per_channel", q, s, dev_u16(Wb), N, K)
    eq, es = orc.quantize_fp8_per_channel(Wb)
    assert np.array_equal(host(s).view(np.uint32), es.view(np.uint32)), "scales differ"
    assert np.array_equal(host(q), eq), "fp8 bytes differ"


@pytest.mark.parametrize("N,K,G", [(32, 128, 128), (64, 3840, 128), (16, 15360, 128), (7, 4096, 64)])
def test_quantize_fp4_per_group_bit_exact(N, K, G):
    Wb = _quant_inputs(np.random.default_rng(N + K + G), N, K)
    q, s = empty_u8(N, K // 2), empty_f32(N, K // G)
    capi.call("quantize_fp4_per_group", q, s, dev_u16(Wb), N, K, G)
    eq, es = orc.quantize_fp4_per_group(Wb, G)
    assert np.array_equal(host(s).view(np.uint32), es.view(np.uint32)), "scales differ"
    assert np.array_equal(host(q), eq), "packed nibbles differ"


def test_quantize_every_bf16_value_fp8_and_fp4_codes():
    """Exhaustive over all finite bf16 inputs in one row per scale regime: the encoders agree
    with the oracle on every representable input (rounding ties, subnormals, saturation)."""
    allb = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    f = orc.from_bf16_bits(allb)
    keep = np.isfinite(f) & (np.abs(f) < 1e30)
    vals = allb[keep]
    K = 65536
    row = np.zeros(K, np.uint16)
    row[: vals.size] = vals
    rows = []
    for cap in (1e30, 448.0, 6.0, 1.0, 1e-3):
        r = row.copy()
        fr = orc.from_bf16_bits(r)
        r[np.abs(fr) > cap] = 0
        rows.append(r)
    Wb = np.stack(rows)
    N = Wb.shape[0]
    q, s = empty_u8(N, K), empty_f32(N)
    capi.call("quantize_fp8_per_channel", q, s, dev_u16(Wb), N, K)
    eq, es = orc.quantize_fp8_per_channel(Wb)
    assert np.array_equal(host(s).view(np.uint32), es.view(np.uint32))
    assert np.array_equal(host(q), eq)
    q4, s4 = empty_u8(N, K // 2), empty_f32(N, K // 128)
    capi.call("quantize_fp4_per_group", q4, s4, dev_u16(Wb), N, K, 128)
    eq4, es4 = orc.quantize_fp4_per_group(Wb, 128)
    assert np.array_equal(host(s4).view(np.uint32), es4.view(np.uint32))
    assert np.array_equal(host(q4), eq4)


def test_quantize_then_matvec_reference_reconstruction_bar():
    """Linear.Cuda.cpp:1046: stored FP8 weight * scale reconstructs w within 0.08|w| + 1e-3."""
    N, K = 32, 64
    Wb = _weights(np.random.default_rng(0), N, K, "closed_form")
    q, s = empty_u8(N, K), empty_f32(N)
    capi.call("quantize_fp8_per_channel", q, s, dev_u16(Wb), N, K)
    rec = orc.E4M3_LUT[host(q)] * host(s)[:, None]
    W = orc.from_bf16_bits(Wb)
    assert np.all(np.abs(rec - W) <= 0.08 * np.abs(W) + 1e-3)


# ---- prefill GEMM -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", [(128, 64, 128), (256, 768, 384), (77, 3840, 200), (2, 64, 32), (300, 1024, 130),
                                   (16, 4096, 256)])
@pytest.mark.parametrize("bias", [False, True])
def test_gemm_bf16(M, K, N, bias):
    rng = np.random.default_rng(M + K + N)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    Y = empty_u16(M, N)
    capi.call("gemm_bf16", Y, dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), dev_u16(bb) if bias else None, M, K, N)
    exp = orc.linear_bf16w(X, Wb, None)
    if bias:   # reference prefill order: round the GEMM to bf16, then add bias (cuda_add_bias)
        exp = orc.round_bf16(exp).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Y), exp, 1 if not bias else 2, _slack(X, orc.from_bf16_bits(Wb)), "gemm_bf16")


@pytest.mark.parametrize("M,K,N", [(128, 64, 128), (200, 3840, 136), (33, 256, 64)])
def test_gemm_fp8_and_fp4_weights_match_dequantize_then_gemm(M, K, N):
    """2-phase reference semantics (CudaLinearOp.ixx:597-644, :716-764): weights rounded to bf16
    after dequantization, then a bf16 GEMM with fp32 accumulation."""
    rng = np.random.default_rng(M * K + N)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    Xd = dev_u16(orc.to_bf16_bits(X))
    Y = empty_u16(M, N)
    q8, s8 = orc.quantize_fp8_per_channel(Wb)
    capi.call("gemm_bf16_w8a16", Y, Xd, dev_u8(q8), dev_f32(s8), None, M, K, N)
    W8 = orc.to_bf16_bits(orc.dequant_fp8(q8, s8))
    assert_bf16_close(bits(Y), orc.linear_bf16w(X, W8), 1, _slack(X, orc.from_bf16_bits(W8)), "gemm w8a16")
    G = 128 if K % 128 == 0 else 64
    q4, s4 = orc.quantize_fp4_per_group(Wb, G)
    capi.call("gemm_bf16_w4a16", Y, Xd, dev_u8(q4), dev_f32(s4), None, M, K, N, G)
    W4 = orc.to_bf16_bits(orc.dequant_fp4(q4, s4, G))
    assert_bf16_close(bits(Y), orc.linear_bf16w(X, W4), 1, _slack(X, orc.from_bf16_bits(W4)), "gemm w4a16")
    # reference's own cross-path bar: prefill vs decode within 1e-1 * row absmax (Linear.Cuda.cpp:760-774)
    y1 = empty_u16(N)
    capi.call("matvec_bf16_qfp4", y1, Xd[0].contiguous(), dev_u8(q4), dev_f32(s4), None, K, N, G)
    a = orc.from_bf16_bits(bits(Y)[0])
    b = orc.from_bf16_bits(bits(y1))
    assert np.abs(a - b).max() <= 1e-1 * np.abs(b).max()


def test_gemm_identity_times_asymmetric_matrix_catches_transposed_tiles():
    """A = I against an asymmetric B: any row/col swap in the MFMA output mapping shows up."""
    M = K = 256
    N = 192
    X = np.eye(M, K, dtype=np.float32)
    W = (np.arange(N)[:, None] * 3 + np.arange(K)[None, :] * 0.25).astype(np.float32) / 64.0
    Wb = orc.to_bf16_bits(W)
    Y = empty_u16(M, N)
    capi.call("gemm_bf16", Y, dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), None, M, K, N)
    assert np.array_equal(bits(Y), Wb.T)


def test_gemm_full_prefill_shape_linearity_property():
    """Config-3 shape (M=2048, K=3840, N=8192): GEMM(X) rows equal the decode matvec of each row
    (spot rows), and integer operands give the exact integer product everywhere."""
    M, K, N = 2048, 3840, 8192
    g = torch.Generator(device="cuda").manual_seed(1)
    Wi = torch.randint(-2, 3, (N, K), device="cuda", generator=g, dtype=torch.int32).to(torch.float32)
    Xi = torch.randint(-1, 2, (M, K), device="cuda", generator=g, dtype=torch.int32).to(torch.float32)
    exact = Xi @ Wi.T                                   # |.| <= 7680: exact in fp32, and every
    W = Wi.to(torch.bfloat16).view(torch.int16).contiguous()      # integer <= 256*... may round in bf16
    X = Xi.to(torch.bfloat16).view(torch.int16).contiguous()
    Y = empty_u16(M, N)
    capi.call("gemm_bf16", Y, X, W, None, M, K, N)
    torch.cuda.synchronize()
    assert torch.equal(Y.view(torch.bfloat16), exact.to(torch.bfloat16))


# ---- error behaviour (reference: std::invalid_argument from the op constructors / build) ---------------
def test_invalid_arguments_are_reported_not_launched():
    y = empty_u16(8)
    with pytest.raises(capi.InvalidArgument):
        capi.call("matvec_bf16", y, y, y, None, 12, 8)           # K % 8
    with pytest.raises(capi.InvalidArgument):
        capi.call("matvec_bf16_qfp4", y, y, y, y, None, 128, 8, 32)   # group size
    with pytest.raises(capi.InvalidArgument):
        capi.call("matvec_bf16", None, y, y, None, 8, 8)
    with pytest.raises(capi.InvalidArgument):
        capi.call("quantize_fp4_per_group", y, y, y, 2, 100, 128)


# the last three: more tiles than CUs -- the persistent form walks 2 / 1 and 4 / 3 tiles per workgroup (K-tile counts 2 and 4), and an odd K-tile count (3) that
# must take the one-workgroup-per-tile launch
@pytest.mark.parametrize("M,K,N,bias", [(2048, 128, 8192, False), (512, 3840, 30720, True), (256, 64, 51200, False), (2048, 192, 3840, True), (2048, 64, 3840, False), (512, 320, 14848, False),
                                        (2048, 128, 14336, True), (2048, 256, 30720, False), (2048, 192, 14336, False)])
def test_gemm_256_tile_kernel_agrees_with_the_128_tile_kernel(M, K, N, bias):
    """shapes with >= 200 tiles of 256 x 256 take the direct-to-LDS 8-wave kernel; same products, fp32
    accumulation in a different order -> equal to the register-staged kernel within 1 bf16 ulp, and to the
    float64 oracle on sampled rows"""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    X = (torch.rand((M, K), device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    W = ((torch.rand((N, K), device="cuda", generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
    b = ((torch.rand((N,), device="cuda", generator=g) - 0.5) * 0.2).to(torch.bfloat16) if bias else None
    Xi, Wi = X.view(torch.int16), W.view(torch.int16)
    bi = b.view(torch.int16) if bias else None
    lib = capi.load()
    Y256, Y128 = empty_u16(M, N), empty_u16(M, N)
    capi.call("gemm_bf16", Y256, Xi, Wi, bi, M, K, N)
    try:
        capi.tune("gemm.force128", 1)
        capi.call("gemm_bf16", Y128, Xi, Wi, bi, M, K, N)
    finally:
        capi.tune_reset()
    a = bits(Y256).astype(np.int32)
    c = bits(Y128).astype(np.int32)
    oa = np.where(a & 0x8000, -(a & 0x7fff), a)
    oc = np.where(c & 0x8000, -(c & 0x7fff), c)
    fa, fc = orc.from_bf16_bits(bits(Y256)), orc.from_bf16_bits(bits(Y128))
    ok = (np.abs(oa - oc) <= 1) | (np.abs(fa - fc) <= 2e-3)
    assert ok.all(), int((~ok).sum())
    rows = sample_rows(M, np.random.default_rng(M + N))       # every 256-row tile-row, every 32-row band of three of them
    Xh = orc.from_bf16_bits(X[rows].view(torch.int16).cpu().numpy().view(np.uint16))
    Wb = W.view(torch.int16).cpu().numpy().view(np.uint16)
    exp = ref_matmul.linear_bf16w(Xh, Wb, None)
    if bias:
        bb = b.view(torch.int16).cpu().numpy().view(np.uint16)
        exp = orc.round_bf16(exp.astype(np.float32)).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Y256)[rows], exp, 2 if bias else 1, 2e-3, "gemm256 vs oracle")


@pytest.mark.parametrize("M,K,N", [(2048, 128, 8192), (512, 256, 30720), (2048, 128, 3840)])
def test_staged_quantized_gemm_equals_register_dequantizing_gemm(M, K, N):
    """2-phase (dequantize to scratch + LDS-DMA GEMM) vs the fused 128-tile kernel: both multiply the same
    bf16-rounded weights; within 1 bf16 ulp of each other (summation order differs)"""
    rng = np.random.default_rng(N)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    Xd = dev_u16(orc.to_bf16_bits(X))
    need = capi.load().mila_cdna4_gemm_staging_bytes(M, K, N)
    assert need == N * K * 2
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    for fmt in (1, 2):
        if fmt == 1:
            q, s = orc.quantize_fp8_per_channel(Wb)
            Wdq = orc.to_bf16_bits(orc.dequant_fp8(q, s))
        else:
            q, s = orc.quantize_fp4_per_group(Wb, 128)
            Wdq = orc.to_bf16_bits(orc.dequant_fp4(q, s, 128))
        Ys, Yf = empty_u16(M, N), empty_u16(M, N)
        if fmt == 1:
            capi.call("gemm_bf16_w8a16_staged", Ys, Xd, dev_u8(q), dev_f32(s), None, M, K, N, scratch, C.c_size_t(need))
            capi.call("gemm_bf16_w8a16", Yf, Xd, dev_u8(q), dev_f32(s), None, M, K, N)
        else:
            capi.call("gemm_bf16_w4a16_staged", Ys, Xd, dev_u8(q), dev_f32(s), None, M, K, N, 128, scratch, C.c_size_t(need))
            capi.call("gemm_bf16_w4a16", Yf, Xd, dev_u8(q), dev_f32(s), None, M, K, N, 128)
        # the staged weights are exactly the oracle's dequantized, bf16-rounded weights
        assert np.array_equal(scratch.view(torch.int16).cpu().numpy().view(np.uint16).reshape(N, K), Wdq)
        fa, fb = orc.from_bf16_bits(bits(Ys)), orc.from_bf16_bits(bits(Yf))
        assert np.abs(fa - fb).max() <= 2 ** -7 * max(1.0, np.abs(fb).max())
        rows = [0, 200, M - 1]
        assert_bf16_close(bits(Ys)[rows], orc.linear_bf16w(X[rows], Wdq), 1, 2e-3, "staged gemm vs oracle")
    with pytest.raises(capi.MilaError):
        capi.call("gemm_bf16_w8a16_staged", Ys, Xd, dev_u8(q), dev_f32(s[:, 0].copy() if s.ndim > 1 else s), None, M, K, N, scratch, C.c_size_t(16))


@pytest.mark.parametrize("M,K,F", [(512, 256, 15360), (2048, 128, 3584), (2048, 128, 15360)])      # the last: 960 tiles, persistent, 4 / 3 tiles per workgroup
def test_gemm_with_geglu_epilogue_is_bit_identical_to_gemm_then_geglu(M, K, F):
    """prefill fc_gate_up + GeGLU in one kernel (Gemma.Block.ixx:343-348): a tile pairs 128 gate rows with the matching
    128 up rows, so the [M, 2F] intermediate never reaches memory; the K loop of every output is unchanged -> same bits as
    gemm_bf16 (256-tile kernel) followed by geglu_bf16, for bf16 weights and for the two staged quantized formats"""
    lib = capi.load()
    assert lib.mila_cdna4_gemm_geglu_applicable(M, K, F) == 1
    assert lib.mila_cdna4_gemm_geglu_applicable(M, K, F + 64) == 0 and lib.mila_cdna4_gemm_geglu_applicable(100, K, F) == 0
    rng = np.random.default_rng(F)
    Wb = _weights(rng, 2 * F, K, "random")
    X = orc.round_bf16(rng.uniform(-2, 2, (M, K)).astype(np.float32))
    Xd = dev_u16(orc.to_bf16_bits(X))
    need = 2 * F * K * 2
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    for fmt in (0, 1, 2):
        GU, Y0, Y1 = empty_u16(M, 2 * F), empty_u16(M, F), empty_u16(M, F)
        if fmt == 0:
            Wd = dev_u16(Wb)
            capi.call("gemm_bf16", GU, Xd, Wd, None, M, K, 2 * F)
            capi.call("gemm_geglu_bf16", Y1, Xd, Wd, M, K, F)
            Wdq = Wb
        elif fmt == 1:
            q, s = orc.quantize_fp8_per_channel(Wb)
            capi.call("gemm_bf16_w8a16_staged", GU, Xd, dev_u8(q), dev_f32(s), None, M, K, 2 * F, scratch, C.c_size_t(need))
            capi.call("gemm_geglu_bf16_w8a16_staged", Y1, Xd, dev_u8(q), dev_f32(s), M, K, F, scratch, C.c_size_t(need))
            Wdq = orc.to_bf16_bits(orc.dequant_fp8(q, s))
        else:
            q, s = orc.quantize_fp4_per_group(Wb, 128)
            capi.call("gemm_bf16_w4a16_staged", GU, Xd, dev_u8(q), dev_f32(s), None, M, K, 2 * F, 128, scratch, C.c_size_t(need))
            capi.call("gemm_geglu_bf16_w4a16_staged", Y1, Xd, dev_u8(q), dev_f32(s), M, K, F, 128, scratch, C.c_size_t(need))
            Wdq = orc.to_bf16_bits(orc.dequant_fp4(q, s, 128))
        capi.call("geglu_bf16", Y0, GU, M, F)
        assert np.array_equal(bits(Y0), bits(Y1)), "fmt %d: fused GeGLU epilogue differs from gemm + geglu" % fmt
        rows = [0, 129, M - 1]
        gu = orc.round_bf16(orc.linear_bf16w(X[rows], Wdq).astype(np.float32)).astype(np.float64)
        g_, u_ = gu[:, :F], gu[:, F:]
        exp = 0.5 * g_ * (1 + np.tanh(0.7978845608028654 * (g_ + 0.044715 * g_ ** 3))) * u_
        assert_bf16_close(bits(Y1)[rows], exp, 2, 2e-3, "gemm+geglu vs oracle fmt %d" % fmt)
    with pytest.raises(capi.InvalidArgument):
        capi.call("gemm_geglu_bf16", Y1, Xd, dev_u16(Wb), M, K, F + 64)


def test_scaled_fp8_mfma_operand_layout():
    """v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands and unit block scales computes C = A B^T exactly for small integers,
    with the lane layout the fp8 GEMM assumes (row = lane & 15, 32 bytes of k per lane)"""
    lib = capi.load()
    rng = np.random.default_rng(3)
    vals = np.array([-3, -2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 2, 3, 4], dtype=np.float32)
    A, B = rng.choice(vals, (16, 128)), rng.choice(vals, (16, 128))
    q = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).cuda()
    Ad, Bd, Cd = q(A), q(B), torch.zeros(256, dtype=torch.float32, device="cuda")
    capi.check(lib.mila_cdna4_selftest_mfma_fp8(C.c_void_p(Cd.data_ptr()), C.c_void_p(Ad.data_ptr()), C.c_void_p(Bd.data_ptr()), 0,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(Cd.cpu().numpy().reshape(16, 16), (A.astype(np.float64) @ B.astype(np.float64).T).astype(np.float32))


@pytest.mark.parametrize("M,K,N,bias", [(2048, 256, 8192, False), (512, 384, 30720, True), (2048, 128, 3840, True), (2048, 1280, 3840, False), (2048, 256, 30720, True)])      # the last: fp8 tiles walked persistently
def test_w4a8_prefill_matches_the_restated_reference(M, K, N, bias):
    """the fp4 policy's default prefill (CudaLinearOp.ixx:646-715): weight scale, fp4 -> e4m3 staging and per-token activation
    quantization are integer outputs -> bit-exact; the fp8 x fp8 MFMA GEMM with the two-step scaling epilogue -> within 2 bf16 ulp
    of the restated reference (fp32 accumulation order is the only freedom), for the 256x256 and the 256x128 kernels"""
    lib = capi.load()
    assert lib.mila_cdna4_gemm_fp8_applicable(M, K, N) == 1 and lib.mila_cdna4_gemm_fp8_applicable(M, K + 8, N) == 0
    rng = np.random.default_rng(N + K)
    Wb = _weights(rng, N, K, "random")
    q4, s4 = orc.quantize_fp4_per_group(Wb, 128)
    X = orc.round_bf16((rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32))
    X[7] = 0.0                                                              # an all-zero token: the 1e-12 guard
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    # 1. per-tensor weight scale
    ws_d = empty_f32(1)
    capi.call("fp4_weight_fp8_scale", ws_d, dev_f32(s4), C.c_int64(s4.size))
    ws = orc.fp8_weight_scale_from_groups(s4)
    assert np.float32(host(ws_d)[0]) == np.float32(ws)
    # 2. weight staging
    W8 = torch.empty((N, K), dtype=torch.uint8, device="cuda")
    capi.call("upcast_fp4_to_fp8", W8, dev_u8(q4), dev_f32(s4), ws_d, N, K, 128)
    w8_exp = orc.upcast_fp4_to_fp8(q4, s4, ws, 128)
    assert np.array_equal(W8.cpu().numpy(), w8_exp)
    # 3. activation quantization
    X8, ts_d = torch.empty((M, K), dtype=torch.uint8, device="cuda"), empty_f32(M)
    capi.call("quantize_fp8_per_token", X8, ts_d, dev_u16(orc.to_bf16_bits(X)), M, K)
    x8_exp, ts_exp = orc.quantize_act_fp8_per_token(X)
    assert np.array_equal(host(ts_d), ts_exp) and np.array_equal(X8.cpu().numpy(), x8_exp)
    # 4. GEMM + epilogue, stand-alone and through the one-call form
    rows = sorted(set(sample_rows(M, rng)) | {7})       # every 256-row tile-row, every 32-row band of three of them, the zero token
    raw = ref_matmul.linear_fp8a_fp8w(x8_exp[rows], np.ones(len(rows), dtype=np.float32), w8_exp, None, ws, None)       # sB * acc
    exp = orc.round_bf16(raw.astype(np.float32)).astype(np.float64) * ts_exp[rows].astype(np.float64)[:, None]
    if bias:
        exp = exp + orc.from_bf16_bits(bb).astype(np.float64)
    Y = empty_u16(M, N)
    capi.call("gemm_fp8_scaled", Y, X8, W8, ts_d, ws_d, dev_u16(bb) if bias else None, M, K, N)
    # two roundings in the reference (GEMM output, then the rescaled + biased result): an fp32 accumulation-order difference that
    # flips the first one moves the final value by up to 2 ulp; outputs that are the difference of large partial sums get 1e-3 of
    # the output range
    assert_bf16_close(bits(Y)[rows], exp, 2, 1e-3 * float(np.abs(exp).max()), "fp8 GEMM vs restated reference")
    need = lib.mila_cdna4_gemm_w4a8_scratch_bytes(M, K, N)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    Y2 = empty_u16(M, N)
    capi.call("gemm_bf16_w4a8", Y2, dev_u16(orc.to_bf16_bits(X)), dev_u8(q4), dev_f32(s4), ws_d, dev_u16(bb) if bias else None, M, K, N, 128,
              scratch, C.c_size_t(need))
    assert np.array_equal(bits(Y2), bits(Y))
    # the W4A8 result stays close to the exact-weight (W4A16) Linear: the reference's own bar for this path is 1e-1 relative
    ref16 = orc.linear_fp4w(X[rows], q4, s4, 128)
    if bias:
        ref16 = ref16 + orc.from_bf16_bits(bb).astype(np.float64)
    got = orc.from_bf16_bits(bits(Y)[rows]).astype(np.float64)
    assert np.abs(got - ref16).max() <= 1e-1 * max(1.0, np.abs(ref16).max())
    with pytest.raises(capi.MilaError):
        capi.call("gemm_bf16_w4a8", Y2, dev_u16(orc.to_bf16_bits(X)), dev_u8(q4), dev_f32(s4), ws_d, None, M, K, N, 128, scratch, C.c_size_t(64))


# (the longer K: five and more fp8 K-tiles run the interior K-tile bodies of the fp8 GeGLU mode, round 4; 2048 x 1024 walks 4 / 3 tiles per workgroup)
@pytest.mark.parametrize("M,K,F", [(512, 256, 15360), (512, 1024, 15360), (2048, 1024, 15360), (512, 1152, 15360)])
def test_w4a8_gemm_with_geglu_epilogue_is_bit_identical_to_w4a8_gemm_then_geglu(M, K, F):
    lib = capi.load()
    assert lib.mila_cdna4_gemm_geglu_w4a8_applicable(M, K, F) == 1
    rng = np.random.default_rng(5)
    Wb = _weights(rng, 2 * F, K, "random")
    q4, s4 = orc.quantize_fp4_per_group(Wb, 128)
    X = dev_u16(orc.to_bf16_bits(orc.round_bf16(rng.uniform(-2, 2, (M, K)).astype(np.float32))))
    ws = empty_f32(1)
    capi.call("fp4_weight_fp8_scale", ws, dev_f32(s4), C.c_int64(s4.size))
    need = lib.mila_cdna4_gemm_w4a8_scratch_bytes(M, K, 2 * F)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    GU, Y0, Y1 = empty_u16(M, 2 * F), empty_u16(M, F), empty_u16(M, F)
    capi.call("gemm_bf16_w4a8", GU, X, dev_u8(q4), dev_f32(s4), ws, None, M, K, 2 * F, 128, scratch, C.c_size_t(need))
    capi.call("geglu_bf16", Y0, GU, M, F)
    capi.call("gemm_geglu_bf16_w4a8", Y1, X, dev_u8(q4), dev_f32(s4), ws, M, K, F, 128, scratch, C.c_size_t(need))
    assert np.array_equal(bits(Y0), bits(Y1))


def _w4a8_operands(rng, M, K, N, G=128):
    Wb = _weights(rng, N, K, "random")
    q4, s4 = orc.quantize_fp4_per_group(Wb, G)
    X = orc.round_bf16((rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32))
    ws = orc.fp8_weight_scale_from_groups(s4)
    w8 = orc.upcast_fp4_to_fp8(q4, s4, ws, G)
    x8, ts = orc.quantize_act_fp8_per_token(X)
    return X, q4, s4, ws, w8, x8, ts


@pytest.mark.parametrize("M,K,N,bias,G", [(2, 3840, 8704, False, 128), (16, 512, 256, True, 128), (33, 192, 250, True, 64), (300, 384, 3840, True, 128), (300, 256, 8192, True, 128), (260, 128, 15360, False, 128),
                                          (2000, 256, 8192, False, 128), (2049, 256, 8192, True, 128), (2048 + 77, 128, 3840, False, 128),
                                          (1024 + 255, 256, 30720, True, 128)])
def test_w4a8_serves_every_row_count_like_the_reference(M, K, N, bias, G):
    """CudaLinearOp.ixx:646-715 runs W4A8 for EVERY M > 1; here the LDS-DMA fp8 kernels take the leading multiple of 256 rows and the masked 128-row
    kernel (csrc/gemm_fp8_tail.hip) the rest, or all of them: gemm_fp8_applicable is true at M in {2, 16, 2000, 2049, ...}, sampled rows of both parts are
    within 2 ulp of the restated reference; a ragged last tile-row runs masked inside the LDS-DMA kernels, tails of <= 64 rows on the skinny weight-streaming kernel"""
    lib = capi.load()
    assert lib.mila_cdna4_gemm_fp8_applicable(M, K, N) == 1
    rng = np.random.default_rng(M * 7 + N)
    X, q4, s4, ws, w8, x8, ts = _w4a8_operands(rng, M, K, N, G)
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    ws_d = dev_f32(np.array([ws], dtype=np.float32))
    X8, W8, ts_d = dev_u8(x8), dev_u8(w8), dev_f32(ts)
    Y = empty_u16(M, N)
    capi.call("gemm_fp8_scaled", Y, X8, W8, ts_d, ws_d, dev_u16(bb) if bias else None, M, K, N)
    main = M - M % 256
    rows = sorted({0, 1, M // 2, M - 1, max(0, main - 1), min(M - 1, main), min(M - 1, main + 127), min(M - 1, main + 128)})
    raw = orc.linear_fp8a_fp8w(x8[rows], np.ones(len(rows), dtype=np.float32), w8, None, ws, None)
    exp = orc.round_bf16(raw.astype(np.float32)).astype(np.float64) * ts[rows].astype(np.float64)[:, None]
    if bias:
        exp = exp + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Y)[rows], exp, 2, 1e-3 * float(np.abs(exp).max()), "fp8 GEMM (ragged M) vs restated reference")
    # the one-call form (stages W8 / X8 itself) gives the same bits
    need = lib.mila_cdna4_gemm_w4a8_scratch_bytes(M, K, N)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    Y2 = empty_u16(M, N)
    capi.call("gemm_bf16_w4a8", Y2, dev_u16(orc.to_bf16_bits(X)), dev_u8(q4), dev_f32(s4), ws_d, dev_u16(bb) if bias else None, M, K, N, G,
              scratch, C.c_size_t(need))
    assert np.array_equal(bits(Y2), bits(Y))
    # the tail kernels over EVERY row (tuning hook): form 1 = masked 128-row LDS tiles -- the LDS-DMA kernels' instruction chain, bit for bit; form 2 = skinny
    # weight-streaming pieces -- the same products summed as eight interleaved K chains, so fp32-rounding-level differences only
    forms = {}
    for form in (1, 2):
        Yf = empty_u16(M, N)
        capi.tune("gemm_fp8.tail_form", form)
        try:
            capi.call("gemm_fp8_scaled", Yf, X8, W8, ts_d, ws_d, dev_u16(bb) if bias else None, M, K, N)
        finally:
            capi.tune_reset()
        forms[form] = bits(Yf)
        assert_bf16_close(forms[form][rows], exp, 2, 1e-3 * float(np.abs(exp).max()), "fp8 GEMM, tail form %d, vs restated reference" % form)
    # who serves which rows by default (csrc/gemm_plan.hip: plan_fp8): with M >= 512 (and K % 128 == N % 128 == 0) the LDS-DMA kernels take every tile-row,
    # a ragged last one masked -- unless the tail is <= 64 rows, which goes to the skinny kernel; below 512 rows: skinny up to 16 (64 without a tile grid), masked LDS tiles beyond
    # -- and below 512 rows wherever their grid still has >= 120 tiles (no skinny split there: the remainder stays in the ragged tile-row)
    tail = M % 256
    tiles = ((M + 255) // 256) * (N // 128)
    if K % 128 or N % 128 or not (M >= 512 or (M > 16 and tiles >= 120)):
        big = 0
    elif M < 512:
        big = M
    else:
        big = M - tail if 0 < tail <= 64 else M
    assert np.array_equal(forms[1][:big], bits(Y)[:big]), "the masked LDS-tile kernel and the LDS-DMA fp8 kernels differ"
    if M - big > 64:
        assert np.array_equal(forms[1][big:], bits(Y)[big:])
    else:
        assert np.array_equal(forms[2][big:], bits(Y)[big:])
    a, b = orc.from_bf16_bits(forms[1]).astype(np.float64), orc.from_bf16_bits(forms[2]).astype(np.float64)
    assert np.abs(a - b).max() <= 2.0 ** -6 * np.abs(a).max(), "the two tail forms differ by more than rounding"


@pytest.mark.parametrize("M,K,F", [(2, 256, 15360), (100, 384, 1000), (512 + 100, 256, 15360), (2049, 128, 15360)])
def test_w4a8_geglu_form_serves_every_row_count(M, K, F):
    """the fused Linear + GeGLU W4A8 form at ragged M: bit-identical to gemm_bf16_w4a8 + geglu_bf16 (Gemma.Block.ixx:343-348), and to itself with every row on
    the masked kernel"""
    lib = capi.load()
    assert lib.mila_cdna4_gemm_geglu_w4a8_applicable(M, K, F) == 1
    rng = np.random.default_rng(M + F)
    Wb = _weights(rng, 2 * F, K, "random")
    q4, s4 = orc.quantize_fp4_per_group(Wb, 128)
    X = dev_u16(orc.to_bf16_bits(orc.round_bf16(rng.uniform(-2, 2, (M, K)).astype(np.float32))))
    ws = empty_f32(1)
    capi.call("fp4_weight_fp8_scale", ws, dev_f32(s4), C.c_int64(s4.size))
    need = lib.mila_cdna4_gemm_w4a8_scratch_bytes(M, K, 2 * F)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    GU, Y0, Y1, Y2 = empty_u16(M, 2 * F), empty_u16(M, F), empty_u16(M, F), empty_u16(M, F)
    capi.call("gemm_bf16_w4a8", GU, X, dev_u8(q4), dev_f32(s4), ws, None, M, K, 2 * F, 128, scratch, C.c_size_t(need))
    capi.call("geglu_bf16", Y0, GU, M, F)
    capi.call("gemm_geglu_bf16_w4a8", Y1, X, dev_u8(q4), dev_f32(s4), ws, M, K, F, 128, scratch, C.c_size_t(need))
    assert np.array_equal(bits(Y0), bits(Y1))
    for form in (1, 2):
        capi.tune("gemm_fp8.tail_form", form)
        try:
            capi.call("gemm_geglu_bf16_w4a8", Y2, X, dev_u8(q4), dev_f32(s4), ws, M, K, F, 128, scratch, C.c_size_t(need))
            capi.call("gemm_bf16_w4a8", GU, X, dev_u8(q4), dev_f32(s4), ws, None, M, K, 2 * F, 128, scratch, C.c_size_t(need))
            capi.call("geglu_bf16", Y0, GU, M, F)
        finally:
            capi.tune_reset()
        assert np.array_equal(bits(Y2), bits(Y0)), "tail form %d: fused GeGLU epilogue != Linear + GeGLU" % form      # per form, the fusion changes no bit
        a, b = orc.from_bf16_bits(bits(Y2)).astype(np.float64), orc.from_bf16_bits(bits(Y1)).astype(np.float64)
        assert np.abs(a - b).max() <= 2.0 ** -5 * max(np.abs(b).max(), 1e-30), "tail form %d differs from the default by more than rounding" % form


@pytest.mark.parametrize("M", [2048 + 77, 1024 + 255, 768 + 1, 512 + 3])
def test_ragged_prompt_lengths_split_between_the_lds_dma_and_the_128_tile_kernels(M):
    """M % 256 != 0 (round 3): the LDS-DMA kernels take the whole M -- a ragged last tile-row stages row M - 1 for the rows past M and masks its stores -- where their
    grid covers the chip, else the 128-tile kernel; rows around every tile-row edge against the float64 oracle, bf16 and (staged) fp4 weights, with bias, and the
    whole output against the 128-tile kernel within 1 bf16 ulp of the larger magnitude (another MFMA shape, same math); a guard row behind Y stays untouched"""
    K, N = 192, 8192
    rng = np.random.default_rng(M)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32))
    Xd = dev_u16(orc.to_bf16_bits(X))
    lib = capi.load()
    Yg = torch.full((M + 1, N), 0x1234, dtype=torch.int16, device="cuda")          # one guard row behind the output: a masked store must not reach it
    Y = Yg[:M]
    capi.call("gemm_bf16", Y, Xd, dev_u16(Wb), dev_u16(bb), M, K, N)
    rows = [0, 255, 256, M - M % 256 - 1, M - M % 256, M - 1]
    exp = orc.round_bf16(orc.linear_bf16w(X[rows], Wb, None)).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Y)[rows], exp, 2, 2e-3, "ragged gemm_bf16")
    assert np.all(Yg[M].cpu().numpy() == 0x1234), "a store past row M - 1"
    Y2 = empty_u16(M, N)
    capi.tune("gemm.force128", 1)
    try:
        capi.call("gemm_bf16", Y2, Xd, dev_u16(Wb), dev_u16(bb), M, K, N)
    finally:
        capi.tune_reset()
    a, b = orc.from_bf16_bits(bits(Y)).astype(np.float64), orc.from_bf16_bits(bits(Y2)).astype(np.float64)
    assert np.abs(a - b).max() <= 2.0 ** -7 * max(np.abs(b).max(), 1e-30)
    need = lib.mila_cdna4_gemm_staging_bytes(M, K, N)
    assert need == N * K * 2                                               # ceil(M / 256) x 64 tiles of 256 x 128: an LDS-DMA grid from 3 tile-rows on (192 tiles)
    q4, s4 = orc.quantize_fp4_per_group(Wb, 64)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    capi.call("gemm_bf16_w4a16_staged", Y, Xd, dev_u8(q4), dev_f32(s4), None, M, K, N, 64, scratch, C.c_size_t(need))
    Wdq = orc.to_bf16_bits(orc.dequant_fp4(q4, s4, 64))                   # the staged path multiplies the bf16-rounded dequantized weights
    assert_bf16_close(bits(Y)[rows], orc.linear_bf16w(X[rows], Wdq), 1, 2e-3, "ragged staged fp4 gemm")


@pytest.mark.parametrize("M,K,N,bias", [(768, 192, 50257, True), (768, 192, 50257 - 128 + 3, False),      # 256 x 128 tiles (K-tile count odd)
                                        (1536, 256, 50257, True), (1280, 128, 50257 - 256 + 8, False), (1280, 128, 50264, True)])     # 256 x 256 tiles with the row-wise epilogue through LDS (round 3: GPT-2's lm_head)
def test_lds_dma_gemm_serves_a_ragged_n_with_an_odd_row_pitch(M, K, N, bias):
    """GPT-2's lm_head (GptTransformer.ixx:854-855: Linear(768 -> 50257), no bias there; bias exercised here too): N is no multiple of the 128-column tile and the output
    row pitch no multiple of 16 bytes -- the 256 x 128 LDS-DMA kernel takes it with a clamped last W tile and element stores under a column mask (round 3; it
    used to fall to the 128-tile register-staged kernel at 1.6 ms of config 2's 6.8).  Rows / columns around every edge against the float64 oracle, and the
    whole output against the 128-tile kernel within 1 bf16 ulp (another MFMA shape, same math)"""
    lib = capi.load()
    rng = np.random.default_rng(N)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    Xd, Wd = dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb)
    Y = torch.full((M, N), 0x7fc0, dtype=torch.int16, device="cuda")          # NaN-poisoned: every element must be written
    guard = torch.full((64,), 0x1234, dtype=torch.int16, device="cuda")
    capi.call("gemm_bf16", Y, Xd, Wd, dev_u16(bb) if bias else None, M, K, N)
    got = bits(Y)
    assert not np.any((got & 0x7fff) > 0x7f80), "unwritten (NaN) outputs"
    rows = [0, 1, 255, 256, 511, M - 1]
    exp = orc.linear_bf16w(X[rows], Wb, None)
    if bias:
        exp = orc.round_bf16(exp).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(got[rows], exp, 2 if bias else 1, 2e-3, "ragged-N gemm_bf16")
    if K % 128 == 0:      # the 256 x 256 and the 256 x 128 LDS-DMA kernels accumulate every output in the same order: same bits
        Y3 = torch.empty((M, N), dtype=torch.int16, device="cuda")
        capi.tune("gemm.schedule", 2)
        try:
            capi.call("gemm_bf16", Y3, Xd, Wd, dev_u16(bb) if bias else None, M, K, N)
        finally:
            capi.tune_reset()
        assert np.array_equal(got, bits(Y3)), "256 x 256 ragged-N tiles differ from the 256 x 128 ones"
    Y2 = torch.empty((M, N), dtype=torch.int16, device="cuda")
    capi.tune("gemm.force128", 1)
    try:
        capi.call("gemm_bf16", Y2, Xd, Wd, dev_u16(bb) if bias else None, M, K, N)
    finally:
        capi.tune_reset()
    a, b = orc.from_bf16_bits(got).astype(np.float64), orc.from_bf16_bits(bits(Y2)).astype(np.float64)
    assert np.abs(a - b).max() <= 2.0 ** -7 * max(np.abs(b).max(), 1e-30)
    assert np.all(guard.cpu().numpy() == 0x1234)


@pytest.mark.parametrize("M,K,N,bias", [(2048, 256, 3072, True),      # 256 x 256 LDS-DMA tiles (GPT-2 fc_1's N)
                                        (1024, 128, 3200, True),      # 256 x 128 tiles (N % 256 != 0)
                                        (768, 192, 50257 - 128 + 3, True),      # 256 x 128 tiles with the ragged-N element epilogue
                                        (1536, 128, 50257, True),               # persistent 256 x 256 tiles with a ragged last tile-column
                                        (300, 136, 520, True), (300, 136, 520, False),      # main rows on LDS-DMA tiles + a 44-row rest on the 128-tile register kernel
                                        (7, 64, 96, True)])           # 128-tile register kernel only
def test_gemm_with_gelu_epilogue_is_bit_identical_to_gemm_then_gelu(M, K, N, bias):
    """the GPT-2 MLP's fc_1 -> gelu (Components/FFN/MLP/MLP.ixx:148-161) in one kernel: every epilogue rounds the Linear output to bf16 exactly as gemm_bf16 stores it
    and applies gelu_bf16's arithmetic to that value, so the result has the bits of the two launches while the [M, N] intermediate never reaches HBM"""
    rng = np.random.default_rng(M * 7 + N)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-2, 2, (M, K)).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.5, 0.5, N).astype(np.float32)) if bias else None
    Xd, Wd, bd = dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), dev_u16(bb) if bias else None
    H, Y0 = empty_u16(M, N), empty_u16(M, N)
    Y1 = torch.full((M, N), 0x7fc0, dtype=torch.int16, device="cuda")
    capi.call("gemm_bf16", H, Xd, Wd, bd, M, K, N)
    capi.call("gelu_bf16", Y0, H, M * N)
    capi.call("gemm_gelu_bf16", Y1, Xd, Wd, bd, M, K, N)
    assert np.array_equal(bits(Y0), bits(Y1)), "fused GELU epilogue differs from gemm + gelu"
    rows = [0, M // 2, M - 1]
    h = orc.linear_bf16w(X[rows], Wb, None)
    if bias:
        h = orc.round_bf16(h).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    h = orc.round_bf16(np.asarray(h, np.float32)).astype(np.float64)
    exp = 0.5 * h * (1 + np.tanh(0.7978845608028654 * (h + 0.044715 * h ** 3)))
    assert_bf16_close(bits(Y1)[rows], exp, 2, 2e-3, "gemm+gelu vs oracle")
    with pytest.raises(capi.InvalidArgument):
        capi.call("gemm_gelu_bf16", Y1, Xd, Wd, bd, M, K + 4, N)


@pytest.mark.parametrize("M,K,N,act", [(2048, 256, 8704, 0),       # 544 tiles of 256 x 128: 2.1 tiles per workgroup
                                       (8192, 128, 3072, 1),       # GPT-2 fc_1 + GELU: 768 tiles, exactly 3 per workgroup, two K-tiles per tile
                                       (1024, 192, 50257, 0),      # ragged last tile-column behind whole tiles (odd pitch), three K-tiles (the ring's period)
                                       (2048, 512, 30720, 0)])     # 960 tiles of 256 x 256 (the two-phase schedule was persistent before round 3)
def test_persistent_tile_walk_gives_the_bits_of_one_workgroup_per_tile(M, K, N, act):
    """round 3: the 256 x 128 ring walks its tiles persistently like the 256 x 256 schedule -- one workgroup per CU, the K pipeline running on across tiles, the epilogue's
    stores draining under the next tile's first K-tile.  Schedule 6 is the same kernels with one workgroup per tile: every output must have the same bits, for bf16
    (+ bias, + GELU), and for the fp8 x fp8 forms (plain and GeGLU) of the same shapes"""
    lib = capi.load()
    rng = np.random.default_rng(N + M)
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    Wb = _weights(rng, N, K, "random")
    bb = orc.to_bf16_bits(rng.uniform(-0.5, 0.5, N).astype(np.float32))
    Xd, Wd, bd = dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), dev_u16(bb)
    fp8 = K % 128 == 0 and N % 256 == 0
    if fp8:
        X8 = dev_u8(rng.integers(0, 0x7e, (M, K), dtype=np.uint8) | (rng.integers(0, 2, (M, K), dtype=np.uint8) << 7))      # finite e4m3 codes
        W8 = dev_u8(rng.integers(0, 0x7e, (N, K), dtype=np.uint8) | (rng.integers(0, 2, (N, K), dtype=np.uint8) << 7))
        ts_d, ws_d = dev_f32(rng.uniform(0.5, 2.0, M).astype(np.float32)), dev_f32(np.array([0.013], dtype=np.float32))
    outs = []
    for persistent in (1, 0):
        capi.tune("gemm.persistent", persistent)
        capi.tune("gemm.walk_min_tiles", 257)      # (the ring's default walks from 769 tiles on; the 544- and 768-tile cases must walk here)
        try:
            Y = torch.full((M, N), 0x7fc0, dtype=torch.int16, device="cuda")
            capi.call("gemm_gelu_bf16" if act else "gemm_bf16", Y, Xd, Wd, bd, M, K, N)
            o = [bits(Y).copy()]
            if fp8:
                Y8 = torch.full((M, N), 0x7fc0, dtype=torch.int16, device="cuda")
                capi.call("gemm_fp8_scaled", Y8, X8, W8, ts_d, ws_d, bd, M, K, N)
                o.append(bits(Y8).copy())
                Yg = torch.full((M, N // 2), 0x7fc0, dtype=torch.int16, device="cuda")
                capi.call("gemm_geglu_fp8_scaled", Yg, X8, W8, ts_d, ws_d, M, K, N // 2)
                o.append(bits(Yg).copy())
            outs.append(o)
        finally:
            capi.tune_reset()
    for a, b, what in zip(outs[0], outs[1], ("bf16", "fp8 x fp8", "fp8 x fp8 + GeGLU")):
        assert not np.any((a & 0x7fff) > 0x7f80), what + ": unwritten (NaN) outputs"
        assert np.array_equal(a, b), what + ": persistent walk differs from one workgroup per tile"
    rows = [0, 255, 256, M - 1]
    exp = orc.round_bf16(orc.linear_bf16w(X[rows], Wb, None)).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    if act:
        h = orc.round_bf16(exp.astype(np.float32)).astype(np.float64)
        exp = 0.5 * h * (1 + np.tanh(0.7978845608028654 * (h + 0.044715 * h ** 3)))
    # (the Linear output is rounded to bf16 BEFORE the bias is added: where the two nearly cancel, one ulp of the product is several of the sum -- hence the absolute floor)
    assert_bf16_close(outs[0][0][rows], exp, 2, 2.0 ** -7 * max(1.0, float(np.abs(exp).max())), "persistent gemm vs oracle")


@pytest.mark.parametrize("M,K,N", [(1, 3840, 8192), (1, 15360, 3840), (1, 4096, 3840), (2, 3840, 30720), (4, 4096, 3840), (3, 2000 + 48, 1000), (4, 8192, 528), (8, 3840, 8192), (16, 2048, 528)])
def test_skinny_whole_x_form_gives_the_staged_forms_bits(M, K, N):
    """round 3: a <= 4-row tail whose e4m3 image fits 32 KB of LDS (the 1-row tail of a prefill chunk) keeps ALL of X in LDS and streams W without a barrier in the K loop;
    same products per wave in the same K order, same wave-order reduction -> the bits of the staged skinny form (gemm_fp8.skinny_whole_x = 0 turns the new form off), plain and GeGLU,
    and both within 2 ulp of the restated reference"""
    lib = capi.load()
    rng = np.random.default_rng(M + K + N)
    X, q4, s4, ws, w8, x8, ts = _w4a8_operands(rng, M, K if K % 128 == 0 else (K // 128 + 1) * 128, N)
    if K % 128 != 0:      # a K that is no multiple of the 128-byte K-tile: drop the padded columns (K % 16 == 0 is what the entry needs)
        x8, w8 = np.ascontiguousarray(x8[:, :K]), np.ascontiguousarray(w8[:, :K])
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32))
    X8, W8, ts_d, ws_d, bd = dev_u8(x8), dev_u8(w8), dev_f32(ts), dev_f32(np.array([ws], dtype=np.float32)), dev_u16(bb)
    outs = []
    for whole_x in (1, 0):
        capi.tune("gemm_fp8.skinny_whole_x", whole_x)
        try:
            Y = torch.full((M, N), 0x7fc0, dtype=torch.int16, device="cuda")
            capi.call("gemm_fp8_scaled", Y, X8, W8, ts_d, ws_d, bd, M, K, N)
            o = [bits(Y).copy()]
            if N % 2 == 0:
                Yg = torch.full((M, N // 2), 0x7fc0, dtype=torch.int16, device="cuda")
                capi.call("gemm_geglu_fp8_scaled", Yg, X8, W8, ts_d, ws_d, M, K, N // 2)
                o.append(bits(Yg).copy())
            outs.append(o)
        finally:
            capi.tune_reset()
    for a, b, what in zip(outs[0], outs[1], ("plain", "GeGLU")):
        assert not np.any((a & 0x7fff) > 0x7f80), what + ": unwritten (NaN) outputs"
        assert np.array_equal(a, b), what + ": the whole-X form differs from the staged skinny form"
    raw = orc.linear_fp8a_fp8w(x8, np.ones(M, dtype=np.float32), w8, None, ws, None)
    exp = orc.round_bf16(raw.astype(np.float32)).astype(np.float64) * ts.astype(np.float64)[:, None] + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(outs[0][0], exp, 2, 1e-3 * float(np.abs(exp).max()), "whole-X skinny vs restated reference")


@pytest.mark.parametrize("M,K,N", [(1, 3840, 8192), (2, 15360, 3840), (16, 768, 3072), (33, 200, 250), (64, 4096, 3840), (7, 64, 96), (100, 256, 520)])
def test_bf16_skinny_kernel_serves_few_rows(M, K, N):
    """round 3: up to 64 rows (a 16-token prompt, the 1-row remainder of a 2049-token one) are a weight stream -- gemm_bf16_skinny_kernel: eight waves take every eighth
    128-byte K-tile of a 16-row strip of W straight from global memory, the partial sums meet in LDS in wave order; one row group whose image fits LDS runs without a
    barrier in the K loop.  Plain (+ bias), Linear + GELU and Linear + GeGLU against the float64 oracle, and against the 128-tile kernel (hook) within 1 ulp of the magnitude;
    100 rows = a 64-row and a 36-row launch... only below 65 rows by default: at 100 the tile kernels keep the call (checked through the hook that turns the skinny kernel off)"""
    lib = capi.load()
    rng = np.random.default_rng(M * 31 + N)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.5, 0.5, N).astype(np.float32))
    Xd, Wd, bd = dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), dev_u16(bb)
    guard = torch.full((M + 1, N), 0x1234, dtype=torch.int16, device="cuda")
    Y = guard[:M]
    capi.call("gemm_bf16", Y, Xd, Wd, bd, M, K, N)
    lin = orc.round_bf16(orc.linear_bf16w(X, Wb, None)).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Y), lin, 2, 2.0 ** -7 * max(1.0, float(np.abs(lin).max())), "skinny gemm_bf16")
    assert np.all(guard[M].cpu().numpy() == 0x1234)
    Yt = empty_u16(M, N)
    capi.tune("gemm.bf16_skinny", 0)              # the tile kernels on the same call
    try:
        capi.call("gemm_bf16", Yt, Xd, Wd, bd, M, K, N)
    finally:
        capi.tune_reset()
    a, b = orc.from_bf16_bits(bits(Y)).astype(np.float64), orc.from_bf16_bits(bits(Yt)).astype(np.float64)
    assert np.abs(a - b).max() <= 2.0 ** -7 * max(np.abs(b).max(), 1e-30)
    if M > 64:
        assert np.array_equal(bits(Y), bits(Yt)), "above 64 rows the default is the tile kernels"
        return
    Yg = empty_u16(M, N)
    capi.call("gemm_gelu_bf16", Yg, Xd, Wd, bd, M, K, N)
    h = orc.round_bf16(lin.astype(np.float32)).astype(np.float64)
    assert_bf16_close(bits(Yg), 0.5 * h * (1 + np.tanh(0.7978845608028654 * (h + 0.044715 * h ** 3))), 2, 2e-2, "skinny gemm_gelu_bf16")
    if N % 2 == 0 and lib.mila_cdna4_gemm_geglu_applicable(M, K, N // 2) == 1:
        F = N // 2
        Ye = empty_u16(M, F)
        capi.call("gemm_geglu_bf16", Ye, Xd, Wd, M, K, F)
        gu = orc.round_bf16(orc.linear_bf16w(X, Wb, None).astype(np.float32)).astype(np.float64)
        g_, u_ = gu[:, :F], gu[:, F:]
        assert_bf16_close(bits(Ye), 0.5 * g_ * (1 + np.tanh(0.7978845608028654 * (g_ + 0.044715 * g_ ** 3))) * u_, 2, 2e-2, "skinny gemm_geglu_bf16")


@pytest.mark.parametrize("M", [2049, 512 + 64, 1024 + 17])
def test_a_long_prompts_short_remainder_goes_to_the_bf16_skinny_kernel(M):
    """bf16 policy, M = 256 k + r with r <= 64: the LDS-DMA kernels on the leading tile-rows and the skinny kernel on the remainder -- plain and fused GeGLU; rows on both
    sides of the seam against the oracle, the leading rows bit-identical to the same call without the remainder"""
    lib = capi.load()
    K, F = 256, 15360
    rng = np.random.default_rng(M)
    Wb = _weights(rng, 2 * F, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    Xd, Wd = dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb)
    main = M - M % 256
    assert lib.mila_cdna4_gemm_geglu_applicable(M, K, F) == 1
    Y, Ym = empty_u16(M, F), empty_u16(main, F)
    capi.call("gemm_geglu_bf16", Y, Xd, Wd, M, K, F)
    capi.call("gemm_geglu_bf16", Ym, Xd, Wd, main, K, F)
    assert np.array_equal(bits(Y)[:main], bits(Ym))
    rows = [0, main - 1, main, M - 1]
    gu = orc.round_bf16(orc.linear_bf16w(X[rows], Wb, None).astype(np.float32)).astype(np.float64)
    g_, u_ = gu[:, :F], gu[:, F:]
    assert_bf16_close(bits(Y)[rows], 0.5 * g_ * (1 + np.tanh(0.7978845608028654 * (g_ + 0.044715 * g_ ** 3))) * u_, 2, 2e-3, "gemm_geglu_bf16 across the seam")
    N = 3840
    Y2 = empty_u16(M, N)
    capi.call("gemm_bf16", Y2, Xd, Wd[:N], None, M, K, N)
    assert_bf16_close(bits(Y2)[rows], orc.linear_bf16w(X[rows], Wb[:N], None), 1, 2e-3, "gemm_bf16 across the seam")


@pytest.mark.parametrize("M,K,N,bias,act", [(300, 2048, 3840, True, 0),        # 60 tiles, K split 4 ways
                                            (100, 2048, 3840, False, 0),       # 30 tiles, 4 ways (8 K-tiles per copy)
                                            (300, 1536, 768, True, 1),         # 12 tiles, K-tile count (24) over 3 copies; + GELU
                                            (255, 1600, 384, True, 0),         # 3 tiles, 25 K-tiles over 3 copies: uneven K ranges (8, 8, 9)
                                            (2048 + 255, 4096, 3840, True, 0),  # a long prompt: 8 whole tile-rows as before + a 255-row remainder split 8 ways
                                            (1024 + 100, 2048, 8192, False, 1),  # 4 whole tile-rows fill the chip (256 tiles); the 100-row remainder (64 tiles) split 4 ways
                                            (16, 15360, 3840, True, 0),        # <= 32 rows: the few-row weight stream (fc_down's shape: 30 x 18 workgroups)
                                            (2, 4096, 3840, False, 1),         # two rows; + GELU
                                            (32, 3840, 8192, True, 0),         # two 16-row groups per wave
                                            (9, 2048, 1200, True, 0),          # a ragged last 128-row block of W (1200 = 9 x 128 + 48), N % 128 != 0
                                            (1, 1024, 3840, True, 0),          # one row: no split-K form, no workspace asked for
                                            (2048, 512, 3840, True, 0)])       # whole tile-rows that fill the chip: no workspace asked for
def test_gemm_with_a_workspace_splits_k_for_short_prompts_and_remainders(M, K, N, bias, act):
    """round 3: gemm_bf16_ws = gemm_bf16 / gemm_gelu_bf16 with the counterpart of the cuBLASLt workspace CudaLinearOp passes (CudaLinearOp.ixx:637-638).  Where the tile
    list covers at most half the CUs, S copies of it take 1 / S of K each and a second kernel sums the fp32 partials in a fixed order and applies the epilogue.  Against
    the float64 oracle at the bar of the plain call, against the plain call within one bf16 ulp of the magnitude (another fp32 summation order), identical bits on a
    second run and with a dirty workspace, nothing written past Y, and the size / alignment errors."""
    lib = capi.load()
    rng = np.random.default_rng(M * 7 + N + act)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16(rng.uniform(-1, 1, (M, K)).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.5, 0.5, N).astype(np.float32)) if bias else None
    Xd, Wd, bd = dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), (dev_u16(bb) if bias else None)
    need = lib.mila_cdna4_gemm_workspace_bytes(M, K, N)
    expect_split = M > 1 and not (M == 2048)
    assert (need > 0) == expect_split, need
    assert need <= 32 << 20
    if M <= 32 and M > 1:                                     # the few-row form: about two workgroups per CU, a slice of >= 4 K-tiles whose X image fits 64 KB
        nk, blocks, nkl_max = K // 64, (N + 127) // 128, 65536 // (M * 128)
        S = min(max(-(-nk // nkl_max), max(1, 512 // blocks)), max(1, nk // 4))
        assert need == S * M * N * 4, (need, S)
    if M == 2048 + 255: assert need == 8 * 255 * N * 4        # the remainder alone, 30 tiles x 8 copies
    if M == 300 and N == 3840: assert need == 4 * 300 * N * 4
    if M == 1024 + 100: assert need == 4 * 100 * N * 4
    ws = torch.full((max(need, 16) // 4 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    guard = torch.full((M + 1, N), 0x1234, dtype=torch.int16, device="cuda")
    Y = guard[:M]
    capi.check(lib.mila_cdna4_gemm_bf16_ws(capi._ptr(Y), capi._ptr(Xd), capi._ptr(Wd), capi._ptr(bd), M, K, N, act, capi._ptr(ws), C.c_size_t(need), capi._stream()))
    torch.cuda.synchronize()
    assert np.all(guard[M].cpu().numpy() == 0x1234)
    first = bits(Y).copy()
    assert not np.any((first & 0x7fff) > 0x7f80), "unwritten / NaN outputs (a K range or a row not covered)"
    # plain call on the same operands
    Yp = empty_u16(M, N)
    capi.call("gemm_gelu_bf16" if act else "gemm_bf16", Yp, Xd, Wd, bd, M, K, N)
    a, b = orc.from_bf16_bits(first).astype(np.float64), orc.from_bf16_bits(bits(Yp)).astype(np.float64)
    assert np.abs(a - b).max() <= 2.0 ** -7 * max(np.abs(b).max(), 1e-30)
    if not expect_split:
        assert np.array_equal(first, bits(Yp)), "no workspace asked for: the call is the plain one"
    # oracle (sampled rows keep it to seconds)
    rows = sorted(set(r for r in [0, 1, M // 2, M - M % 256 - 1 if M >= 256 else 0, M - M % 256 if M % 256 else 0, M - 1] if r < M))
    lin = orc.linear_bf16w(X[rows], Wb, None)
    if bias: lin = orc.round_bf16(lin.astype(np.float32)).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    if act:
        h = orc.round_bf16(np.asarray(lin, dtype=np.float32)).astype(np.float64)
        lin = 0.5 * h * (1 + np.tanh(0.7978845608028654 * (h + 0.044715 * h ** 3)))
    assert_bf16_close(first[rows], lin, 2, 2.0 ** -7 * max(1.0, float(np.abs(lin).max())) if (bias or act) else 2e-3, "gemm_bf16_ws")
    # the same bits again, with other garbage in the workspace
    ws.fill_(1.0e30)
    Y2 = empty_u16(M, N)
    capi.check(lib.mila_cdna4_gemm_bf16_ws(capi._ptr(Y2), capi._ptr(Xd), capi._ptr(Wd), capi._ptr(bd), M, K, N, act, capi._ptr(ws), C.c_size_t(need), capi._stream()))
    assert np.array_equal(bits(Y2), first)
    if need:
        rc = lib.mila_cdna4_gemm_bf16_ws(capi._ptr(Y2), capi._ptr(Xd), capi._ptr(Wd), capi._ptr(bd), M, K, N, act, capi._ptr(ws), C.c_size_t(need - 1), capi._stream())
        assert rc == capi.MILA_E_SCRATCH_TOO_SMALL
        rc = lib.mila_cdna4_gemm_bf16_ws(capi._ptr(Y2), capi._ptr(Xd), capi._ptr(Wd), capi._ptr(bd), M, K, N, act, None, C.c_size_t(0), capi._stream())
        assert rc == capi.MILA_E_SCRATCH_TOO_SMALL
        rc = lib.mila_cdna4_gemm_bf16_ws(capi._ptr(Y2), capi._ptr(Xd), capi._ptr(Wd), capi._ptr(bd), M, K, N, act, C.c_void_p(ws.data_ptr() + 4), C.c_size_t(need), capi._stream())
        assert rc == capi.MILA_E_INVALID_ARGUMENT
    rc = lib.mila_cdna4_gemm_bf16_ws(capi._ptr(Y2), capi._ptr(Xd), capi._ptr(Wd), capi._ptr(bd), M, K, N, 2, capi._ptr(ws), C.c_size_t(need), capi._stream())
    assert rc == capi.MILA_E_INVALID_ARGUMENT


@pytest.mark.parametrize("M,K,N,bias", [(300, 4096, 3840, True),            # 60 tiles, K (32 K-tiles of 128) split 4 ways
                                        (100, 2048, 3840, False),           # 30 tiles, 16 K-tiles split 2 ways
                                        (255, 3200, 384, True),             # 3 tiles, 25 K-tiles over 3 copies (8, 8, 9)
                                        (2048 + 255, 4096, 3840, True),     # long prompt: 8 whole tile-rows as before + the 255-row remainder split 4 ways
                                        (16, 4096, 3840, True),             # one 16-row group: the skinny weight stream keeps it, no workspace asked for
                                        (2048, 1024, 3840, False)])         # whole tile-rows that fill the chip: none either
def test_w4a8_gemm_with_a_workspace_splits_k(M, K, N, bias):
    """gemm_fp8_scaled_ws: the W4A8 GEMM with a caller workspace (the fp4 policy's prefill, CudaLinearOp.ixx:646-715 with the cuBLASLt workspace of :706-707).  The split-K
    form sums S fp32 partials in a fixed order and applies the kernels' epilogue, y = bf16(float(bf16(acc sB)) s_m + bias): sampled rows against the restated reference, the
    whole output against the plain call within one bf16 ulp of the magnitude, the same bits again from a dirty workspace and from the one-call form gemm_bf16_w4a8 (whose
    scratch carries the workspace), nothing written past Y, size / alignment errors"""
    lib = capi.load()
    rng = np.random.default_rng(M * 11 + N)
    X, q4, s4, ws, w8, x8, ts = _w4a8_operands(rng, M, K, N, 128)
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
    ws_d = dev_f32(np.array([ws], dtype=np.float32))
    X8, W8, ts_d, bd = dev_u8(x8), dev_u8(w8), dev_f32(ts), (dev_u16(bb) if bias else None)
    need = lib.mila_cdna4_gemm_fp8_workspace_bytes(M, K, N)
    expect = {300: 4 * 300, 100: 2 * 100, 255: 3 * 255, 2048 + 255: 4 * 255, 16: 0, 2048: 0}[M] * N * 4
    assert need == expect, (need, expect)
    wsb = torch.full((max(need, 16) // 4 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    guard = torch.full((M + 1, N), 0x1234, dtype=torch.int16, device="cuda")
    Y = guard[:M]
    args = lambda y, w, nb: (capi._ptr(y), capi._ptr(X8), capi._ptr(W8), capi._ptr(ts_d), capi._ptr(ws_d), capi._ptr(bd), M, K, N, w, C.c_size_t(nb), capi._stream())
    capi.check(lib.mila_cdna4_gemm_fp8_scaled_ws(*args(Y, capi._ptr(wsb), need)))
    torch.cuda.synchronize()
    assert np.all(guard[M].cpu().numpy() == 0x1234)
    first = bits(Y).copy()
    assert not np.any((first & 0x7fff) > 0x7f80), "unwritten / NaN outputs"
    Yp = empty_u16(M, N)
    capi.call("gemm_fp8_scaled", Yp, X8, W8, ts_d, ws_d, bd, M, K, N)
    a, b = orc.from_bf16_bits(first).astype(np.float64), orc.from_bf16_bits(bits(Yp)).astype(np.float64)
    assert np.abs(a - b).max() <= 2.0 ** -7 * max(np.abs(b).max(), 1e-30)
    if not need:
        assert np.array_equal(first, bits(Yp))
    main = M - M % 256
    rows = sorted({0, 1, M // 2, M - 1, max(0, main - 1), min(M - 1, main)})
    raw = orc.linear_fp8a_fp8w(x8[rows], np.ones(len(rows), dtype=np.float32), w8, None, ws, None)
    exp = orc.round_bf16(raw.astype(np.float32)).astype(np.float64) * ts[rows].astype(np.float64)[:, None]
    if bias:
        exp = exp + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(first[rows], exp, 2, 1e-3 * float(np.abs(exp).max()), "gemm_fp8_scaled_ws vs restated reference")
    wsb.fill_(-1.0e30)
    Y2 = empty_u16(M, N)
    capi.check(lib.mila_cdna4_gemm_fp8_scaled_ws(*args(Y2, capi._ptr(wsb), need)))
    assert np.array_equal(bits(Y2), first)
    need1 = lib.mila_cdna4_gemm_w4a8_scratch_bytes(M, K, N)
    assert need1 >= N * K + M * K + 4 * M + need
    scratch = torch.empty(need1, dtype=torch.uint8, device="cuda")
    Y3 = empty_u16(M, N)
    capi.call("gemm_bf16_w4a8", Y3, dev_u16(orc.to_bf16_bits(X)), dev_u8(q4), dev_f32(s4), ws_d, bd, M, K, N, 128, scratch, C.c_size_t(need1))
    assert np.array_equal(bits(Y3), first), "the one-call form (workspace inside its scratch) differs"
    if need:
        assert lib.mila_cdna4_gemm_fp8_scaled_ws(*args(Y2, capi._ptr(wsb), need - 1)) == capi.MILA_E_SCRATCH_TOO_SMALL
        assert lib.mila_cdna4_gemm_fp8_scaled_ws(*args(Y2, None, 0)) == capi.MILA_E_SCRATCH_TOO_SMALL
        assert lib.mila_cdna4_gemm_fp8_scaled_ws(*args(Y2, C.c_void_p(wsb.data_ptr() + 4), need)) == capi.MILA_E_INVALID_ARGUMENT


@pytest.mark.parametrize("M,K,N", [(2048, 1024, 8704), (2048 + 100, 1024, 8704)])
def test_column_split_of_a_tile_list_that_ends_in_a_nearly_empty_round(M, K, N):
    """Gemma's global qkv_proj (N = 8704) at T = 2048 is 272 tiles of 256 x 256 on 256 CUs: with a workspace the first 8192 columns run as whole rounds of 256 x 256 tiles and
    the last 512 through the split-K ring, both writing their column range of Y with the pitch of the whole row (csrc/gemm_plan.hip: colsplit_columns).  bf16, W4A8 and W8A8:
    sampled rows x ALL columns (both sides of the cut) against the float64 oracle, a guard row behind Y, and the form that ran."""
    lib = capi.load()
    rng = np.random.default_rng(M + N)
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16((rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32))
    bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32))
    rows = [0, 255, 256, M // 2, M - 1]
    # bf16
    need = lib.mila_cdna4_gemm_workspace_bytes(M, K, N)
    tm = (M + 255) // 256
    cut = ((tm * (N // 256)) // 256 * 256) // tm * 256                      # columns of the whole rounds: 8192 at eight tile-rows, 7168 at nine
    assert need == 2 * M * (N - cut) * 4, need                              # S = 2 copies of the rest (16 K-tiles: 8 per copy)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    Yg = torch.full((M + 1, N), 0x1234, dtype=torch.int16, device="cuda")
    capi.last_form()
    capi.call("gemm_bf16_ws", Yg[:M], dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), dev_u16(bb), M, K, N, 0, ws, C.c_size_t(need))
    assert capi.last_form() == ["gemm256_colsplit", "gemm256", "gemm256x128_splitk"]
    exp = orc.round_bf16(orc.linear_bf16w(X[rows], Wb, None)).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Yg[:M])[rows], exp, 2, 2e-3, "column-split gemm_bf16_ws")
    assert np.all(Yg[M].cpu().numpy() == 0x1234), "a store past row M - 1"
    # without the split (tuning variable) the other kernels agree to the last-bit freedom of another summation order
    Y0 = empty_u16(M, N)
    capi.tune("gemm.colsplit", 0)
    try:
        assert lib.mila_cdna4_gemm_workspace_bytes(M, K, N) == 0
        capi.call("gemm_bf16_ws", Y0, dev_u16(orc.to_bf16_bits(X)), dev_u16(Wb), dev_u16(bb), M, K, N, 0, None, C.c_size_t(0))
    finally:
        capi.tune_reset()
    a, b = orc.from_bf16_bits(bits(Yg[:M])).astype(np.float64), orc.from_bf16_bits(bits(Y0)).astype(np.float64)
    assert np.array_equal(bits(Yg[:M])[:, :cut], bits(Y0)[:, :cut]), "the 256 x 256 tiles and the 256 x 128 ring sum K in one order: same bits left of the cut"
    assert np.abs(a - b).max() <= 2.0 ** -7 * np.abs(b).max()
    # fp8 x fp8: W8A8 (per-channel scales, offset with the column range) and W4A8 (per-tensor scale); a K-tile is 128 bytes there: K = 2048 for two copies of 8 K-tiles
    K = 2048
    Wb = _weights(rng, N, K, "random")
    X = orc.round_bf16((rng.standard_normal((M, K)) * rng.uniform(0.2, 3.0, (M, 1))).astype(np.float32))
    w8, sc = orc.quantize_fp8_per_channel(Wb)
    x8, ts = orc.quantize_act_fp8_per_token(X)
    need8 = lib.mila_cdna4_gemm_fp8_workspace_bytes(M, K, N)
    assert need8 > 0
    ws8 = torch.empty(need8, dtype=torch.uint8, device="cuda")
    Y8 = empty_u16(M, N)
    capi.last_form()
    capi.call("gemm_fp8_w8a8_ws", Y8, dev_u8(x8), dev_u8(w8), dev_f32(ts), dev_f32(sc), dev_u16(bb), M, K, N, ws8, C.c_size_t(need8))
    assert capi.last_form() == ["fp8_gemm256_colsplit", "fp8_gemm256", "fp8_gemm256x128_splitk"]
    exp8 = orc.linear_fp8a_fp8w(x8[rows], ts[rows], w8, sc, 1.0, None).astype(np.float64) + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Y8)[rows], exp8, 2, 1e-3 * float(np.abs(exp8).max()), "column-split W8A8")
    wsc = dev_f32(np.array([0.37], dtype=np.float32))
    capi.call("gemm_fp8_scaled_ws", Y8, dev_u8(x8), dev_u8(w8), dev_f32(ts), wsc, dev_u16(bb), M, K, N, ws8, C.c_size_t(need8))
    raw = orc.linear_fp8a_fp8w(x8[rows], np.ones(len(rows), dtype=np.float32), w8, None, 0.37, None)
    exp4 = orc.round_bf16(raw.astype(np.float32)).astype(np.float64) * ts[rows].astype(np.float64)[:, None] + orc.from_bf16_bits(bb).astype(np.float64)
    assert_bf16_close(bits(Y8)[rows], exp4, 2, 1e-3 * float(np.abs(exp4).max()), "column-split W4A8 epilogue")
