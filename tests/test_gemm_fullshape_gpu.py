"""GPU parity: EVERY element of the prefill GEMMs' output at the four Gemma-4 12B Linear shapes, full K, M = 2048 and M = 2303, against float64.

The other GEMM tests look at a handful of rows at these shapes (the oracle is scalar double loops) and cover the rest by bit-identity between kernels of one family, which
share their instruction chain on purpose.  The kernels are 8 waves as 2 x 4, each wave owning 64-row bands in 64 x 32 quadrants, tiles walked persistently 2 / 1 or 4 / 3
per workgroup, K = 30 / 32 / 120 K-tiles through the interior K-tile bodies: an error confined to interior tile-rows, one wave band, one walked tile or one K-tile is
invisible to sampled rows.  Here the expectation is tests/ref_matmul.py (float64 BLAS, pinned to the oracle in test_oracle_kats.py; exact for fp8 x fp8), the outputs
are poisoned before the call, and the bar is elementwise (gpu_util.assert_gemm_close): max_ulp bf16 ulp of RNE(exact), or |got - exact| <= min(1e-3 x max|exact|,
2^-17 x sum_k |x w| x scales of THAT element).  test_gemm_bar_cpu.py shows the bar passes the device arithmetic and fails four kinds of wrong kernel.

Legs (entry points as RocmLinearOp calls them, workspace from the *_workspace_bytes query):
  bf16      gemm_bf16_ws                                     orc.linear_bf16w, bias added after the bf16 rounding (reference prefill order)
  w8a16     gemm_bf16_w8a16_staged (one shape: it is the bf16 kernel on the staged weights)     bf16(dequantized W)
  w8a8      gemm_fp8_w8a8_ws, gemm_bf16_w8a8 bit-identical   orc.linear_fp8a_fp8w with scale[n]
  w4a8      gemm_fp8_scaled_ws, gemm_bf16_w4a8 bit-identical the two-step composition of test_linear_gpu.test_w4a8_prefill_matches_the_restated_reference
  geglu-*   fc_gate_up only: gemm_geglu_bf16 / gemm_geglu_fp8_w8a8 / gemm_geglu_fp8_scaled bit-identical to the leg's Linear then geglu_bf16, and all M x F against
            orc.geglu of the bf16-rounded float64 gate / up
After each Linear call the kernel form that served it (capi.last_form) must be the one tests/golden/dispatch_ladder.json records for that policy / shape / M, so the test
provably ran the kernel it claims.  Each (leg, shape, M) prints the worst ulp distance (over ALL elements: an output that is the difference of large partial sums is
thousands of ulp from its exact value and still correct -- that is what the slack is for), how many elements over max_ulp the slack let through, the worst
|got - exact| / mag among those, and how many passed against the second expectation of a two-rounding composition (run with -s; profiles/r05_gemm_fullshape.txt holds
the record: 1.5e-5 of the elements of the bf16 legs go through the slack, 4e-4 .. 7e-4 of the fp8 x fp8 legs -- the fp8 matrix-core instruction's own arithmetic, see
gpu_util.SLACK -- and nothing fails)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import orc
import ref_matmul
from gpu_util import (assert_bf16_close, assert_gemm_close, bits, dev_f32, dev_u16, dev_u8, empty_f32, empty_u16, empty_u8, f32_to_bf16_bits, host)
from mila_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = {"qkv_proj(local)": (3840, 8192, False), "o_proj(local)": (4096, 3840, True), "fc_gate_up": (3840, 30720, False), "fc_down": (15360, 3840, True)}   # K, N, bias
ROWS = (2048, 2303)                 # full tiles and persistent walks; 2048 + 255: the ladder's largest ragged length (remainder forms, split-K through the workspace)
MMAX = max(ROWS)
LEGS = [(s, leg) for s in SHAPES for leg in (["bf16", "w8a8", "w4a8"] + (["w8a16"] if s == "qkv_proj(local)" else []) +
                                             (["geglu-bf16", "geglu-w8a8", "geglu-w4a8"] if s == "fc_gate_up" else []))]
POLICY = {"bf16": "bf16", "w8a16": "fp8", "w8a8": "fp8-w8a8", "w4a8": "fp4"}
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_ladder.json")))

_cache = {}                         # operands and float64 expectations of ONE shape at a time (the parametrization is shape-major), shared by that shape's legs


def _shape_cache(name):
    if _cache.get("name") != name:
        _cache.clear()
        _cache["name"] = name
    return _cache


def _get(name, key, make):
    c = _shape_cache(name)
    if key not in c:
        c[key] = make()
    return c[key]


def _operands(name):
    """as test_w8a8_gpu._operands: channel scales over 4 octaves, token scales 0.2 - 3.0, row 7 all zero; MMAX rows, of which M = 2048 uses the first 2048"""
    def make():
        K, N, bias = SHAPES[name]
        rng = np.random.default_rng(K * 7 + N)
        Wb = orc.to_bf16_bits((rng.standard_normal((N, K), dtype=np.float32) / np.float32(np.sqrt(K)) * rng.uniform(0.25, 4.0, (N, 1)).astype(np.float32)))
        X = orc.round_bf16(rng.standard_normal((MMAX, K), dtype=np.float32) * rng.uniform(0.2, 3.0, (MMAX, 1)).astype(np.float32))
        X[7] = 0.0
        bb = orc.to_bf16_bits(rng.uniform(-0.1, 0.1, N).astype(np.float32)) if bias else None
        return dict(K=K, N=N, Wb=Wb, X=X, bb=bb)
    return _get(name, "operands", make)


def _x8(name):
    return _get(name, "x8", lambda: orc.quantize_act_fp8_per_token(_operands(name)["X"]))


def _w8(name):
    return _get(name, "w8", lambda: orc.quantize_fp8_per_channel(_operands(name)["Wb"]))


def _w4(name):
    def make():
        q4, s4 = orc.quantize_fp4_per_group(_operands(name)["Wb"], 128)
        ws = orc.fp8_weight_scale_from_groups(s4)
        return q4, s4, ws, orc.upcast_fp4_to_fp8(q4, s4, ws, 128)
    return _get(name, "w4", make)


def _bias64(o):
    return 0.0 if o["bb"] is None else ref_matmul.bf16_bits_to_f64(o["bb"])[None, :]


def _round_bf16_f64(a):
    return ref_matmul.bf16_bits_to_f64(f32_to_bf16_bits(a.astype(np.float32)))


def _expectation(name, leg):
    """(exact [MMAX, N] float64, mag(m_idx, n_idx), max_ulp, inner) of a Linear leg; inner = (g, post) where the composition rounds the GEMM result g to bf16 before the
    bias is added (the bf16 legs with a bias, W4A8): see gpu_util.assert_gemm_close"""
    o = _operands(name)

    def make():
        X, Wb = o["X"], o["Wb"]
        if leg == "bf16":
            g = ref_matmul.linear_bf16w(X, Wb)
            mag = lambda m, n: ref_matmul.abs_products("bf16", X, Wb, at=(m, n))
            if o["bb"] is None:
                return g, mag, 1, None
            return _round_bf16_f64(g) + _bias64(o), mag, 2, (g, None)       # reference prefill order: round the GEMM to bf16, then add bias (cuda_add_bias)
        if leg == "w8a16":
            w8, sc = _w8(name)
            Wdq = ref_matmul.dequant_fp8_bf16_bits(w8, sc)
            g = ref_matmul.linear_bf16w(X, Wdq)
            mag = lambda m, n: ref_matmul.abs_products("bf16", X, Wdq, at=(m, n))
            if o["bb"] is None:
                return g, mag, 1, None
            return _round_bf16_f64(g) + _bias64(o), mag, 2, (g, None)
        x8, ts = _x8(name)
        if leg == "w8a8":
            w8, sc = _w8(name)
            return ref_matmul.linear_fp8a_fp8w(x8, ts, w8, sc, 1.0, o["bb"]), (lambda m, n: ref_matmul.abs_products("fp8a_fp8w", x8, w8, (ts, sc), at=(m, n))), 2, None
        q4, s4, ws, w8u = _w4(name)                        # W4A8 (CudaLinearOp.ixx:646-715): sB * acc rounded to bf16, then x s_m + bias rounded again
        raw = ref_matmul.linear_fp8a_fp8w(x8, np.ones(len(ts), dtype=np.float32), w8u, None, ws)
        exact = _round_bf16_f64(raw) * ts.astype(np.float64)[:, None] + _bias64(o)
        return exact, (lambda m, n: ref_matmul.abs_products("fp8a_fp8w", x8, w8u, (ts, np.float32(ws)), at=(m, n))), 2, (raw, ts.astype(np.float64))
    return _get(name, "exp-" + leg, make)


def _device_operands(name, leg):
    """device tensors of a leg; the integer steps (weight quantization, fp4 -> e4m3 staging, activation quantization) asserted bit-exact against the oracle"""
    o = _operands(name)
    K, N = o["K"], o["N"]
    d = dict(X=dev_u16(orc.to_bf16_bits(o["X"])), bias=dev_u16(o["bb"]) if o["bb"] is not None else None)
    if leg == "bf16":
        d["W"] = dev_u16(o["Wb"])
    if leg in ("w8a16", "w8a8"):
        w8, sc = _w8(name)
        d["W8"], d["SC"] = empty_u8(N, K), empty_f32(N)
        capi.call("quantize_fp8_per_channel", d["W8"], d["SC"], dev_u16(o["Wb"]), N, K)
        assert np.array_equal(host(d["W8"]), w8) and np.array_equal(host(d["SC"]), sc), "fp8 weight quantization is not bit-exact"
    if leg == "w4a8":
        q4, s4, ws, w8u = _w4(name)
        d["Q4"], d["S4"], d["WS"] = dev_u8(q4), dev_f32(s4), empty_f32(1)
        capi.call("fp4_weight_fp8_scale", d["WS"], d["S4"], C.c_int64(s4.size))
        assert np.float32(host(d["WS"])[0]) == np.float32(ws)
        d["W8"] = empty_u8(N, K)
        capi.call("upcast_fp4_to_fp8", d["W8"], d["Q4"], d["S4"], d["WS"], N, K, 128)
        assert np.array_equal(host(d["W8"]), w8u), "fp4 -> e4m3 staging is not bit-exact"
    if leg in ("w8a8", "w4a8"):
        x8, ts = _x8(name)
        d["X8"], d["TS"] = empty_u8(MMAX, K), empty_f32(MMAX)
        capi.call("quantize_fp8_per_token", d["X8"], d["TS"], d["X"], MMAX, K)
        assert np.array_equal(host(d["X8"]), x8) and np.array_equal(host(d["TS"]), ts), "activation quantization is not bit-exact"
    return d


def _linear(leg, d, M, K, N):
    """the leg's Linear through its workspace entry on a poisoned output; returns (Y bits [M, N], the forms that ran)"""
    lib = capi.load()
    Y = empty_u16(M, N)
    capi.last_form()
    if leg == "bf16":
        need = lib.mila_cdna4_gemm_workspace_bytes(M, K, N)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        capi.call("gemm_bf16_ws", Y, d["X"][:M], d["W"], d["bias"], M, K, N, 0, ws if need else None, C.c_size_t(need))
    elif leg == "w8a16":
        need = lib.mila_cdna4_gemm_staging_bytes(M, K, N)
        assert need >= N * K * 2                            # the staged weights, and behind them the workspace of the bf16 GEMM
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        capi.call("gemm_bf16_w8a16_staged", Y, d["X"][:M], d["W8"], d["SC"], d["bias"], M, K, N, scratch, C.c_size_t(need))
    else:
        assert lib.mila_cdna4_gemm_fp8_applicable(M, K, N) == 1
        need = lib.mila_cdna4_gemm_fp8_workspace_bytes(M, K, N)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        if leg == "w8a8":
            capi.call("gemm_fp8_w8a8_ws", Y, d["X8"][:M], d["W8"], d["TS"][:M], d["SC"], d["bias"], M, K, N, ws if need else None, C.c_size_t(need))
        else:
            capi.call("gemm_fp8_scaled_ws", Y, d["X8"][:M], d["W8"], d["TS"][:M], d["WS"], d["bias"], M, K, N, ws if need else None, C.c_size_t(need))
    return bits(Y), capi.last_form()


def _one_call_form(leg, d, M, K, N):
    """gemm_bf16_w8a8 / gemm_bf16_w4a8: quantize the activations themselves"""
    lib = capi.load()
    Y = empty_u16(M, N)
    if leg == "w8a8":
        need = lib.mila_cdna4_gemm_w8a8_scratch_bytes(M, K, N)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        capi.call("gemm_bf16_w8a8", Y, d["X"][:M], d["W8"], d["SC"], d["bias"], M, K, N, scratch, C.c_size_t(need))
    else:
        need = lib.mila_cdna4_gemm_w4a8_scratch_bytes(M, K, N)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        capi.call("gemm_bf16_w4a8", Y, d["X"][:M], d["Q4"], d["S4"], d["WS"], d["bias"], M, K, N, 128, scratch, C.c_size_t(need))
    return bits(Y)


def _emit(line):
    print(line)


def _report(leg, name, M, forms, stats):
    _emit("FULLSHAPE %-10s %-16s M=%d forms=%s elements=%d worst_ulp=%d over_max_ulp_let_through=%d (%.3g of all) worst_err/mag=%.3g (2^%.1f) inner_rounding_flips=%d"
          % (leg, name, M, "+".join(forms), stats["n"], stats["worst_ulp"], stats["over_ulp"], stats["over_ulp"] / stats["n"], stats["worst_ratio"],
             np.log2(stats["worst_ratio"]) if stats["worst_ratio"] > 0 else -np.inf, stats["inner_flips"]))


def _linear_leg(name, leg):
    o = _operands(name)
    K, N = o["K"], o["N"]
    exact, mag, max_ulp, inner = _expectation(name, leg)
    atol = 1e-3 * float(np.abs(exact).max())
    d = _device_operands(name, leg)
    for M in ROWS:
        Y, forms = _linear(leg, d, M, K, N)
        assert forms, "no kernel form was noted"
        assert forms == GOLDEN["%s/%s/%d" % (POLICY[leg], name, M)], (forms, "the dispatch ladder records another form for this call")
        stats = {}
        assert_gemm_close(Y, exact[:M], mag, max_ulp, "%s %s M=%d via %s" % (leg, name, M, "+".join(forms)), atol, stats,
                          inner=None if inner is None else (inner[0][:M], None if inner[1] is None else inner[1][:M]))
        _report(leg, name, M, forms, stats)
        if leg in ("w8a8", "w4a8"):
            assert np.array_equal(_one_call_form(leg, d, M, K, N), Y), "the one-call form differs from the workspace entry"


def _geglu_leg(name, leg):
    lin = leg.split("-")[1]
    o = _operands(name)
    K, N = o["K"], o["N"]
    F = N // 2
    assert o["bb"] is None
    exact = _expectation(name, lin)[0]
    d = _device_operands(name, lin)
    lib = capi.load()
    for M in ROWS:
        assert (lib.mila_cdna4_gemm_geglu_applicable(M, K, F) if lin == "bf16" else lib.mila_cdna4_gemm_geglu_w4a8_applicable(M, K, F)) == 1
        GU, _ = _linear(lin, d, M, K, N)
        Y0, Y1 = empty_u16(M, F), empty_u16(M, F)
        capi.call("geglu_bf16", Y0, dev_u16(GU), M, F)
        capi.last_form()
        if lin == "bf16":
            capi.call("gemm_geglu_bf16", Y1, d["X"][:M], d["W"], M, K, F)
        elif lin == "w8a8":
            capi.call("gemm_geglu_fp8_w8a8", Y1, d["X8"][:M], d["W8"], d["TS"][:M], d["SC"], M, K, F)
        else:
            capi.call("gemm_geglu_fp8_scaled", Y1, d["X8"][:M], d["W8"], d["TS"][:M], d["WS"], M, K, F)
        forms = capi.last_form()
        assert forms, "no kernel form was noted for the fused GeGLU entry"
        got = bits(Y1)
        assert np.array_equal(got, bits(Y0)), "%s M=%d via %s: the fused GeGLU epilogue differs from Linear then geglu_bf16" % (leg, M, "+".join(forms))
        # all M x F: gate / up rounded to bf16 as the Linear stores them, GeGLU in double
        exp = orc.geglu(_round_bf16_f64(exact[:M]).astype(np.float32))
        worst = assert_bf16_close(got, exp, 2, 2e-3 * float(np.abs(exp).max()), "%s M=%d via %s vs the float64 composition" % (leg, M, "+".join(forms)))
        _emit("FULLSHAPE %-10s %-16s M=%d forms=%s elements=%d worst_ulp=%d (all M x F, 2 ulp or 2e-3 x max; bit-identical to Linear then geglu_bf16)"
              % (leg, name, M, "+".join(forms), got.size, worst))


@pytest.mark.parametrize("name,leg", LEGS, ids=["%s-%s" % sl for sl in LEGS])
def test_every_element_of_the_full_shape_against_float64(name, leg):
    try:
        if leg.startswith("geglu-"):
            _geglu_leg(name, leg)
        else:
            _linear_leg(name, leg)
    finally:
        if (name, leg) == [sl for sl in LEGS if sl[0] == name][-1]:
            _cache.clear()                                  # the last leg of a shape: give its operands and expectations back
