"""BASELINE.json configs 3-5 at FULL size (Gemma-4 12B: D 3840, 48 layers, F 15360, V 262144; bf16 / PerChannelFp8 / PerGroupFp4
weights; prefill T = 2048 then decode) through size-independent properties, because the CPU oracle cannot finish a 12-billion
parameter forward in test time:

  * the decode schedules agree bit for bit (reference-order launches, fused schedule, hipGraph replay), after a real T = 2048 prefill;
  * prefill is deterministic, and -- on the first 6 layers at full width -- its last-position logits agree with DECODING the same last
    token on the prefix's cache (two different kernel families, MFMA GEMMs + flash prefill vs matvecs + flash-decode, computing the
    same function; bf16 bar).  Only 6 layers: with RANDOM weights a bf16 rounding difference grows ~1.4x per layer (measured
    tools/depth_probe.py: 5e-2 of the logit range at 6 layers, 0.39 at 12, decorrelated from 24 on), so at full depth only
    bit-identity properties are meaningful;
  * the GEMM schedules (all waves in lockstep vs the staggered two-barrier schedules) give the same bits;
  * resident prefill staging (the default) gives the bits of per-forward staging (fp8, fp4), on the real LDS-DMA shapes;
  * (a quantized model is NOT compared with the bf16 one here: with random weights the e4m3 / e2m1 weight error decorrelates the
    logits within 6 layers, cosine 0.42 for fp8; the quantized Linears are held to the oracle on the same quantized weights
    op by op in tests/test_linear_gpu.py and model-wide on the small configurations).

The small-configuration tests hold the same code to the oracle; these hold the full-size kernel selections to each other."""
import numpy as np
import pytest

from mila_amd import capi, host

pytestmark = pytest.mark.gpu

T = 2048
V = host.GEMMA4_12B["vocab_size"]
TOKS = [int((7919 * i + 13) % V) for i in range(T)]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def bf16_run():
    """one bf16 model: prefill logits, then the three decode schedules at the next positions"""
    g = host.Gemma("bf16", max_seq=T + 16, max_prefill=T, seed=1234)
    pre = g.prefill(TOKS)
    pre2 = g.prefill(TOKS)
    out = {"prefill": pre, "prefill_again": pre2, "decode": {}}
    nxt = int(np.argmax(pre))
    for mode in ("reference", "fused", "graph"):
        out["decode"][mode] = g.decode(nxt, T, mode)          # each call rewrites row T of every cache with the same values
    out["next"] = nxt
    g.close()
    return out


SIX = dict(host.GEMMA4_12B, num_layers=6)


@pytest.fixture(scope="module")
def six_layers():
    """full width, 6 layers (5 sliding-window + 1 global): where cross-kernel-family comparisons are still meaningful"""
    g = host.Gemma("bf16", SIX, max_seq=T + 16, max_prefill=T, seed=1234)
    out = {"prefill": g.prefill(TOKS)}
    # the last prompt token decoded on the cache of the first T - 1: the same function as the prefill's last row
    out["redecode_last"] = g.decode(TOKS[-1], T - 1, "fused")
    g.close()
    return out


def test_full_size_prefill_is_deterministic_and_finite(bf16_run):
    p = bf16_run["prefill"]
    assert p.shape == (V,) and np.all(np.isfinite(p))
    assert np.array_equal(p.view(np.uint32), bf16_run["prefill_again"].view(np.uint32))


def test_full_size_decode_schedules_are_bit_identical(bf16_run):
    d = bf16_run["decode"]
    assert np.all(np.isfinite(d["reference"]))
    assert np.array_equal(d["reference"].view(np.uint32), d["fused"].view(np.uint32))
    assert np.array_equal(d["reference"].view(np.uint32), d["graph"].view(np.uint32))


def test_full_width_prefill_and_decode_compute_the_same_function(six_layers):
    """row T - 1 through the prefill kernels vs the decode kernels at D 3840 / F 15360 / V 262144, T 2048: the bar is the bf16 one
    used for the small models (1e-1 of the logit range worst case); measured 5e-2, cosine 0.997"""
    a, b = six_layers["prefill"], six_layers["redecode_last"]
    assert _rel(b, a) < 1e-1, _rel(b, a)
    assert float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b))) > 0.99
    srt = np.sort(a)
    if srt[-1] - srt[-2] > 0.1 * np.abs(a).max():
        assert int(np.argmax(a)) == int(np.argmax(b))


@pytest.mark.parametrize("policy", ["bf16", "fp4"])
def test_full_size_gemm_schedules_give_the_same_bits(policy, bf16_run):
    """lockstep vs ping-pong schedules accumulate in the same order: identical prefill logits on the real shapes (the fp4 policy
    compares the two staggered forms that keep its fp8 shapes on the same kernels: 1 vs 3); and the default schedule with one workgroup per tile
    instead of the persistent tile walk of both LDS-DMA kernels (gemm.persistent = 0) gives the same bits again"""
    lib = capi.load()
    outs = []
    try:
        # (the split-K forms -- here the column split of the global qkv_proj, csrc/gemm_plan.hip: colsplit_columns -- exist under the default schedule only and sum K in
        # another order: the schedules are compared on ONE decomposition, with the column split off; the default decomposition is compared across its own two forms below)
        capi.tune("gemm.colsplit", 0)
        for sched, persistent in (((0, 1), (3, 1), (5, 0), (5, 1)) if policy == "bf16" else ((1, 1), (3, 1), (5, 0), (5, 1))):
            capi.tune("gemm.schedule", sched)       # an inert hook (MILA_CDNA4_TUNING unset) must fail the test, not compare the default with itself
            capi.tune("gemm.persistent", persistent)
            g = host.Gemma(policy, max_seq=T + 16, max_prefill=T, seed=1234)
            outs.append(g.prefill(TOKS))
            g.close()
        capi.tune("gemm.colsplit", 1)
        capi.tune("gemm.persistent", 0)               # the default decomposition with one workgroup per tile instead of the persistent walk
        g = host.Gemma(policy, max_seq=T + 16, max_prefill=T, seed=1234)
        one_per_tile = g.prefill(TOKS)
        capi.tune("gemm.persistent", 1)
        default = g.prefill(TOKS)
        g.close()
    finally:
        capi.tune_reset()
    for o in outs[1:]:
        assert np.array_equal(outs[0].view(np.uint32), o.view(np.uint32))
    assert np.array_equal(one_per_tile.view(np.uint32), default.view(np.uint32))
    if policy == "bf16":
        assert np.array_equal(default.view(np.uint32), bf16_run["prefill"].view(np.uint32))


@pytest.mark.parametrize("policy", ["fp8", "fp4"])
def test_full_size_quantized_policies(policy, bf16_run):
    g = host.Gemma(policy, max_seq=T + 16, max_prefill=T, seed=1234)
    pre = g.prefill(TOKS)
    g.set_resident_prefill_weights(False)                     # the reference's per-forward staging
    pre_staged = g.prefill(TOKS)
    assert np.all(np.isfinite(pre)) and np.array_equal(pre.view(np.uint32), pre_staged.view(np.uint32))
    nxt = bf16_run["next"]
    d = {m: g.decode(nxt, T, m) for m in ("reference", "fused", "graph")}
    assert np.array_equal(d["reference"].view(np.uint32), d["fused"].view(np.uint32))
    assert np.array_equal(d["reference"].view(np.uint32), d["graph"].view(np.uint32))
    g.close()
