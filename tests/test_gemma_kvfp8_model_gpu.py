"""The Gemma model over the FP8 KV cache (GemmaConfig::kv_fp8: PerChannelKvFp8<> on every layer) on tests/test_gemma_conditioned_gpu.py's conditioned 12-layer model.

The oracle is tests/ref_gemma_kvfp8.py: RefGemma whose appended K / V rows come back as bf16(e4m3 * scale).  The bar is max(1e-3, 2 x the distance between that oracle
and its float32-norm twin on the CPU model), capped at 3e-3, the project's bar for paths that re-quantize to e4m3.  Measured CPU distance: 1.62e-3 (tests/
test_gemma_kvfp8_cpu.py), so the bar is the cap, 3e-3.  Measured GPU error against the oracle (max |logit - oracle| / max |oracle|, MI355X; bf16 / fp8 weights):
decode, worst of 20 positions 1.04e-3 / 1.04e-3; prefill T = 20 9.8e-4 / 9.6e-4; a decode on the prefilled caches 9.5e-4 / 1.01e-3; chunked prefill (8 + 8 + 4) and
the decode behind it the same figures (EXPERIMENTS.md section 11).

Paths that must agree bit for bit do: reference-order / fused / graph decode, fused / per-op prefill, a rewound model and a fresh one."""
import numpy as np
import pytest

import ref_gemma_kvfp8 as rk
from mila_amd import capi, host
from ref_gemma import CONDITIONED_PROFILE
from test_gemma_conditioned_gpu import CFG, MAX_SEQ, TOKENS, _report

pytestmark = pytest.mark.gpu

POLICIES = ["bf16", "fp8"]


@pytest.fixture(scope="module")
def bar():
    b = rk.gpu_bar()
    print("CPU distance %.3e -> GPU bar %.1e" % (rk.cpu_distance(), b))
    return b


_ORACLES = {}


def _oracle(policy, staged_prefill):
    """one oracle per weight policy for the whole module (building it quantizes every weight on the host); forward() at position 0 starts its K / V history afresh.
    staged_prefill: the T > 1 arithmetic of a quantized weight policy (tests/ref_gemma.py), as tests/test_gemma_conditioned_gpu.py sets it for its prefill legs"""
    if policy not in _ORACLES:
        _ORACLES[policy] = rk.RefGemmaKvFp8(CFG, policy, seed=7, profile=CONDITIONED_PROFILE)
    _ORACLES[policy].staged_prefill = staged_prefill
    return _ORACLES[policy]


def _model(policy, kv_fp8=True, max_prefill=1, cfg=CFG, max_seq=MAX_SEQ, profile=CONDITIONED_PROFILE):
    return host.Gemma(policy, cfg, max_seq=max_seq, max_prefill=max_prefill, seed=7, profile=profile, kv_fp8=kv_fp8)


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("policy", POLICIES)
def test_decode_reference_fused_and_graph_agree_bit_for_bit_and_with_the_oracle(policy, bar):
    ref = _oracle(policy, staged_prefill=False)
    g = {m: _model(policy) for m in ("reference", "fused", "graph")}
    worst = 0.0
    for pos, tok in enumerate(TOKENS):
        exp = ref.forward([tok], pos, MAX_SEQ)
        out = {m: mdl.decode(tok, pos, m) for m, mdl in g.items()}
        assert _same(out["reference"], out["fused"]), "fused != reference order at %d" % pos
        assert _same(out["reference"], out["graph"]), "graph replay != reference order at %d" % pos
        assert np.all(np.isfinite(out["graph"]))
        if pos in (0, 7, 8, 9, len(TOKENS) - 1):
            worst = max(worst, _report("kv-fp8 %s decode @%d" % (policy, pos), out["graph"], exp))
        else:
            worst = max(worst, float(np.abs(out["graph"] - exp).max() / np.abs(exp).max()))
    print("kv-fp8 %s decode: worst %.3e (bar %.1e)" % (policy, worst, bar))
    for mdl in g.values():
        mdl.close()
    assert worst <= bar, worst


@pytest.mark.parametrize("policy", POLICIES)
def test_prefill_fused_and_per_op_agree_bit_for_bit_and_with_the_oracle(policy, bar):
    refp = _oracle(policy, staged_prefill=True)
    exp = refp.forward(TOKENS, 0, MAX_SEQ)
    exp1 = refp.forward([5], len(TOKENS), MAX_SEQ)
    p = _model(policy, max_prefill=32)
    got = p.prefill(TOKENS)
    p.set_fused_prefill(False)
    per_op = p.prefill(TOKENS)
    assert _same(got, per_op), "fused prefill != one launch per reference op"
    errs = [_report("kv-fp8 %s prefill T=%d" % (policy, len(TOKENS)), got, exp),
            _report("kv-fp8 %s decode after prefill" % policy, p.decode(5, len(TOKENS), "fused"), exp1)]
    p.close()
    # the same prompt in chunks of 8 (8 + 8 + 4: the later chunks attend through the cache), then a decode
    c = _model(policy, max_prefill=8)
    errs.append(_report("kv-fp8 %s chunked prefill (8)" % policy, c.prefill_from(TOKENS, 0), exp))
    errs.append(_report("kv-fp8 %s decode after chunked prefill" % policy, c.decode(5, len(TOKENS), "fused"), exp1))
    c.close()
    assert max(errs) <= bar, errs


def test_the_switch_changes_the_logits_the_footprint_and_the_launch_count():
    on, off = _model("bf16", max_prefill=32), _model("bf16", kv_fp8=False, max_prefill=32)
    try:
        a, b = on.prefill(TOKENS), off.prefill(TOKENS)
        assert np.abs(a - b).max() > 0.0, "kv_fp8 is ignored"
        son, soff = on.memory_stats(), off.memory_stats()
        assert son["required"] == son["actual"] and soff["required"] == soff["actual"]
        saved = 0
        for i in range(CFG["num_layers"]):
            glb = (i + 1) % CFG["sliding_window_pattern"] == 0
            hs, nkv = (CFG["global_head_dim"], CFG["num_global_kv_heads"]) if glb else (CFG["head_dim"], CFG["num_kv_heads"])
            saved += 2 * nkv * MAX_SEQ * (hs - 4)                                    # 2 bytes -> 1 byte per element, + one fp32 scale per row, K and V
        assert soff["actual"]["device_state_bytes"] - son["actual"]["device_state_bytes"] == saved
        assert soff["actual"]["device_parameter_bytes"] == son["actual"]["device_parameter_bytes"]
        # one launch more per layer on the graph path: append and attention are two nodes (nothing splits at 64 keys: no combine nodes on either side)
        on.decode(5, len(TOKENS), "graph")
        off.decode(5, len(TOKENS), "graph")
        assert capi.attn_decode_kvfp8_plan(1, CFG["num_heads"], CFG["num_global_kv_heads"], CFG["global_head_dim"], MAX_SEQ, 0, MAX_SEQ)["splits"] == 1
        assert on.graph_node_count() == off.graph_node_count() + CFG["num_layers"]
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_a_rewound_model_continues_like_a_fresh_one(policy):
    other = [(11 * i + 5) % CFG["vocab_size"] for i in range(4)]
    a, b = _model(policy), _model(policy)
    try:
        for pos, tok in enumerate(TOKENS):
            a.decode(tok, pos, "fused")
        assert a.rewind(10)
        for pos, tok in enumerate(TOKENS[:10]):
            b.decode(tok, pos, "fused")
        for i, tok in enumerate(other):
            mode = ("fused", "reference")[i % 2]
            assert _same(a.decode(tok, 10 + i, mode), b.decode(tok, 10 + i, mode)), "position %d" % (10 + i)
    finally:
        a.close()
        b.close()


def test_the_graph_is_recaptured_at_the_band_bucket_where_the_global_layer_takes_the_matrix_cores():
    """a local layer (HS 256, 16 / 8 heads) and a global one (HS 512, 16 / 1): positions 4094 .. 4098 cross the 4096-key bucket; from there the captured global-layer
    launch is the 8192-key bucket's, the matrix-core form"""
    cfg = dict(vocab_size=2048, embedding_dim=1280, num_layers=2, num_heads=16, num_kv_heads=8, head_dim=256, hidden_dim=2560, global_head_dim=512,
               num_global_kv_heads=1, window=1024, sliding_window_pattern=2, global_rotary_dim=128)
    max_seq, T = 8192, 4094
    prompt = [(7 * i + 3) % 2048 for i in range(T)]
    bucket = capi.load().mila_cdna4_attn_decode_band_bucket
    assert [bucket(n, max_seq) for n in (4095, 4096, 4097, 4099)] == [4096, 4096, 8192, 8192]
    assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, max_seq, 0, 8192)["form"] == "attn_decode_kvfp8_mfma"
    assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, max_seq, 0, 4096)["form"] == "attn_decode_kvfp8"
    g, r = (_model("bf16", max_prefill=2048, cfg=cfg, max_seq=max_seq, profile=CONDITIONED_PROFILE) for _ in range(2))
    try:
        assert _same(g.prefill_from(prompt, 0), r.prefill_from(prompt, 0))
        for i in range(5):
            tok, pos = (13 * i + 1) % 2048, T + i
            assert _same(g.decode(tok, pos, "graph"), r.decode(tok, pos, "reference")), "graph replay != reference order at %d" % pos
            assert g.graph_capture_count() == (1 if pos + 1 <= 4096 else 2), pos
    finally:
        g.close()
        r.close()


def test_rejected_combinations_raise_value_error():
    with pytest.raises(ValueError, match="bounded_local_kv"):
        host.Gemma("bf16", dict(CFG, bounded_local_kv=1), max_seq=MAX_SEQ, max_prefill=8, seed=7, kv_fp8=True)
    with pytest.raises(ValueError, match="64, 128, 256 or 512"):
        host.Gemma("bf16", dict(CFG, head_dim=32), max_seq=MAX_SEQ, max_prefill=8, seed=7, kv_fp8=True)
    g = _model("bf16", max_prefill=8)
    try:
        with pytest.raises(ValueError, match="kv_fp8"):
            g.set_prefill_overlap(True)
        g.set_prefill_overlap(False)
    finally:
        g.close()


def test_the_model_entries_take_the_switch():
    """GemmaModel (GemmaModelConfig::withKvFp8 through fromSynthetic): greedy generate() -- chunked prefill, then the captured graph with the sampler as its last node --
    emits the tokens a GemmaTransformer with kv_fp8 yields by prefill + graph decode + argmax; and the switch does arrive: with bounded_local_kv it is rejected"""
    prompt, n = TOKENS[:12], 6
    g = _model("bf16", max_prefill=16)
    m = host.GemmaModel.synthetic("bf16", CFG, context=MAX_SEQ, prefill_chunk=16, seed=7, profile=CONDITIONED_PROFILE, kv_fp8=True)
    try:
        exp = [int(np.argmax(g.prefill(prompt)))]
        for i in range(n - 1):
            exp.append(int(np.argmax(g.decode(exp[-1], len(prompt) + i, "graph"))))
        got, status, _ = m.generate(prompt, max_new_tokens=n, stop_tokens=[CFG["vocab_size"] - 1])
        assert status == "length" and got == exp, (status, got, exp)
    finally:
        g.close()
        m.close()
    with pytest.raises(ValueError, match="bounded_local_kv"):
        host.GemmaModel.synthetic("bf16", dict(CFG, bounded_local_kv=1), context=MAX_SEQ, prefill_chunk=16, seed=7, kv_fp8=True)
