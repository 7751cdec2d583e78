"""CPU-only: the FP8 KV cache under batched rows at its two boundaries.  GemmaConfig::validate() with kv_fp8_rows (host.validate_gemma_config) -- what the switch admits
and what it still refuses, with today's messages -- and the three kernel entries (fused_qkv_post_kvfp8_rows_devpos, attn_decode_kvfp8_rows, kv_rows_fork_layers_kvfp8):
declared, exported, bound, and every refusal of their host-side validation, which is decided from host-known values before any device call -- every device address
here is a dummy that is never dereferenced (tests/test_kv_rows_fork_layers_cpu.py shows the pattern)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from mila_amd import build, capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = capi.MILA_E_INVALID_ARGUMENT
SMALL = dict(vocab_size=1024, embedding_dim=256, num_layers=6, num_heads=4, num_kv_heads=2, head_dim=64, hidden_dim=512, global_head_dim=128, num_global_kv_heads=1, window=8,
             sliding_window_pattern=6, global_rotary_dim=32)      # the geometry of tests/test_gemma_host_gpu.py (a GPU module: not imported here)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


# ---- the configuration ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2, 3, 4])
def test_the_switch_admits_every_batch_size(lib, b):
    host.validate_gemma_config(SMALL, b, 0, kv_fp8_rows=True)


def test_plain_kv_fp8_keeps_its_refusal_and_the_switch_keeps_the_other_three(lib):
    with pytest.raises(ValueError, match=r"max_batch > 1 cannot be combined with kv_fp8 \(the FP8 KV cache's fused append is B = 1\)"):
        host.validate_gemma_config(SMALL, 2, 0, kv_fp8=True)
    host.validate_gemma_config(SMALL, 2, 0, kv_fp8=True, kv_fp8_rows=True)      # the switch implies the policy: naming both is the same configuration
    with pytest.raises(ValueError, match=r"draft_tokens > 0 cannot be combined with kv_fp8 \(the FP8 KV cache's fused append is B = 1; the chain over it is not built\)"):
        host.validate_gemma_config(SMALL, 1, 1, kv_fp8_rows=True)
    with pytest.raises(ValueError, match=r"draft_tokens > 0 cannot be combined with max_batch > 1"):
        host.validate_gemma_config(SMALL, 2, 1, kv_fp8_rows=True)
    with pytest.raises(ValueError, match=r"kv_fp8 cannot be combined with bounded_local_kv \(the FP8 KV cache is unbounded\)"):
        host.validate_gemma_config(dict(SMALL, bounded_local_kv=1), 1, 0, kv_fp8_rows=True)
    with pytest.raises(ValueError, match=r"max_batch > 1 cannot be combined with bounded_local_kv \(the ring needs a rewind rule per row\)"):      # (the rows' own refusal comes first)
        host.validate_gemma_config(dict(SMALL, bounded_local_kv=1), 3, 0, kv_fp8_rows=True)
    for b in (1, 3):
        with pytest.raises(ValueError, match=r"kv_fp8 needs head dimensions of 64, 128, 256 or 512 \(head_dim 32, global_head_dim 128\)"):
            host.validate_gemma_config(dict(SMALL, head_dim=32), b, 0, kv_fp8_rows=True)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="outside 1 .. 4"):
            host.validate_gemma_config(SMALL, bad, 0, kv_fp8_rows=True)


def test_the_python_surface():
    assert inspect.signature(host.Gemma.__init__).parameters["kv_fp8_rows"].default is False
    assert inspect.signature(host.GemmaModel.synthetic).parameters["kv_fp8_rows"].default is False
    assert inspect.signature(host.validate_gemma_config).parameters["kv_fp8_rows"].default is False


# ---- the three entries at the drop-in boundary ----------------------------------------------------------------------------------------------------------------
def test_the_entries_and_the_record_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    assert re.search(r"MILA_API\s+int\s+mila_cdna4_kv_rows_fork_layers_kvfp8\s*\(\s*const\s+mila_kv_fork_layer_fp8\s*\*", text)
    for name in ("fused_qkv_post_kvfp8_rows_devpos", "attn_decode_kvfp8_rows", "kv_rows_fork_layers_kvfp8"):
        assert re.search(r"MILA_API\s+int\s+mila_cdna4_%s\s*\(" % name, text), name
        assert name in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + name), name
    assert lib.mila_cdna4_abi_version() == 4      # additive
    assert C.sizeof(capi.KvForkLayerFp8) == 48    # four pointers, four 32-bit words: the header's record


def test_the_header_still_compiles_as_c_and_the_record_has_the_bound_layout(tmp_path):
    src = tmp_path / "record.c"
    src.write_text('#include <stddef.h>\n#include "mila_cdna4.h"\n'
                   "typedef char size_is_48[sizeof(mila_kv_fork_layer_fp8) == 48 ? 1 : -1];\n"
                   "typedef char v8_at_8[offsetof(mila_kv_fork_layer_fp8, V8) == 8 ? 1 : -1];\n"
                   "typedef char vs_at_24[offsetof(mila_kv_fork_layer_fp8, Vs) == 24 ? 1 : -1];\n"
                   "typedef char nkv_at_32[offsetof(mila_kv_fork_layer_fp8, NKV) == 32 ? 1 : -1];\n"
                   "typedef char hs_at_40[offsetof(mila_kv_fork_layer_fp8, HS) == 40 ? 1 : -1];\n"
                   "int (*fork)(const mila_kv_fork_layer_fp8*, int, int, int, unsigned, int, mila_stream_t) = mila_cdna4_kv_rows_fork_layers_kvfp8;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


# ---- (a) the append -------------------------------------------------------------------------------------------------------------------------------------------
POST_PTRS = ["q_out", "K8", "V8", "Ks", "Vs", "q", "k", "v_src", "qw", "kw", "vw", "cos", "sin", "positions"]
POST = dict({n: 4096 * (i + 1) for i, n in enumerate(POST_PTRS)}, stride=512, B=3, NH=4, NKV=2, HS=64, capacity=40)


def _post(lib, **change):
    a = dict(POST, **change)
    rc = lib.mila_cdna4_fused_qkv_post_kvfp8_rows_devpos(a["q_out"], a["K8"], a["V8"], a["Ks"], a["Vs"], a["q"], a["k"], a["v_src"], a["stride"], a["qw"], a["kw"], a["vw"], a["cos"],
                                                         a["sin"], a["B"], a["NH"], a["NKV"], a["HS"], a["positions"], a["capacity"], 1e-6, None)
    return rc, lib.mila_cdna4_last_error().decode()


@pytest.mark.parametrize("change, telling", [(dict([(n, None)]), "null pointer") for n in POST_PTRS if n != "vw"] + [
    (dict(B=1), "B=1"), (dict(B=0), "B=0"), (dict(B=5), "B=5"), (dict(B=-2), "B=-2"),
    (dict(HS=32), "HS=32"), (dict(HS=96), "HS=96"), (dict(HS=1024), "HS=1024"), (dict(HS=0), "HS=0"),
    (dict(stride=516), "row stride 516"), (dict(stride=-8), "row stride -8"), (dict(stride=0), "row stride 0"),
    (dict(capacity=0), "capacity=0"), (dict(capacity=-40), "capacity=-40"),
    (dict(NH=0), "bad sizes"), (dict(NKV=0), "bad sizes"),
])
def test_the_append_refuses_before_any_device_work(lib, change, telling):
    rc, err = _post(lib, **change)
    assert rc == INV and "fused_qkv_post_kvfp8_rows_devpos" in err and telling in err, (change, rc, err)


# ---- (b) the decode -------------------------------------------------------------------------------------------------------------------------------------------
DEC_PTRS = ["Y", "Q", "K8", "V8", "Ks", "Vs", "positions"]
DEC = dict({n: 4096 * (i + 1) for i, n in enumerate(DEC_PTRS)}, scratch=65536, scratch_bytes=1 << 30, B=2, NH=4, NKV=2, HS=64, capacity=400, max_len=300, window=0)


def _dec(lib, **change):
    a = dict(DEC, **change)
    rc = lib.mila_cdna4_attn_decode_kvfp8_rows(a["Y"], a["Q"], a["K8"], a["V8"], a["Ks"], a["Vs"], a["scratch"], C.c_size_t(a["scratch_bytes"]), a["B"], a["NH"], a["NKV"], a["HS"],
                                               a["capacity"], a["positions"], a["max_len"], a["window"], 0.125, None)
    return rc, lib.mila_cdna4_last_error().decode()


@pytest.mark.parametrize("change, telling", [(dict([(n, None)]), "null pointer") for n in DEC_PTRS] + [
    (dict(B=1), "B=1"), (dict(B=5), "B=5"), (dict(B=0), "B=0"),
    (dict(HS=32), "HS=32"), (dict(HS=1024), "HS=1024"),
    (dict(NH=3), "bad head counts"), (dict(NH=6, NKV=2), "group size 3"),
    (dict(capacity=0, max_len=0), "must be positive"), (dict(max_len=0), "must be positive"), (dict(max_len=401), "max_len 401"),
    (dict(window=-1), "negative window"),
    (dict(scratch_bytes=16), "scratch 16 bytes"), (dict(scratch=None), "scratch"),
])
def test_the_decode_refuses_before_any_device_work(lib, change, telling):
    assert capi.attn_decode_kvfp8_plan(1, DEC["NH"], DEC["NKV"], DEC["HS"], DEC["capacity"], 0, DEC["max_len"])["splits"] > 1      # (so that the scratch is asked for)
    rc, err = _dec(lib, **change)
    assert rc == INV and "attn_decode_kvfp8_rows" in err and telling in err, (change, rc, err)


def test_the_rows_scratch_is_the_one_row_plan_times_the_rows(lib):
    """the plan is ONE row's; the partials are sized for all of them: B times the one-row plan's need passes the check, one byte less does not"""
    need = capi.attn_decode_kvfp8_plan(1, DEC["NH"], DEC["NKV"], DEC["HS"], DEC["capacity"], 0, DEC["max_len"])["scratch_need"]
    assert need > 0
    for B in (2, 3, 4):
        rc, err = _dec(lib, B=B, scratch_bytes=B * need - 1)
        assert rc == INV and "required %d" % (B * need) in err, (B, rc, err)
        assert lib.mila_cdna4_attn_decode_scratch_bytes(B, DEC["NH"], DEC["HS"]) >= B * need


# ---- (c) the fork ---------------------------------------------------------------------------------------------------------------------------------------------
A = dict(K8=4096, V8=8192, Ks=12288, Vs=16388, NKV=2, capacity=24, HS=64)       # (Vs on a 4-byte boundary that is no 16-byte one: allowed)
B_ = dict(K8=16384, V8=32768, Ks=49156, Vs=65536, NKV=1, capacity=40, HS=128)
GOOD = dict(layers=[A, B_, A], rows=4, src=1, dst_mask=0b1101, len=24)


def _table(layers):
    t = (capi.KvForkLayerFp8 * max(len(layers), 1))()
    for i, l in enumerate(layers):
        t[i].K8, t[i].V8, t[i].Ks, t[i].Vs, t[i].NKV, t[i].capacity, t[i].HS, t[i].reserved = l["K8"], l["V8"], l["Ks"], l["Vs"], l["NKV"], l["capacity"], l["HS"], 0
    return t


def _fork(lib, layer=None, at=1, **change):
    a = dict(GOOD, **change)
    layers = [dict(l) for l in a["layers"]]
    if layer:
        layers[at].update(layer)
    n = a.get("n_layers", len(layers))
    table = None if a.get("null_table") else _table(layers)
    rc = lib.mila_cdna4_kv_rows_fork_layers_kvfp8(table, n, a["rows"], a["src"], a["dst_mask"], a["len"], None)
    return rc, lib.mila_cdna4_last_error().decode()


@pytest.mark.parametrize("change, telling", [
    (dict(null_table=True), "null layer table"),
    (dict(n_layers=0), "n_layers=0"),
    (dict(n_layers=-2), "n_layers=-2"),
    (dict(rows=1), "rows=1"),
    (dict(rows=5, dst_mask=0b10001), "rows=5"),
    (dict(src=-1), "src=-1"),
    (dict(src=4), "src=4"),
    (dict(dst_mask=0), "empty dst_mask"),
    (dict(dst_mask=0b0010), "names the source row 1"),
    (dict(dst_mask=0b0111), "names the source row 1"),
    (dict(dst_mask=0b10001), "names a row outside the 4 rows"),
    (dict(rows=2, src=0, dst_mask=0b0100), "names a row outside the 2 rows"),
    (dict(len=0), "len=0"),
    (dict(len=-3), "len=-3"),
    (dict(len=25), "layer 0: len=25"),                       # above the SMALLEST capacity, though layer 1 would hold it
    (dict(len=41), "layer 0: len=41"),
    (dict(layer=dict(capacity=23)), "layer 1: len=24"),
    (dict(layer=dict(K8=None)), "layer 1: null pointer"),
    (dict(layer=dict(V8=None), at=2), "layer 2: null pointer"),
    (dict(layer=dict(Ks=None), at=0), "layer 0: null pointer"),
    (dict(layer=dict(Vs=None)), "layer 1: null pointer"),
    (dict(layer=dict(HS=72)), "layer 1: HS=72"),             # a multiple of 8 (the bf16 entry's unit), not of 16
    (dict(layer=dict(HS=8)), "layer 1: HS=8"),
    (dict(layer=dict(HS=0)), "layer 1: bad sizes"),
    (dict(layer=dict(NKV=0), at=0), "layer 0: bad sizes"),
    (dict(layer=dict(capacity=0)), "layer 1: bad sizes"),
    (dict(layer=dict(K8=16392)), "layer 1: K8 and V8 must be 16-byte aligned"),
    (dict(layer=dict(V8=8196), at=2), "layer 2: K8 and V8 must be 16-byte aligned"),
    (dict(layer=dict(Ks=49158)), "layer 1: Ks and Vs must be 4-byte aligned"),
    (dict(layer=dict(Vs=16389), at=0), "layer 0: Ks and Vs must be 4-byte aligned"),
])
def test_the_fork_refuses_before_any_device_work(lib, change, telling):
    rc, err = _fork(lib, **change)
    assert rc == INV and "kv_rows_fork_layers_kvfp8" in err and telling in err, (change, rc, err)


def test_a_table_of_more_layers_than_one_launch_is_checked_to_its_end(lib):
    bad = [dict(A) for _ in range(70)]
    bad[69]["HS"] = 24
    rc, err = _fork(lib, layers=bad)
    assert rc == INV and "layer 69: HS=24" in err, (rc, err)
