"""CPU-only: the bounded sliding-window KV cache under batched rows at its two boundaries.  GemmaConfig::validate() with bounded_local_kv_rows
(host.validate_gemma_config; tests/cpp/gemma_ring_rows_traits.cpp) -- what the switch admits and what it refuses, with the messages -- and the band fork entry
(kv_rows_fork_layers_band_bf16): declared, exported, bound, and every refusal of its host-side validation, which is decided from host-known values before any device call
-- every device address here is a dummy that is never dereferenced (tests/test_kv_rows_fork_layers_cpu.py shows the pattern)."""
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
RING = dict(K=4096, V=8192, NKV=2, capacity=11, HS=64, window=8)       # a ring layer and a flat one, as the small model has them
FLAT = dict(K=16384, V=32768, NKV=1, capacity=64, HS=128, window=0)
GOOD = dict(layers=[RING, FLAT, RING], rows=4, src=1, dst_mask=0b1101, len=24)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


# ---- the configuration ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2, 3, 4])
def test_the_switch_admits_every_batch_size(lib, b):
    host.validate_gemma_config(SMALL, b, 0, bounded_local_kv_rows=True)
    host.validate_gemma_config(dict(SMALL, bounded_local_kv=1), b, 0, bounded_local_kv_rows=True)      # the switch implies the policy: naming both is the same configuration


def test_plain_bounded_local_kv_keeps_its_refusal_and_the_switch_has_its_own(lib):
    with pytest.raises(ValueError, match=r"max_batch > 1 cannot be combined with bounded_local_kv \(the ring needs a rewind rule per row\)"):
        host.validate_gemma_config(dict(SMALL, bounded_local_kv=1), 2, 0)
    host.validate_gemma_config(dict(SMALL, bounded_local_kv=1), 1, 0)
    with pytest.raises(ValueError, match=r"bounded_local_kv_rows cannot be combined with kv_fp8 \(the FP8 KV cache is unbounded; FP8 rings are not built\)"):
        host.validate_gemma_config(SMALL, 1, 0, kv_fp8=True, bounded_local_kv_rows=True)
    with pytest.raises(ValueError, match=r"bounded_local_kv_rows cannot be combined with kv_fp8"):
        host.validate_gemma_config(SMALL, 2, 0, kv_fp8_rows=True, bounded_local_kv_rows=True)
    with pytest.raises(ValueError, match=r"bounded_local_kv_rows cannot be combined with draft_tokens > 0 \(rejected drafts leave stale rows"):
        host.validate_gemma_config(SMALL, 1, 2, bounded_local_kv_rows=True)
    for w in (0, -3):
        with pytest.raises(ValueError, match=r"bounded_local_kv_rows needs a sliding window \(window %d\)" % w):
            host.validate_gemma_config(dict(SMALL, window=w), 2, 0, bounded_local_kv_rows=True)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="outside 1 .. 4"):
            host.validate_gemma_config(SMALL, bad, 0, bounded_local_kv_rows=True)


def test_the_python_surface_and_the_runner_entries(lib):
    assert inspect.signature(host.Gemma.__init__).parameters["bounded_local_kv_rows"].default is False
    assert inspect.signature(host.GemmaModel.synthetic).parameters["bounded_local_kv_rows"].default is False
    assert inspect.signature(host.validate_gemma_config).parameters["bounded_local_kv_rows"].default is False
    names = [n for n, _ in host.GemmaConfigC._fields_]
    assert names[-2:] == ["bounded_local_kv", "kv_fp8"]      # mila_gemma_config is unchanged: the switch travels through the _ring entries
    h = host.load()
    for n in ("validate_config_ring", "create_rows_ring", "model_synthetic_rows_ring"):
        assert hasattr(h, "mila_gemma_" + n), n
    for make in (host.Gemma, host.GemmaModel.synthetic):      # refused before the library is asked to build anything
        with pytest.raises(ValueError, match="bounded_local_kv_rows"):
            make("bf16", SMALL, max_batch=2, kv_fp8_rows=True, bounded_local_kv_rows=True)
        with pytest.raises(ValueError, match="bounded_local_kv_rows"):
            make("bf16", SMALL, draft_tokens=1, bounded_local_kv_rows=True)


def test_the_traits_program(tmp_path):
    """tests/cpp/gemma_ring_rows_traits.cpp, compiled with the host flags and RUN (host code only, no device call)"""
    src = os.path.join(ROOT, "tests", "cpp", "gemma_ring_rows_traits.cpp")
    exe = str(tmp_path / "gemma_ring_rows_traits")
    libdir = os.path.dirname(capi.LIB_PATH)
    flags = [f for f in build.HOST_FLAGS if f not in ("-fPIC", "-fvisibility=hidden")]
    p = subprocess.run([build.HOSTCXX] + flags + [src, "-o", exe, "-L" + libdir, "-lmila_cdna4", "-L/opt/rocm/lib", "-lamdhip64", "-lrocprofiler-sdk-roctx",
                                                  "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ring rows traits OK" in r.stdout, r.stdout


# ---- the band fork entry at the drop-in boundary ---------------------------------------------------------------------------------------------------------------
def _table(layers):
    t = (capi.KvForkLayerBand * max(len(layers), 1))()
    for i, l in enumerate(layers):
        t[i].K, t[i].V, t[i].NKV, t[i].capacity, t[i].HS, t[i].window = l["K"], l["V"], l["NKV"], l["capacity"], l["HS"], l["window"]
    return t


def _fork(lib, layer=None, at=1, **change):
    a = dict(GOOD, **change)
    layers = [dict(l) for l in a["layers"]]
    if layer:
        layers[at].update(layer)
    n = a.get("n_layers", len(layers))
    table = None if a.get("null_table") else _table(layers)
    rc = lib.mila_cdna4_kv_rows_fork_layers_band_bf16(table, n, a["rows"], a["src"], a["dst_mask"], a["len"], None)
    return rc, lib.mila_cdna4_last_error().decode()


def test_the_entry_and_its_record_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    assert re.search(r"MILA_API\s+int\s+mila_cdna4_kv_rows_fork_layers_band_bf16\s*\(\s*const\s+mila_kv_fork_layer_band\s*\*", text)
    assert "kv_rows_fork_layers_band_bf16" in capi.EXPORTED and hasattr(lib, "mila_cdna4_kv_rows_fork_layers_band_bf16")
    assert lib.mila_cdna4_abi_version() == 4      # additive
    assert C.sizeof(capi.KvForkLayerBand) == 32   # two pointers, four 32-bit words: the header's record


def test_the_header_still_compiles_as_c_and_the_record_has_the_bound_layout(tmp_path):
    src = tmp_path / "record.c"
    src.write_text('#include <stddef.h>\n#include "mila_cdna4.h"\n'
                   "typedef char size_is_32[sizeof(mila_kv_fork_layer_band) == 32 ? 1 : -1];\n"
                   "typedef char v_at_8[offsetof(mila_kv_fork_layer_band, V) == 8 ? 1 : -1];\n"
                   "typedef char nkv_at_16[offsetof(mila_kv_fork_layer_band, NKV) == 16 ? 1 : -1];\n"
                   "typedef char hs_at_24[offsetof(mila_kv_fork_layer_band, HS) == 24 ? 1 : -1];\n"
                   "typedef char window_at_28[offsetof(mila_kv_fork_layer_band, window) == 28 ? 1 : -1];\n"
                   "int (*entry)(const mila_kv_fork_layer_band*, int, int, int, unsigned, int, mila_stream_t) = mila_cdna4_kv_rows_fork_layers_band_bf16;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


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
    (dict(len=65), "layer 1: band=65 of len=65 (window 0) above capacity 64"),      # a flat layer with len > capacity; the rings take any len
    (dict(layer=dict(capacity=23)), "layer 1: band=24"),
    (dict(layer=dict(window=12), at=0), "layer 0: band=12 of len=24 (window 12) above capacity 11"),      # a ring whose window exceeds its capacity
    (dict(layer=dict(window=-1), at=2), "layer 2: window=-1"),
    (dict(layer=dict(K=None)), "layer 1: null pointer"),
    (dict(layer=dict(V=None), at=2), "layer 2: null pointer"),
    (dict(layer=dict(HS=60)), "layer 1: HS=60"),
    (dict(layer=dict(HS=4)), "layer 1: HS=4"),
    (dict(layer=dict(HS=0)), "layer 1: bad sizes"),
    (dict(layer=dict(NKV=0), at=0), "layer 0: bad sizes"),
    (dict(layer=dict(capacity=0)), "layer 1: bad sizes"),
    (dict(layer=dict(K=16386)), "layer 1: K and V must be 16-byte aligned"),
    (dict(layer=dict(V=8200), at=2), "layer 2: K and V must be 16-byte aligned"),
])
def test_every_refusal_comes_before_any_device_work(lib, change, telling):
    rc, err = _fork(lib, **change)
    assert rc == INV and "kv_rows_fork_layers_band_bf16" in err and telling in err, (change, rc, err)


def test_a_table_of_more_layers_than_one_launch_is_checked_to_its_end(lib):
    """the records travel 64 to a launch: the check still covers every one before the first launch"""
    bad = [dict(RING) for _ in range(70)]
    bad[69]["HS"] = 12
    rc, err = _fork(lib, layers=bad)
    assert rc == INV and "layer 69: HS=12" in err, (rc, err)
