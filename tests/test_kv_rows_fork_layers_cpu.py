"""CPU-only: mila_cdna4_kv_rows_fork_layers_bf16 at the drop-in boundary -- declared with its record type, exported, bound -- and every refusal of its host-side
validation, which is decided from host-known values before any device call: the cache addresses in the records are dummies that are never dereferenced
(tests/test_kv_rows_fork_cpu.py shows the pattern for the one-layer entry).  The refusals of GemmaTransformer::forkRowPrefix need a built model, i.e. a device: they
are in tests/test_gemma_prefix_cache_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = capi.MILA_E_INVALID_ARGUMENT
A = dict(K=4096, V=8192, NKV=2, capacity=24, HS=64)       # the two layer kinds of the small model, at unequal capacities
B = dict(K=16384, V=32768, NKV=1, capacity=40, HS=128)
GOOD = dict(layers=[A, B, A], rows=4, src=1, dst_mask=0b1101, len=24)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def _table(layers):
    t = (capi.KvForkLayer * max(len(layers), 1))()
    for i, l in enumerate(layers):
        t[i].K, t[i].V, t[i].NKV, t[i].capacity, t[i].HS, t[i].reserved = l["K"], l["V"], l["NKV"], l["capacity"], l["HS"], 0
    return t


def _fork(lib, layer=None, at=1, **change):
    a = dict(GOOD, **change)
    layers = [dict(l) for l in a["layers"]]
    if layer:
        layers[at].update(layer)
    n = a.get("n_layers", len(layers))
    table = None if a.get("null_table") else _table(layers)
    rc = lib.mila_cdna4_kv_rows_fork_layers_bf16(table, n, a["rows"], a["src"], a["dst_mask"], a["len"], None)
    return rc, lib.mila_cdna4_last_error().decode()


def test_the_entry_and_its_record_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    assert re.search(r"MILA_API\s+int\s+mila_cdna4_kv_rows_fork_layers_bf16\s*\(\s*const\s+mila_kv_fork_layer\s*\*", text)
    assert "kv_rows_fork_layers_bf16" in capi.EXPORTED and hasattr(lib, "mila_cdna4_kv_rows_fork_layers_bf16")
    assert lib.mila_cdna4_abi_version() == 4      # additive
    assert C.sizeof(capi.KvForkLayer) == 32       # two pointers, four 32-bit words: the header's record


def test_the_header_still_compiles_as_c_and_the_record_has_the_bound_layout(tmp_path):
    src = tmp_path / "record.c"
    src.write_text('#include <stddef.h>\n#include "mila_cdna4.h"\n'
                   "typedef char size_is_32[sizeof(mila_kv_fork_layer) == 32 ? 1 : -1];\n"
                   "typedef char v_at_8[offsetof(mila_kv_fork_layer, V) == 8 ? 1 : -1];\n"
                   "typedef char nkv_at_16[offsetof(mila_kv_fork_layer, NKV) == 16 ? 1 : -1];\n"
                   "typedef char hs_at_24[offsetof(mila_kv_fork_layer, HS) == 24 ? 1 : -1];\n"
                   "int (*entry)(const mila_kv_fork_layer*, int, int, int, unsigned, int, mila_stream_t) = mila_cdna4_kv_rows_fork_layers_bf16;\n")
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
    (dict(len=25), "layer 0: len=25"),                       # above the SMALLEST capacity, though layer 1 would hold it
    (dict(len=41), "layer 0: len=41"),
    (dict(layer=dict(capacity=23)), "layer 1: len=24"),
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
    assert rc == INV and "kv_rows_fork_layers_bf16" in err and telling in err, (change, rc, err)


def test_a_table_of_more_layers_than_one_launch_is_checked_to_its_end(lib):
    """the records travel 64 to a launch: the check still covers every one before the first launch"""
    layers = [A] * 70
    bad = [dict(l) for l in layers]
    bad[69]["HS"] = 12
    rc, err = _fork(lib, layers=bad)
    assert rc == INV and "layer 69: HS=12" in err, (rc, err)


def test_the_python_surface():
    import inspect

    from mila_amd import host
    assert list(inspect.signature(host.Gemma.fork_row_prefix).parameters) == ["self", "src", "dst_mask", "length"]
    assert list(inspect.signature(host.GemmaModel.serve_requests_prefix).parameters) == ["self", "requests", "logprobs", "prefix_cache", "min_prefix"]
    assert inspect.signature(host.GemmaModel.serve_requests_prefix).parameters["min_prefix"].default == 1
    for bad in (0, -1, 1.5, "2", True, None):      # before the model is asked
        with pytest.raises(ValueError, match="min_prefix must be"):
            host.GemmaModel.serve_requests_prefix(object(), [dict(prompt=[1, 2])], min_prefix=bad)
