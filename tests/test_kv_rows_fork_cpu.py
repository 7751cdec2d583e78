"""CPU-only: mila_cdna4_kv_rows_fork_bf16 at the drop-in boundary -- declared, exported, bound -- and every refusal of its host-side validation, which comes before any
device call: the pointers handed in are dummies that are never dereferenced (tests/test_decode_rows_cpu.py shows the pattern for the rows entries)."""
import ctypes as C
import os
import re

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = capi.MILA_E_INVALID_ARGUMENT
GOOD = dict(K=4096, V=8192, rows=4, NKV=2, capacity=48, HS=64, src=1, dst_mask=0b1101, len=33)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def _fork(lib, **change):
    a = dict(GOOD, **change)
    rc = lib.mila_cdna4_kv_rows_fork_bf16(C.c_void_p(a["K"]), C.c_void_p(a["V"]), a["rows"], a["NKV"], a["capacity"], a["HS"], a["src"], a["dst_mask"], a["len"], None)
    return rc, lib.mila_cdna4_last_error().decode()


def test_the_entry_is_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    assert re.search(r"MILA_API\s+int\s+mila_cdna4_kv_rows_fork_bf16\s*\(", text)
    assert "kv_rows_fork_bf16" in capi.EXPORTED and hasattr(lib, "mila_cdna4_kv_rows_fork_bf16")
    assert lib.mila_cdna4_abi_version() == 4      # additive


@pytest.mark.parametrize("change, telling", [
    (dict(K=None), "null pointer"),
    (dict(V=None), "null pointer"),
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
    (dict(len=49), "len=49"),
    (dict(HS=60), "HS=60"),
    (dict(HS=4), "HS=4"),
    (dict(HS=0), "bad sizes"),
    (dict(NKV=0), "bad sizes"),
    (dict(capacity=0), "bad sizes"),
    (dict(K=4098), "16-byte aligned"),
])
def test_every_refusal_comes_before_any_device_work(lib, change, telling):
    rc, err = _fork(lib, **change)
    assert rc == INV and "kv_rows_fork_bf16" in err and telling in err, (change, rc, err)

