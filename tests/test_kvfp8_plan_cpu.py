"""The plan of the FP8 KV cache's decode (capi.attn_decode_kvfp8_plan -> csrc/attention.hip: plan_decode) and the two device-position entries, checked without a GPU:
attn_decode_kvfp8 launches from the bf16 cache's plan for the shape -- the same form rule (HS 512, group size a multiple of 16, band bucket >= attn.mfma_min_band), the
same split count, band and scratch need -- so it takes its matrix-core kernel exactly where attn_decode_bf16 takes its own; attn.kvfp8_mfma_decode 0 pins it to the
wave-per-position kernel.  The new entries are declared, listed and exported, and reject bad arguments before any device work."""
import ctypes as C
import os
import re

import pytest

from mila_amd import build, capi
from test_attention_gpu import GEOMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kv_write_fp8_devpos", "attn_decode_kvfp8_devpos", "attn_decode_kvfp8_plan_describe"]
SCALAR, MFMA = "attn_decode_kvfp8", "attn_decode_kvfp8_mfma"
SAME = ("splits", "band_max", "heads_per_group", "head_groups", "flat", "prologue", "partial_floats", "scratch_need")      # every field but the form's name


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def _both(*shape):
    return capi.attn_decode_kvfp8_plan(*shape), capi.attn_decode_plan(*shape)


def test_a_long_band_takes_the_matrix_core_form(lib):
    p8, p16 = _both(1, 16, 1, 512, 32768, 0, 32768)
    assert p8["form"] == MFMA and p16["form"] == "attn_decode_mfma"
    assert p8["splits"] == p16["splits"] == 256 and p8["band_max"] == p16["band_max"] == 32768 and p8["scratch_need"] == p16["scratch_need"] == 16 * 256 * 516 * 4


@pytest.mark.parametrize("shape", [(1, 16, 1, 512, 32768, 0, 4096), (1, 16, 1, 256, 32768, 0, 32768), (1, 16, 8, 512, 32768, 0, 32768)], ids=["len_4096", "hs_256", "nkv_8"])
def test_shapes_outside_the_rule_stay_on_the_scalar_form(lib, shape):
    p8, p16 = _both(*shape)
    assert p8["form"] == SCALAR and p16["form"] == "attn_decode"
    for f in ("splits", "heads_per_group", "head_groups", "scratch_need"):
        assert p8[f] == p16[f], f


def _sweep():
    """B 1-2 x the GEOMS geometries (+ two 16-head groups per KV head, and 16 heads on each of two KV heads) x three capacities x both sides of every bucket edge"""
    geoms = [(NH, NKV, HS, window) for _, NH, NKV, HS, window, _ in GEOMS] + [(32, 1, 512, 0), (32, 2, 512, 0), (16, 1, 512, 1024)]
    for B in (1, 2):
        for NH, NKV, HS, window in geoms:
            for cap in (1024, 8192, 32768):
                for hint in sorted({0, 1, 1024, 4096, 4097, 8192, 8193, 16384, 16385, 32768} | {cap}):
                    if hint <= cap:
                        yield B, NH, NKV, HS, cap, window, hint


def test_the_plan_is_the_bf16_plan_over_a_sweep_and_never_exceeds_the_scratch_query(lib):
    forms = set()
    for shape in _sweep():
        B, NH, NKV, HS, cap, window, hint = shape
        p8, p16 = _both(*shape)
        assert {k: p8[k] for k in SAME} == {k: p16[k] for k in SAME}, shape
        mfma = HS == 512 and (NH // NKV) % 16 == 0 and p8["band_max"] >= 8192
        assert p8["form"] == (MFMA if mfma else SCALAR) and p16["form"] == ("attn_decode_mfma" if mfma else "attn_decode"), shape
        if mfma:
            assert p8["splits"] == max(1, min((p8["band_max"] + 127) // 128, 256 // (B * NH // 16), 256)), shape
        assert p8["scratch_need"] <= lib.mila_cdna4_attn_decode_scratch_bytes(B, NH, HS), shape
        assert p8["scratch_need"] == (4 * B * NH * p8["splits"] * (HS + 4) if mfma or p8["splits"] > 1 else 0), shape
        forms.add(p8["form"])
    assert forms == {SCALAR, MFMA}
    # the bucket edges: 4096 keys are the last scalar length of a long cache, 4097 the first matrix-core one (bucket 8192)
    assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, 8192, 0, 4096)["form"] == SCALAR
    assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, 8192, 0, 4097) == dict(capi.attn_decode_plan(1, 16, 1, 512, 8192, 0, 4097), form=MFMA)
    assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, 8192, 0, 4097)["splits"] == 64
    # no plan: a head size the fp8 cache has no kernels for, or a bad shape
    buf = C.create_string_buffer(64)
    assert lib.mila_cdna4_attn_decode_kvfp8_plan_describe(1, 16, 1, 96, 1024, 0, 0, buf, 64) == 0 and buf.value == b""
    assert lib.mila_cdna4_attn_decode_kvfp8_plan_describe(1, 16, 3, 512, 1024, 0, 0, buf, 64) == 0
    assert lib.mila_cdna4_attn_decode_kvfp8_plan_describe(1, 16, 1, 512, 1024, 0, 0, None, 0) > 0      # (the size alone)


def test_the_tunables_steer_the_form(lib):
    try:
        capi.tune("attn.kvfp8_mfma_decode", 0)
        for shape in _sweep():
            B, NH, NKV, HS, cap, window, hint = shape
            p8 = capi.attn_decode_kvfp8_plan(*shape)
            assert p8["form"] == SCALAR and p8["splits"] <= 64, shape
            assert p8["scratch_need"] <= lib.mila_cdna4_attn_decode_scratch_bytes(B, NH, HS), shape
        # ... and the scalar plan is the parent's: the bf16 cache's with its own matrix-core form off
        capi.tune("attn.mfma_decode", 0)
        p8, p16 = _both(1, 16, 1, 512, 32768, 0, 32768)
        assert {k: p8[k] for k in SAME} == {k: p16[k] for k in SAME} and p8["splits"] == 32
        capi.tune_reset()
        assert capi.attn_decode_plan(1, 16, 1, 512, 32768, 0, 32768)["form"] == "attn_decode_mfma"      # (the switch is the fp8 cache's alone)
        capi.tune("attn.mfma_min_band", 256)
        p8, p16 = _both(1, 16, 1, 512, 1024, 0, 300)
        assert p8["form"] == MFMA and p8["splits"] == p16["splits"] == 8 and p8["band_max"] == 1024
        assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, 320, 300, 1000)["splits"] == 3                 # a 300-key window: ceil(300 / 128)
        capi.tune("attn.mfma_decode", 0)                                                                  # the bf16 cache's own switch holds for both
        assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, 1024, 0, 300)["form"] == SCALAR
    finally:
        capi.tune_reset()
    assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, 1024, 0, 300)["form"] == SCALAR


def test_the_new_entries_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    declared = set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", header))
    main = C.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert "mila_cdna4_" + n in declared, n
        assert n in capi.EXPORTED and n not in capi.INTERNAL, n
        assert hasattr(main, "mila_cdna4_" + n), n
    doc = header[header.index("PerChannelKvFp8<>"):header.index("mila_cdna4_attn_prefill_kvfp8(")]
    assert "kv_write_fp8_devpos / attn_decode_kvfp8_devpos" in doc and "the split count of\n" not in doc
    assert lib.mila_cdna4_abi_version() == 4      # additive
    tunables = C.create_string_buffer(8192)
    lib.mila_cdna4_tune_list.restype = C.c_size_t
    lib.mila_cdna4_tune_list(tunables, C.c_size_t(8192))
    assert b"attn.kvfp8_mfma_decode=1 (default 1)" in tunables.value


def test_the_device_position_entries_validate_without_touching_the_device(lib):
    null, one = C.c_void_p(None), C.c_void_p(16)     # never dereferenced: validation fails first
    INV = capi.MILA_E_INVALID_ARGUMENT
    big = C.c_size_t(1 << 40)
    err = lib.mila_cdna4_last_error

    def write(K8=one, V8=one, Ks=one, Vs=one, k=one, v=one, B=1, NKV=2, HS=256, pos=one, cap=16):
        return lib.mila_cdna4_kv_write_fp8_devpos(K8, V8, Ks, Vs, k, v, B, NKV, HS, pos, cap, null)

    def decode(Y=one, Q=one, K8=one, V8=one, Ks=one, Vs=one, scratch=one, nbytes=big, B=1, NH=16, NKV=8, HS=256, cap=2048, pos=one, max_len=1500, window=0):
        return lib.mila_cdna4_attn_decode_kvfp8_devpos(Y, Q, K8, V8, Ks, Vs, scratch, nbytes, B, NH, NKV, HS, cap, pos, max_len, window, 1.0, null)

    for fn, ptrs in ((write, ("K8", "V8", "Ks", "Vs", "k", "v", "pos")), (decode, ("Y", "Q", "K8", "V8", "Ks", "Vs", "pos"))):
        for p in ptrs:
            assert fn(**{p: null}) == INV and b"null pointer" in err() and b"_devpos" in err(), (fn.__name__, p)
        for hs in (0, 32, 96, 192, 384, 1024):
            assert fn(HS=hs) == INV and b"must be 64, 128, 256 or 512" in err(), (fn.__name__, hs)
        assert fn(cap=0) == INV and fn(cap=-3) == INV and fn(B=0) == INV, fn.__name__
    assert write(NKV=0) == INV
    assert decode(NH=16, NKV=3) == INV and decode(NH=24, NKV=8) == INV and b"group size 3" in err()
    assert decode(max_len=0) == INV and b"max_len" in err()
    assert decode(max_len=-1) == INV
    assert decode(max_len=2049) == INV and b"exceeds the cache capacity" in err()            # unwindowed: max_len in [1, capacity]
    assert decode(window=-1) == INV
    assert decode(max_len=5000, window=1024, nbytes=C.c_size_t(0)) == INV and b"scratch" in err()      # (a windowed band fits; the scratch is short)
    need = capi.attn_decode_kvfp8_plan(1, 16, 8, 256, 2048, 0, 1500)["scratch_need"]
    assert need > 0
    assert decode(nbytes=C.c_size_t(need - 1)) == INV and b"scratch" in err()
    assert decode(scratch=null) == INV and b"scratch" in err()
    # the matrix-core form's need at the 32K shape: 256 splits, in both entries
    need = 16 * 256 * 516 * 4
    assert capi.attn_decode_kvfp8_plan(1, 16, 1, 512, 32768, 0, 32768)["scratch_need"] == need
    assert decode(NH=16, NKV=1, HS=512, cap=32768, max_len=32768, nbytes=C.c_size_t(need - 1)) == INV and b"scratch" in err()
    assert lib.mila_cdna4_attn_decode_kvfp8(one, one, one, one, one, one, one, C.c_size_t(need - 1), 1, 16, 1, 512, 32768, 32768, 0, C.c_float(1.0), null) == INV and b"scratch" in err()
