"""The FP8 KV cache (PerChannelKvFp8<>) without a GPU: the C ABI additions are declared, listed and exported; their argument validation rejects bad calls before any
device work; the host mirror's policy type, trait row and op surface hold at compile time (tests/cpp/kvfp8_traits.cpp)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kv_write_fp8", "attn_decode_kvfp8", "kv_dequant_fp8_bf16", "attn_prefill_kvfp8_scratch_bytes", "attn_prefill_kvfp8"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_entries_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    declared = set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", header))
    main = C.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert "mila_cdna4_" + n in declared, n
        assert n in capi.EXPORTED and n not in capi.INTERNAL, n
        assert hasattr(main, "mila_cdna4_" + n), n
    # each entry answers to a place in the reference
    doc = header[header.index("PerChannelKvFp8<>"):header.index("mila_cdna4_attn_prefill_kvfp8(")]
    assert "QuantPolicy.ixx:56-88" in doc and "CudaGqa.cuh" in doc
    assert lib.mila_cdna4_abi_version() == 4      # additive


def test_validation_rejects_bad_arguments_without_touching_the_device(lib):
    null, one = C.c_void_p(None), C.c_void_p(16)     # never dereferenced: validation fails first
    INV = capi.MILA_E_INVALID_ARGUMENT
    big = C.c_size_t(1 << 40)
    err = lib.mila_cdna4_last_error

    def write(K8=one, V8=one, Ks=one, Vs=one, k=one, v=one, B=1, chunk=4, NKV=2, HS=256, start=0, cap=16):
        return lib.mila_cdna4_kv_write_fp8(K8, V8, Ks, Vs, k, v, B, chunk, NKV, HS, start, cap, null)

    def decode(Y=one, Q=one, K8=one, V8=one, Ks=one, Vs=one, scratch=one, nbytes=big, B=1, NH=16, NKV=8, HS=256, cap=2048, length=1500, window=0):
        return lib.mila_cdna4_attn_decode_kvfp8(Y, Q, K8, V8, Ks, Vs, scratch, nbytes, B, NH, NKV, HS, cap, length, window, 1.0, null)

    def dequant(Kc=one, Vc=one, K8=one, V8=one, Ks=one, Vs=one, B=1, NKV=2, HS=256, cap=16, first=0, count=4):
        return lib.mila_cdna4_kv_dequant_fp8_bf16(Kc, Vc, K8, V8, Ks, Vs, B, NKV, HS, cap, first, count, null)

    def prefill(Y=one, Q=one, K8=one, V8=one, Ks=one, Vs=one, scratch=one, nbytes=big, B=1, chunk=8, NH=16, NKV=8, HS=256, cap=64, pos=0, window=0):
        return lib.mila_cdna4_attn_prefill_kvfp8(Y, Q, K8, V8, Ks, Vs, scratch, nbytes, B, chunk, NH, NKV, HS, cap, pos, window, 1.0, null)

    for fn, ptrs in ((write, ("K8", "V8", "Ks", "Vs", "k", "v")), (decode, ("Y", "Q", "K8", "V8", "Ks", "Vs")), (dequant, ("Kc", "Vc", "K8", "V8", "Ks", "Vs")),
                     (prefill, ("Y", "Q", "K8", "V8", "Ks", "Vs", "scratch"))):
        for p in ptrs:
            assert fn(**{p: null}) == INV and b"null pointer" in err(), (fn.__name__, p)
        for hs in (0, 32, 96, 192, 384, 1024):
            assert fn(HS=hs) == INV and b"must be 64, 128, 256 or 512" in err(), (fn.__name__, hs)
        assert fn(cap=0) == INV and fn(cap=-3) == INV, fn.__name__
    assert write(chunk=17) == INV and b"exceeds the cache capacity" in err()       # chunk > capacity, as kv_write_bf16
    assert write(start=-1) == INV
    assert decode(NH=16, NKV=3) == INV and prefill(NH=16, NKV=3) == INV              # NH % NKV
    assert decode(NH=24, NKV=8) == INV and b"group size 3" in err()
    assert decode(length=0) == INV and decode(length=2049) == INV and b"exceeds the cache capacity" in err()      # unwindowed: len in [1, capacity]
    assert decode(length=5000, window=1024, nbytes=C.c_size_t(0)) == INV and b"scratch" in err()                   # (a windowed band fits; the scratch is short)
    assert decode(window=-1) == INV
    need = 16 * capi.attn_decode_plan(1, 16, 8, 256, 2048, 0, 1500)["splits"] * 260 * 4
    assert capi.attn_decode_plan(1, 16, 8, 256, 2048, 0, 1500)["splits"] > 1
    assert decode(nbytes=C.c_size_t(need - 1)) == INV and b"scratch" in err()
    assert decode(scratch=null) == INV and b"scratch" in err()
    assert need <= lib.mila_cdna4_attn_decode_scratch_bytes(1, 16, 256)              # what the entry asks for is what attn_decode_scratch_bytes covers
    assert dequant(count=0) == INV and dequant(count=17) == INV and dequant(first=-1) == INV
    assert lib.mila_cdna4_attn_prefill_kvfp8_scratch_bytes(2, 8, 256, 64) == 2 * 2 * 8 * 64 * 256 * 2
    assert lib.mila_cdna4_attn_prefill_kvfp8_scratch_bytes(1, 8, 256, 0) == 0
    assert prefill(nbytes=C.c_size_t(2 * 8 * 64 * 256 * 2 - 1)) == INV and b"scratch" in err()
    assert prefill(pos=60, chunk=8) == INV and b"do not fit the cache capacity" in err()                       # unwindowed: keys [0, 67] in 64 rows
    assert prefill(chunk=0) == INV and prefill(pos=-1) == INV and prefill(window=-1) == INV
    # the fp8 cache never takes the matrix-core form: its split count is the scalar kernel's, which the partial layout of attn_decode_scratch_bytes covers
    assert capi.attn_decode_plan(1, 16, 1, 512, 32768, 0, 32768)["form"] == "attn_decode_mfma"                 # (the bf16 cache's plan is unchanged)
    assert decode(NH=16, NKV=1, HS=512, cap=32768, length=32768, nbytes=C.c_size_t(16 * 32 * 516 * 4 - 1)) == INV and b"scratch" in err()


def _compile_traits(*extra):
    src = os.path.join(ROOT, "tests", "cpp", "kvfp8_traits.cpp")
    return subprocess.run([build.HOSTCXX] + build.HOST_FLAGS + ["-fsyntax-only", src] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)


def test_the_host_mirror_resolves_the_policy_at_compile_time():
    """the trait for all three KV policies, the QuantKvPolicy facts, the op surface, and GemmaTransformer's block aliases -- static_asserts of tests/cpp/kvfp8_traits.cpp"""
    p = _compile_traits()
    assert p.returncode == 0, p.stdout


def test_e5m2_storage_is_rejected_with_a_readable_message():
    p = _compile_traits("-DKVFP8_ASK_E5M2")
    assert p.returncode != 0
    assert "static assertion failed" in p.stdout and "FP8_E5M2 storage has no GroupedQueryAttentionOp row" in p.stdout, p.stdout


def test_nothing_under_the_host_mirror_names_the_kernel_internals():
    for root, _, files in os.walk(os.path.join(ROOT, "mila_amd", "host")):
        for f in files:
            text = open(os.path.join(root, f)).read()
            assert "internal.h" not in text and "attention_decode_plan.h" not in text and "fp8_quant.h" not in text, f
