"""The FP8 KV cache in the Gemma model without a GPU: the three quantizing q/k/v entries (fused_qkv_post_kvfp8 / _prefill / _devpos) are declared, listed and
exported and reject bad arguments before any device work; the host mirror's two block aliases on PerChannelKvFp8<> and the kv_fp8 switches hold at compile time
(tests/cpp/gemma_kvfp8_traits.cpp); and the whole-model bar of tests/test_gemma_kvfp8_model_gpu.py is measured: the distance between the fp8-KV oracle composition
(tests/ref_gemma_kvfp8.py) and its float32-norm twin on tests/test_conditioned_cpu.py's model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ref_gemma_kvfp8 as rk
import test_conditioned_cpu
from mila_amd import build, capi, host
from ref_gemma import CONDITIONED_PROFILE, RefGemma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fused_qkv_post_kvfp8", "fused_qkv_post_kvfp8_prefill", "fused_qkv_post_kvfp8_devpos"]


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
    # inside the FP8 KV section, each form answering to the place its bf16 counterpart cites
    section = header[header.index("PerChannelKvFp8<>"):header.index("Normalisation / activations")]
    for n in NAMES:
        assert "mila_cdna4_" + n + "(" in section, n
    doc = section[section.index("fused_qkv_post_kvfp8 /"):section.index("MILA_API")]
    assert "Gemma.Block.ixx:315-337" in doc and "Gemma.Block.ixx:215-262" in doc and "Gemma4InferenceReview.md:71-84" in doc
    assert lib.mila_cdna4_abi_version() == 4      # additive


def test_validation_rejects_bad_arguments_without_touching_the_device(lib):
    null, one = C.c_void_p(None), C.c_void_p(16)     # never dereferenced: validation fails first
    INV = capi.MILA_E_INVALID_ARGUMENT
    err = lib.mila_cdna4_last_error
    PTRS = ("q_out", "K8", "V8", "Ks", "Vs", "q", "k", "v_src", "qw", "kw", "vw", "cos", "sin")

    def ptrs(kw):
        return [kw.pop(n, one) for n in PTRS]

    def eager(NH=4, NKV=2, HS=64, pos=3, cap=24, **kw):
        a = ptrs(kw)
        assert not kw
        return lib.mila_cdna4_fused_qkv_post_kvfp8(*a, NH, NKV, HS, pos, cap, 1e-6, null)

    def prefill(stride=512, T=5, NH=4, NKV=2, HS=64, pos=3, cap=24, **kw):
        a = ptrs(kw)
        assert not kw
        return lib.mila_cdna4_fused_qkv_post_kvfp8_prefill(*a[:8], stride, *a[8:], T, NH, NKV, HS, pos, cap, 1e-6, null)

    def devpos(NH=4, NKV=2, HS=64, pos_dev=one, cap=24, **kw):
        a = ptrs(kw)
        assert not kw
        return lib.mila_cdna4_fused_qkv_post_kvfp8_devpos(*a, NH, NKV, HS, pos_dev, cap, 1e-6, null)

    for fn in (eager, prefill, devpos):
        for p in PTRS:
            if p == "vw":      # optional: a null V weight is the unit weight, as in fused_qkv_post
                continue
            assert fn(**{p: null}) == INV and b"null pointer" in err(), (fn.__name__, p)
        for hs in (0, 16, 32, 96, 192, 384, 1024):
            assert fn(HS=hs) == INV and b"must be 64, 128, 256 or 512" in err(), (fn.__name__, hs)
        assert fn(cap=0) == INV and fn(cap=-3) == INV, fn.__name__
        assert fn(NH=0) == INV and fn(NKV=0) == INV, fn.__name__
        assert fn.__name__.encode() in b"eager prefill devpos" and (b"fused_qkv_post_kvfp8" in err())
    assert devpos(pos_dev=null) == INV and b"null pointer" in err()
    assert eager(pos=-1) == INV and prefill(pos=-1) == INV                                   # negative position
    assert prefill(T=25) == INV and b"do not fit the cache capacity" in err()               # T > capacity
    assert prefill(T=0) == INV
    for stride in (511, 60, 4, 0, -8):                                                        # not a multiple of 8, or shorter than a head row
        assert prefill(stride=stride) == INV and b"row stride" in err(), stride


def _compile_traits(*extra):
    src = os.path.join(ROOT, "tests", "cpp", "gemma_kvfp8_traits.cpp")
    return subprocess.run([build.HOSTCXX] + build.HOST_FLAGS + ["-fsyntax-only", src] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)


def test_the_model_is_wired_to_the_policy_at_compile_time():
    """the two new block aliases instantiate on PerChannelKvFp8<>, GemmaConfig::kv_fp8 and GemmaModelConfig::withKvFp8 exist -- tests/cpp/gemma_kvfp8_traits.cpp"""
    p = _compile_traits()
    assert p.returncode == 0, p.stdout


def test_the_python_binding_carries_the_switch():
    names = [n for n, _ in host.GemmaConfigC._fields_]
    assert names[-2:] == ["bounded_local_kv", "kv_fp8"]                                      # mila_gemma_config: kv_fp8 after bounded_local_kv
    runner = open(os.path.join(ROOT, "mila_amd", "host", "src", "gemma_runner.cpp")).read()
    struct = runner[runner.index("struct mila_gemma_config"):runner.index("HOST_API const char* mila_host_last_error")]
    assert struct.index("int64_t bounded_local_kv;") < struct.index("int64_t kv_fp8;")
    import inspect
    for fn in (host.Gemma.__init__, host.GemmaModel.synthetic, host.GemmaModel.from_pretrained):
        assert inspect.signature(fn).parameters["kv_fp8"].default is False, fn


def test_the_oracle_quantizes_the_appended_rows_and_nothing_else():
    """RefGemmaKvFp8 against RefGemma on one token: the first position attends to its own quantized K / V row only, so the two differ by the e4m3 rounding of V (softmax
    over one key is 1 whatever K is) -- more than 0, and by no more than the 2^-4 relative step of e4m3 allows downstream on the conditioned model"""
    x = np.asarray([[0.0] * 64, np.linspace(-3, 3, 64), [448.0] + [1.0] * 63], dtype=np.float32)
    deq = rk.quantize_rows(x)
    assert np.all(deq[0] == 0) and deq[2, 0] == 448.0 and deq[2, 1] == 1.0
    assert np.abs(deq[1] - x[1]).max() <= 3.0 / 16 and np.any(deq[1] != x[1])
    a = rk.RefGemmaKvFp8(rk.CPU_CFG, "bf16", 7, profile=CONDITIONED_PROFILE).forward(rk.CPU_TOK[:1], 0, 32)
    b = RefGemma(rk.CPU_CFG, "bf16", 7, profile=CONDITIONED_PROFILE).forward(rk.CPU_TOK[:1], 0, 32)
    d = np.abs(a - b).max() / np.abs(b).max()
    assert 0.0 < d < 2e-2, d


def test_two_correct_fp8_kv_compositions_and_the_gpu_bar():
    """The distance between the fp8-KV oracle and its float32-norm twin on tests/test_conditioned_cpu.py's model: measured 1.62e-3 (a 1-ulp bf16 difference upstream of a
    quantized K / V row flips e4m3 codes, as in the W4A8 leg there, which measures 1.5e-3).  The GPU bar is max(1e-3, 2 x this) capped at 3e-3: 3e-3."""
    assert rk.CPU_CFG == test_conditioned_cpu.CFG and rk.CPU_TOK == test_conditioned_cpu.TOK
    d = rk.cpu_distance()
    print("fp8-KV oracle vs its float32-norm twin: %.3e of max|logit|; GPU bar %.1e" % (d, rk.gpu_bar()))
    assert 0.0 < d <= rk.BAR_CAP, d
    assert rk.BAR_FLOOR <= rk.gpu_bar() <= rk.BAR_CAP
    assert rk.gpu_bar() == min(rk.BAR_CAP, max(rk.BAR_FLOOR, 2 * d))
