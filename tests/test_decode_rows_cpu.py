"""CPU-only: the batched-decode kernel entries (2 .. 4 rows per step) at the drop-in boundary -- declared, exported, listed in the binding -- and the host plan of the
multi-row decode Linear (csrc/matvec_rows.hip: plan_rows): its chunks in flight U are the one-row launch's for every row count and tuning, because U is part of a row's
arithmetic; the x images fit the 160 KiB of LDS; what does not fit is refused."""
import ctypes as C
import os
import re

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Gemma 4 12B decode Linears (K, N, geglu, f32_out): qkv_proj, o_proj, fc_gate_up (N = F), fc_down, lm_head
D, F, QKV, AO, VOCAB = 3840, 15360, 8192, 4096, 262144
GEMMA_SHAPES = [(D, QKV, 0, 0), (AO, D, 0, 0), (D, F, 1, 0), (F, D, 0, 0), (D, VOCAB, 0, 1)]
LDS_LIMIT = 163840


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def _declared(*path):
    text = open(os.path.join(ROOT, *path)).read()
    return set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", text))


def test_the_rows_entries_are_declared_exported_and_bound(lib):
    public, internal = _declared("include", "mila_cdna4.h"), _declared("mila_amd", "csrc", "internal.h")
    for n in ("matvec_rows", "fused_attn_decode_rows_bf16", "sample_argmax_rows_final_advance", "advance_positions_rows"):
        assert "mila_cdna4_" + n in public and n in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + n), n
    assert "mila_cdna4_matvec_rows_plan_describe" in internal and "matvec_rows_plan_describe" in capi.INTERNAL
    assert hasattr(C.CDLL(capi.LIB_PATH), "mila_cdna4_matvec_rows_plan_describe")
    assert lib.mila_cdna4_abi_version() == 4      # additive
    # the argument block mirrors the header's: the one-row block first, then bias, rows and four 64-bit strides
    assert capi.matvec_rows_args.a.offset == 0 and capi.matvec_rows_args.bias.offset == C.sizeof(capi.fused_matvec_args)
    assert C.sizeof(capi.matvec_rows_args) == C.sizeof(capi.fused_matvec_args) + 8 + 8 + 4 * 8


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_rows_plan_keeps_the_one_row_chunks_in_flight(lib, fmt):
    try:
        for tuned_U in (0, 1, 2, 4):
            if tuned_U:
                capi.tune("matvec.chunks_in_flight", tuned_U)
            for K, N, geglu, f32 in GEMMA_SHAPES:
                one = capi.matvec_rows_plan(fmt, K, N, geglu, f32, rows=1)
                assert one is not None and one["lds_bytes"] <= 65536 and one["xc"] == (1 if K <= 8192 else 2)
                if tuned_U and one["R"] == 1:
                    assert one["U"] == tuned_U
                epc = (8, 16, 32)[fmt]
                steps = -(-(K // epc) // (64 * one["U"]))
                assert one["lds_bytes"] == steps * 64 * one["U"] * epc * 2
                for rows in (2, 3, 4):
                    p = capi.matvec_rows_plan(fmt, K, N, geglu, f32, rows=rows)
                    assert p is not None, (fmt, K, N, rows)
                    assert p["U"] == one["U"], (fmt, K, N, rows, tuned_U, p, one)
                    assert p["xc"] == one["xc"] and p["lds_bytes"] == rows * one["lds_bytes"] <= LDS_LIMIT
                    assert 1 <= p["workgroups"] <= 512
                    if f32:
                        assert p["workgroups"] <= lib.mila_cdna4_sample_scratch_bytes() // 8      # one sampler partial per workgroup and row
    finally:
        capi.tune_reset()
    # the largest image: fc_down's K at four rows is 128 KiB in every format
    assert capi.matvec_rows_plan(fmt, F, D, rows=4)["lds_bytes"] == 4 * 2 * 16384


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_rows_plan_refuses_what_does_not_fit(lib, fmt):
    assert capi.matvec_rows_plan(fmt, D, QKV, rows=5) is None and capi.matvec_rows_plan(fmt, D, QKV, rows=0) is None
    assert capi.matvec_rows_plan(fmt, 16416, D, rows=2) is None and capi.matvec_rows_plan(fmt, 16416, D, rows=1) is None      # beyond the register-staged x limit
    assert capi.matvec_rows_plan(fmt, 16384, D, rows=4)["lds_bytes"] <= LDS_LIMIT
    assert capi.matvec_rows_plan(fmt, D + 4, QKV, rows=2) is None      # no multiple of the format's 16-byte chunk
    assert capi.matvec_rows_plan(3, D, QKV, rows=2) is None


def test_the_entry_validates_before_any_device_work(lib):
    one = 16      # never dereferenced: validation fails first
    a = capi.fused_matvec_args(y=one, x=one, W=one, fmt=0, K=256, N=40, eps=1e-6, post_scale=1.0)
    r = capi.matvec_rows_args(a=a, rows=5, x_stride=256, y_stride=40)
    assert lib.mila_cdna4_matvec_rows(C.byref(r), None) == capi.MILA_E_UNSUPPORTED and b"rows=5" in lib.mila_cdna4_last_error()
    r.rows = 1
    assert lib.mila_cdna4_matvec_rows(C.byref(r), None) == capi.MILA_E_UNSUPPORTED
    r.rows, r.x_stride = 2, 255
    assert lib.mila_cdna4_matvec_rows(C.byref(r), None) == capi.MILA_E_INVALID_ARGUMENT and b"x_stride" in lib.mila_cdna4_last_error()
    r.x_stride, r.a.K = 16416, 16416
    assert lib.mila_cdna4_matvec_rows(C.byref(r), None) == capi.MILA_E_INVALID_ARGUMENT and b"16384" in lib.mila_cdna4_last_error()
    r.x_stride, r.a.K, r.a.geglu = 256, 256, 1
    assert lib.mila_cdna4_matvec_rows(C.byref(r), None) == capi.MILA_E_INVALID_ARGUMENT and b"norm_w" in lib.mila_cdna4_last_error()
    null = C.c_void_p(None)
    assert lib.mila_cdna4_sample_argmax_rows_final_advance(null, null, C.c_size_t(0), 1, null, null, 2, null) == capi.MILA_E_INVALID_ARGUMENT
    assert lib.mila_cdna4_advance_positions_rows(C.c_void_p(one), C.c_void_p(one), 0, null) == capi.MILA_E_INVALID_ARGUMENT
    nb = lib.mila_cdna4_sample_scratch_bytes()
    assert lib.mila_cdna4_sample_argmax_rows_final_advance(C.c_void_p(one), C.c_void_p(one), C.c_size_t(3 * nb), 4, C.c_void_p(one), C.c_void_p(one), 4, null) \
        == capi.MILA_E_SCRATCH_TOO_SMALL


def test_the_rows_linear_preloads_the_one_row_kernels_leading_arguments():
    """built with kernarg preload like the one-row kernel, and led by the same 11 dwords (W, x, norm_w, res, K, N, workgroups): read from the kernel descriptors"""
    from test_kernarg_preload_cpu import _code_objects, _kernel_descriptors
    build.build()
    kds = {}
    for elf in _code_objects(open(capi.LIB_PATH, "rb").read()):
        kds.update(_kernel_descriptors(elf))
    mine = {k: v[0] for k, v in kds.items() if k.startswith("_ZN4mila18matvec_rows_kernel")}
    assert len(mine) == 3 * 3 * 8 * 2 * 3, len(mine)      # formats x chunks in flight x entry forms x x-chunks per thread x row counts
    assert set(mine.values()) == {11}, sorted(set(mine.values()))


def test_max_batch_is_validated_and_the_rows_surface_exists(tmp_path):
    """tests/cpp/gemma_rows_traits.cpp, compiled with the host flags and RUN (host code only, no device call): max_batch 0 and 5 throw, 2 with kv_fp8 or with
    bounded_local_kv throws; the cache-row and rows-step members exist on the block interface, the op and the three transformers"""
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "gemma_rows_traits.cpp")
    exe = str(tmp_path / "gemma_rows_traits")
    libdir = os.path.dirname(capi.LIB_PATH)
    flags = [f for f in build.HOST_FLAGS if f not in ("-fPIC", "-fvisibility=hidden")]
    p = subprocess.run([build.HOSTCXX] + flags + [src, "-o", exe, "-L" + libdir, "-lmila_cdna4", "-L/opt/rocm/lib", "-lamdhip64", "-lrocprofiler-sdk-roctx",
                                                  "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "rows traits OK" in r.stdout, r.stdout


def test_the_host_binding_carries_the_rows_entries(lib):
    from mila_amd import host
    names = [n for n, _ in host.GemmaConfigC._fields_]
    assert names[-2:] == ["bounded_local_kv", "kv_fp8"]      # mila_gemma_config is unchanged: max_batch travels through mila_gemma_create_rows
    h = host.load()
    for n in ("create_rows", "prefill_row", "set_active", "reset_row", "decode_rows", "rows_graph_info", "time_decode_rows"):
        assert hasattr(h, "mila_gemma_" + n), n
    import inspect
    assert inspect.signature(host.Gemma.__init__).parameters["max_batch"].default is None
