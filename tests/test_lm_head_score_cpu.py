"""CPU-only checks of the scoring lm_head's entries (csrc/lm_head_score.hip): they are declared and exported, the scratch size is host logic (the slab rule), and the
validation refuses a bad call before any device work."""
import ctypes as C
import os
import subprocess

import pytest

from mila_amd import build, capi
from test_capi_cpu import _declared

NAMES = ("lm_head_score_scratch_bytes", "lm_head_score_bf16")
V, K = 262144, 3840
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_entries_are_declared_and_exported(lib):
    declared = _declared()
    for n in NAMES:
        assert "mila_cdna4_" + n in declared, n
        assert n in capi.EXPORTED, n
        assert hasattr(lib, "mila_cdna4_" + n), n
    assert lib.mila_cdna4_abi_version() == 4


def test_the_header_still_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mila_cdna4.h"\nint main(void) { return mila_cdna4_lm_head_score_scratch_bytes(0, 0) != 0; }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_the_slab_rule_looks_at_the_vocabulary_alone():
    assert capi.lm_head_score_slab(V) == 1024                        # 2048 tiles over 256 slabs
    assert capi.lm_head_score_slab(1000) == 128 and capi.lm_head_score_slab(32768) == 128 and capi.lm_head_score_slab(32769) == 256
    assert capi.lm_head_score_slab(40000) == 256 and capi.lm_head_score_slab(1) == 128


def test_scratch_bytes_is_32_bytes_per_row_and_slab_and_monotone_in_rows(lib):
    sb = capi.lm_head_score_scratch_bytes
    for vocab in (1, 127, 128, 129, 1000, 32768, 32769, 40000, V, 2 ** 31 - 1):
        S = capi.lm_head_score_slab(vocab)
        slabs = -(-vocab // S)
        assert slabs <= 256
        sizes = [sb(rows, vocab) for rows in (1, 2, 3, 8, 128, 129, 2048)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
        assert sizes[0] == slabs * 32 and sizes[-1] == 2048 * sizes[0], (vocab, sizes)
    assert sb(2048, V) == 2048 * 256 * 32
    assert sb(2 ** 31 - 1, V) == (2 ** 31 - 1) * 256 * 32               # size_t arithmetic


def test_scratch_bytes_is_zero_for_what_the_entry_refuses(lib):
    sb = capi.lm_head_score_scratch_bytes
    for rows, vocab in ((0, V), (-1, V), (1, 0), (1, -5), (0, 0)):
        assert sb(rows, vocab) == 0, (rows, vocab)


def test_validation_rejects_bad_arguments_without_touching_the_device(lib):
    null = C.c_void_p(None)
    one = C.c_void_p(16)     # never dereferenced: validation fails first
    z, f = C.c_size_t, C.c_float
    INV, SMALL = capi.MILA_E_INVALID_ARGUMENT, capi.MILA_E_SCRATCH_TOO_SMALL
    fn = lib.mila_cdna4_lm_head_score_bf16
    need = capi.lm_head_score_scratch_bytes(8, V)

    def call(x=one, stride=K, W=one, scales=null, fmt=0, k=K, vocab=V, targets=one, rows=8, lp=one, am=one, alp=one, scratch=one, nbytes=need):
        return fn(x, z(stride), W, scales, fmt, k, vocab, targets, rows, f(30.0), lp, am, alp, scratch, z(nbytes), null)

    for kw in (dict(x=null), dict(W=null), dict(targets=null), dict(lp=null)):
        assert call(**kw) == INV, kw
        assert b"null pointer" in lib.mila_cdna4_last_error()
    for kw in (dict(am=null), dict(alp=null)):
        assert call(**kw) == INV, kw
        assert b"argmax" in lib.mila_cdna4_last_error()
    for kw in (dict(fmt=2), dict(fmt=-1)):
        assert call(**kw) == INV, kw
        assert b"fmt" in lib.mila_cdna4_last_error()
    assert call(fmt=1) == INV and b"scales" in lib.mila_cdna4_last_error()
    for kw in (dict(rows=0), dict(rows=-3)):
        assert call(**kw) == INV and b"rows" in lib.mila_cdna4_last_error(), kw
    for kw in (dict(vocab=0), dict(vocab=-1)):
        assert call(**kw) == INV and b"vocab" in lib.mila_cdna4_last_error(), kw
    for kw in (dict(k=K + 4, stride=K + 4), dict(k=0), dict(k=-8), dict(fmt=1, scales=one, k=K + 8, stride=K + 8)):
        assert call(**kw) == INV and b"K=" in lib.mila_cdna4_last_error(), kw
    # K = 72 is a bf16 shape and K % 16 == 0 an e4m3 one: both get as far as the scratch check
    assert call(k=72, stride=72, nbytes=0) == SMALL
    assert call(fmt=1, scales=one, k=K + 16, stride=K + 16, nbytes=0) == SMALL
    assert call(stride=K - 1) == INV and b"x_stride" in lib.mila_cdna4_last_error()
    assert call(nbytes=need - 1) == SMALL and b"scratch" in lib.mila_cdna4_last_error()
    assert call(scratch=null) == SMALL
    assert call(scratch=C.c_void_p(24)) == INV and b"aligned" in lib.mila_cdna4_last_error()
    # both argmax outputs NULL is a shape of its own: it gets as far as the scratch check
    assert call(am=null, alp=null, nbytes=8) == SMALL
