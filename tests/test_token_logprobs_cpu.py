"""CPU-only checks of the token log-probability entries (csrc/logprobs.hip): they are declared and exported, the sizes they report, and the validation that refuses
a bad call before any device work."""
import ctypes as C

import pytest

from mila_amd import build, capi
from test_capi_cpu import _declared

NAMES = ("token_logprobs_record_words", "token_logprobs_scratch_bytes", "token_logprobs_rows_fp32", "token_logprobs_publish_fp32")
V = 262144


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_four_entries_are_declared_and_exported(lib):
    declared = _declared()
    for n in NAMES:
        assert "mila_cdna4_" + n in declared, n
        assert n in capi.EXPORTED, n
        assert hasattr(lib, "mila_cdna4_" + n), n
    assert lib.mila_cdna4_abi_version() == 4


def test_record_words(lib):
    assert capi.token_logprobs_record_words() == 44      # tag, token, logprob, top_n, 20 ids, 20 logprobs


def test_scratch_bytes_is_zero_for_what_the_entries_refuse(lib):
    sb = capi.token_logprobs_scratch_bytes
    assert sb(1, V, 0) > 0 and sb(4, V, 20) > 0
    for rows in (0, 5, -1):
        assert sb(rows, V, 5) == 0
    for top_n in (-1, 21):
        assert sb(1, V, top_n) == 0
    assert sb(1, 7, 8) == 0 and sb(1, 7, 7) > 0            # top_n = V + 1, top_n = V
    assert sb(1, 0, 0) == 0 and sb(1, -3, 0) == 0


def test_scratch_bytes_is_monotone_in_rows_and_top_n(lib):
    sb = capi.token_logprobs_scratch_bytes
    for top_n in range(0, 21):
        sizes = [sb(rows, V, top_n) for rows in (1, 2, 3, 4)]
        assert sizes == sorted(sizes) and len(set(sizes)) == 4, sizes
        assert sizes[3] == 4 * sizes[0]                    # every row its own region
    for rows in (1, 2, 3, 4):
        sizes = [sb(rows, V, top_n) for top_n in range(0, 21)]
        assert sizes == sorted(sizes) and len(set(sizes)) == 21, sizes


def test_validation_rejects_bad_arguments_without_touching_the_device(lib):
    null = C.c_void_p(None)
    one = C.c_void_p(16)     # never dereferenced: validation fails first
    z = C.c_size_t
    f = C.c_float
    INV, SMALL = capi.MILA_E_INVALID_ARGUMENT, capi.MILA_E_SCRATCH_TOO_SMALL
    rows_fn, pub_fn = lib.mila_cdna4_token_logprobs_rows_fp32, lib.mila_cdna4_token_logprobs_publish_fp32
    big = z(1 << 30)

    def rows_call(logits=one, stride=V, tokens=one, rows=2, vocab=V, top_n=5, active=null, count=null, lp=one, ids=one, tlp=one, scratch=one, nbytes=big):
        return rows_fn(logits, z(stride), tokens, rows, vocab, f(30.0), top_n, active, count, lp, ids, tlp, scratch, nbytes, null)

    for kw in (dict(logits=null), dict(tokens=null), dict(lp=null), dict(ids=null), dict(tlp=null)):
        assert rows_call(**kw) == INV, kw
        assert b"null pointer" in lib.mila_cdna4_last_error()
    for kw in (dict(rows=0), dict(rows=5), dict(rows=-1)):
        assert rows_call(**kw) == INV, kw
        assert b"rows" in lib.mila_cdna4_last_error()
    for kw in (dict(top_n=-1), dict(top_n=21), dict(vocab=4, stride=4, top_n=5)):
        assert rows_call(**kw) == INV, kw
        assert b"top_n" in lib.mila_cdna4_last_error()
    assert rows_call(vocab=0) == INV and rows_call(vocab=-1) == INV
    assert rows_call(stride=V - 1) == INV
    assert b"logits_stride" in lib.mila_cdna4_last_error()
    need = capi.token_logprobs_scratch_bytes(2, V, 5)
    assert rows_call(nbytes=z(need - 1)) == SMALL
    assert b"scratch" in lib.mila_cdna4_last_error()
    assert rows_call(scratch=null) == SMALL
    assert rows_call(scratch=C.c_void_p(18)) == INV        # misaligned

    def pub_call(logits=one, token=one, vocab=V, top_n=5, seq=one, ring=one, ring_size=8, scratch=one, nbytes=big):
        return pub_fn(logits, token, vocab, f(0.0), top_n, seq, ring, ring_size, scratch, nbytes, null)

    for kw in (dict(logits=null), dict(token=null), dict(seq=null), dict(ring=null)):
        assert pub_call(**kw) == INV, kw
        assert b"null pointer" in lib.mila_cdna4_last_error()
    for kw in (dict(top_n=-1), dict(top_n=21), dict(vocab=3, top_n=4), dict(vocab=0), dict(ring_size=0), dict(ring_size=-2)):
        assert pub_call(**kw) == INV, kw
    need = capi.token_logprobs_scratch_bytes(1, V, 5)
    assert pub_call(nbytes=z(need - 1)) == SMALL
    assert pub_call(scratch=null) == SMALL
    # top_n = 0 needs no list outputs: with a short scratch the call gets as far as the scratch check
    assert rows_call(top_n=0, ids=null, tlp=null, nbytes=z(8)) == SMALL
