"""CPU-only: the speculative greedy decode's surface -- the chain attention entry and the accept sampler tail declared, exported and bound; their argument checks
(no device is touched); GemmaConfig::draft_tokens and what it refuses; and the default drafter (prompt lookup) against a Python restatement of its rule."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mila_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fused_attn_decode_chain_bf16", "attn_decode_chain_scratch_bytes", "fused_qkv_post_rows_devpos", "sample_argmax_chain_accept")

SMALL = dict(vocab_size=4096, embedding_dim=512, num_layers=6, num_heads=4, num_kv_heads=2, head_dim=128, hidden_dim=1024, global_head_dim=256, num_global_kv_heads=1,
             window=64, sliding_window_pattern=6, global_rotary_dim=64)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return capi.load()


def test_the_chain_entries_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "mila_cdna4.h")).read()
    public = set(re.findall(r"MILA_API\s+[\w\s\*]+?\b(mila_cdna4_\w+)\s*\(", text))
    for n in NEW:
        assert "mila_cdna4_" + n in public and n in capi.EXPORTED and hasattr(lib, "mila_cdna4_" + n), n
    assert lib.mila_cdna4_abi_version() == 4      # additive
    # the contract is stated where the entry is declared
    for phrase in ("bit-identical to T successive fused_attn_decode_bf16 calls", "no other cache row is written", "UNBOUNDED caches", "the longest correct draft prefix"):
        assert phrase in text, phrase


def test_the_header_still_compiles_as_plain_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "mila_cdna4.h")])


def _chain(lib, T=2, HS=64, position=0, capacity=64, position_dev=None, max_len=0, null_at=None, NH=4, NKV=2, stride=512, scratch_bytes=1 << 20):
    one = 16      # never dereferenced: validation fails first
    ptrs = [one] * 12      # Y Kc Vc q k v | qw kw vw cos sin scratch
    if null_at is not None:
        ptrs[null_at] = None
    p = [C.c_void_p(v) for v in ptrs]
    return lib.mila_cdna4_fused_attn_decode_chain_bf16(p[0], p[1], p[2], p[3], p[4], p[5], C.c_int64(stride), p[6], p[7], p[8], p[9], p[10], p[11], C.c_size_t(scratch_bytes), T,
                                                       NH, NKV, HS, capacity, position, C.c_void_p(position_dev), max_len, 0, C.c_float(1.0), C.c_float(1e-6), None)


def test_the_chain_entry_validates_before_any_device_work(lib):
    E = capi.MILA_E_INVALID_ARGUMENT
    for T in (0, 1, 5, -1):
        assert _chain(lib, T=T) == E and b"outside 2 .. 4" in lib.mila_cdna4_last_error(), T
    for HS in (32, 96, 192, 1024):
        assert _chain(lib, HS=HS) == E and b"head size" in lib.mila_cdna4_last_error(), HS
    for null_at in (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11):      # (vw, index 8, may be NULL: unit weight)
        assert _chain(lib, null_at=null_at) == E and b"null pointer" in lib.mila_cdna4_last_error(), null_at
    # eager: the T rows must fit the cache -- the chain is for unbounded caches, it never wraps a ring
    for T in (2, 3, 4):
        assert _chain(lib, T=T, position=64 - T + 1) == E and b"do not fit the cache capacity" in lib.mila_cdna4_last_error(), T
    assert _chain(lib, position=-1) == E
    assert _chain(lib, position_dev=16, max_len=65) == E and b"max_len" in lib.mila_cdna4_last_error()
    assert _chain(lib, stride=60) == E and b"raw_b_stride" in lib.mila_cdna4_last_error()
    assert _chain(lib, scratch_bytes=64) == capi.MILA_E_SCRATCH_TOO_SMALL
    # the scratch query: the partials of T rows plus the roped q rows; 0 for what the entry refuses
    f = lib.mila_cdna4_attn_decode_chain_scratch_bytes
    for T in (2, 3, 4):
        for NH, HS in ((4, 64), (16, 256)):
            assert f(T, NH, HS) == T * NH * 64 * (HS + 4) * 4 + T * NH * HS * 2, (T, NH, HS)
        assert f(T, 16, 512) == T * 16 * 256 * 516 * 4 + T * 16 * 512 * 2
        assert f(T, 16, 512) == lib.mila_cdna4_attn_decode_scratch_bytes(T, 16, 512)
    assert f(1, 4, 64) == 0 and f(5, 4, 64) == 0 and f(2, 4, 96) == 0 and f(2, 0, 64) == 0


def test_the_accept_tail_and_the_rows_prologue_validate_before_any_device_work(lib):
    E = capi.MILA_E_INVALID_ARGUMENT
    null, one = C.c_void_p(None), C.c_void_p(16)
    nb = lib.mila_cdna4_sample_scratch_bytes()
    acc = lib.mila_cdna4_sample_argmax_chain_accept
    assert acc(null, one, one, C.c_size_t(4 * nb), 4, one, 2, None) == E and b"null pointer" in lib.mila_cdna4_last_error()
    assert acc(one, null, one, C.c_size_t(4 * nb), 4, one, 2, None) == E
    assert acc(one, one, one, C.c_size_t(4 * nb), 4, null, 2, None) == E
    for T in (1, 5):
        assert acc(one, one, one, C.c_size_t(8 * nb), 4, one, T, None) == E and b"outside 2 .. 4" in lib.mila_cdna4_last_error()
    assert acc(one, one, one, C.c_size_t(4 * nb), 0, one, 2, None) == E
    assert acc(one, one, one, C.c_size_t(2 * nb), 4, one, 3, None) == capi.MILA_E_SCRATCH_TOO_SMALL
    post = lib.mila_cdna4_fused_qkv_post_rows_devpos
    args = lambda pos, T=2, stride=512: (one, one, one, one, one, one, C.c_int64(stride), one, one, null, one, one, T, 4, 2, 64, pos, 64, C.c_float(1e-6), None)
    assert post(*args(null)) == E and b"null pointer" in lib.mila_cdna4_last_error()
    assert post(*args(one, T=65)) == E and post(*args(one, stride=60)) == E


def test_draft_tokens_is_validated_and_refuses_what_the_chain_cannot_serve(lib):
    from mila_amd import host
    host.validate_gemma_config(SMALL, 1, 0)
    for k in (1, 2, 3):
        host.validate_gemma_config(SMALL, 1, k)
    for k in (-1, 4, 7):
        with pytest.raises(ValueError, match="draft_tokens .* outside 0 .. 3"):
            host.validate_gemma_config(SMALL, 1, k)
    with pytest.raises(ValueError, match="draft_tokens > 0 cannot be combined with max_batch > 1 .*ONE sequence"):
        host.validate_gemma_config(SMALL, 2, 1)
    with pytest.raises(ValueError, match="draft_tokens > 0 cannot be combined with kv_fp8"):
        host.validate_gemma_config(SMALL, 1, 2, kv_fp8=True)
    with pytest.raises(ValueError, match="draft_tokens > 0 cannot be combined with bounded_local_kv .*stale rows"):
        host.validate_gemma_config(dict(SMALL, bounded_local_kv=1), 1, 3)
    with pytest.raises(ValueError, match="head dimensions of 64, 128, 256 or 512"):
        host.validate_gemma_config(dict(SMALL, head_dim=32), 1, 1)
    # the refusals that were there stay: the new axis lifts none of them
    with pytest.raises(ValueError, match="max_batch 5 outside"):
        host.validate_gemma_config(SMALL, 5, 0)
    with pytest.raises(ValueError, match="max_batch > 1 cannot be combined with kv_fp8"):
        host.validate_gemma_config(SMALL, 2, 0, kv_fp8=True)
    with pytest.raises(ValueError, match="max_batch > 1 cannot be combined with bounded_local_kv"):
        host.validate_gemma_config(dict(SMALL, bounded_local_kv=1), 2, 0)


def test_the_host_binding_carries_the_chain_entries(lib):
    import inspect
    from mila_amd import host
    assert [n for n, _ in host.GemmaConfigC._fields_][-2:] == ["bounded_local_kv", "kv_fp8"]      # mila_gemma_config is unchanged: draft_tokens travels through new create entries
    h = host.load()
    for n in ("gemma_create_chain", "gemma_chain_decode", "gemma_chain_graph_info", "gemma_time_chain_decode", "gemma_validate_config", "gemma_prompt_lookup_draft",
              "gemma_model_synthetic_chain", "gemma_model_generate_spec", "gemma_model_speculation_stats"):
        assert hasattr(h, "mila_" + n), n
    assert inspect.signature(host.Gemma.__init__).parameters["draft_tokens"].default is None
    assert inspect.signature(host.GemmaModel.synthetic).parameters["draft_tokens"].default is None
    assert inspect.signature(host.GemmaModel.generate).parameters["draft_hint"].default is None
    for n in ("decode_chain", "chain_graph_info"):
        assert hasattr(host.Gemma, n), n
    assert hasattr(host.GemmaModel, "speculation_stats")


def _lookup(history, k):
    """the rule restated: for n = 3, 2, 1 the latest occurrence of the last n tokens that starts before the suffix does; the up-to-k tokens behind it"""
    h = len(history)
    for n in (3, 2, 1):
        if h < n + 1:
            continue
        suffix = history[h - n:]
        starts = [j for j in range(h - n) if history[j:j + n] == suffix]
        if starts:
            first = starts[-1] + n
            return history[first:first + k]
    return []


def test_the_default_drafter_is_prompt_lookup(lib):
    from mila_amd import host
    cases = {
        "no match": [1, 2, 3, 4, 5, 6],
        "match at n = 1 only": [7, 1, 2, 3, 9, 8, 7],                       # ... 7 follows nothing like [8, 7] or [9, 8, 7]
        "two candidates, the latest wins": [5, 6, 7, 1, 1, 5, 6, 7, 2, 2, 5, 6, 7],
        "fewer than k followers": [4, 4, 9, 3, 4, 4, 9],                   # the occurrence [4, 4, 9] at 0 is followed by 3, 4, 4, 9
        "the latest occurrence overlaps the suffix": [3, 3, 3, 3],
        "a longer n decides before a later shorter match": [1, 2, 3, 8, 3, 9, 1, 2, 3],
        "short histories": [5],
        "two tokens": [5, 5],
        "empty": [],
    }
    for name, hist in cases.items():
        for k in (1, 2, 3):
            assert host.prompt_lookup_draft(hist, k) == _lookup(hist, k), (name, k)
    assert host.prompt_lookup_draft(cases["no match"], 3) == []
    assert host.prompt_lookup_draft(cases["match at n = 1 only"], 3) == [1, 2, 3]
    assert host.prompt_lookup_draft(cases["two candidates, the latest wins"], 3) == [2, 2, 5]
    assert host.prompt_lookup_draft([9, 1, 2, 3, 4, 7, 9], 2) == [1, 2]
    assert host.prompt_lookup_draft([4, 8, 4], 3) == [8, 4]              # fewer than k followers: the history ends
    assert host.prompt_lookup_draft([3, 3, 3, 3], 3) == [3]
    assert host.prompt_lookup_draft([5, 6, 7], 0) == []
    rng = __import__("random").Random(7)
    for _ in range(200):
        hist = [rng.randrange(4) for _ in range(rng.randrange(0, 24))]
        k = rng.randrange(1, 4)
        assert host.prompt_lookup_draft(hist, k) == _lookup(hist, k), (hist, k)
