"""GPU: the three kernel entries of the FP8 KV cache under batched rows, through the C ABI -- fused_qkv_post_kvfp8_rows_devpos, attn_decode_kvfp8_rows (both kernel forms)
and kv_rows_fork_layers_kvfp8.  THE ORACLE of the first two is the one-row entry (fused_qkv_post_kvfp8_devpos, attn_decode_kvfp8_devpos with B = 1) on the row's own
slices at the row's own position, compared as bit patterns -- the rows forms are twins of entries that are pinned bit for bit already -- plus one decode case against
float64 on the dequantized caches at the bar of tests/test_kvfp8_gpu.py, so that a mistake the twin shares would not pass.  The fork is compared with a numpy copy, byte
for byte.  Cache rows a call must not touch hold a sentinel, cache rows a row must not read hold the e4m3 NaN code and a NaN scale."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from gpu_util import assert_bf16_close, bits, dev_i32, dev_u16, empty_u16, host
from mila_amd import capi
from test_kvfp8_gpu import POISON8, Cache8, _bf, _d, _quantize

pytestmark = pytest.mark.gpu

EPS = 1e-6
SENT8, SENTS = 0xA5, 0x7fc12345      # a byte the quantizer may emit anywhere, so the comparison is positional; a NaN pattern no scale computation produces


def _u32(t):
    return host(t).view(np.uint32)


def _scratch(B, NH, HS):
    n = capi.load().mila_cdna4_attn_decode_scratch_bytes(B, NH, HS)
    return torch.empty(n, dtype=torch.uint8, device="cuda"), C.c_size_t(n)


# ---- (a) the append ---------------------------------------------------------------------------------------------------------------------------------------------
CAP = 40
POSITIONS = [0, 5, CAP - 1, 17]


def _sentinel_caches(B, NKV, HS):
    K8 = torch.full((B, NKV, CAP, HS), SENT8, dtype=torch.uint8, device="cuda")
    Ks = torch.from_numpy(np.full((B, NKV, CAP), SENTS, np.uint32).view(np.float32)).cuda()
    return K8, K8.clone(), Ks, Ks.clone()


@pytest.mark.parametrize("glob", [False, True], ids=["local", "global"])
@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("NH,NKV", [(4, 2), (16, 1)])
@pytest.mark.parametrize("HS", [64, 128, 256, 512])
def test_the_rows_append_is_the_one_row_append_per_row(HS, NH, NKV, B, glob):
    """row b of one call against fused_qkv_post_kvfp8_devpos on row b's slices at positions[b]: q_out, bytes and scales; every other cache row keeps the sentinel.
    NH + 2 NKV (8, 18) is no multiple of the head rows a wave takes at any of the head sizes' 4 x 64 / (HS / 16) per workgroup: the last workgroup is partial.  glob:
    the call of a global layer, v_src == k"""
    rng = np.random.default_rng(HS + NH + B)
    PK = (NH + 2 * NKV) * HS + 24                      # the rows of the packed projection are wider than what this layer reads (a multiple of 8)
    raw = dev_u16(orc.to_bf16_bits(_bf(rng.standard_normal((B, PK)))))
    qw, kw, vw = (dev_u16(orc.to_bf16_bits(_bf(1 + 0.1 * rng.uniform(-1, 1, HS)))) for _ in range(3))
    ang = rng.uniform(0, 2 * np.pi, (CAP, HS // 2)).astype(np.float32)
    cos, sin = torch.from_numpy(np.cos(ang)).cuda(), torch.from_numpy(np.sin(ang)).cuda()
    pos = POSITIONS[:B]
    q_of = lambda b: raw[b]
    k_of = lambda b: raw[b, NH * HS:]
    v_of = lambda b: k_of(b) if glob else raw[b, (NH + NKV) * HS:]

    got, q_got = _sentinel_caches(B, NKV, HS), empty_u16(B, NH * HS)
    capi.call("fused_qkv_post_kvfp8_rows_devpos", q_got, *got, q_of(0), k_of(0), v_of(0), C.c_int64(PK), qw, kw, vw, cos, sin, B, NH, NKV, HS, dev_i32(pos), CAP, EPS)

    exp, q_exp = _sentinel_caches(B, NKV, HS), empty_u16(B, NH * HS)
    for b in range(B):
        capi.call("fused_qkv_post_kvfp8_devpos", q_exp[b], *[t[b] for t in exp], q_of(b), k_of(b), v_of(b), qw, kw, vw, cos, sin, NH, NKV, HS, dev_i32([pos[b]]), CAP, EPS)
    assert np.array_equal(bits(q_got), bits(q_exp)), "q_out"
    for name, g, e in zip(("K8", "V8"), got[:2], exp[:2]):
        assert np.array_equal(host(g), host(e)), name
    for name, g, e in zip(("Ks", "Vs"), got[2:], exp[2:]):
        assert np.array_equal(_u32(g), _u32(e)), name
    # the oracle itself wrote one cache row per (row, head) and nothing else: B x NKV rows differ from the sentinel, the ones at positions[b]
    ks = _u32(got[2])
    for b in range(B):
        written = np.nonzero((ks[b] != SENTS).any(axis=0))[0]
        assert list(written) == [pos[b]], (b, written)


# ---- (b) the decode, wave-per-position form -----------------------------------------------------------------------------------------------------------------------
CAP_D, MAX_LEN = 320, 300


def _random_caches(B, NKV, cap, HS, seed):
    """valid e4m3 codes (no NaN code) and positive scales, straight on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    def code():
        return (torch.randint(0, 0x7f, (B, NKV, cap, HS), generator=g, device="cuda", dtype=torch.int32) | (torch.randint(0, 2, (B, NKV, cap, HS), generator=g, device="cuda", dtype=torch.int32) << 7)).to(torch.uint8)
    def scale():
        return torch.rand((B, NKV, cap), generator=g, device="cuda") * 0.004 + 0.001
    return code(), code(), scale(), scale()


def _poison_outside(caches, lens, window):
    """what row b must not read: positions >= its live length and, under a window, the ones older than its band"""
    K8, V8, Ks, Vs = caches
    for b, n in enumerate(lens):
        dead = [(n, K8.shape[2])] + ([(0, n - window)] if window > 0 and n > window else [])
        for lo, hi in dead:
            K8[b, :, lo:hi] = POISON8
            V8[b, :, lo:hi] = POISON8
            Ks[b, :, lo:hi] = float("nan")
            Vs[b, :, lo:hi] = float("nan")


def _rows_decode(caches, q, NH, NKV, HS, cap, pos, max_len, window, scale):
    B = len(pos)
    scratch, n = _scratch(B, NH, HS)
    Y = empty_u16(B, NH * HS)
    capi.call("attn_decode_kvfp8_rows", Y, q, *caches, scratch, n, B, NH, NKV, HS, cap, dev_i32(pos), max_len, window, float(scale))
    return bits(Y)


def _alone_decode(caches, q, b, NH, NKV, HS, cap, position, max_len, window, scale):
    scratch, n = _scratch(1, NH, HS)
    Y = empty_u16(1, NH * HS)
    capi.call("attn_decode_kvfp8_devpos", Y, q[b], *[t[b] for t in caches], scratch, n, 1, NH, NKV, HS, cap, dev_i32([position]), max_len, window, float(scale))
    return bits(Y)[0]


@pytest.mark.parametrize("window", [0, 8])
@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("GS", [1, 2, 8])
@pytest.mark.parametrize("HS", [64, 128, 256, 512])
def test_the_rows_decode_is_the_one_row_decode_per_row(HS, GS, B, window):
    """unwindowed: the band of max_len = 300 is split (asserted), rows at position 0 (one key: every split but the first is idle), at max_len - 1, at 3 and at 150.
    window = 8: one split (asserted), rows at max_len - 1 (far above the window), 0, 20 (above it) and 5 (below it).  Row b against attn_decode_kvfp8_devpos with
    B = 1 on its slices, the same max_len"""
    NKV = 2
    NH = NKV * GS
    plan = capi.attn_decode_kvfp8_plan(1, NH, NKV, HS, CAP_D, window, MAX_LEN)
    assert plan["form"] == "attn_decode_kvfp8" and (plan["splits"] > 1 if window == 0 else plan["splits"] == 1), plan
    pos = ([0, MAX_LEN - 1, 3, 150] if window == 0 else [MAX_LEN - 1, 0, 20, 5])[:B]
    caches = _random_caches(B, NKV, CAP_D, HS, HS + GS + B + window)
    _poison_outside(caches, [p + 1 for p in pos], window)
    q = dev_u16(orc.to_bf16_bits(_bf(np.random.default_rng(HS * GS + B).uniform(-1, 1, (B, NH * HS)))))
    scale = HS ** -0.5
    capi.last_form()
    got = _rows_decode(caches, q, NH, NKV, HS, CAP_D, pos, MAX_LEN, window, scale)
    assert capi.last_form() == ["attn_decode_kvfp8"]
    assert np.isfinite(orc.from_bf16_bits(got)).all(), "a dead cache row was read"
    for b in range(B):
        want = _alone_decode(caches, q, b, NH, NKV, HS, CAP_D, pos[b], MAX_LEN, window, scale)
        assert np.array_equal(got[b], want), "row %d at position %d" % (b, pos[b])


def test_the_rows_decode_against_float64_on_the_dequantized_caches():
    """three rows of different histories at positions 0, 299 and 37 on (NH 16, NKV 8, HS 256) -- the Gemma local geometry of tests/test_kvfp8_gpu.py, unwindowed so that
    the band is split -- against orc.gqa_attention on the dequantized values, at that file's bar for the shape: <= 1 bf16 ulp + 2e-3 abs"""
    rng = np.random.default_rng(41)
    B, NH, NKV, HS, cap, scale = 3, 16, 8, 256, CAP_D, 1.0
    pos = [0, MAX_LEN - 1, 37]
    assert capi.attn_decode_kvfp8_plan(1, NH, NKV, HS, cap, 0, MAX_LEN)["splits"] > 1
    hk = _bf(rng.uniform(-1, 1, (B, MAX_LEN, NKV, HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (B, MAX_LEN, NKV, HS)))
    q = _bf(rng.uniform(-1, 1, (B, 1, NH, HS)))
    c = Cache8(B, NKV, cap, HS).fill(hk, hv, 128)
    for b, p in enumerate(pos):      # a row holds its own history only
        for t8 in (c.K8, c.V8):
            t8[b, :, p + 1:] = POISON8
        for ts in (c.Ks, c.Vs):
            ts[b, :, p + 1:] = float("nan")
    got = _rows_decode(c.arrays(), _d(q).reshape(B, NH * HS), NH, NKV, HS, cap, pos, MAX_LEN, 0, scale)
    dk, dv = _quantize(hk)[2], _quantize(hv)[2]
    for b, p in enumerate(pos):
        exp = orc.gqa_attention(q[b:b + 1], dk[b:b + 1, :p + 1], dv[b:b + 1, :p + 1], p, 0, scale)[:, 0]
        assert_bf16_close(got[b], exp, 1, 2e-3, "row %d at position %d" % (b, p))


# ---- (b) the decode, matrix-core form ---------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_core_rows_decode_is_the_one_row_decode_per_row():
    """16 heads on one KV head at HS 512, a bound in the bucket above 8192 keys: rows at 8200 and at 3 (four keys: nearly every split idle)"""
    B, NH, NKV, HS, cap, max_len, pos = 2, 16, 1, 512, 8320, 8201, [8200, 3]
    plan = capi.attn_decode_kvfp8_plan(1, NH, NKV, HS, cap, 0, max_len)
    assert plan["form"] == "attn_decode_kvfp8_mfma" and plan["splits"] > 1, plan
    caches = _random_caches(B, NKV, cap, HS, 512)
    _poison_outside(caches, [p + 1 for p in pos], 0)
    q = dev_u16(orc.to_bf16_bits(_bf(np.random.default_rng(5).uniform(-1, 1, (B, NH * HS)))))
    capi.last_form()
    got = _rows_decode(caches, q, NH, NKV, HS, cap, pos, max_len, 0, HS ** -0.5)
    assert capi.last_form() == ["attn_decode_kvfp8_mfma"]
    assert np.isfinite(orc.from_bf16_bits(got)).all(), "a dead cache row was read"
    for b in range(B):
        want = _alone_decode(caches, q, b, NH, NKV, HS, cap, pos[b], max_len, 0, HS ** -0.5)
        assert np.array_equal(got[b], want), "row %d at position %d" % (b, pos[b])


# ---- (c) the fork -----------------------------------------------------------------------------------------------------------------------------------------------
LAYERS = [(2, 37, 64), (1, 50, 128)]      # (NKV, capacity, HS)
ROWS, SRC, MASK = 4, 2, 0b1011


def _fork_layer(rng, NKV, cap, HS):
    K8 = rng.integers(0, 256, (ROWS, NKV, cap, HS), dtype=np.uint8)
    V8 = rng.integers(0, 256, (ROWS, NKV, cap, HS), dtype=np.uint8)
    K8[SRC, :, 0, :8] = [0x7f, 0xff, 0x00, 0x80, 0x7e, 0xfe, 0x01, 0x81]      # the NaN codes, both zeros, the extremes
    V8[SRC, :, 0, -4:] = [0xff, 0x7f, 0xff, 0x7f]
    Ks = rng.integers(0, 2 ** 32, (ROWS, NKV, cap), dtype=np.uint32)
    Vs = rng.integers(0, 2 ** 32, (ROWS, NKV, cap), dtype=np.uint32)
    Ks[SRC, :, 0] = 0x7fc00001      # a NaN with a payload
    Vs[SRC, :, 0] = 0x80000000      # -0.0
    Ks[SRC, 0, 0] = 0x00000001      # the smallest denormal
    Vs[SRC, 0, 0] = 0xff800001      # a signalling NaN
    return K8, V8, Ks, Vs


@pytest.mark.parametrize("length", [1, 5, 37])
def test_the_fork_copies_bytes_and_scale_words_bit_for_bit_and_nothing_else(length):
    """two layers of different (NKV, capacity, HS), row 2 into rows 0, 1 and 3; len 1, 5 (odd against four-word alignment: a head's scale run starts at capacity * 4
    bytes, 37 and 50 words apart) and 37 (layer 0's whole capacity).  The source row, and everything at [len, capacity) of every row, stay as they were"""
    rng = np.random.default_rng(length)
    hosts = [_fork_layer(rng, *l) for l in LAYERS]
    dev = [[torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in h] for h in hosts]
    table = (capi.KvForkLayerFp8 * len(LAYERS))()
    for i, ((NKV, cap, HS), d) in enumerate(zip(LAYERS, dev)):
        table[i].K8, table[i].V8, table[i].Ks, table[i].Vs = (t.data_ptr() for t in d)
        table[i].NKV, table[i].capacity, table[i].HS, table[i].reserved = NKV, cap, HS, 0
    capi.call("kv_rows_fork_layers_kvfp8", table, len(LAYERS), ROWS, SRC, MASK, length)
    for i, (h, d) in enumerate(zip(hosts, dev)):
        for name, a, t in zip(("K8", "V8", "Ks", "Vs"), h, d):
            want = a.copy()
            for r in range(ROWS):
                if (MASK >> r) & 1:
                    want[r, :, :length] = a[SRC, :, :length]
            got = host(t)
            got = got.view(np.uint32) if a.dtype == np.uint32 else got
            assert np.array_equal(got, want), "layer %d %s" % (i, name)
            assert np.array_equal(got[SRC], a[SRC]) and np.array_equal(got[:, :, length:], a[:, :, length:]), "layer %d %s: outside the copy" % (i, name)
    with pytest.raises(capi.InvalidArgument):      # beyond layer 0's capacity, though layer 1 would hold it
        capi.call("kv_rows_fork_layers_kvfp8", table, len(LAYERS), ROWS, SRC, MASK, 38)
