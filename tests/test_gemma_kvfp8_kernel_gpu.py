"""fused_qkv_post_kvfp8 / _prefill / _devpos (csrc/fused.hip): the q/k/v post-processing launch with a quantizing append into the FP8 KV cache.  The contract is bit
equality with a chain of two existing entries -- fused_qkv_post[_prefill|_devpos] into bf16 scratch caches, then kv_write_fp8[_devpos] on the rows it wrote -- for
q_out, the cache bytes and the scales; every cache starts poisoned, and no row other than the appended ones may change.

Shapes: the smallest that reach every lane-group class of the kernel (hv = HS / 16 lanes per row: 4, 8, 16, 32) and its row tail -- HS 64: 8 rows of a 64-row
workgroup; HS 128: 6 of 32 (global form: v_src == k, no V weight); HS 256: 32 rows = two workgroups of 16; HS 512: 18 rows = three workgroups of 8, the last with 2
(global form).  Ring capacity 24: the eager and device-position legs append at positions 29 / 30 (rows 5 / 6), the prefill leg 5 tokens from 22 (rows 22, 23, 0, 1, 2)
from packed rows whose stride is not the sum of the parts.  One token of the prefill leg has an all-zero raw K row for KV head 0: scale 1, zero bytes."""
import numpy as np
import pytest
import torch

import orc
from gpu_util import bits, dev_i32, dev_u16, empty_f32, empty_u16, host
from mila_amd import capi

pytestmark = pytest.mark.gpu

CAP, MAX_SEQ, EPS = 24, 32, 1e-6
POISON16, POISON8 = 0x7fc0, 0xff
SHAPES = [(64, 4, 2, False), (128, 4, 1, True), (256, 16, 8, False), (512, 16, 1, True)]      # HS, NH, NKV, global form


def _bf(x):
    return orc.to_bf16_bits(np.asarray(x, dtype=np.float32))


class Case:
    def __init__(self, HS, NH, NKV, shared, T, zero_k_row=None):
        rng = np.random.default_rng(1000 * HS + 10 * NH + T)
        self.HS, self.NH, self.NKV, self.shared, self.T = HS, NH, NKV, shared, T
        qd, kd = NH * HS, NKV * HS
        self.stride = qd + kd * (1 if shared else 2) + 24                      # a multiple of 8 that is not the sum of the parts
        rows = rng.standard_normal((T, self.stride)).astype(np.float32) * rng.uniform(0.25, 4.0, (T, 1)).astype(np.float32)
        if zero_k_row is not None:
            rows[zero_k_row, qd:qd + HS] = 0.0                                  # raw K of KV head 0 (and, in the global form, its V source)
        self.P = dev_u16(_bf(rows))
        self.q, self.k = self.P[0, 0:], self.P[0, qd:]
        self.v = self.k if shared else self.P[0, qd + kd:]
        self.qw, self.kw = (dev_u16(_bf(0.35 + 0.035 * rng.uniform(-1, 1, HS))) for _ in range(2))
        self.vw = None if shared else dev_u16(_bf(1 + 0.1 * rng.uniform(-1, 1, HS)))
        self.cos, self.sin = empty_f32(MAX_SEQ, HS // 2), empty_f32(MAX_SEQ, HS // 2)
        capi.call("rope_build_cache", self.cos, self.sin, MAX_SEQ, HS, 1e6 if shared else 1e4, HS // 4 if shared else 0)

    def bf16_caches(self):
        return [torch.full((self.NKV, CAP, self.HS), POISON16, dtype=torch.int16, device="cuda") for _ in range(2)]

    def fp8_caches(self):
        return ([torch.full((self.NKV, CAP, self.HS), POISON8, dtype=torch.uint8, device="cuda") for _ in range(2)] +
                [torch.full((self.NKV, CAP), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)])

    def gather(self, Kc, rows):
        """cache rows [NKV, CAP, HS] at `rows` -> kv_write_fp8's source layout [1, T, NKV * HS]"""
        idx = torch.as_tensor(rows, device="cuda")
        return Kc[:, idx, :].permute(1, 0, 2).contiguous()

    def check(self, got_q, exp_q, got, exp, rows, what):
        assert np.array_equal(bits(got_q), bits(exp_q)), what + ": q_out"
        assert not np.any(bits(got_q) == POISON16), what + ": q_out not fully written"
        others = np.setdiff1d(np.arange(CAP), np.asarray(rows) % CAP)
        for name, g, e in zip(("K8", "V8", "Ks", "Vs"), got, exp):
            g, e = host(g), host(e)
            gv, ev = (g.view(np.uint32), e.view(np.uint32)) if g.dtype == np.float32 else (g, e)
            assert np.array_equal(gv, ev), "%s: %s differs from the two-entry chain" % (what, name)
            if g.dtype == np.float32:
                assert np.all(np.isnan(g[:, others])) and np.all(np.isfinite(g[:, np.asarray(rows) % CAP])), "%s: %s rows" % (what, name)
            else:
                assert np.all(g[:, others] == POISON8), "%s: %s wrote a row that was not appended" % (what, name)
        return [host(t) for t in got]


@pytest.mark.parametrize("HS,NH,NKV,shared", SHAPES)
def test_eager_form_is_the_two_entry_chain(HS, NH, NKV, shared):
    c, pos = Case(HS, NH, NKV, shared, 1), 29                                     # row 29 % 24 = 5: the ring has wrapped
    Kc, Vc = c.bf16_caches()
    q0 = empty_u16(NH, HS)
    capi.call("fused_qkv_post", q0, Kc, Vc, c.q, c.k, c.v, c.qw, c.kw, c.vw, c.cos, c.sin, NH, NKV, HS, pos, CAP, EPS)
    exp = c.fp8_caches()
    capi.call("kv_write_fp8", *exp, c.gather(Kc, [pos % CAP]), c.gather(Vc, [pos % CAP]), 1, 1, NKV, HS, pos, CAP)
    got, q1 = c.fp8_caches(), empty_u16(NH, HS)
    capi.call("fused_qkv_post_kvfp8", q1, *got, c.q, c.k, c.v, c.qw, c.kw, c.vw, c.cos, c.sin, NH, NKV, HS, pos, CAP, EPS)
    c.check(q1, q0, got, exp, [pos], "eager HS=%d" % HS)


@pytest.mark.parametrize("HS,NH,NKV,shared", SHAPES)
def test_prefill_form_is_the_two_entry_chain_and_a_zero_row_gets_scale_one(HS, NH, NKV, shared):
    T, pos0 = 5, 22                                                                # rows 22, 23, 0, 1, 2: the chunk wraps inside itself
    c = Case(HS, NH, NKV, shared, T, zero_k_row=3)
    rows = [(pos0 + t) % CAP for t in range(T)]
    Kc, Vc = c.bf16_caches()
    q0 = empty_u16(T, NH * HS)
    capi.call("fused_qkv_post_prefill", q0, Kc, Vc, c.q, c.k, c.v, capi.C.c_int64(c.stride), c.qw, c.kw, c.vw, c.cos, c.sin, T, NH, NKV, HS, pos0, CAP, EPS)
    exp = c.fp8_caches()
    capi.call("kv_write_fp8", *exp, c.gather(Kc, rows), c.gather(Vc, rows), 1, T, NKV, HS, pos0, CAP)
    got, q1 = c.fp8_caches(), empty_u16(T, NH * HS)
    capi.call("fused_qkv_post_kvfp8_prefill", q1, *got, c.q, c.k, c.v, capi.C.c_int64(c.stride), c.qw, c.kw, c.vw, c.cos, c.sin, T, NH, NKV, HS, pos0, CAP, EPS)
    K8, V8, Ks, Vs = c.check(q1, q0, got, exp, rows, "prefill HS=%d" % HS)
    # the all-zero raw K row of KV head 0: scale 1 and zero bytes, as the weight quantizer does (0x00 or 0x80: the rotation 0 * cos - 0 * sin leaves signed zeros in the
    # bf16 row, and the quantizer keeps the sign)
    zr = rows[3]
    assert Ks[0, zr] == 1.0 and not (K8[0, zr] & 0x7f).any()
    if shared:                                                                     # ... and V comes from the same raw row in the global form
        assert Vs[0, zr] == 1.0 and not (V8[0, zr] & 0x7f).any()
    live = np.ones((NKV, CAP), bool)
    live[0, zr] = False
    live[:, np.setdiff1d(np.arange(CAP), rows)] = False
    assert np.all((K8[live] & 0x7f).max(axis=-1) == 0x7e)                          # every other appended row reaches +-448: absmax / 448 scaling
    # the bytes are the oracle quantizer's on the chain's bf16 rows (the chain itself is pinned by tests/test_kvfp8_gpu.py; this ties the new entry to the oracle directly)
    kq, ks = orc.quantize_fp8_per_channel(bits(Kc)[:, rows, :].reshape(-1, HS))
    assert np.array_equal(kq.reshape(NKV, T, HS), K8[:, rows, :]) and np.array_equal(ks.reshape(NKV, T), Ks[:, rows])


@pytest.mark.parametrize("HS,NH,NKV,shared", SHAPES)
def test_device_position_form_is_the_two_entry_chain(HS, NH, NKV, shared):
    c, pos = Case(HS, NH, NKV, shared, 1), 30
    pos_dev = dev_i32([pos])
    Kc, Vc = c.bf16_caches()
    q0 = empty_u16(NH, HS)
    capi.call("fused_qkv_post_devpos", q0, Kc, Vc, c.q, c.k, c.v, c.qw, c.kw, c.vw, c.cos, c.sin, NH, NKV, HS, pos_dev, CAP, EPS)
    exp = c.fp8_caches()
    capi.call("kv_write_fp8_devpos", *exp, c.gather(Kc, [pos % CAP]), c.gather(Vc, [pos % CAP]), 1, NKV, HS, pos_dev, CAP)
    got, q1 = c.fp8_caches(), empty_u16(NH, HS)
    capi.call("fused_qkv_post_kvfp8_devpos", q1, *got, c.q, c.k, c.v, c.qw, c.kw, c.vw, c.cos, c.sin, NH, NKV, HS, pos_dev, CAP, EPS)
    c.check(q1, q0, got, exp, [pos], "devpos HS=%d" % HS)
    assert host(pos_dev)[0] == pos                                                 # read, not advanced
