"""GPU parity of prefill attention (attn_prefill_bf16: flash_prefill_kernel, flash_prefill_kernel_s1, flash_prefill_pp_kernel) with the float64 oracle at every class of
tests/attn_prefill_classes.py: each instantiation the default flash.form reaches, windowed and unwindowed, batches of 2 and 3, workgroups of 1 to 11 key tiles -- so
every lean-loop pair count of the double-buffered kernels and the register-staged kernel's two-tiles-ahead staging past tile 2 --, ragged query tiles, chunks of 1 to
65 rows behind a history, wrapped rings, and the heavy / light work list with a partly filled last round.  tests/test_attn_prefill_classes_cpu.py holds every row of
the table to the plan it is there for.

Data as in tests/test_attention_gpu.py: q uniform(-1, 1), K uniform(-1, 1) * 0.5, V uniform(-1, 1), bf16-rounded; caches filled through kv_write_bf16; every batch row
has a history of its own, so a kernel that reads another row's cache or query fails.  Dead cache rows hold NaN -- rows the history has not reached yet, and rows below
the tile-aligned first key of a launch's band (the kernels read the rows between that and the band, masked: those stay finite) -- and Y holds NaN bits before every
launch: an element no workgroup wrote fails.  After every launch capi.last_form() must name the instantiation the row is there for.  The bar is the project's:
<= 1 bf16 ulp + 2e-3 abs against orc.gqa_attention on the linear history.

A row's history is drawn once (functools.lru_cache) and never modified."""
import ctypes as C
import functools
import types
import zlib

import numpy as np
import pytest
import torch

import orc
from attn_prefill_classes import (BY_NAME, FORMS, FROM_ZERO_T, HISTORY, PARTIAL_ROWS, PARTIAL_T, ROWS, SPIKE_GAIN, history_len, partial_sample_rows, poison_floor,
                                  ring_capacity, schedule, spikes)
from gpu_util import assert_bf16_close, bits, dev_u16, empty_u16
from mila_amd import capi

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7fc0
ALL = dict(BY_NAME, **{r.name: r for r, _ in PARTIAL_ROWS})
IDS = [r.name for r in ROWS]
WINDOWED = [r.name for r in ROWS if r.window]
TUNABLE = [r.name for r in ROWS if r.HS >= 256]      # (below HS 256 every flash.form plans the register-staged kernel: tests/test_attn_prefill_classes_cpu.py)


def _bf(x):
    return orc.round_bf16(np.asarray(x, dtype=np.float32))


def _d(x):
    return dev_u16(orc.to_bf16_bits(x))


@functools.lru_cache(maxsize=2)
def _data(name, spiked=False):
    """q [B, T, NH, HS] (row t is the query at position t), hk / hv [B, T, NKV, HS]: the history of a row; spiked: the from_zero history, with the K rows of
    attn_prefill_classes.spikes set to half a query of their batch row"""
    row = ALL[name]
    T = PARTIAL_T if name not in BY_NAME else history_len(row)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    q = _bf(rng.uniform(-1, 1, (row.B, T, row.NH, row.HS)))
    hk = _bf(rng.uniform(-1, 1, (row.B, T, row.NKV, row.HS)) * 0.5)
    hv = _bf(rng.uniform(-1, 1, (row.B, T, row.NKV, row.HS)))
    if spiked:
        for key, qrow, head in spikes(row):
            hk[:, key, head // (row.NH // row.NKV)] = _bf(q[:, qrow, head] * SPIKE_GAIN)
    for a in (q, hk, hv):
        a.setflags(write=False)
    return types.SimpleNamespace(T=T, q=q, hk=hk, hv=hv, qd=_d(q), kd=_d(hk), vd=_d(hv))


def _poisoned(row, cap):
    return tuple(torch.full((row.B, row.NKV, cap, row.HS), NAN_BITS, dtype=torch.int16, device="cuda") for _ in range(2))


def _append(row, d, Kc, Vc, cap, first, end):
    capi.call("kv_write_bf16", Kc, Vc, d.kd[:, first:end].contiguous(), d.vd[:, first:end].contiguous(), row.B, end - first, row.NKV, row.HS, first, cap)


def _prefill(row, d, Kc, Vc, cap, pos, chunk, want_form):
    """one launch over rows pos .. pos + chunk - 1 into NaN-filled Y; the bits"""
    Y = empty_u16(row.B, chunk, row.NH * row.HS)
    capi.last_form()                        # (clears the record)
    capi.call("attn_prefill_bf16", Y, d.qd[:, pos:pos + chunk].contiguous(), Kc, Vc, row.B, chunk, row.NH, row.NKV, row.HS, cap, pos, row.window, float(row.scale))
    assert capi.last_form() == [want_form], "launch (%d, %d) of %s" % (pos, chunk, row.name)
    return bits(Y).copy()


def _form_name(row, pos, chunk):
    return capi.prefill_form_name(capi.attn_prefill_plan(row.HS, row.NH, row.NKV, chunk, pos, row.window), row.HS)


def _run(row, d, launches, cap, unbounded=True):
    """the launches of a schedule, each behind the kv_write of the rows in front of it and of its own; an unbounded cache loses (to NaN) the rows below every later
    band's tile-aligned first key.  -> (caches, [bits of Y per launch])"""
    Kc, Vc = _poisoned(row, cap)
    out, written = [], 0
    for pos, chunk in launches:
        _append(row, d, Kc, Vc, cap, written, pos + chunk)
        written = pos + chunk
        if unbounded:
            floor = poison_floor(pos, row.window)
            Kc[:, :, :floor] = NAN_BITS
            Vc[:, :, :floor] = NAN_BITS
        out.append(_prefill(row, d, Kc, Vc, cap, pos, chunk, _form_name(row, pos, chunk)))
    return (Kc, Vc), out


def _oracle(row, d, pos, chunk):
    return orc.gqa_attention(d.q[:, pos:pos + chunk], d.hk[:, :pos + chunk], d.hv[:, :pos + chunk], pos, row.window, row.scale)


def _check(row, d, launches, ys, what):
    for (pos, chunk), y in zip(launches, ys):
        assert_bf16_close(y, _oracle(row, d, pos, chunk), 1, 2e-3, "%s %s launch (%d, %d)" % (what, row.name, pos, chunk))
        print("PREFILL_CLASS %-16s %-15s pos %4d chunk %4d via %s" % (row.name, what, pos, chunk, _form_name(row, pos, chunk)))


@pytest.mark.parametrize("name", IDS)
def test_from_zero_matches_the_oracle_in_every_class(name):
    """one chunk of 229 rows from position 0: workgroups of 1 to 8 key tiles (unwindowed), a ragged last query tile, two spiked keys that move a head's running maximum
    late in its band (inside the lean loop where there is one); all of Y against the oracle, and attn_decode_bf16 at the last position against the same oracle row"""
    row = BY_NAME[name]
    assert capi.attn_prefill_plan(row.HS, row.NH, row.NKV, FROM_ZERO_T, 0, row.window)["form"] == row.plan["form"]
    d = _data(name, True)
    launches = schedule(row, "from_zero")
    cap = FROM_ZERO_T + 64
    (Kc, Vc), ys = _run(row, d, launches, cap)
    _check(row, d, launches, ys, "from_zero")
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(row.B, row.NH, row.HS)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    Yd = empty_u16(row.B, row.NH * row.HS)
    capi.call("attn_decode_bf16", Yd, d.qd[:, FROM_ZERO_T - 1].contiguous(), Kc, Vc, scratch, C.c_size_t(nbytes), row.B, row.NH, row.NKV, row.HS, cap, FROM_ZERO_T,
              row.window, float(row.scale))
    assert_bf16_close(bits(Yd), _oracle(row, d, 0, FROM_ZERO_T)[:, FROM_ZERO_T - 1], 1, 2e-3, "decode at the last from_zero row of " + name)


@pytest.mark.parametrize("name", IDS)
def test_short_start_matches_the_oracle_in_every_class(name):
    """chunks of 20, 45 and 31 rows from position 0: one key tile for every workgroup shape, and three for the 64-row ones"""
    row = BY_NAME[name]
    d = _data(name)
    launches = schedule(row, "short_start")
    _, ys = _run(row, d, launches, HISTORY + 32)
    _check(row, d, launches, ys, "short_start")


@pytest.mark.parametrize("name", IDS)
def test_behind_history_matches_the_oracle_in_every_class(name):
    """96 cached positions, then chunks of 1, 15, 16, 17, 31, 32, 33, 63, 64 and 65 rows back to back: fewer rows than, as many as and more than a workgroup holds at every
    workgroup shape, a one-row prefill, and -- unwindowed -- at least four key tiles in every workgroup of every launch"""
    row = BY_NAME[name]
    d = _data(name)
    launches = schedule(row, "behind_history")
    _, ys = _run(row, d, launches, d.T + 32)
    _check(row, d, launches, ys, "behind_history")


@pytest.mark.parametrize("name", WINDOWED)
def test_ring_equals_unbounded_and_the_oracle_in_every_class(name):
    """chunks of 40 rows into a ring of window + 39 rows -- exactly the rows the entry asks for -- until the history is three capacities long: every launch whose last
    position is at or beyond the capacity takes the wrapped-ring path of its kernel (every tile in the general form); its bits are those of an unbounded cache whose
    rows below the band hold NaN, and meet the oracle"""
    row = BY_NAME[name]
    d = _data(name)
    launches = schedule(row, "ring")
    cap = ring_capacity(row)
    assert sum(p + c - 1 >= cap for p, c in launches) >= 6
    _, ring = _run(row, d, launches, cap, unbounded=False)
    _, flat = _run(row, d, launches, d.T)
    for (pos, chunk), yr, yf in zip(launches, ring, flat):
        assert np.array_equal(yr, yf), "%s launch (%d, %d): the ring differs from the unbounded cache" % (name, pos, chunk)
    _check(row, d, launches, ring, "ring")
    with pytest.raises(capi.InvalidArgument):     # a chunk whose band does not fit the ring
        Kc, Vc = _poisoned(row, cap)
        capi.call("attn_prefill_bf16", empty_u16(row.B, 41, row.NH * row.HS), d.qd[:, cap:cap + 41].contiguous(), Kc, Vc, row.B, 41, row.NH, row.NKV, row.HS, cap, cap,
                  row.window, float(row.scale))


@pytest.mark.parametrize("name", TUNABLE)
@pytest.mark.parametrize("sched", ["from_zero", "behind_history"])
def test_tuning_forms_give_the_bits_of_the_default_in_every_class(sched, name):
    """flash.form 9, 10, 11, 2 and 1 wherever they plan a launch of the schedule otherwise than the default 8: the instantiation the plan names serves it, and writes
    the default's bits (which the tests above hold to the oracle)"""
    row = BY_NAME[name]
    d = _data(name, sched == "from_zero")
    launches = schedule(row, sched)
    cap = d.T + 32
    plans8 = [capi.attn_prefill_plan(row.HS, row.NH, row.NKV, c, p, row.window) for p, c in launches]
    _, want = _run(row, d, launches, cap)
    ran = []
    try:
        for form in FORMS:
            capi.tune("flash.form", form)
            if [capi.attn_prefill_plan(row.HS, row.NH, row.NKV, c, p, row.window) for p, c in launches] == plans8:
                continue
            _, got = _run(row, d, launches, cap)
            ran.append(form)
            for (pos, chunk), y, y8 in zip(launches, got, want):
                assert np.array_equal(y, y8), "%s launch (%d, %d): form %d (%s) differs from the default" % (name, pos, chunk, form, _form_name(row, pos, chunk))
    finally:
        capi.tune_reset()
    assert 1 in ran, ran      # (the register-staged kernels serve every HS 256 / 512 shape under form 1; HS 512 with fewer than four heads per KV head has no other)


@pytest.mark.parametrize("name,n_items", [(r.name, n) for r, n in PARTIAL_ROWS])
def test_partly_filled_last_round_of_the_work_list(name, n_items):
    """one launch of 2070 rows: 260 / 520 workgroups per batch row, so the last round of 256 workgroup ids of the heavy / light list holds 4 (odd round, from the light
    end) / 8 (even round).  Every element of Y is written; every row of the first three and last three query tiles and every 37th row, all heads, against the oracle"""
    row = ALL[name]
    plan = capi.attn_prefill_plan(row.HS, row.NH, row.NKV, PARTIAL_T, 0, row.window)
    assert plan["n_items"] == n_items
    d = _data(name)
    (_, _), (y,) = _run(row, d, [(0, PARTIAL_T)], PARTIAL_T + 64)
    y = y.reshape(row.B, PARTIAL_T, row.NH * row.HS)
    assert np.all(np.isfinite(orc.from_bf16_bits(y))), "an element of Y was not written, or a dead cache row was read"
    rows = partial_sample_rows(plan["QROWS"])
    # runs of consecutive rows go to the oracle together, over the keys their band can hold
    runs, start = [], 0
    for i in range(1, len(rows) + 1):
        if i == len(rows) or rows[i] != rows[i - 1] + 1:
            runs.append((rows[start], rows[i - 1] + 1))
            start = i
    for r0, r1 in runs:
        lo = max(0, r0 - row.window + 1)
        exp = orc.gqa_attention(d.q[:, r0:r1], d.hk[:, lo:r1], d.hv[:, lo:r1], r0 - lo, row.window, row.scale)
        assert_bf16_close(y[:, r0:r1], exp, 1, 2e-3, "%s rows %d .. %d" % (name, r0, r1 - 1))
