"""tests/attn_prefill_classes.py against the plan (csrc/attention_prefill.hip: plan_prefill), without a GPU: every launch of every row lands on the instantiation the
row names -- form, heads, d-shares and waves per workgroup, query rows per workgroup, workgroup count, as capi.attn_prefill_plan reports them --, and the table as a
whole reaches the loop classes tests/test_attn_prefill_classes_gpu.py is there for, counted with the kernels' own index arithmetic restated in Python.  A change of a plan
rule that moves a shape out of its class fails here; the cure is another shape for the class, not another class."""
import pytest

from attn_prefill_classes import (BEHIND_CHUNKS, BY_NAME, FORMS, FROM_ZERO_T, HISTORY, NUM_CU, PARTIAL_ROWS, PARTIAL_T, RING_CHUNK, ROWS, double_buffered, history_len,
                                  lean_pairs, partial_sample_rows, poison_floor, ring_capacity, schedule, schedules_of, spike_in_lean_loop, spikes, workgroups)
from mila_amd import capi

FIELDS = ("form", "HB", "DS", "NW", "QROWS")
DEFAULT_INSTANTIATIONS = (["flash_hs%d_hb%d_ds1_nw4" % (HS, HB) for HS in (64, 128) for HB in (4, 2, 1)] + ["flash_dma_hs256_hb%d_ds1_nw4" % HB for HB in (4, 2, 1)]
                          + ["flash_dma_hs512_hb4_ds2_nw8", "flash_dma_hs512_hb2_ds2_nw4", "flash_dma_hs512_hb1_ds2_nw4"])
# ... and what the tunings add: the register-staged kernels at HS 256 / 512 (forms 2 and 1), lockstep 8-wave workgroups at HS 256 (9), the software-pipelined loop (11),
# the ping-pong kernel (10)
TUNED_INSTANTIATIONS = (["flash_hs%d_hb%d_ds1_nw4" % (HS, HB) for HS in (256, 512) for HB in (4, 2, 1)]
                        + ["flash_dma_hs256_hb2_ds1_nw8", "flash_dma_pipe_hs512_hb4_ds2_nw8", "flash_dma_pipe_hs256_hb2_ds1_nw4", "flash_pp_hs512_hb4_ds2_nw8", "flash_pp_hs256_hb2_ds1_nw8"])


def _plan(row, pos, chunk):
    return capi.attn_prefill_plan(row.HS, row.NH, row.NKV, chunk, pos, row.window)


def _launches(row):
    return [(s, pos, chunk) for s in schedules_of(row) for pos, chunk in schedule(row, s)]


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_launch_of_a_row_lands_on_its_instantiation(row):
    assert capi.load().mila_cdna4_attn_prefill_plan_describe(row.HS, row.NH, row.NKV, 0, 0, row.window, None, 0) == 0      # a bad shape has no plan
    assert row.NH <= 8 and row.NH % row.NKV == 0 and (row.NH // row.NKV) % row.plan["HB"] == 0
    assert row.scale in (1.0, row.HS ** -0.5)
    for s, pos, chunk in _launches(row):
        got = _plan(row, pos, chunk)
        assert {f: got[f] for f in FIELDS} == row.plan, (row.name, s, pos, chunk, got)
        Q = row.plan["QROWS"]
        assert (got["n_qtiles"], got["n_hblk"]) == (-(-chunk // Q), row.NH // row.plan["HB"])
        assert got["n_items"] == len(workgroups(Q, pos, chunk, row.window)) * (row.NH // row.plan["HB"])
        assert capi.prefill_form_name(got, row.HS) == "%s_hs%d_hb%d_ds%d_nw%d" % (row.plan["form"], row.HS, row.plan["HB"], row.plan["DS"], row.plan["NW"])


def test_the_schedules_are_the_ones_the_classes_need():
    for row in ROWS:
        assert schedule(row, "from_zero") == [(0, FROM_ZERO_T)] and all(FROM_ZERO_T % n for n in (16, 32, 64))
        behind = schedule(row, "behind_history")
        assert behind[0] == (HISTORY, 1) and [c for _, c in behind] == list(BEHIND_CHUNKS) and all(p + c == q for (p, c), (q, _) in zip(behind, behind[1:]))
        for Q in (16, 32, 64):      # a chunk shorter than, equal to and longer than the query rows of a workgroup; a one-row prefill
            assert {Q - 1, Q, Q + 1} <= set(BEHIND_CHUNKS)
        assert 1 in BEHIND_CHUNKS
        if not row.window:
            assert all(nt >= 4 for p, c in behind for _, _, _, nt in workgroups(row.plan["QROWS"], p, c, 0))
            continue
        cap, ring = ring_capacity(row), schedule(row, "ring")
        assert cap == row.window + RING_CHUNK - 1 and all(c == RING_CHUNK for _, c in ring)
        assert ring[-1][0] + RING_CHUNK >= 3 * cap > ring[-1][0]
        # the entry's own rule: every key a row of the chunk may see is still in the ring -- exactly
        assert all((p + c - 1) - max(0, p - row.window + 1) + 1 <= cap for p, c in ring) and ring[-1][0] - row.window + 1 > 0
        wrapped = [p for p, c in ring if p + c - 1 >= cap]
        assert len(wrapped) >= 2 * len(ring) // 3 - 1 and len(wrapped) < len(ring)      # launches in front of the wrap and behind it
        assert row.window % 16 != 0
    assert history_len(BY_NAME["rs64_hb1_w129"]) == 520 and history_len(BY_NAME["rs64_hb4"]) == HISTORY + sum(BEHIND_CHUNKS)


def test_the_table_holds_every_class():
    reached = {}                                                    # instantiation -> [(row, ntiles of every workgroup, chunk, QROWS)]
    for row in ROWS:
        for s, pos, chunk in _launches(row):
            got = _plan(row, pos, chunk)
            nts = [w[3] for w in workgroups(got["QROWS"], pos, chunk, row.window)]
            ring = s == "ring"
            reached.setdefault(capi.prefill_form_name(got, row.HS), []).append((row, nts, chunk, got["QROWS"], ring))
    assert sorted(reached) == sorted(DEFAULT_INSTANTIATIONS)
    for name, launches in reached.items():
        rows = {l[0].name for l in launches}
        assert len(rows) == 2 and len({BY_NAME[r].window > 0 for r in rows}) == 2, (name, rows)      # each instantiation windowed and unwindowed
        ntiles = {nt for l in launches for nt in l[1]}
        assert ntiles >= {1, 2, 3, 4, 5, 6, 7}, (name, sorted(ntiles))
        assert any(chunk % Q for _, _, chunk, Q, _ in launches), name                                 # a ragged last query tile
        if double_buffered(launches[0][0].HS, launches[0][0].plan):
            pairs = {lean_pairs(nt) for l in launches if not l[4] for nt in l[1]}
            assert pairs >= {0, 1, 2}, (name, sorted(pairs))
    assert sum(double_buffered(r.HS, r.plan) for r in ROWS) == 8                                      # <256, 4 | 2 | 1, 1, 4> and <512, 4, 2, 8>, two rows each
    # batches of 2 and 3, in every kernel group; an odd number of head blocks; both scales
    assert {r.B for r in ROWS} == {1, 2, 3}
    for group in ("rs", "dma256", "dma512"):
        assert any(r.B > 1 for r in ROWS if r.name.startswith(group)), group
    assert any((r.NH // r.plan["HB"]) % 2 for r in ROWS) and all(r.NH // r.NKV in (1, 2, 4) for r in ROWS)      # (group sizes the decode entry takes too)
    assert {r.scale == 1.0 for r in ROWS} == {True, False}
    # a wrapped ring at every default instantiation
    assert {capi.prefill_form_name(r.plan, r.HS) for r in ROWS if r.window} == set(DEFAULT_INSTANTIATIONS)


def test_the_tunings_reach_every_other_instantiation_with_a_ragged_tile():
    reached = {}
    try:
        for form in FORMS:
            capi.tune("flash.form", form)
            for row in ROWS:
                for s in ("from_zero", "behind_history"):
                    for pos, chunk in schedule(row, s):
                        got = _plan(row, pos, chunk)
                        assert row.HS >= 256 or {f: got[f] for f in FIELDS} == row.plan      # below HS 256 there is the register-staged kernel only
                        reached.setdefault(capi.prefill_form_name(got, row.HS), set()).add(chunk % got["QROWS"] != 0)
    finally:
        capi.tune_reset()
    assert set(reached) == set(DEFAULT_INSTANTIATIONS) | set(TUNED_INSTANTIATIONS), sorted(set(reached) ^ (set(DEFAULT_INSTANTIATIONS) | set(TUNED_INSTANTIATIONS)))
    assert all(True in ragged for ragged in reached.values())
    assert _plan(ROWS[0], 0, FROM_ZERO_T)["form"] == ROWS[0].plan["form"]      # (the reset holds)


def test_the_spiked_keys_move_the_maximum_inside_the_lean_loop():
    for row in ROWS:
        sp = spikes(row)
        assert len(sp) == 2 and len({k for k, _, _ in sp}) == 2
        for key, qrow, head in sp:
            assert 0 <= key < qrow < FROM_ZERO_T and 0 <= head < row.NH
            assert not row.window or key >= qrow - row.window + 1, "the query row must see its spiked key"
            assert key >= 64, "late in the band: behind at least two tiles of ordinary scores"
        if double_buffered(row.HS, row.plan):
            assert any(spike_in_lean_loop(row, key, qrow) for key, qrow, _ in sp), row.name


def test_the_poison_floor_stays_below_every_row_a_kernel_reads():
    for row in ROWS:
        for s, pos, chunk in _launches(row):
            floor = poison_floor(pos, row.window)
            assert floor % 32 == 0 and floor <= min(w[2] for w in workgroups(row.plan["QROWS"], pos, chunk, row.window))
            assert floor == 0 or row.window


def test_partly_filled_last_rounds_of_the_work_list():
    """the heavy / light list at 260 and 520 items: the last round of 256 workgroup ids holds 4 (an odd round, dealt from the light end) and 8 (an even one); the map
    bid -> item of the kernels, restated, visits every item once"""
    seen_rounds = set()
    for row, n_items in PARTIAL_ROWS:
        got = _plan(row, 0, PARTIAL_T)
        assert {f: got[f] for f in FIELDS} == row.plan and got["n_items"] == n_items and got["NW"] == 4 and row.HS <= 256 and row.window
        rounds, rest = divmod(n_items, NUM_CU)
        assert 0 < rest < NUM_CU
        seen_rounds.add(rounds + 1)
        items = []
        for bid in range(n_items):
            rnd = bid // NUM_CU
            k = (rnd >> 1) * NUM_CU + bid % NUM_CU
            items.append(n_items - 1 - k if rnd & 1 else k)
        assert sorted(items) == list(range(n_items))
        rows = partial_sample_rows(got["QROWS"])
        Q, n = got["QROWS"], got["n_qtiles"]
        assert set(range(3 * Q)) <= set(rows) and set(range((n - 3) * Q, PARTIAL_T)) <= set(rows) and set(range(0, PARTIAL_T, 37)) <= set(rows)
        assert PARTIAL_T % Q and rows[-1] == PARTIAL_T - 1 and len(rows) < 400
    assert seen_rounds == {2, 3}
    assert {r.plan["form"] for r, _ in PARTIAL_ROWS} == {"flash", "flash_dma"}
