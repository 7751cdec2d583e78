"""tests/attn_decode_classes.py against the plan (csrc/attention.hip: plan_decode), without a GPU: every row of the class table lands in the class it names -- heads per
workgroup, workgroups per KV head, split count and kernel form, as attn_decode_plan and attn_decode_kvfp8_plan report them at every length the row runs at -- and the
table as a whole holds every split-count, head-group and heads-per-workgroup class the GPU test is there for.  A change of a plan rule that moves a shape out of its
class fails here; the cure is another shape for the class, not another class."""
import pytest

from attn_decode_classes import FORM, FORM_KVFP8, FUSED_ROWS, GH512_ROW, GH512_TUNING, RING_ROWS, ROWS, BY_NAME, class_lengths, ring_case
from mila_amd import capi

FIELDS = ("heads_per_group", "head_groups", "splits", "form")


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_row_lands_in_its_class_at_every_length(row):
    assert row.plan["form"] == FORM
    assert len(row.lengths) == len(set(row.lengths)) and all(n >= 1 for n in row.lengths)
    for length in row.lengths:
        assert row.window > 0 or length <= row.capacity, "an unwindowed row cannot run beyond its capacity"
        got = capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, row.capacity, row.window, length)
        assert {f: got[f] for f in FIELDS} == row.plan, (row.name, length, got)
        got8 = capi.attn_decode_kvfp8_plan(row.B, row.NH, row.NKV, row.HS, row.capacity, row.window, length)
        assert {f: got8[f] for f in FIELDS} == dict(row.plan, form=FORM_KVFP8), (row.name, length, got8)
        # a fused entry without hooks (fused_attn_decode_batch_bf16) splits the band the same way
        gotf = capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, row.capacity, row.window, length, fused=True)
        assert {f: gotf[f] for f in FIELDS} == row.plan, (row.name, length, gotf)
    assert row.plan["head_groups"] * row.plan["heads_per_group"] == row.NH // row.NKV


def test_the_lengths_of_a_row_follow_the_rule():
    s64 = BY_NAME["splits64"]
    assert s64.lengths == (1, 63, 64, 65, 4095, 4096, 4097, 8192)
    # both buckets of the 8192-row cache are met, and both give the ceiling
    lib = capi.load()
    assert {lib.mila_cdna4_attn_decode_band_bucket(n, s64.capacity) for n in s64.lengths} == {4096, 8192}
    assert BY_NAME["unsplit_long"].lengths == (1, 2, 63, 64, 65, 600)
    assert BY_NAME["gs32_hs512"].lengths == (1, 15, 16, 17, 1023, 1024, 1025, 2048)
    assert BY_NAME["gs8_hs128"].lengths == (1, 31, 32, 33, 2047, 2048)      # 64 * 32 + 1 exceeds the capacity
    assert BY_NAME["gs8_hs256_w150"].lengths == (1, 2, 3, 4, 149, 150, 151, 191, 192, 193, 337, 2048)
    assert BY_NAME["splits33"].lengths == (1, 32, 33, 34, 2079, 2099, 2100, 2101, 2111, 2112, 2113, 4096, 4237)      # 4237: beyond twice the window, the cache is a ring
    for row in ROWS:
        assert set(class_lengths(row.capacity, row.window, row.plan["splits"])) <= set(row.lengths)
        assert {1, row.capacity} <= set(row.lengths)
        if row.window:
            assert {row.window - 1, row.window, row.window + 1} <= set(row.lengths) and max(row.lengths) > 2 * row.window
        # a length that fills every split exactly
        band = [min(n, row.window) if row.window else n for n in row.lengths]
        assert any(b % row.plan["splits"] == 0 and b >= 8 * row.plan["splits"] for b in band) or row.plan["splits"] == 1, row.name


def test_the_table_holds_every_class():
    splits = {r.plan["splits"] for r in ROWS}
    assert splits >= {1, 2, 3, 10, 16, 17, 32, 33, 64}, sorted(splits)
    for HS in (64, 128, 256, 512):
        assert any(r.HS == HS and r.plan["head_groups"] > 1 for r in ROWS), "no row with head_groups > 1 at HS %d" % HS
    assert {r.plan["heads_per_group"] for r in ROWS} >= {1, 2, 4}
    # batch rows beyond the first at HS 256 and 512, against truth
    assert any(r.B > 1 and r.HS == 256 for r in ROWS) and any(r.B > 1 and r.HS == 512 for r in ROWS)
    # HS 512 with one head per workgroup, and an unsplit launch over a band longer than one 64-key group
    assert any(r.HS == 512 and r.plan["heads_per_group"] == 1 for r in ROWS)
    assert any(r.plan["splits"] == 1 and max(r.lengths) > 64 for r in ROWS)
    # a split count above 16 that is no multiple of 8 (the combine pads its fma chain to a multiple of 8 and prefetches the first 16), and the ceiling
    assert any(s > 16 and s % 8 for s in splits) and 64 in splits
    # the XCD-local grid applies to some rows and not to others
    tiles = [(r.NKV * r.plan["head_groups"]) % 8 == 0 for r in ROWS]
    assert any(tiles) and not all(tiles)


def test_the_ring_and_fused_selections():
    assert set(RING_ROWS) <= set(BY_NAME) and set(FUSED_ROWS) <= set(BY_NAME)
    assert {BY_NAME[n].HS for n in RING_ROWS} == {64, 128, 256, 512} and any(BY_NAME[n].B > 1 for n in RING_ROWS)
    for name in RING_ROWS:
        row = BY_NAME[name]
        window, cap, length = ring_case(row)
        assert cap == window + 3 and length > 2 * cap
        # the ring and the unbounded cache of `length` rows split the band the same way, into more than one split
        ring = capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, cap, window, length)
        assert ring == capi.attn_decode_plan(row.B, row.NH, row.NKV, row.HS, length, window, length) and ring["splits"] > 1
        assert (ring["heads_per_group"], ring["head_groups"]) == (row.plan["heads_per_group"], row.plan["head_groups"])
    # the fused prologue's hg == 0 rule: workgroups per KV head of 2, 4 and 8 below HS 512, and a batch
    fused = [BY_NAME[n] for n in FUSED_ROWS]
    assert {r.plan["head_groups"] for r in fused if r.HS < 512} >= {2, 4, 8} and {r.HS for r in fused} == {64, 128, 256}
    assert sum(r.B > 1 for r in fused) >= 2 and "batch3_local" in FUSED_ROWS


def test_four_heads_per_workgroup_at_hs512_is_a_tuning_of_the_bf16_cache():
    r = GH512_ROW
    assert capi.attn_decode_plan(r.B, r.NH, r.NKV, r.HS, r.capacity, r.window, 1)["heads_per_group"] == 2
    try:
        capi.tune(*GH512_TUNING)
        for length in r.lengths:
            got = capi.attn_decode_plan(r.B, r.NH, r.NKV, r.HS, r.capacity, r.window, length)
            assert {f: got[f] for f in FIELDS} == r.plan, (length, got)
    finally:
        capi.tune_reset()
