"""tests/row_kernel_classes.py and tests/ref_row_kernels.py against themselves, without a GPU:
  - every row of the table reaches the kernel form it names (capi.row_kernel_form: the host functions of csrc/row_kernel_plan.h the entries launch from), the table's
    forms are the library's list, and every form has a row whose last pass is ragged and one where it is whole;
  - every row's weighted position holds at least 3/4 of its reduction;
  - the oracle's own outputs rounded to the output format, and an fp32 emulation of each reduction in a plain lane-then-group order, pass every assertion of
    tests/test_row_kernel_classes_gpu.py -- a correct fp32 kernel can meet the bars on these inputs;
  - a model of each reduction that leaves out the weighted chunk fails that assertion on EVERY slice of EVERY row -- and passes on the Gaussian rows of
    test_rmsnorm_rows at dim 3840: the blind spot the weighted rows close."""
import numpy as np
import pytest

import orc
import ref_row_kernels as ref
import row_kernel_classes as tbl
from gpu_util import assert_bf16_close, f32_to_bf16_bits
from mila_amd import build, capi

IDS = [c.name for c in tbl.CASES]
BASE = [c for c in tbl.CASES if not c.op.startswith("fused_tail_norm")]
TAIL = [c for c in tbl.CASES if c.op.startswith("fused_tail_norm")]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()


def test_every_row_reaches_the_form_it_names():
    for c in tbl.CASES:
        assert capi.row_kernel_form(c.op, tbl.outer_of(c), c.dim, c.inner) == c.form, c.name
    for q in tbl.QKV_CASES:
        for op in ("fused_qkv_post_kvfp8", "fused_qkv_post_kvfp8_prefill", "fused_qkv_post_kvfp8_devpos") if q.fp8 else ("fused_qkv_post", "fused_qkv_post_prefill", "fused_qkv_post_devpos"):
            assert capi.row_kernel_form(op, q.T, q.HS) == q.form, (q.name, op)
        hv = q.HS // 16
        rows_per_workgroup = 4 * (64 // hv if hv <= 32 else 1)
        assert ((q.NH + 2 * q.NKV) % rows_per_workgroup != 0) == q.ragged, q.name
        assert q.T * q.NKV >= q.HS // 8 and q.T * q.NH >= q.HS // 8, q.name         # the rows of each stream cover every chunk of the head
    for form, HS, T, NH in tbl.ROPE_BEYOND:
        assert capi.row_kernel_form("rope_forward_bf16", T, HS) == form
        assert T * NH * (HS // 16 if form == "rope_vec" else HS // 2) > tbl.GRID_CAP           # the grid-stride loop makes a second trip
    assert capi.row_kernel_form("rmsnorm_bf16", 1, 0) is None and capi.row_kernel_form("no_such_entry", 1, 8) is None
    assert capi.row_kernel_form("fused_tail_norm_bf16", 1, 1024) is None and capi.row_kernel_form("fused_tail_norm_bf16", 1, 8200) is None
    assert capi.row_kernel_form("fused_qkv_post", 1, 48) is None and capi.row_kernel_form("fused_qkv_post_kvfp8", 1, 32) is None


def test_the_tables_forms_are_the_librarys_and_every_form_has_a_ragged_and_a_whole_row():
    assert sorted(tbl.forms_in_table()) == sorted(capi.row_kernel_forms())
    by_form = {}
    for c in tbl.CASES:
        by_form.setdefault(c.form, set()).add(c.dim % c.granule != 0)
    for q in tbl.QKV_CASES:
        by_form.setdefault(q.form, set()).add(q.ragged)
    assert {f: sorted(v) for f, v in by_form.items() if v != {False, True}} == {}
    # both sides of the boundaries between the wave and the block RMSNorm kernels
    for dim, form in ((1024, "rmsnorm_wave"), (1032, "rmsnorm_block"), (131072, "rmsnorm_block"), (131080, "rmsnorm_wave")):
        assert tbl.BY_NAME["rmsnorm_bf16_%d_gemma" % dim].form == form
    # a wave-per-row case whose row count is no multiple of the 4 rows of a workgroup
    assert any(tbl.outer_of(c) % 4 for c in tbl.CASES if c.form == "rmsnorm_wave")
    for K in tbl.MATVEC_K:
        assert K % 128 == 0 and K <= 16384
    assert tbl.N_VEC8 // 8 > tbl.GRID_CAP and tbl.N_VEC8 % 8 and (tbl.N_VEC8 // 8) % 256 and tbl.N_ELEM > tbl.GRID_CAP
    assert tbl.GEGLU_BEYOND[0] * tbl.GEGLU_BEYOND[1] // 8 > tbl.GRID_CAP and tbl.SPLIT3_BEYOND[0] * sum(tbl.SPLIT3_BEYOND[1:]) // 8 > tbl.GRID_CAP


def test_the_positions_follow_the_rule():
    assert tbl.chunk_positions(512, 0) == list(range(512))                       # 4096 elements: every chunk
    p = tbl.chunk_positions(1920, 0)                                             # 15360 elements: the edge set
    assert {0, 63, 64, 127, 255, 256, 1023, 1024, 1856, 1919} <= set(p) and len(p) <= 2 * 30 + 8 + 8
    p = tbl.chunk_positions(16385, 0)                                            # 131080 elements: a last group of one chunk
    assert {16383, 16384} <= set(p)
    p = tbl.element_positions(50257, 64, 0)
    assert set(range(64)) <= set(p) and set(range(50257 - 128, 50257)) <= set(p) and {4095, 4096} <= set(p)
    for K in tbl.MATVEC_K:
        n = K // 8
        assert set(tbl.matvec_positions(K)) == {c for c in (0, 63, 64, 1023, 1024, n - 1) if c < n}


@pytest.mark.parametrize("case", tbl.CASES, ids=IDS)
def test_the_weighted_position_holds_three_quarters_of_the_reduction(case):
    P = tbl.positions(case)
    seen = set()
    for s0, s1 in ref.block_ranges(case):
        inp = ref.build_inputs(case, s0, s1)
        if not case.op.startswith("softmax"):
            share = ref.weight_share(case, inp)
            assert share.min() >= 0.75, (case.name, float(share.min()))
        seen.update((inp["e"] // case.unit).tolist())
    assert seen == set(P)                                                        # one launch of the case weights every position


@pytest.mark.parametrize("case", BASE, ids=[c.name for c in BASE])
def test_the_oracle_and_an_fp32_emulation_pass_and_every_omitted_chunk_fails(case):
    for s0, s1 in ref.block_ranges(case):
        inp = ref.build_inputs(case, s0, s1)
        ex = ref.expect(case, inp)
        ref.check(case, inp, ref.oracle_as_outputs(case, inp), ex)
        ref.check(case, inp, ref.model(case, inp, np.float32), ex)
        for omit, T in ref.reductions(case):
            out = ref.model(case, inp, T, omit=omit)
            with pytest.raises(AssertionError):
                ref.check(case, inp, out, ex)
            bad = ref.failing_slices(case, inp, out, ex)
            assert bad == list(range(0, s1 - s0, case.inner)), (case.name, omit, "slices that pass with the chunk left out", sorted(set(range(0, s1 - s0, case.inner)) - set(bad))[:8])


def test_softmax_at_height_20_does_not_see_a_lost_max_and_at_120_does():
    """why the table has two heights: exp(x - m) with m short of the weighted element by 20 is finite in fp32, the result the same function"""
    c20, c120 = tbl.BY_NAME["softmax_fp32_1024_h20"], tbl.BY_NAME["softmax_fp32_1024_h120"]
    i20, i120 = ref.build_inputs(c20), ref.build_inputs(c120)
    ref.check(c20, i20, ref.model(c20, i20, np.float32, omit="max"))
    with pytest.raises(AssertionError):
        ref.check(c120, i120, ref.model(c120, i120, np.float32, omit="max"))


@pytest.mark.parametrize("case", TAIL, ids=[c.name for c in TAIL])
def test_a_tail_norm_reduction_without_its_weighted_chunk_changes_bits_on_every_row(case):
    """the GPU test of the sandwich tail is bit equality with the chain of base kernels (each of them in this table at the same dim); the weighted rows make that
    equality sensitive: a float64 model of the tail differs in the bits of r or xn on EVERY row when the reduction the row weights leaves out the chunk"""
    inp = ref.build_inputs(case)
    r0, x0 = ref.tail_model(case, inp)
    first = case.mode.startswith("A")
    if not first and inp["nw"] is None:
        return          # RES weights the second reduction, which this form does not run: the row is there for the residual stream's own bits
    r1, x1 = ref.tail_model(case, inp, omit=1 if first else 2)
    differs = (r0 != r1).any(axis=1)
    if x0 is not None:
        differs |= (x0 != x1).any(axis=1)
    assert differs.all(), (case.name, np.flatnonzero(~differs)[:8])


def test_the_gaussian_rows_of_the_old_test_do_not_see_a_lost_chunk_at_model_width():
    """the blind spot on record: test_rmsnorm_rows' inputs at dim 3840 and 15360 (i.i.d. N(0, 9), gemma mode), a sum of squares without its last chunk -- and without
    its last 64 elements at 15360 -- against test_rmsnorm_rows' own assertion: it PASSES.  At dim 256 the same mutant fails."""
    def mutant(outer, dim, lost):
        rng = np.random.default_rng(outer * dim)
        X = ref.bf(rng.standard_normal((outer, dim)) * 3)
        w = ref.bf(1 + 0.1 * rng.uniform(-1, 1, dim))
        exp, er = orc.rmsnorm(X, w, None, eps=1e-6, w_offset=0.0, return_rstd=True)
        X64 = X.astype(np.float64)
        rstd = 1.0 / np.sqrt((X64[:, :dim - lost] ** 2).sum(axis=1) / dim + 1e-6)
        Y = f32_to_bf16_bits((X64 * rstd[:, None] * w.astype(np.float64)).astype(np.float32))
        assert_bf16_close(Y, exp, 1, 1e-30, "rmsnorm")
        assert_bf16_close(f32_to_bf16_bits(rstd.astype(np.float32)), er, 1, 0, "rstd")
    mutant(5, 3840, 8)
    mutant(2, 15360, 8)
    mutant(2, 15360, 64)
    with pytest.raises(AssertionError):
        mutant(64, 256, 8)
