"""The prefill GEMM plan (csrc/gemm_plan.hip: shape -> list of kernel-form launches) checked without a GPU: the plan is data, so the decision is readable here.

Parity with the build the fixtures were recorded from (tools/gemm_plan_fixtures.py, run BEFORE the rules were gathered into gemm_plan.hip; re-record only on purpose):
  * tests/golden/gemm_plan_queries.json: the six size / applicability queries of the ABI over 15 shapes x 28 row counts, at the defaults and under 14 single tunings;
  * tests/golden/gemm_plan_forms.json: mila_cdna4_last_form of the six entry points on an MI355X -- the forms a plan lists are the forms the call notes;
  * tests/golden/dispatch_ladder.json (tests/test_dispatch_ladder_gpu.py checks it on the GPU): the plan of the entry RocmLinearOp uses per policy gives the committed forms.
Soundness of every plan of the sweep: the steps' rectangles tile [0, M) x [0, N) exactly once; ws_bytes is the largest S * rows * cols * 4 over the split steps; no
split step without a workspace; and gemm.tile256_min_fill moves the 256 x 256 grid's rule and both column splits together."""
import json
import os

import pytest

from mila_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QUERIES = json.load(open(os.path.join(GOLDEN, "gemm_plan_queries.json")))
FORMS = json.load(open(os.path.join(GOLDEN, "gemm_plan_forms.json")))
ROWS = QUERIES["rows"]
SHAPES = [tuple(int(v) for v in k.split(",")) for k in QUERIES["default"]]
GEGLU = ("gemm_geglu_bf16", "gemm_geglu_fp8_scaled")


@pytest.fixture
def tuned():
    """set single tunings through the returned function; every default is back afterwards"""
    capi.tune_reset()

    def set_(setting):
        capi.tune_reset()
        if setting != "default":
            name, value = setting.split("=")
            capi.tune(name, int(value))
    yield set_
    capi.tune_reset()


def _query(name, M, K, N):
    fn = getattr(capi.load(), "mila_cdna4_" + name)
    if "geglu" in name:
        return int(fn(M, K, N // 2)) if N % 2 == 0 else 0
    return int(fn(M, K, N))


def _noted(plan):
    """the forms projection of a plan as mila_cdna4_last_form reports it: runtime.hip's note_form keeps 255 characters and drops a form that no longer fits"""
    out, used = [], 0
    for step in plan:
        n = len(step[0])
        if used + n + 2 >= 256:
            continue
        used += n + (1 if used else 0)
        out.append(step[0])
    return out


def _settings(table):
    return ["default"] + sorted(table["tuned"])


def _row(table, setting, shape, name):
    if setting == "default":
        return table["default"][shape][name]
    row = table["tuned"][setting][shape][name]
    return table["default"][shape][name] if row == "same" else row


@pytest.mark.parametrize("setting", _settings(QUERIES))
def test_the_size_and_applicability_queries_answer_as_the_recorded_build_did(tuned, setting):
    tuned(setting)
    diff, nonzero = [], 0
    for K, N in SHAPES:
        for name in QUERIES["default"]["%d,%d" % (K, N)]:
            want = _row(QUERIES, setting, "%d,%d" % (K, N), name)
            want = [int(c) for c in want] if isinstance(want, str) else want
            got = [_query(name, M, K, N) for M in ROWS]
            nonzero += sum(1 for v in got if v)
            diff += [(name, M, K, N, g, w) for M, g, w in zip(ROWS, got, want) if g != w]
    assert not diff, "%d answers differ from tests/golden/gemm_plan_queries.json, first: %s" % (len(diff), diff[:5])
    assert nonzero > 100, "the sweep is vacuous"


@pytest.mark.parametrize("setting", _settings(FORMS))
def test_the_plan_lists_the_forms_the_recorded_build_ran_on_the_gpu(tuned, setting):
    tuned(setting)
    diff, calls = [], 0
    for K, N in SHAPES:
        for entry in capi.PLAN_ENTRIES:
            for forms, Ms in _row(FORMS, setting, "%d,%d" % (K, N), entry).items():
                for M in Ms:
                    got = "+".join(_noted(capi.gemm_plan(entry, M, K, N // 2 if entry in GEGLU else N)))
                    calls += 1
                    if got != forms:
                        diff.append((entry, M, K, N, got, forms))
    assert not diff, "%d plans differ from tests/golden/gemm_plan_forms.json, first: %s" % (len(diff), diff[:5])
    assert calls > 1500


def test_the_plan_gives_the_forms_of_the_committed_dispatch_ladder(tuned):
    """RocmLinearOp::forward at M > 1 (host/include/Mila/Operations.h): bf16 weights and the fp8 policy's W8A16 prefill (dequantized weights, resident or staged) go
    through the plan of gemm_bf16_ws -- the staged call keeps the dequantizing 128-tile kernel where gemm_staging_bytes is 0 --, W8A8 and W4A8 through gemm_fp8_scaled_ws's"""
    shapes = {"qkv_proj(local)": (3840, 8192), "o_proj(local)": (4096, 3840), "fc_gate_up": (3840, 30720), "fc_down": (15360, 3840)}      # test_dispatch_ladder_gpu.SHAPES
    ladder = json.load(open(os.path.join(GOLDEN, "dispatch_ladder.json")))
    diff, seen = {}, 0
    for key, forms in ladder.items():
        policy, name, M = key.split("/")
        (K, N), M = shapes[name], int(M)
        if M == 1:
            continue
        if policy == "fp8" and not _query("gemm_staging_bytes", M, K, N):
            got = ["gemm128_w8a16"]
        else:
            got = _noted(capi.gemm_plan("gemm_bf16_ws" if policy in ("bf16", "fp8") else "gemm_fp8_scaled_ws", M, K, N))
        seen += 1
        if got != forms:
            diff[key] = (got, forms)
    assert not diff and seen == 4 * 4 * 17, diff


def _check_sound(entry, M, K, N, plan):
    steps = [s for s in plan if s[2] > 0]
    where = "%s M=%d K=%d N=%d: %s" % (entry, M, K, N, plan)
    assert all(s[2] > 0 and s[4] > 0 and s[1] >= 0 and s[3] >= 0 and s[1] + s[2] <= M and s[3] + s[4] <= N for s in steps), where
    assert sum(s[2] * s[4] for s in steps) == M * N, "the steps do not cover the output exactly once: " + where
    for i, a in enumerate(steps):                      # pairwise disjoint + equal total area = an exact tiling
        for b in steps[i + 1:]:
            assert a[1] + a[2] <= b[1] or b[1] + b[2] <= a[1] or a[3] + a[4] <= b[3] or b[3] + b[4] <= a[3], "two steps overlap: " + where
    markers = [s for s in plan if s[2] == 0]
    assert len(markers) <= 1 and plan[:len(markers)] == markers and all(s[0].endswith("_colsplit") for s in markers), where
    return max([s[5] * s[2] * s[4] * 4 for s in steps if s[5]] or [0])


@pytest.mark.parametrize("setting", _settings(QUERIES) + ["gemm_fp8.tail_form=2"])
def test_every_plan_tiles_its_output_once_and_sizes_its_own_workspace(tuned, setting):
    tuned(setting)
    lib = capi.load()
    split_plans = 0
    for K, N in SHAPES:
        for M in ROWS:
            for entry in capi.PLAN_ENTRIES:
                if entry in GEGLU and N % 2:
                    continue
                cols = N // 2 if entry in GEGLU else N
                plan = capi.gemm_plan(entry, M, K, cols)
                if entry in GEGLU and not plan:        # the fused forms do not serve every shape
                    assert entry == "gemm_geglu_bf16" and not lib.mila_cdna4_gemm_geglu_applicable(M, K, cols)
                    continue
                ws = _check_sound(entry, M, K, cols, plan)
                if entry == "gemm_bf16_ws":
                    assert ws == lib.mila_cdna4_gemm_workspace_bytes(M, K, N), (M, K, N, plan)
                elif entry == "gemm_fp8_scaled_ws":
                    assert ws == lib.mila_cdna4_gemm_fp8_workspace_bytes(M, K, N), (M, K, N, plan)
                else:
                    assert ws == 0, "a split step in a plan without a workspace: %s M=%d K=%d N=%d %s" % (entry, M, K, N, plan)
                split_plans += ws != 0
    assert split_plans > 50 or setting in ("gemm.force128=1", "gemm.splitk=0", "gemm.schedule=2", "gemm.schedule=3", "gemm_fp8.tail_form=1", "gemm_fp8.tail_form=2")


def _whole_gemm256(M, K, N):
    """the 256 x 256 grid accepts the shape whole (gemm256_applicable, read off the plan of gemm_bf16)"""
    return capi.gemm_plan("gemm_bf16", M, K, N) == [("gemm256", 0, M, 0, N, 0)]


def test_the_fill_tuning_moves_the_grid_rule_and_the_column_splits_together(tuned):
    """gemm.tile256_min_fill judges the 256 x 256 grid's fill everywhere: a shape the grid accepts whole is never column-split, a shape a column split takes (bf16 or
    fp8: both cut the same 256 x 256 tile list) is one the grid refuses.  (The workspace entry points used to split at a literal 80 % whatever the tuning said.)"""
    splits = {}
    for fill in (70, 80, 90):
        tuned("gemm.tile256_min_fill=%d" % fill)
        splits[fill] = set()
        for K, N in SHAPES:
            for M in ROWS:
                for entry in ("gemm_bf16_ws", "gemm_fp8_scaled_ws"):
                    plan = capi.gemm_plan(entry, M, K, N)
                    if plan[0][2] == 0:                                          # the marker: a column split over the rows of its first step
                        rows = plan[1][2]
                        assert not _whole_gemm256(rows, K, N), "fill %d: %s column-splits M=%d K=%d N=%d, which the 256 x 256 grid accepts whole" % (fill, entry, rows, K, N)
                        splits[fill].add((entry, M, K, N))
                    _check_sound(entry, M, K, N, plan)
    assert splits[80] - splits[70], "no shape of the sweep fills 70 .. 80 % of its rounds: the check is vacuous"
    assert splits[70] <= splits[80] <= splits[90]
