"""tests/matvec_classes.py against the library's launch plan and against itself, without a GPU:
  - every case launches what it names: capi.matvec_rows_plan (R, U, x chunks per thread, LDS bytes, workgroups) under the tunings the case runs with; the combine cases
    the fixed shape of launch_combine_t;
  - the table reaches EVERY instantiation the library holds, the default rule's regimes, every pipeline class per (format, R, U) on the plain forms and once per entry
    form on the others, and the edges;
  - on the exact operands every output and every partial sum is exactly representable, every bf16 rounding of the reference is of a bf16 value or at least 2^-12
    (relative) away from a rounding boundary, and the prologues' normed rows are the x the stream is modelled with;
  - the model of the stream (per wave: row group, step, slot, lane -> weight row, chunk or pad, x position), summed in integers, gives the reference;
  - every mutant of the model changes an output in every case that reaches it, and every mutant is reached (the nine tall and huge default-rule cases, 8195 .. 100003
    columns, meet the mutants of the epilogue only: the others would each walk millions of visits again);
  - on the dense Gaussian operands of the float64 leg a dropped 16-byte chunk passes the 1 ulp / slack bar in more than 5 % of the columns -- the blind spot the exact
    operands close -- and the slack is the weaker bar on at most 15 % of the outputs of every case of that leg, on its own draws, formats and forms."""
import collections

import numpy as np
import pytest

import matvec_classes as mc
from mila_amd import build, capi

_OPS = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()


def _ops(c):
    if c.name not in _OPS:
        _OPS[c.name] = mc.operands(c)
    return _OPS[c.name]




def test_every_case_launches_the_plan_it_names():
    try:
        for c in mc.CASES:
            g, f = mc.geometry(c), mc.FORM[c.form]
            if c.entry == "combine":
                assert (g.R, g.U, g.xc) == (1, (4, 2, 1)[c.fmt], 1) and c.K == (c.K // c.hs) * c.hs <= 8192 and g.blocks == min(-(-c.N // 16), 256), c.name
                assert g.lds <= 65536
                continue
            capi.tune_reset()
            for k, v in mc.tunings(c).items():
                capi.tune(k, v)
            plan = capi.matvec_rows_plan(c.fmt, c.K, c.N, geglu=f.geglu, f32_out=f.f32, rows=c.rows)
            assert plan is not None, c.name
            assert plan == dict(R=g.R, U=g.U, xc=g.xc, lds_bytes=g.lds, workgroups=g.blocks), (c.name, plan, g)
            assert (g.R, g.U) == (c.R, c.U), c.name
            assert g.lds <= (65536 if c.rows == 1 else 160 * 1024 - c.rows * 2 * 16 * g.xc * 4), c.name
            assert g.blocks <= mc.ARGMAX_PARTIALS
    finally:
        capi.tune_reset()


def test_the_table_reaches_every_instantiation_the_library_holds():
    reached = {mc.instantiation(c) for c in mc.CASES}
    lib = mc.library_instantiations()
    assert reached == lib, (sorted(lib - reached)[:5], sorted(reached - lib)[:5])
    # per format: XC 1, 2 x (six (PRO, GEGLU, F32OUT) without GeGLU x six (R, U) + two with x five) one-row kernels, eight x XC x 3 U x 3 row counts rows kernels; 2 combine
    assert len(lib) == 3 * (2 * (6 * 6 + 2 * 5) + 8 * 2 * 3 * 3) + 6 == 714
    # ... and each of the eight entry forms on each of them (bias or not, argmax or not are arguments, not instantiations)
    by_form = collections.defaultdict(set)
    for c in mc.CASES:
        if c.entry != "combine":
            g = mc.geometry(c)
            by_form[c.form].add((c.entry, c.fmt, g.R, g.U, g.xc, c.rows))
    for f in mc.FORMS:
        want = {("one", fmt, R, U, xc, 1) for fmt in range(3) for R, U in mc.RU for xc in (1, 2) if not (f.geglu and R > 2)}
        want |= {("rows", fmt, 1, U, xc, nb) for fmt in range(3) for U in mc.ROWS_U for xc in (1, 2) for nb in (2, 3, 4)}
        assert want <= by_form[f.name], (f.name, sorted(want - by_form[f.name])[:5])


def test_the_default_rules_regimes_are_in_the_table():
    for fmt in range(3):
        d = [c for c in mc.CASES if not c.tuned and not c.wg and c.fmt == fmt and c.K == 256 and c.entry == "one"]
        plain = {c.N: c for c in d if c.form == "plain_bias"}
        assert {203, 16387, 100003} <= set(plain) and 100003 % 4 == 3
        shapes = [mc.launch_shape(fmt, False, N, False) for N in (203, 16387, 100003)]
        assert shapes == [[(1, 4, 256), (2, 2, 512), (4, 2, 512)], [(1, 2, 256), (2, 2, 256), (4, 2, 512)], [(1, 1, 256), (2, 1, 256), (2, 2, 512)]][fmt]
        gg = [c for c in d if c.form == "norm_geglu"]
        assert gg and all(c.N < 16384 <= 2 * c.N for c in gg)
        assert mc.launch_shape(fmt, True, gg[0].N, False)[0] == 1 and mc.launch_shape(fmt, False, gg[0].N, False)[0] == 1     # tall through 2 N: one column = two rows per step


PIPE = {"T0", "T1", "T2", "T3", "Teven", "Todd", "pairs2", "S1", "S2", "Sodd_2rg", "partial", "lt64"}


def test_every_pipeline_class_per_format_R_U_on_the_plain_forms_and_once_per_form_on_the_others():
    per_key, per_form = collections.defaultdict(set), collections.defaultdict(set)
    small = collections.defaultdict(set)
    for c in mc.CASES:
        if c.entry == "combine":
            continue
        g, cl = mc.geometry(c), mc.classes(c)
        per_form[(c.entry, c.form)] |= cl
        if c.form in ("plain_bias", "plain_f32"):
            per_key[(c.entry, c.fmt, g.R, g.U)] |= cl
            if c.wg in (1, 3) and c.N <= 200:
                small[(c.entry, c.fmt, g.R, g.U)] |= cl
    keys = [("one", fmt, R, U) for fmt in range(3) for R, U in mc.RU] + [("rows", fmt, 1, U) for fmt in range(3) for U in mc.ROWS_U]
    assert sorted(per_key) == sorted(keys)
    for k in keys:
        want = set(PIPE)
        if mc.k_for(k[1], k[3], 3) <= 16384:
            want.add("S3")
        assert want <= small[k], (k, sorted(want - small[k]))                 # matvec.max_workgroups 1 and 3 give them at N <= 200
    for entry in ("one", "rows"):
        for f in mc.FORMS[2:]:
            have = per_form[(entry, f.name)]
            assert PIPE | {"S3"} <= have, (entry, f.name, sorted((PIPE | {"S3"}) - have))
    # the peeled third step (T odd >= 3; T = nrg S is even at S = 2) at S = 1 and at S = 3, with one and with two x chunks per thread, in both kernels
    third = set()
    for c in mc.CASES:
        g = mc.geometry(c)
        if c.entry != "combine" and ((mc.wave_steps(c)[1] % 2 == 1) & (mc.wave_steps(c)[1] >= 3)).any():
            third.add((c.entry, min(g.S, 4), g.xc))
    assert {(e, S, 1) for e in ("one", "rows") for S in (1, 3)} | {(e, S, 2) for e in ("one", "rows") for S in (3, 4)} <= third, sorted(third)


def test_the_edges_are_in_the_table():
    by = collections.defaultdict(set)
    for c in mc.CASES:
        g = mc.geometry(c)
        if c.entry == "one":
            by["n_mod_r"].add((c.fmt, g.R, c.N % g.R))
        by["K"].add((c.fmt, c.group, c.K))
        if mc.FORM[c.form].bias and c.N % 2:
            by["odd_bias"].add((c.entry, c.fmt))
        if c.entry == "rows":
            by["rows"].add((c.fmt, c.rows))
    for fmt in range(3):
        assert {(fmt, 2, 1), (fmt, 4, 1), (fmt, 4, 2), (fmt, 4, 3)} <= by["n_mod_r"]
        for group in ((64, 128) if fmt == 2 else (0,)):
            assert {(fmt, group, 8192), (fmt, group, 8192 + (8, 16, group)[fmt]), (fmt, group, 16384)} <= by["K"]
        assert {("one", fmt), ("rows", fmt)} <= by["odd_bias"] and {(fmt, 2), (fmt, 3), (fmt, 4)} <= by["rows"]
    assert {(c.fmt, c.hs) for c in mc.CASES if c.entry == "combine"} == {(f, h) for f in range(3) for h in (256, 512)}
    assert any(c.entry == "combine" and c.hs == 256 and (c.K // 256) % 2 for c in mc.CASES)      # an odd head count: the last wave's second head clamps
    assert {c.ps for c in mc.CASES if mc.FORM[c.form].pro == 2} == {1.0, 0.75}


def test_the_exact_operands_are_exact():
    worst = np.inf
    ties = collections.Counter()
    for c in mc.CASES:
        f, g, o = mc.FORM[c.form], mc.geometry(c), _ops(c)
        w = o.w
        # one nonzero in {+-1, +-2} per 64-chunk group of every weight row, at lane (row + 5 group) % 64 (columns 0 .. 3: the row's last chunk)
        G = -(-g.nchunks // 64)
        assert w["val"].shape == (g.nrows, G) and set(np.unique(np.abs(w["val"]))) <= {1, 2}
        assert ((o.Wi != 0).sum(1) == G).all() and (np.count_nonzero(o.Wi.reshape(g.nrows, g.nchunks, g.epc), axis=2) <= 1).all(), c.name
        chunk = 64 * np.arange(G)[None, :] + w["lane"]
        assert (chunk // 64 == np.arange(G)[None, :]).all() and (chunk < g.nchunks).all()
        same_row = o.rid == np.arange(g.nrows)
        full = (np.arange(G) < G - 1) | (g.nchunks % 64 == 0)
        assert (w["lane"][same_row][4:, full] == ((np.arange(g.nrows)[same_row][4:, None] + 5 * np.arange(G)[None, full]) % 64)).all()
        if "partial" in mc.classes(c):
            assert (chunk == g.nchunks - 1).any(1).sum() >= 4, c.name           # the last chunk of the row is nonzero in at least 4 columns
        if c.N >= 64 and not f.argmax:           # (the argmax cases overwrite five columns with copies of another)
            assert len(np.unique(chunk)) == g.nchunks, c.name                   # every chunk position is nonzero in some column
            assert len(np.unique(w["slot"])) >= (g.epc // 4 + 3 if f.geglu else g.epc), c.name     # ... and every slot of a chunk (GeGLU: those its sums allow)
        assert set(np.unique(np.abs(o.X))) <= {1, 2, 3} and (c.rows == 1 or all((o.X[b] != o.X[b - 1]).any() for b in range(1, c.rows)))
        if c.fmt == 1:
            assert set(np.unique(w["s8"])) <= {0.5, 1.0, 2.0} and (len(np.unique(w["s8"])) == 3 or c.N < 20)
        if c.fmt == 2:
            assert set(np.unique(w["s4"])) == {0.5, 1.0, 2.0} and w["s4"].shape == (g.nrows, c.K // c.group)
        # every partial sum is a multiple of 1/2 (1/4 under the channel scale) far below 2^24: exact in fp32 in any order
        assert (np.abs(w["val"]) * 3 * w["sc"] * 4).sum(1).max() * 2 < 2 ** 24
        # every output is exactly representable in its type
        y = o.y
        if f.f32:
            assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
        else:
            assert np.array_equal(mc.rne_bf16(y), y), c.name
        if f.geglu:
            assert (o.gate >= 1).all() and (o.gate <= 64).all() and (o.gate == np.rint(o.gate)).all()
            assert (o.up != 0).all() and (np.abs(o.up) <= 64).all() and (o.up == np.rint(o.up)).all()
            assert o.margins[0] >= 2.0 ** -12, c.name
            worst = min(worst, o.margins[0])
        if f.pro:
            p = mc.prologue_inputs(c, o.X)
            assert np.array_equal(p.xn, o.X.astype(np.float64)), c.name          # the normed row IS the modelled x
            assert p.margin >= 2.0 ** -12, (c.name, p.margin)
            worst = min(worst, p.margin)
            for a in (p.x, p.norm_w, p.post_w, p.res, p.res_out):
                if a is not None:
                    mc.bf16_bits(a)                                               # bf16 values, all of them
            if f.pro == 2:
                assert (np.abs(p.res_out) == (3 if c.ps != 1.0 else np.array([1.0, 2.0, 3.0, 2.0])[:c.rows][::-1, None])).all()
        if f.argmax:
            assert (o.y[0] == o.y[0].max()).sum() >= 2, c.name                     # the planted ties
            assert mc.tie_kinds(c, o), c.name
            ties.update((c.entry, k) for k in mc.tie_kinds(c, o))
    assert worst >= 2.0 ** -12
    # ties at the maximum inside one wave, across the waves of a workgroup and across workgroups: each kind in at least ten cases of each kernel
    assert all(ties[(e, k)] >= 10 for e in ("one", "rows") for k in ("wave", "workgroup", "grid")), dict(ties)
    print("argmax ties (kernel, where): cases", dict(ties))


def test_the_fp32_claims_behind_the_prologue_operands():
    """(c rstd) w in fp32, with rstd the fp32 value nearest to 1 / sqrt(c^2 + eps) and its two neighbours (v_rsq's error), rounds to the bf16 value w"""
    for cv in (1.0, 2.0, 3.0, 4.0):
        r = np.float32(1.0 / np.sqrt(cv * cv + mc.EPS))
        for rr in (np.nextafter(r, np.float32(0)), r, np.nextafter(r, np.float32(2))):
            for wv in (1.0, 2.0, 3.0):
                v = np.float32(np.float32(cv) * rr) * np.float32(wv)
                assert mc.rne_bf16(float(v)) == wv and mc.bf16_margin(float(v)) > 2.0 ** -10


def test_the_model_of_the_stream_gives_the_reference():
    for c in mc.CASES:
        o = _ops(c)
        assert mc.same(mc.model(c, o), mc.reference(c, o)), c.name


def test_every_mutant_changes_an_output_wherever_it_is_reachable():
    hits, left = collections.Counter(), collections.Counter()
    for c in mc.CASES:
        o = _ops(c)
        ref = mc.reference(c, o)
        # the tall and huge regimes (9 cases of 8195 .. 100003 columns) meet the mutants of the epilogue, on the stream's sums computed once; the others are left out there
        stream = mc.stream_sums(c, o) if c.N > mc.ALL_MUTANTS_MAX_N else None
        for m in mc.MUTANTS:
            if not mc.reachable(c, m):
                continue
            if stream is not None and m not in mc.EPILOGUE_MUTANTS:
                left[m] += 1
                continue
            assert not mc.same(mc.model(c, o, m, stream=stream if m in mc.EPILOGUE_MUTANTS else None), ref), (c.name, m)
            hits[m] += 1
    assert sum(1 for c in mc.CASES if c.N > mc.ALL_MUTANTS_MAX_N) == 9
    print("mutants x cases left out (tall and huge regimes):", dict(left), "total", sum(left.values()))
    assert set(hits) == set(mc.MUTANTS), sorted(set(mc.MUTANTS) - set(hits))
    print("mutants x cases:", dict(hits), "total", sum(hits.values()))


def _dense_ref(K, N, rows, seed):
    x, W = mc.dense_operands(K, N, rows, seed)
    return x, W, x @ W.T, np.abs(x) @ np.abs(W).T


def test_on_dense_operands_a_dropped_chunk_passes_the_bar_in_more_than_5_percent_of_the_columns():
    """the blind spot on record: y without one 16-byte chunk of the row against the bar of the float64 leg (1 bf16 ulp of RNE(exact), or 2^-17 sum |x w|)"""
    for K in (3840, 15360):
        x, W, exact, mag = _dense_ref(K, 512, 1, K)
        live = np.abs(W).sum(1) > 0
        c0 = 8 * (K // 16)
        got = mc.rne_bf16(exact - x[:, c0:c0 + 8] @ W[:, c0:c0 + 8].T)
        _, e = np.frexp(np.abs(mc.rne_bf16(exact)))
        ulp = np.ldexp(1.0, e - 8)
        ok = (np.abs(got - mc.rne_bf16(exact)) <= ulp) | (np.abs(got - exact) <= mc.SLACK * mag)
        share = ok[0, live].mean()
        print("K %d: a dropped chunk passes in %.1f %% of the columns" % (K, 100 * share))
        assert share > 0.05


def test_the_slack_is_the_weaker_bar_on_at_most_15_percent_of_the_outputs_of_every_case_of_the_float64_leg():
    """on the draws, shapes, formats and forms the GPU leg runs (mc.dense_case, mc.dense_combine_case, the oracle's quantizers), from the reference alone; the rows behind
    a prologue by its float64 composition"""
    worst, redraws = {}, 0
    for fmt in range(3):
        for f in mc.FORMS:
            for K, N in mc.DENSE_SHAPES:
                for rows in mc.DENSE_ROWS:
                    d = mc.dense_case(fmt, f.name, K, N, rows)
                    share = mc.dense_share(f.name, d)
                    worst[K] = max(worst.get(K, 0.0), share)
                    redraws += d["redraws"]
                    assert share <= 0.15, (fmt, f.name, K, N, rows, share)
        for HS, NH, splits in mc.DENSE_COMBINE:
            part, Wv = mc.dense_combine_case(fmt, HS, NH, splits)
            _, _, Wd = mc.quantized64(fmt, Wv)
            stage = mc.rne_bf16(mc.merge64(part, HS))[None, :]
            exact, mag = stage @ Wd.T, np.abs(stage) @ np.abs(Wd).T
            live = mag[0] > 0
            share = mc.slack_share(exact[:, live], mag[:, live])
            worst["combine"] = max(worst.get("combine", 0.0), share)
            assert share <= 0.15, (fmt, HS, NH, splits, share)
    print("the slack is the weaker bar on at most", {k: "%.1f %%" % (100 * v) for k, v in worst.items()}, "after %d redraws in 96 cases" % redraws)
    # the same at the K classes of the issue, on plain bf16 draws
    for K, N in mc.DENSE_SHAPES + ((256, 129), (8192, 129), (16384, 72)):
        x, W, exact, mag = _dense_ref(K, N, 3, K + N)
        live = np.abs(W).sum(1) > 0
        share = mc.slack_share(exact[:, live], mag[:, live])
        print("K %d: the slack is the weaker bar on %.1f %% of the outputs" % (K, 100 * share))
        assert share <= 0.15
        assert (exact[:, ~live] == 0).all() and (~live).sum() == 1
