"""The instantiation, pipeline and edge classes of the decode Linear's weight stream (csrc/matvec_body.h: matvec_body, csrc/matvec.hip: matvec_kernel and
matvec_attn_combine, csrc/matvec_rows.hip: matvec_rows_kernel) as a table of cases, with the kernels' index arithmetic restated beside it, operands on which every output
is an exactly representable number whatever the order of the additions, and a model of the stream -- which (weight row, chunk, x position) every lane of every wave visits
at every pipeline step -- that sums those operands in integers and that can be mutated the ways the stream can go wrong.

tests/test_matvec_classes_cpu.py holds every case to the launch plan (capi.matvec_rows_plan), the table to the classes it is there for, the model to the reference and
every mutant to a changed output; tests/test_matvec_classes_gpu.py runs every case and asks for the reference's bits.

A plain module: no pytest settings, no fixtures; numpy only (quantized64 alone asks the oracle's quantizers of tests/orc.py)."""
import collections
import math

import numpy as np

# ---- the restated launch arithmetic -------------------------------------------------------------------------------------------------------------------------------
EPC = (8, 16, 32)           # elements per 16-byte weight chunk: bf16, fp8, fp4 (matvec_body.h: Fmt<FMT>::kElemsPerChunk)
WAVES = 16                  # kMatvecWaves: one 1024-thread workgroup
NUM_CU = 256                # csrc/common.h: kNumCU
ARGMAX_PARTIALS = 2 * NUM_CU
RU = ((1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (4, 2))      # the instantiated (R, U) of matvec_kernel (matvec.hip: dispatch_RU)
ROWS_U = (1, 2, 4)                                          # ... and the U of matvec_rows_kernel (R is 1 there)
COMBINE_U = (4, 2, 1)                                       # launch_combine: U by format; R 1, XC 1, workgroups min(ceil(N / 16), kNumCU)
EPS = 1e-6
PAD = 9                     # poisoned elements behind every output row
POISON16 = 0x7fc0

Form = collections.namedtuple("Form", "name pro geglu f32 bias argmax")
FORMS = (Form("plain_bias", 0, False, False, True, False), Form("plain_f32", 0, False, True, False, False),
         Form("norm_bf16", 1, False, False, False, False), Form("norm_geglu", 1, True, False, False, False), Form("norm_f32", 1, False, True, False, False),
         Form("tail_bf16", 2, False, False, False, False), Form("tail_geglu", 2, True, False, False, False), Form("tail_f32_argmax", 2, False, True, False, True))
FORM = {f.name: f for f in FORMS}
FORM["combine"] = Form("combine", 0, False, False, False, False)
FORM_NAMES = tuple(f.name for f in FORMS)

# entry: "one" (matvec_* / matvec_f32out / fused_norm_matvec), "rows" (matvec_rows) or "combine" (matvec_attn_combine, HS in `group`'s place for bf16 / fp8: see hs).
# tuned: the case runs under matvec.rows_per_wave = R and matvec.chunks_in_flight = U; otherwise R and U are what the default rule must give.  wg: matvec.max_workgroups
# (0: not set).  ps: post_scale of the tail forms.  hs: head size of the combine cases.
Case = collections.namedtuple("Case", "name entry form fmt group R U K N rows tuned wg ps hs")


def tunings(c):
    t = {}
    if c.tuned:
        if c.entry == "one":
            t["matvec.rows_per_wave"] = c.R
        t["matvec.chunks_in_flight"] = c.U
    if c.wg:
        t["matvec.max_workgroups"] = c.wg
    return t


def launch_shape(fmt, geglu, N, argmax, tR=0, tU=0, tWG=0):
    """matvec.hip: matvec_launch_shape -> (R, U, max_blocks)"""
    rows = 2 * N if geglu else N
    tall, huge = rows >= 16384, rows >= 100000
    if fmt == 0:
        rps, U = (4 if huge else (2 if tall else 1)), (2 if tall else 4)
    elif fmt == 1:
        rps, U = (4 if huge else (2 if tall else 1)), 2
    else:
        rps, U = (2 if tall else 1), (2 if huge else 1)
    max_blocks = 2 * NUM_CU if (huge or (tall and fmt == 0)) else NUM_CU
    R = (rps // 2 if rps >= 2 else 1) if geglu else rps
    R, U, max_blocks = tR or R, tU or U, tWG or max_blocks
    if argmax and max_blocks > ARGMAX_PARTIALS:
        max_blocks = ARGMAX_PARTIALS
    if geglu and R > 2:
        R = 2
    if R == 1:
        U = U if U in (1, 2) else 4
    elif R == 2:
        U = 1 if U == 1 else 2
    else:
        R, U = (2 if geglu else 4), 2
    return R, U, max_blocks


Geo = collections.namedtuple("Geo", "epc nchunks S n_rg R U NR blocks total_waves xc lds nrows")


def geometry(c):
    """what the kernel of a case computes its indices from; R is the kernel's (1 in the rows kernel and the combine launch)"""
    f = FORM[c.form]
    epc = EPC[c.fmt]
    nchunks = c.K // epc
    if c.entry == "combine":
        R, U, max_blocks = 1, COMBINE_U[c.fmt], NUM_CU
    else:
        t = tunings(c)
        R, U, max_blocks = launch_shape(c.fmt, f.geglu, c.N, f.argmax, t.get("matvec.rows_per_wave", 0), t.get("matvec.chunks_in_flight", 0), t.get("matvec.max_workgroups", 0))
        if c.entry == "rows":
            R = 1
    S = -(-nchunks // (64 * U))
    n_rg = -(-c.N // R)
    blocks = max(1, min(-(-n_rg // WAVES), max_blocks))
    return Geo(epc, nchunks, S, n_rg, R, U, (2 * R if f.geglu else R), blocks, blocks * WAVES, 1 if c.K <= 8192 else 2, c.rows * S * 64 * U * epc * 2, (2 * c.N if f.geglu else c.N))


def wave_steps(c):
    """per wave g of the launch: its row groups nrg_w (g, g + 16 blocks, ...) and pipeline steps T = nrg_w S"""
    g = geometry(c)
    w = np.arange(g.total_waves)
    nrg = np.where(w < g.n_rg, (g.n_rg - 1 - w) // g.total_waves + 1, 0)
    return nrg, nrg * g.S


def column_owner(N, g):
    """per output column: the wave (row group % (16 blocks)) and the workgroup that compute and store it"""
    wave = (np.arange(N) // g.R) % g.total_waves
    return wave, wave // WAVES


def tie_kinds(c, ops, b=0):
    """where the columns that tie at row b's maximum lie relative to each other: two of them in the same wave, in two waves of one workgroup, in two workgroups"""
    top = np.flatnonzero(ops.y[b] == ops.y[b].max())
    wave, blk = column_owner(c.N, ops.geo)
    out = set()
    for i, n in enumerate(top):
        for m in top[i + 1:]:
            out.add("wave" if wave[n] == wave[m] else ("workgroup" if blk[n] == blk[m] else "grid"))
    return out


def loop_pairs(T):
    return max(0, (T - 2) // 2)


def classes(c):
    """the pipeline classes a case's waves take"""
    g = geometry(c)
    nrg, T = wave_steps(c)
    out = {"S%d" % g.S if g.S <= 3 else "S>3"}
    for t in set(int(v) for v in T):
        out.add("T%d" % t if t <= 3 else ("Teven" if t % 2 == 0 else "Todd"))
        if loop_pairs(t) >= 2:
            out.add("pairs2")
        assert t - 2 * loop_pairs(t) == (t if t <= 3 else 2 + t % 2)
    if g.S % 2 == 1 and int(nrg.max()) >= 2:
        out.add("Sodd_2rg")
    if g.nchunks % (64 * g.U):
        out.add("partial")
    if g.nchunks < 64:
        out.add("lt64")
    return out


def instantiation(c):
    """the kernel instantiation a case launches, as the template arguments"""
    g, f = geometry(c), FORM[c.form]
    if c.entry == "combine":
        return ("matvec_kernel", c.fmt, 1, g.U, 0, False, False, 1, "combine%d" % c.hs)
    if c.entry == "rows":
        return ("matvec_rows_kernel", c.fmt, g.U, f.pro, f.geglu, f.f32, g.xc, c.rows)
    return ("matvec_kernel", c.fmt, g.R, g.U, f.pro, f.geglu, f.f32, g.xc, "plain")


def library_instantiations():
    """every instantiation the library holds: dispatch_RU x dispatch_fmt x launch (XC) for the eight (PRO, GEGLU, F32OUT) the entries reach, launch_rows_*, launch_combine"""
    kinds = sorted({(f.pro, f.geglu, f.f32) for f in FORMS})
    out = set()
    for fmt in range(3):
        for pro, geglu, f32 in kinds:
            for xc in (1, 2):
                for R, U in RU:
                    if not (geglu and R > 2):
                        out.add(("matvec_kernel", fmt, R, U, pro, geglu, f32, xc, "plain"))
                for U in ROWS_U:
                    for nb in (2, 3, 4):
                        out.add(("matvec_rows_kernel", fmt, U, pro, geglu, f32, xc, nb))
        for hs in (256, 512):
            out.add(("matvec_kernel", fmt, 1, COMBINE_U[fmt], 0, False, False, 1, "combine%d" % hs))
    return out


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------
def k_for(fmt, U, S, partial=True):
    """a K whose rows take S pipeline steps at U chunk positions in flight, the last with 40 of its 64 U positions (partial) or all of them"""
    return EPC[fmt] * (64 * U * (S - 1) + (40 if partial else 64 * U))


def k_xc2(fmt):
    return 8192 + 40 * EPC[fmt]          # two x chunks per thread, a partial last step at every U


def _first_above_8192(fmt, group):
    return 8192 + (8, 16, group)[fmt]


def _build():
    cases = []

    def add(entry, form, fmt, R, U, K, N, rows=1, tuned=True, wg=0, group=None, ps=1.0, hs=0, tag=""):
        if group is None:
            group = (64 if (len(cases) % 2) else 128) if fmt == 2 else 0
        if fmt == 2 and K % group:
            group = 64
        name = "%s/%s/f%d%s/R%dU%d/K%dN%d%s%s%s" % (entry if rows == 1 else "rows%d" % rows, form, fmt, "g%d" % group if fmt == 2 else "", R, U, K, N,
                                                  "/wg%d" % wg if wg else "", "" if tuned else "/default", tag)
        cases.append(Case(name, entry, form, fmt, group, R, U, K, N, rows, tuned, wg, ps, hs))

    # every instantiation: the one-row kernel ...
    for fmt in range(3):
        for R, U in RU:
            for i, f in enumerate(FORMS):
                if f.geglu and R > 2:
                    continue
                for xc in (1, 2):
                    K = k_for(fmt, U, 1) if xc == 1 else k_xc2(fmt)
                    add("one", f.name, fmt, R, U, K, 131 + i, wg=3, ps=(0.75 if (i + xc + fmt) % 2 else 1.0))
        # ... and the rows kernel
        for U in ROWS_U:
            for i, f in enumerate(FORMS):
                for xc in (1, 2):
                    for nb in (2, 3, 4):
                        K = k_for(fmt, U, 1) if xc == 1 else k_xc2(fmt)
                        add("rows", f.name, fmt, 1, U, K, 67 + i + nb, rows=nb, wg=3, ps=(0.75 if (i + xc + nb) % 2 else 1.0))
    # the pipeline classes on the plain forms, per (format, R, U) of the one-row kernel and per (format, U) of the rows kernel: one workgroup of 16 waves over 199 .. 5
    # columns of one step each (K = 256: fewer than 64 chunks in every format), then S = 2, 3 and a whole last step on three workgroups
    for fmt in range(3):
        keys = [("one", R, U, 1) for R, U in RU] + [("rows", 1, U, 2 + i) for i, U in enumerate(ROWS_U)]
        for entry, R, U, rows in keys:
            n = 0
            for N in (199, 101, 41, 17, 5):
                add(entry, FORM_NAMES[n % 2], fmt, R, U, 256, N, rows=rows, wg=1)
                n += 1
            add(entry, FORM_NAMES[n % 2], fmt, R, U, k_for(fmt, U, 2), 198, rows=rows, wg=3)
            add(entry, FORM_NAMES[(n + 1) % 2], fmt, R, U, k_for(fmt, U, 1, partial=False), 70, rows=rows, wg=3)
            if k_for(fmt, U, 3) <= 16384:
                add(entry, FORM_NAMES[n % 2], fmt, R, U, k_for(fmt, U, 3), 197, rows=rows, wg=3)
                add(entry, FORM_NAMES[(n + 1) % 2], fmt, R, U, k_for(fmt, U, 3), 199, rows=rows, wg=1)
    # ... and once per entry form on the others, in both kernels and every format, at U = 1: idle waves and waves of one step (6 columns on 16 waves), S = 2 beside idle
    # waves (17 columns on 32 waves), S = 3 with two and three row groups per wave (40 columns on 16 waves: T = 6 and 9)
    for fmt in range(3):
        for i, f in enumerate(FORMS[2:]):
            for entry, rows in (("one", 1), ("rows", 2 + (i + fmt) % 3)):
                ps = 0.75 if (i + fmt + rows) % 2 else 1.0
                add(entry, f.name, fmt, 1, 1, 256, 6, rows=rows, wg=1, ps=ps)
                add(entry, f.name, fmt, 1, 1, k_for(fmt, 1, 2), 17, rows=rows, wg=3, ps=ps)
                add(entry, f.name, fmt, 1, 1, k_for(fmt, 1, 3), 40, rows=rows, wg=1, ps=ps)
    # the default rule's regimes at real column counts (no tuning): short, tall, huge (N % 4 == 3), and tall through the 2 N rows of GeGLU
    for fmt in range(3):
        for N in (203, 16387, 100003):
            R, U, _ = launch_shape(fmt, False, N, False)
            add("one", "plain_bias", fmt, R, U, 256, N, tuned=False)
        R, U, _ = launch_shape(fmt, True, 8195, False)
        add("one", "norm_geglu", fmt, R, U, 256, 8195, tuned=False)
        R, U, _ = launch_shape(fmt, False, 203, False)
        add("rows", "plain_bias", fmt, 1, U, 256, 203, rows=3, tuned=False)
    # K at 8192, the first K above it the format takes, and 16384; fp4 with both group sizes
    for fmt in range(3):
        for group in ((64, 128) if fmt == 2 else (0,)):
            for K in (8192, _first_above_8192(fmt, group), 16384):
                R, U, _ = launch_shape(fmt, False, 45, False)
                add("one", "plain_bias", fmt, R, U, K, 45, tuned=False, group=group)
                add("rows", "tail_bf16", fmt, 1, U, K, 45, rows=2, tuned=False, group=group, ps=0.75)
    # o_proj with the attention combine as its prologue: HS 256 with an odd head count (the last wave's second head clamps), HS 512
    for fmt in range(3):
        for hs, nh in ((256, 5), (512, 3)):
            add("combine", "combine", fmt, 1, COMBINE_U[fmt], nh * hs, 150, group=(64 if hs == 256 else 128) if fmt == 2 else 0, hs=hs)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ALL_MUTANTS_MAX_N = 1024    # up to this many columns a case meets every mutant it reaches; the tall and huge regimes those of the store and the bias (the cheap ones)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------------------------------
def _h(*parts):
    """a 64-bit integer hash of integer arrays (broadcast), position by position"""
    acc = np.zeros(np.broadcast(*[np.asarray(p) for p in parts]).shape, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    for p in parts:
        acc = (acc ^ np.asarray(p).astype(np.uint64)) * np.uint64(0x100000001B3)
        acc ^= acc >> np.uint64(29)
    acc = acc * np.uint64(0xBF58476D1CE4E5B9)
    acc ^= acc >> np.uint64(32)
    return (acc >> np.uint64(8)).astype(np.int64)


SCALE_SET = np.array([0.5, 1.0, 2.0])
BF16_OF_INT = {0: 0x0000, 1: 0x3f80, 2: 0x4000, 3: 0x4040, 4: 0x4080}
_W_BF16 = np.array([0xc000, 0xbf80, 0, 0x3f80, 0x4000], dtype=np.uint16)       # -2 .. 2
_W_FP8 = np.array([0xc0, 0xb8, 0, 0x38, 0x40], dtype=np.uint8)                # e4m3
_W_FP4 = np.array([0xc, 0xa, 0, 0x2, 0x4], dtype=np.uint8)                    # e2m1; the even element in the low nibble


def rne_bf16(v):
    """float64 -> the nearest bf16 value (ties to even), as float64"""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(v)
    return np.ldexp(np.rint(m * 256.0), e - 8)


def bf16_margin(v):
    """relative distance of v from the nearest bf16 rounding boundary (inf where v is a bf16 value)"""
    v = np.asarray(v, dtype=np.float64)
    m, _ = np.frexp(np.abs(v))
    y = m * 256.0                                        # in [128, 256): boundaries at the half-integers
    frac = y - np.floor(y)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((frac == 0) | (v == 0), np.inf, np.abs(frac - 0.5) / y)


def bf16_bits(v):
    """exactly representable float64 values -> bf16 bit patterns"""
    f = np.ascontiguousarray(v, dtype=np.float32)
    u = f.view(np.uint32)
    assert not (u & 0xffff).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def gelu64(g):
    g = np.asarray(g, dtype=np.float64)
    return 0.5 * g * (1.0 + np.tanh(0.7978845608028654 * (g + 0.044715 * g ** 3)))


def x_pattern(c):
    """the effective x of every row -- what the stream multiplies the weights with: sign(b, k) m(b, k), m in {1, 2, 3}; rows b >= 1 flip the sign where k % 4 == b, and the
    plain forms vary the magnitude by row as well (behind a norm prologue the magnitude is norm_w's, shared by the rows)"""
    f = FORM[c.form]
    k = np.arange(c.K)
    sign0 = 1 - 2 * (_h(k, 11) & 1)
    X = np.empty((c.rows, c.K), dtype=np.int64)
    for b in range(c.rows):
        mag = 1 + (_h(k, 12) + (b if f.pro == 0 else 0)) % 3
        X[b] = sign0 * np.where((k % 4 == b) & (b > 0), -1, 1) * mag
    return X


def _weight_rows(c, g, rid, salt, X0):
    """the one nonzero of every (weight row, 64-chunk group): lane, slot, value, and the fp8 / fp4 scales.  rid is the identity a row is generated from (a duplicated row
    carries another row's), salt the per-row retry count of the GeGLU conditions"""
    f = FORM[c.form]
    nW, N = g.nrows, c.N
    G = -(-g.nchunks // 64)
    gi = np.arange(G)[None, :]
    cnt = np.minimum(64, g.nchunks - 64 * gi)
    r, sl = rid[:, None], salt[:, None]
    col = r % N if f.geglu else r                                                    # gate row n and up row N + n share what is decided per column
    lane = (r + 5 * gi) % cnt
    lane = np.where((gi == G - 1) & (r < 4), cnt - 1, lane)                           # the last chunk of the row: nonzero in columns 0 .. 3
    hs = _h(r, gi, sl, 1)
    if f.geglu:
        slot = 4 * (hs % (g.epc // 4))                                                # positions no row flips ...
        slot = np.where((r >= N) & (gi == 0), slot + 1 + col % 3, slot)               # ... but the up row's first group
    else:
        slot = (3 * r + 7 * gi) % g.epc                                               # every slot of a chunk within EPC consecutive columns
    mag = 1 + (_h(r, gi, sl, 2) & 1)
    sgn = 1 - 2 * (_h(r, gi, sl, 3) & 1)
    pos = (64 * gi + lane) * g.epc + slot
    s8 = SCALE_SET[_h(rid, 7) % 3] if c.fmt == 1 else np.ones(nW)
    if c.fmt == 2:
        ng = c.K // c.group
        s4 = SCALE_SET[_h(rid[:, None], np.arange(ng)[None, :], 8) % 3]
        sc = np.take_along_axis(s4, pos // c.group, axis=1)
    else:
        s4, sc = None, np.ones((nW, G))
    if f.geglu:
        # integer sums: a nonzero under a scale of 0.5 is +-2; then signs greedily, so that the gate stays in 1 .. 64 and the up sum in +-(1 .. 52)
        mag = np.where((sc * s8[:, None]) == 0.5, 2, mag)
        tau = np.where(np.arange(nW) >= N, 1 - 2 * (_h(col[:, 0], sl[:, 0], 5) & 1), 1)
        cap = np.where(np.arange(nW) >= N, 52, 64)
        run = np.zeros(nW)
        for j in range(G):
            t = mag[:, j] * np.abs(X0[pos[:, j]]) * sc[:, j] * s8
            up = run + t <= cap
            want = np.where(up, 1, -1) * tau                                          # the sign the term should have
            sgn[:, j] = want * np.sign(X0[pos[:, j]])
            run = run + np.where(up, t, -t)
    return dict(lane=lane, slot=slot, val=sgn * mag, pos=pos, s8=s8, s4=s4, sc=sc, G=G)


Ops = collections.namedtuple("Ops", "geo X w rid bias Wi y gate up res_out margins")


def _sums(c, g, w, X, bias):
    """[rows, weight rows] exact float64: sum over the groups of val x scale, the channel scale, the bias"""
    raw = np.stack([(w["val"] * X[b][w["pos"]] * w["sc"]).sum(1) for b in range(c.rows)])
    out = raw * w["s8"][None, :]
    return out + bias[None, :] if bias is not None else out


def operands(c):
    """everything a case runs on, and its reference: the float64 composition of the entry's arithmetic, exact on these operands"""
    f, g = FORM[c.form], geometry(c)
    X = x_pattern(c)
    nW = g.nrows
    rid, salt = np.arange(nW), np.zeros(nW, dtype=np.int64)
    bias = ((_h(np.arange(nW), 9) % 9) - 4).astype(np.float64) if f.bias else None
    margins = []
    w = _weight_rows(c, g, rid, salt, X[0])
    if f.argmax:
        # exact ties at row 0's maximum: its weight row again in the lowest and the highest other column that the SAME WAVE owns, that ANOTHER WAVE of its workgroup
        # owns and that ANOTHER WORKGROUP owns (as far as the launch has such columns); the lowest column must win
        y0 = _sums(c, g, w, X, bias)[0]
        win = int(np.argmax(y0))
        wave, blk = column_owner(c.N, g)
        col = np.arange(c.N)
        for kind in ((wave == wave[win]) & (col != win), (blk == blk[win]) & (wave != wave[win]), blk != blk[win]):
            cand = col[kind & (col >= 4)]             # (columns 0 .. 3 keep their own rows: the ones whose last chunk is nonzero)
            if cand.size:
                rid[[cand[0], cand[-1]]] = win
        w = _weight_rows(c, g, rid, salt, X[0])
    gate = up = None
    if f.geglu:
        for _ in range(64):
            s = _sums(c, g, w, X, None)
            gate, up = s[:, :c.N], s[:, c.N:]
            yv = gelu64(gate) * up
            bad = ((gate < 1) | (gate > 64) | (up == 0) | (np.abs(up) > 64) | (bf16_margin(yv) < 2.0 ** -12)).any(0)
            if not bad.any():
                break
            salt[:c.N][bad] += 1
            salt[c.N:][bad] += 1
            w = _weight_rows(c, g, rid, salt, X[0])
        margins.append(bf16_margin(yv).min())
        y = rne_bf16(yv)
    else:
        y = _sums(c, g, w, X, bias)
    Wi = np.zeros((nW, c.K), dtype=np.int8)
    np.put_along_axis(Wi, w["pos"], w["val"].astype(np.int8), axis=1)
    return Ops(g, X, w, rid, bias, Wi, y, gate, up, None, margins)


def encode_weights(c, Wi):
    idx = Wi.astype(np.int64) + 2
    if c.fmt == 0:
        return _W_BF16[idx]
    if c.fmt == 1:
        return _W_FP8[idx]
    nib = _W_FP4[idx]
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def scales_of(c, w):
    return None if c.fmt == 0 else (w["s8"].astype(np.float32) if c.fmt == 1 else w["s4"].astype(np.float32))


Prologue = collections.namedtuple("Prologue", "x norm_w post_w res res_out xn margin")


def prologue_inputs(c, X):
    """the inputs of a norm (PRO 1) or sandwich-tail (PRO 2) case whose normed row is X exactly, as float64 arrays of bf16 values, and the float64 composition of the
    documented arithmetic on them (rms_common.h): rstd = 1 / sqrt(mean(x^2) + eps); PRO 1: xn = bf16(x rstd norm_w); PRO 2: a = bf16(x rstd post_w), r = bf16(bf16(res + a)
    post_scale) = res_out, xn = bf16(r rstd_r norm_w).  margin: the smallest relative distance of a rounded value from a bf16 rounding boundary (inf: all exact)"""
    f = FORM[c.form]
    k = np.arange(c.K)
    sg, m = np.sign(X), np.abs(X[0]).astype(np.float64)
    cb = np.array([1.0, 2.0, 3.0, 2.0])[:c.rows, None]
    margin = np.inf

    def rnd(v):
        nonlocal margin
        margin = min(margin, float(bf16_margin(v).min()))
        return rne_bf16(v)

    def rstd(v):
        ss = (v * v).sum(1, keepdims=True)
        assert ss.max() < 2 ** 24                                    # the fp32 sum of squares is exact in any order
        return 1.0 / np.sqrt(ss / c.K + EPS)

    if f.pro == 1:
        x = sg * cb
        xn = rnd(x * rstd(x) * m)
        return Prologue(x, m, None, None, None, xn, margin)
    p = (1 + _h(k, 13) % 3).astype(np.float64)
    sa = (1 - 2 * (_h(k[None, :], np.arange(c.rows)[:, None], 14) & 1)).astype(np.float64)
    x = sa * cb
    c2 = np.full((c.rows, 1), 3.0) if c.ps != 1.0 else cb[::-1]
    res = sg * (c2 / c.ps) - sa * p
    a = rnd(x * rstd(x) * p)
    r = rnd(res + a)
    if c.ps != 1.0:
        r = rnd(r * c.ps)
    xn = rnd(r * rstd(r) * m)
    return Prologue(x, m, p, res, r, xn, margin)


def combine_partials(c, X):
    """flash-decode split partials [NH, 3, HS + 4] fp32 (values, then m, l) whose merge is X[0] exactly: two splits with the same maximum and l = 0.5 each, whose values
    add up to x, and an empty third (m = -inf, l = 0)"""
    nh = c.K // c.hs
    x = X[0].reshape(nh, c.hs).astype(np.float32)
    d = (1 - 2 * (_h(np.arange(c.K), 15) & 1)).reshape(nh, c.hs).astype(np.float32)
    part = np.zeros((nh, 3, c.hs + 4), dtype=np.float32)
    part[:, 0, :c.hs], part[:, 1, :c.hs] = x - d, d
    part[:, 0:2, c.hs], part[:, 0:2, c.hs + 1] = 0.25, 0.5
    part[:, 2, c.hs] = -np.inf
    return part


# ---- the model of the stream ----------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("tail_stale_buffer", "t1_consumes_second", "no_clear_odd_S", "clamped_takes_last_x", "ragged_stores_clamped", "fp4_neighbour_scale", "fp4_group64_as_128",
           "fp8_scale_row_xor1", "bias_row_xor1", "geglu_up_at_col", "rows_prev_image", "xc2_second_unstaged")


def reachable(c, mutant):
    """does the mutated code run in this case, where an output could show it"""
    f, g = FORM[c.form], geometry(c)
    nrg, T = wave_steps(c)
    return {
        "tail_stale_buffer": bool(((T >= 3) & (T % 2 == 1)).any()),                   # a third peeled step: consume(ba) after the late refill
        "t1_consumes_second": c.entry == "rows" and bool((T == 1).any()),             # (the one-row kernel's finish drops a column >= N; the rows kernel's does not look)
        "no_clear_odd_S": g.S % 2 == 1 and int(nrg.max()) >= 2,
        "clamped_takes_last_x": g.nchunks % (64 * g.U) != 0,
        "ragged_stores_clamped": c.N % g.R != 0,
        "fp4_neighbour_scale": c.fmt == 2,
        "fp4_group64_as_128": c.fmt == 2 and c.group == 64,
        "fp8_scale_row_xor1": c.fmt == 1,
        "bias_row_xor1": f.bias,
        "geglu_up_at_col": f.geglu,
        "rows_prev_image": c.entry == "rows",
        "xc2_second_unstaged": c.K > 8192,
    }[mutant]


EPILOGUE_MUTANTS = ("ragged_stores_clamped", "bias_row_xor1", "fp8_scale_row_xor1")      # they change nothing before the reduced sums: model(..., stream=stream_sums(c, ops))


def stream_sums(c, ops, mutant=None):
    """the reduced sums of the stream, per stored row group: (acc [rows, groups, NR] in units of 1 / 4, the weight row and the first column of each group)"""
    return model(c, ops, mutant, sums_only=True)


def model(c, ops, mutant=None, stream=None, sums_only=False):
    """the outputs [rows, N + PAD] (float64, NaN where nothing was stored) of the stream as the kernels walk it: per wave the steps t = 0 .. T - 1 over (row group, step s),
    per step the visits (weight row j of the group, slot u, lane) -> (weight row, chunk min(c, nchunks - 1), x chunk c of the zero-padded image), summed in integers (units
    of 1 / 4), then the epilogue.  `mutant`: one of MUTANTS"""
    f, g = FORM[c.form], ops.geo
    N, R, U, S, NR, nW = c.N, g.R, g.U, g.S, g.NR, g.nrows
    w = ops.w
    if stream is not None:
        assert mutant is None or mutant in EPILOGUE_MUTANTS
        return _epilogue(c, ops, mutant, *stream)
    nrg, T = wave_steps(c)
    wv = np.repeat(np.arange(g.total_waves), T)
    first = np.repeat(np.cumsum(T) - T, T)
    t = np.arange(int(T.sum())) - first
    Tq = np.repeat(T, T)
    rg, s = wv + g.total_waves * (t // S), t % S
    extra = np.zeros(t.size, dtype=bool)
    if mutant == "t1_consumes_second":
        # a wave with one step also consumes its second buffer: the (clamped) column one grid further, computed and -- in the rows kernel -- stored
        one = np.flatnonzero(T == 1)
        wv, t, Tq = np.concatenate([wv, one]), np.concatenate([t, np.ones(one.size, dtype=np.int64)]), np.concatenate([Tq, np.ones(one.size, dtype=np.int64)])
        rg, s, extra = np.concatenate([rg, one + g.total_waves]), np.concatenate([s, np.zeros(one.size, dtype=np.int64)]), np.concatenate([extra, np.ones(one.size, dtype=bool)])
    Q = t.size
    # chunk tables of the weight rows: value and slot of the nonzero of chunk c (0: none)
    cval, cslot = np.zeros((nW, g.nchunks), dtype=np.int64), np.zeros((nW, g.nchunks), dtype=np.int64)
    cidx = 64 * np.arange(w["G"])[None, :] + w["lane"]
    np.put_along_axis(cval, cidx, w["val"], axis=1)
    np.put_along_axis(cslot, cidx, w["slot"], axis=1)
    # the x images, zero-padded to S 64 U chunks
    Xp = np.zeros((c.rows, S * 64 * U * g.epc), dtype=np.int64)
    Xp[:, :c.K] = ops.X
    if mutant == "xc2_second_unstaged":
        Xp[:, 8192:] = 0
    if mutant == "rows_prev_image":
        Xp[1:] = Xp[:-1].copy()
    # weight rows of a step
    j = np.arange(NR)
    jc = (j >> 1) if f.geglu else j
    col = np.minimum(rg[:, None] * R + jc[None, :], N - 1)                              # [Q, NR]
    is_up = np.broadcast_to((j & 1).astype(bool) if f.geglu else np.zeros(NR, dtype=bool), col.shape)
    row = np.where(is_up, (0 if mutant == "geglu_up_at_col" else N) + col, col)
    s_w = s.copy()
    row_w = row.copy()
    if mutant == "tail_stale_buffer":
        # the refill of the third peeled step is lost: its consume reads what the buffer held two steps earlier
        hit = np.flatnonzero((t == Tq - 1) & (Tq >= 3) & (Tq % 2 == 1))
        row_w[hit], s_w[hit] = row[hit - 2], s[hit - 2]
    u, lane = np.arange(U)[None, :, None], np.arange(64)[None, None, :]
    term = np.empty((c.rows, Q, NR), dtype=np.int64)
    for q0 in range(0, Q, 8192):                                                        # (in slices of the steps: the huge regime has 50 000 of them)
        q = slice(q0, q0 + 8192)
        cw = np.minimum(s_w[q, None, None] * 64 * U + 64 * u + lane, g.nchunks - 1)     # [Q, U, 64]
        cx = s[q, None, None] * 64 * U + 64 * u + lane
        if mutant == "clamped_takes_last_x":
            cx = np.minimum(cx, g.nchunks - 1)
        rw = row_w[q, :, None, None]
        val = cval[rw, cw[:, None]]                                                     # [Q, NR, U, 64]
        xk = cx[:, None] * g.epc + cslot[rw, cw[:, None]]
        if c.fmt == 2:
            flat = (4 * w["s4"]).astype(np.int64).reshape(-1)
            shift, ng = (2 if c.group == 128 else 1), c.K // c.group
            if mutant == "fp4_group64_as_128":
                shift, ng = 2, c.K // 128
            gi = cw[:, None] >> shift
            if mutant == "fp4_neighbour_scale":
                gi = np.minimum(gi ^ 1, ng - 1)
            sc = flat[np.minimum(rw * ng + gi, flat.size - 1)]
        else:
            sc = 4
        for b in range(c.rows):
            term[b, q] = (val * Xp[b][xk] * sc).sum((2, 3))
    # a row group's steps are consecutive: its sum, reduced and stored at its last step
    end = (s == S - 1) | extra
    gid = np.cumsum(end) - end
    acc = np.zeros((c.rows, int(end.sum()), NR), dtype=np.int64)
    for b in range(c.rows):
        np.add.at(acc[b], gid, term[b])
    e = np.flatnonzero(end)
    if mutant == "no_clear_odd_S":
        # the clear after a row group that ends in the first buffer (an even step) is lost: the wave's next row group starts from its sum
        for i in range(1, e.size):
            if wv[e[i]] == wv[e[i - 1]] and t[e[i - 1]] % 2 == 0:
                acc[:, i] += acc[:, i - 1]
    if sums_only:
        return acc, row[e], rg[e] * R
    return _epilogue(c, ops, mutant, acc, row[e], rg[e] * R)


def _epilogue(c, ops, mutant, acc, erow, ecol0):
    """the channel scale, the bias, GeGLU and the stores of the reduced sums"""
    f, g, w = FORM[c.form], ops.geo, ops.w
    N, R, nW = c.N, g.R, g.nrows
    s8 = np.append((4 * w["s8"]).astype(np.int64), 4)
    frow = np.minimum(erow ^ 1, nW) if mutant == "fp8_scale_row_xor1" else erow
    v = acc * s8[frow][None] // 4
    if ops.bias is not None:
        b4 = np.append((4 * ops.bias).astype(np.int64), 0)
        v = v + b4[np.minimum(erow ^ 1, nW) if mutant == "bias_row_xor1" else erow][None]
    out = np.full((c.rows, N + PAD), np.nan)
    for r in range(R):
        cols = ecol0 + r
        keep = cols < N
        if mutant == "ragged_stores_clamped" or (c.entry == "rows" and mutant == "t1_consumes_second"):
            cols = np.minimum(cols, N + PAD - 1)          # an unguarded store: into the padding, or -- recorded in its last element -- beyond it
            keep = cols >= 0
        if f.geglu:
            gt, upv = v[:, :, 2 * r] / 4.0, v[:, :, 2 * r + 1] / 4.0
            val_r = rne_bf16(gelu64(gt) * upv)
        else:
            val_r = v[:, :, r] / 4.0
        out[:, cols[keep]] = val_r[:, keep]
    return out


def reference(c, ops):
    out = np.full((c.rows, c.N + PAD), np.nan)
    out[:, :c.N] = ops.y
    return out


def same(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ---- the float64 leg: dense operands ---------------------------------------------------------------------------------------------------------------------------------
DENSE_SHAPES = ((3840, 129), (15360, 72))          # XC 1 with a partial last step at every default U; XC 2
DENSE_ROWS = (1, 3)
SLACK = 2.0 ** -17


def dense_operands(K, N, rows, seed):
    """x ~ N(0, 1) as bf16 values [rows, K]; W ~ N(0, 1 / K) times a per-channel factor in 0.25 .. 4 as bf16 values [N, K], column N // 2 all zero"""
    rng = np.random.default_rng(seed)
    x = rne_bf16(rng.standard_normal((rows, K)))
    W = rng.standard_normal((N, K)) / math.sqrt(K) * np.exp2(rng.uniform(-2, 2, N))[:, None]
    W[N // 2] = 0.0
    return x, rne_bf16(W)


DENSE_COMBINE = ((256, 5, 2), (256, 5, 7), (512, 3, 8), (256, 7, 64), (512, 7, 7))      # (HS, NH, splits): splits 2, 7, 8, 64; an odd head count at HS 256
DENSE_COMBINE_N = 129


def dense_case(fmt, form, K, N, rows):
    """the draws of one case of the float64 leg, the same on the GPU and in the CPU test: x, W (2 N rows for GeGLU) in the case's format (q, s: codes and scales, Wd: the
    float64 values the kernel multiplies with), and what the form adds.  The condition on the slack -- from the reference alone, at most 15 % of the outputs have
    2^-17 sum |x w| above one bf16 ulp of the exact value -- decides the draw: the first of the seeds seed, seed + 1000, ... that meets it (d["redraws"] counts)"""
    f = FORM[form]
    for redraws in range(8):
        seed = K + 7 * N + 100 * fmt + rows + 1000 * redraws
        xv, Wv = dense_operands(K, 2 * N if f.geglu else N, rows, seed)
        rng = np.random.default_rng(seed + 1)
        d = dict(x=xv, W=Wv, bias=None, norm_w=None, post_w=None, res=None, post_scale=0.75, redraws=redraws)
        if f.bias:
            d["bias"] = rne_bf16(rng.uniform(-0.1, 0.1, N))
        if f.pro:
            d["norm_w"] = rne_bf16(1 + 0.1 * rng.uniform(-1, 1, K))
        if f.pro == 2:
            d["post_w"], d["res"] = rne_bf16(1 + 0.1 * rng.uniform(-1, 1, K)), rne_bf16(rng.standard_normal((rows, K)))
        d["q"], d["s"], d["Wd"] = quantized64(fmt, Wv)
        d["share"] = dense_share(form, d)
        if d["share"] <= 0.15:
            return d
    raise AssertionError("no draw meets the condition on the slack")


def dense_share(form, d):
    stage = dense_stage64(form, d)
    exact = stage @ d["Wd"].T
    if d["bias"] is not None:
        exact = exact + d["bias"][None, :]
    mag = np.abs(stage) @ np.abs(d["Wd"]).T
    live = mag[0] > 0
    return slack_share(exact[:, live], mag[:, live])


def rms64(x, w):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + EPS) * w


def dense_stage64(form, d):
    """the row the stream receives, by the float64 composition of the prologue with its bf16 roundings (the device's own bits differ from it by at most one ulp)"""
    f = FORM[form]
    if f.pro == 0:
        return d["x"]
    src = d["x"]
    if f.pro == 2:
        src = rne_bf16(rne_bf16(d["res"] + rne_bf16(rms64(d["x"], d["post_w"]))) * d["post_scale"])
    return rne_bf16(rms64(src, d["norm_w"]))


def dense_combine_case(fmt, HS, NH, splits):
    """hand-written split partials [NH, splits, HS + 4] fp32 with one empty split, and the o_proj weights"""
    rng = np.random.default_rng(HS + NH + splits + fmt)
    part = np.zeros((NH, splits, HS + 4), dtype=np.float32)
    part[:, :, :HS] = rng.standard_normal((NH, splits, HS))
    part[:, :, HS], part[:, :, HS + 1] = rng.standard_normal((NH, splits)), rng.uniform(0.5, 2.0, (NH, splits))
    e = splits // 2
    part[:, e, :HS], part[:, e, HS], part[:, e, HS + 1] = 0.0, -np.inf, 0.0
    _, Wv = dense_operands(NH * HS, DENSE_COMBINE_N, 1, NH * HS + DENSE_COMBINE_N + fmt)
    return part, Wv


def merge64(part, HS):
    m, l = part[:, :, HS].astype(np.float64), part[:, :, HS + 1].astype(np.float64)
    fs = np.where(np.isneginf(m), 0.0, np.exp(m - m.max(1, keepdims=True)))
    L = (l * fs).sum(1)
    return ((part[:, :, :HS].astype(np.float64) * fs[:, :, None]).sum(1) / L[:, None]).reshape(-1)


def quantized64(fmt, Wv, group=128):
    """bf16 values Wv in a weight format: (codes, scales, the float64 values the kernel multiplies with); the quantizers are the oracle's (tests/orc.py)"""
    import orc
    Wb = bf16_bits(Wv)
    if fmt == 0:
        return Wb, None, np.asarray(Wv, dtype=np.float64)
    if fmt == 1:
        q, s = orc.quantize_fp8_per_channel(Wb)
        return q, s, orc.E4M3_LUT[q].astype(np.float64) * s.astype(np.float64)[:, None]
    q, s = orc.quantize_fp4_per_group(Wb, group)
    codes = np.empty((q.shape[0], 2 * q.shape[1]), dtype=np.uint8)
    codes[:, 0::2], codes[:, 1::2] = q & 0xf, q >> 4                                   # the even element in the low nibble
    return q, s, orc.E2M1_LUT[codes].astype(np.float64) * np.repeat(s.astype(np.float64), group, axis=1)


def f32_bound(c_S, U, epc, mag):
    """|got - exact| of an fp32 output: half an ulp per dot2 accumulation on a lane (S U EPC / 2 of them) and per butterfly level (6), twice for the dot2 instruction's
    own rounding"""
    return 2.0 ** -23 * (c_S * U * epc / 2 + 6) * mag


def slack_share(exact, mag):
    """the share of outputs whose slack 2^-17 mag is the weaker bar: above one bf16 ulp of the exact value"""
    _, e = np.frexp(np.abs(exact))
    ulp = np.ldexp(1.0, e - 8)
    return float((SLACK * mag > ulp).mean())
