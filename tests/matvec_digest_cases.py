"""The cases of tests/test_matvec_digests_gpu.py: the decode Linear (csrc/matvec.hip, csrc/matvec_rows.hip) at 1 .. 4 rows, each as a
SHA-256 of the bytes the launches leave behind.  tests/golden/matvec_digests.json holds the digests of the build the kernels were last allowed to change bits in
(tools/record_matvec_digests.py writes it); a refactor of the kernels must reproduce every one of them.  The batch-invariance tests (test_matvec_rows_gpu.py) compare
the rows entry with the one-row entry: a shift common to both (as a merge of the two kernels could produce) passes them and fails here.

A case is (form, weight format, rows).  rows = 1: the one-row entry (matvec_* / fused_norm_matvec) on each of the four input rows in turn; rows = 2 .. 4: one
matvec_rows launch on the first `rows` of the same four.  Outputs are handed in poisoned with one more row than the batch and wider than N, and are hashed whole.
Inputs come from the seeded generators of test_matvec_rows_gpu.py.

A plain module: no pytest settings, no fixtures.  CASES needs nothing but this file; run() needs the GPU."""
import ctypes as C
import hashlib
import zlib

import numpy as np

FMTS = (0, 1, 2)
ROWS = (1, 2, 3, 4)
MAX_ROWS = 4
PLAIN_SHAPES = ((256, 40), (4096, 129), (15360, 96))      # one partial step; a ragged last group of waves; two x chunks per thread
NORM_SHAPE = (3840, 129)
GEGLU_SHAPE, GEGLU_POST_SCALE = (3840, 261), 0.75
F32_SHAPE = (256, 300)
# matvec.max_workgroups = 1: 16 waves walk all columns, S pipeline steps each.  K = 256 is S = 1 in every format, so 200 / 100 / 40 / 17 / 5 columns give waves with
# 12 or 13, 6 or 7, 2 or 3, 1 or 2 and 0 or 1 steps: every peeled tail of the two-buffer loop; K = 6144 is S = 3 at bf16 (the refill of the third step)
SMALL_GRID = ((256, 200), (256, 100), (256, 40), (256, 17), (256, 5), (6144, 40))


def _cases():
    forms = ["plain/%dx%d" % kn for kn in PLAIN_SHAPES] + ["norm", "tail_geglu", "f32_argmax", "one_workgroup"]
    return [("%s/f%d/rows%d" % (form, fmt, rows), (form, fmt, rows)) for form in forms for fmt in FMTS for rows in ROWS]


CASES = _cases()
NAMES = [n for n, _ in CASES]
_BY_CASE = dict(CASES)


def toolchain():
    from attn_decode_digest_cases import toolchain as t
    return t()


def _rng(form, fmt):
    return np.random.default_rng(zlib.crc32(("%s/f%d" % (form, fmt)).encode()))      # the same inputs at every row count of a (form, format)


def _plain(fmt, rows, K, N, rng, with_bias):
    import test_matvec_rows_gpu as t
    from gpu_util import empty_u16
    W, s = t._weights(N, K, fmt)
    xs, ys = K + 24, N + 9
    X = t._rows_in(rng, MAX_ROWS, K, xs)
    bias = t._d(t._bf(rng.standard_normal(N))) if with_bias else None
    if rows == 1:
        out = []
        for b in range(MAX_ROWS):
            y = empty_u16(N + 9)
            t._plain_one(fmt, y, X[b, :K].clone(), W, s, bias, K, N)
            out.append(y)
        return out
    Y = empty_u16(rows + 1, ys)
    a = t._fused_args(y=Y, x=X, W=W, scales=s if s is not None else 0, norm_w=0, post_w=0, res=0, res_out=0, post_scale=1.0, eps=t.EPS, fmt=fmt, K=K, N=N, group=128,
                      geglu=0, f32_out=0)
    t._run_rows(t._rows_args(a, rows, xs, ys, bias=bias))
    return [Y]


def _fused(fmt, rows, K, N, rng, tail_geglu):
    """norm prologue, or sandwich tail + GeGLU (y and the residual stream res_out)"""
    import test_matvec_rows_gpu as t
    from gpu_util import empty_u16
    W, s = t._weights(2 * N if tail_geglu else N, K, fmt)
    nw = t._d(t._bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    pw = t._d(t._bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    xs, rs, ros, ys = K + 8, K + 16, K + 24, N + 5
    X, R = t._rows_in(rng, MAX_ROWS, K, xs, 2.0), t._rows_in(rng, MAX_ROWS, K, rs)
    kw = dict(W=W, scales=s if s is not None else 0, norm_w=nw, eps=t.EPS, fmt=fmt, K=K, N=N, group=128, f32_out=0)
    if tail_geglu:
        kw.update(post_w=pw, post_scale=GEGLU_POST_SCALE, geglu=1)
    else:
        kw.update(post_w=0, res=0, res_out=0, post_scale=1.0, geglu=0)
    if rows == 1:
        out = []
        for b in range(MAX_ROWS):
            y, ro = empty_u16(ys), empty_u16(ros)
            if tail_geglu:
                t._run_one(t._fused_args(y=y, x=X[b, :K].clone(), res=R[b, :K].clone(), res_out=ro, **kw))
            else:
                t._run_one(t._fused_args(y=y, x=X[b, :K].clone(), **kw))
            out += [y, ro]
        return out
    Y, RO = empty_u16(rows + 1, ys), empty_u16(rows + 1, ros)
    if tail_geglu:
        t._run_rows(t._rows_args(t._fused_args(y=Y, x=X, res=R, res_out=RO, **kw), rows, xs, ys, rs, ros))
    else:
        t._run_rows(t._rows_args(t._fused_args(y=Y, x=X, **kw), rows, xs, ys))
    return [Y, RO]


def _f32_argmax(fmt, rows, K, N, rng):
    """fp32 logits behind the norm prologue, and the sampler's first stage: one (value, column) partial per workgroup and row"""
    import torch
    import test_matvec_rows_gpu as t
    from gpu_util import empty_f32
    from mila_amd import capi
    W, s = t._weights(N, K, fmt)
    nw = t._d(t._bf(1 + 0.1 * rng.uniform(-1, 1, K)))
    xs, ys = K + 8, N + 7
    X = t._rows_in(rng, MAX_ROWS, K, xs)
    nb = capi.load().mila_cdna4_sample_scratch_bytes()
    kw = dict(W=W, scales=s if s is not None else 0, norm_w=nw, post_w=0, res=0, res_out=0, post_scale=1.0, eps=t.EPS, fmt=fmt, K=K, N=N, group=128, geglu=0, f32_out=1)
    blocks = C.c_int(0)

    def partials(scratch):
        """the whole scratch (handed in as 0x5A bytes, one row's worth more than the launch may write), and the partial count the entry reported"""
        return [scratch, torch.tensor([blocks.value], dtype=torch.int32)]

    if rows == 1:
        out = []
        for b in range(MAX_ROWS):
            y = empty_f32(ys)
            scratch = torch.full((2 * nb,), 0x5A, dtype=torch.uint8, device="cuda")
            a = t._fused_args(y=y, x=X[b, :K].clone(), **kw)
            a.argmax_scratch, a.argmax_scratch_bytes, a.argmax_blocks = scratch.data_ptr(), nb, C.pointer(blocks)
            t._run_one(a)
            out += [y] + partials(scratch)
        return out
    Y = empty_f32(rows + 1, ys)
    scratch = torch.full(((rows + 1) * nb,), 0x5A, dtype=torch.uint8, device="cuda")
    a = t._fused_args(y=Y, x=X, **kw)
    a.argmax_scratch, a.argmax_scratch_bytes, a.argmax_blocks = scratch.data_ptr(), rows * nb, C.pointer(blocks)
    t._run_rows(t._rows_args(a, rows, xs, ys))
    return [Y] + partials(scratch)


def _outputs(case):
    from mila_amd import capi
    form, fmt, rows = _BY_CASE[case]
    rng = _rng(form, fmt)
    if form.startswith("plain/"):
        K, N = (int(v) for v in form[6:].split("x"))
        return _plain(fmt, rows, K, N, rng, True)
    if form == "norm":
        return _fused(fmt, rows, *NORM_SHAPE, rng, False)
    if form == "tail_geglu":
        return _fused(fmt, rows, *GEGLU_SHAPE, rng, True)
    if form == "f32_argmax":
        return _f32_argmax(fmt, rows, *F32_SHAPE, rng)
    capi.tune("matvec.max_workgroups", 1)
    try:
        out = []
        for K, N in SMALL_GRID:
            out += _plain(fmt, rows, K, N, rng, False)
        return out
    finally:
        capi.tune_reset()


def run(case):
    """run one case on the GPU: the SHA-256 (hex) of its outputs' bytes, in order"""
    import torch
    outs = _outputs(case)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for o in outs:
        h.update(o.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()
