"""The kernel forms and tail classes of the row kernels -- RMSNorm, LayerNorm, softmax, the sandwich tail, per-token FP8 quantization, the q/k/v post-processing, the norm
prologue of the decode Linear (csrc/norm.hip, quantize.hip, fused.hip, rope.hip, elementwise.hip, matvec_body.h) -- as a table of shapes: one row per (entry, form, tail).

Why the rows are WEIGHTED.  On i.i.d. Gaussian rows every element carries 1 / dim of a reduction, so a kernel that drops one 16-byte chunk from a sum of squares moves
rstd by about 4 / dim -- at model width (3840, 15360) far below the one bf16 ulp the float64 comparisons allow, and the test passes with the chunk missing
(tests/test_row_kernel_classes_cpu.py keeps that blind spot on record).  Here each slice of the input carries at least 3/4 of its reduction in ONE position -- one
element of +-16.0 over a background of bf16(2^-6 N(0, 1)), in slot `slice % 8` of the chunk -- and different slices weight different positions, so one launch of
`number of positions` slices checks every position: losing, doubling or misplacing the weighted chunk moves every output of that slice by far more than the bar.

Positions (chunks of 8 elements for the 16-byte kernels, elements for the strided / scalar ones): every one up to 4096 elements; above, the edge set -- first and last of
every 64-chunk group (the wave butterfly), either side of every multiple of 256 (a workgroup pass) and of 1024 (the decode Linear's pass), the last, and 8 drawn ones.
The scalar kernels above 4096 elements have no group structure beyond their thread stride W (64 lanes or 256 threads): there the set is the first W elements (every lane
on its first trip), the last 2 W (every lane on its last whole trip and on the ragged one), either side of every multiple of 4096, and 8 drawn ones.

tests/test_row_kernel_classes_cpu.py holds every row to the form it names (capi.row_kernel_form) and the table to the library's list of forms;
tests/test_row_kernel_classes_gpu.py runs every row against float64 or, for the fused forms, bit for bit against the chain of base kernels.

A plain module: no pytest settings, no fixtures."""
import collections

import numpy as np

# op = the entry point; dim = the reduced axis (K of the quantizer); inner = the stride of the reduced axis; form = the kernel the row is there for
# (capi.row_kernel_form); unit = elements per position (8: a 16-byte chunk of bf16, 4: one of fp32, 1: an element); granule = the elements one full pass of the form covers -- the row's last
# pass is ragged when dim % granule != 0; mode = the weight / bias mode of test_rmsnorm_rows, or bias / nobias for LayerNorm.
Case = collections.namedtuple("Case", "name op dim inner form unit granule mode")

MIN_SLICES = 5            # not a multiple of the 4 rows a wave-per-row workgroup takes: the last workgroup of every small case has idle waves
SPIKE = 16.0
BACKGROUND = 2.0 ** -6
MODES = ("gemma", "bias", "unit_offset", "noweight")


def chunk_positions(n, seed, unit=8):
    """positions out of n (chunks of `unit` elements) by the module's rule"""
    if n * unit <= 4096:
        return list(range(n))
    s = {0, n - 1}
    for g in range(0, n, 64):
        s.update((g, min(g + 63, n - 1)))
    for m in (256, 1024):
        for b in range(m, n, m):
            s.update((b - 1, b))
    s.update(int(v) for v in np.random.default_rng(seed).integers(n, size=8))
    return sorted(s)


def element_positions(n, width, seed):
    """positions out of n (elements) for a scalar kernel whose threads stride by `width`"""
    if n <= 4096:
        return list(range(n))
    s = set(range(width)) | set(range(n - 2 * width, n))
    for b in range(4096, n, 4096):
        s.update((b - 1, b))
    s.update(int(v) for v in np.random.default_rng(seed).integers(n, size=8))
    return sorted(s)


def positions(case):
    if case.unit > 1:
        return chunk_positions(case.dim // case.unit, case.dim, case.unit)
    return element_positions(case.dim, 256 if case.form.startswith("layernorm_block") else 64, case.dim)


def slices(case):
    """slices of a case's launch: slice s weights positions(case)[s % len]"""
    return max(len(positions(case)), MIN_SLICES)


def outer_of(case):
    return -(-slices(case) // case.inner)


def _cases():
    out = []

    def add(op, dim, form, unit, granule, modes, inner=1):
        for m in modes:
            out.append(Case("%s_%d%s_%s" % (op, dim, "x%d" % inner if inner > 1 else "", m), op, dim, inner, form, unit, granule, m))

    # rmsnorm_bf16: the four modes on the smallest dim of each form
    for i, d in enumerate((8, 16, 24, 32, 64, 128, 256, 512, 1024, 131080)):
        add("rmsnorm_bf16", d, "rmsnorm_wave", 8, 512, MODES if i == 0 else ("gemma",))
    for i, d in enumerate((1032, 2048, 2056, 3840, 4096, 4104, 6144, 6152, 8192, 15360, 131072)):
        add("rmsnorm_bf16", d, "rmsnorm_block", 8, 512, MODES if i == 0 else ("gemma",))
    add("rmsnorm_bf16", 40, "rmsnorm_strided", 1, 64, MODES, inner=6)
    add("rmsnorm_bf16", 1001, "rmsnorm_strided", 1, 64, ("gemma",))         # inner == 1, reached because dim % 8 != 0
    add("rmsnorm_bf16", 64, "rmsnorm_strided", 1, 64, ("gemma",), inner=2)   # one whole trip of the 64 lanes, no ragged one
    add("rmsnorm_fp32", 12, "rmsnorm_fp32_vec", 4, 256, MODES)
    add("rmsnorm_fp32", 3840, "rmsnorm_fp32_vec", 4, 256, ("gemma",))
    add("rmsnorm_fp32", 40, "rmsnorm_fp32_scalar", 1, 64, MODES, inner=3)
    add("rmsnorm_fp32", 513, "rmsnorm_fp32_scalar", 1, 64, ("gemma",))
    add("rmsnorm_fp32", 128, "rmsnorm_fp32_scalar", 1, 64, ("gemma",), inner=2)
    # layernorm
    for d, nv in ((8, 1), (512, 1), (768, 2), (1024, 2), (1536, 4), (2048, 4), (2056, 8), (4096, 8)):
        add("layernorm_bf16", d, "layernorm_wave_nv%d" % nv, 8, 512 * nv, ("bias", "nobias"))
    for d in (1001, 4104, 8192):
        add("layernorm_bf16", d, "layernorm_block", 1, 256, ("bias", "nobias"))
    for d in (512, 1001, 4104):
        add("layernorm_fp32", d, "layernorm_block_fp32", 1, 256, ("bias", "nobias"))
    # softmax: mode = the spike's height above the N(0, 1) background (20: a sum that misses the element; 120: a max that misses it -- exp overflows in fp32)
    for op in ("softmax_fp32", "softmax_bf16"):
        for d in (5, 64, 65, 1024, 50257):
            add(op, d, "softmax_wave_" + op[-4:], 1, 64, ("h20", "h120"))
        add(op, 4, "softmax_wave_" + op[-4:], 1, 64, ("h20", "h120"), inner=5)
    # per-token FP8 quantization: the weighted position holds the row's absmax
    for K, nch in ((8, 2), (2048, 2), (4096, 2), (4104, 4), (8192, 4), (8200, 8), (15360, 8), (16384, 8), (16392, 0), (20480, 0)):
        add("quantize_fp8_per_token", K, "quant_token_nch%d" % nch if nch else "quant_token_reread", 8, 2048 * nch if nch else 2048, ("absmax",))
    # the sandwich tail: mode = where the weight sits (A: the first reduction, RES: the second) x post_scale x with / without next_w; the quantizing form needs next_w
    for d in (1032, 2048, 2056, 3840, 4096, 4104, 6144, 6152, 8192):
        nch = (d // 8 + 255) // 256
        add("fused_tail_norm_bf16", d, "tail_norm_nch%d" % nch, 8, 2048 * nch, ("A_s1_next", "RES_s1_next", "A_s075_next", "RES_s075_next", "A_s075_nonext", "RES_s1_nonext"))
        add("fused_tail_norm_quant_bf16", d, "tail_norm_nch%d_quant" % nch, 8, 2048 * nch, ("A_s1_next", "RES_s075_next"))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the q/k/v post-processing: HS, NH, NKV, T tokens, rot (0 = full rotary), kv_shared, fp8 cache.  A (token, head) row r = t * heads + h of each of q, k and v weights
# chunk r % (HS / 8), and T * NKV >= HS / 8, so the rows of each stream cover every chunk of the head.  `ragged`: NH + 2 NKV is no multiple of the 4 * rows_per_wave rows a
# workgroup takes, so its last wave has lane groups without a row (HS 1024: idle waves).
QkvCase = collections.namedtuple("QkvCase", "name HS NH NKV T rot kv_shared fp8 form ragged")


def _qkv_cases():
    out = []
    for HS in (16, 32, 64, 128, 256, 512, 1024):
        hv = HS // 16
        form = "qkv_post_hv%d" % hv if hv <= 32 else "qkv_post_wave"
        rpw = 64 // hv if hv <= 32 else 1
        n = HS // 8
        out.append(QkvCase("qkv_bf16_hs%d" % HS, HS, 3, 2, -(-n // 2), HS // 4 if HS == 128 else 0, HS == 256, False, form, True))
        # a whole workgroup of rows: NH + 2 NKV == 4 * rows_per_wave
        nkv = max(1, rpw)
        out.append(QkvCase("qkv_bf16_hs%d_full" % HS, HS, 4 * rpw - 2 * nkv, nkv, -(-n // nkv), 0, False, False, form, False))
    for HS in (64, 128, 256, 512):
        hv, n = HS // 16, HS // 8
        rpw = 64 // hv
        out.append(QkvCase("qkv_fp8_hs%d" % HS, HS, 3, 2, -(-n // 2), HS // 2 if HS == 64 else 0, HS == 512, True, "qkv_post_kvfp8_hv%d" % hv, True))
        out.append(QkvCase("qkv_fp8_hs%d_full" % HS, HS, 4 * rpw - 2 * rpw, rpw, -(-n // rpw), 0, False, True, "qkv_post_kvfp8_hv%d" % hv, False))
    return out


QKV_CASES = _qkv_cases()

# the norm (PRO 1) and sandwich (PRO 2, with res) prologues of the decode Linear: K x fmt (0 bf16, 1 fp8, 2 fp4 group 128) x geglu, N = 24.  Position classes only -- a
# launch per position: first chunk, last chunk, chunks 63 / 64 (the wave butterfly's edge), 1023 / 1024 (the 1024-thread pass: XC = 2 above K 8192), and the last chunk
# of the ragged last 64-chunk group (the last chunk again: listed once).
MATVEC_K = (128, 640, 8192, 8320, 16384)
MATVEC_N = 24


def matvec_positions(K):
    n = K // 8
    return sorted({0, n - 1} | {c for c in (63, 64, 1023, 1024) if c < n})


# beyond the grid cap: csrc/elementwise.hip's grid_for and rope_forward_bf16 launch at most 2048 workgroups of 256 threads and stride over the rest, so the second trip
# of the loop runs only from 2048 * 256 work items on; both tails (the 16-byte one and, where the kernel has it, the scalar one) are non-empty
GRID_CAP = 2048 * 256
N_VEC8 = GRID_CAP * 8 + 8 * 3 + 5        # gelu_bf16, residual_bf16, scale_bf16 (8 elements per thread)
N_ELEM = GRID_CAP + 5                    # gelu_fp32, residual_fp32, convert_* (an element per thread)
GEGLU_BEYOND = (35, 122880)              # tokens, half: 35 * 15360 vectors
SPLIT3_BEYOND = (35, 122880, 61440, 61440)    # rows, na, nb, nc: the same rows as q | k | v, 35 * 30720 vectors
ROPE_BEYOND = (("rope_vec", 256, 1030, 32), ("rope_pair", 24, 1400, 32))      # form, HS, T, NH: 1030 * 32 * 16 vectors, 1400 * 32 * 12 pairs


def forms_in_table():
    return {c.form for c in CASES} | {c.form for c in QKV_CASES} | {f for f, _, _, _ in ROPE_BEYOND}
