"""The cases of tests/test_attn_decode_digests_gpu.py: every instantiation of the wave-per-position decode kernels (attn_decode_kernel, attn_decode_kvfp8_kernel) and
every hook the bf16 kernel keeps (fused prologue, one-pass tail, partials for a consumer, warm blocks, device position, ring), each as a SHA-256 of the bytes the launch
leaves behind.  tests/golden/attn_decode_digests.json holds the digests of the build the kernels were last allowed to change bits in
(tools/record_attn_decode_digests.py writes it); a refactor of the kernels must reproduce every one of them.

Inputs are bf16 BIT PATTERNS drawn with numpy.random.default_rng(seed).integers -- sign, a biased exponent from a narrow range, 7 mantissa bits -- with seeds that
are the CRC-32 of a name: no float sampler, whose stream a numpy release may change, and only finite values below 1 (K below 0.5), so that scores stay in the
range where the softmax keeps many keys alive and the running maximum moves from group to group (the rescale branch).

A plain module: no pytest settings, no fixtures.  CASES needs nothing but this file and attn_decode_classes; run() needs the GPU."""
import ctypes as C
import functools
import hashlib
import subprocess
import zlib

import numpy as np

from attn_decode_classes import BY_NAME, FUSED_ROWS, GH512_ROW, GH512_TUNING, RING_ROWS, ROWS, Row, class_lengths, ring_case

NAN_BITS, POISON8 = 0x7fc0, 0x7F
EPS = 1e-6
FUSED_KINDS = ("first", "middle", "last", "ring")      # the order of test_attn_decode_classes_gpu._fused_positions
# the two Gemma layers the hooks of the bf16 kernel serve (local: sliding window; global: one KV head, v = k, unit V weight)
HOOK_ROWS = {
    "local": Row("gemma_local", 1, 16, 8, 256, 2048, 1024, (), None),
    "global": Row("gemma_global", 1, 16, 1, 512, 2048, 0, (), None),
}
HOOK_POSITION = 1500
HOOKS = ("onepass", "partials", "warm")
# instantiations no row of attn_decode_classes.ROWS reaches: two query heads per KV head below HS 512 (<128, 2> and <64, 2>; one workgroup per KV head, 32 splits)
EXTRA_ROWS = [Row("gs2_hs128", 1, 16, 8, 128, 2048, 0, class_lengths(2048, 0, 32), None), Row("gs2_hs64", 1, 16, 8, 64, 2048, 0, class_lengths(2048, 0, 32), None)]
ALL_ROWS = dict(BY_NAME, **{GH512_ROW.name: GH512_ROW}, **{r.name: r for r in list(HOOK_ROWS.values()) + EXTRA_ROWS})


def _devpos_length(row):
    return row.lengths[len(row.lengths) // 2]


def _cases():
    out = []
    for r in ROWS + EXTRA_ROWS:
        for n in r.lengths:
            out.append(("bf16/%s/%d" % (r.name, n), ("decode", "bf16", r.name, n)))
            out.append(("kvfp8/%s/%d" % (r.name, n), ("decode", "kvfp8", r.name, n)))
        out.append(("devpos_bf16/%s" % r.name, ("devpos", "bf16", r.name, _devpos_length(r))))
        out.append(("devpos_kvfp8/%s" % r.name, ("devpos", "kvfp8", r.name, _devpos_length(r))))
        if r.name in FUSED_ROWS:
            out += [("fused/%s/%s" % (r.name, k), ("fused", r.name, k)) for k in FUSED_KINDS]
        if r.name in RING_ROWS:
            out += [("ring_%s/%s" % (c, r.name), ("ring", c, r.name)) for c in ("bf16", "kvfp8")]
    out += [("gh512/%d" % n, ("gh512", n)) for n in GH512_ROW.lengths]
    out += [("%s/%s" % (h, layer), ("hook", h, layer)) for layer in HOOK_ROWS for h in HOOKS]
    return out


CASES = _cases()
NAMES = [n for n, _ in CASES]
_BY_CASE = dict(CASES)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
def seed_of(name):
    return zlib.crc32(name.encode())


def bf16_pattern(name, shape, exp_lo, exp_hi):
    """uint16 bf16 bit patterns of `shape`: random sign and mantissa, biased exponent in [exp_lo, exp_hi] (127 = [1, 2)): finite, |x| in [2^(exp_lo-127), 2^(exp_hi-126))"""
    rng = np.random.default_rng(seed_of(name))
    sign = rng.integers(0, 2, size=shape, dtype=np.uint16)
    exp = rng.integers(exp_lo, exp_hi + 1, size=shape, dtype=np.uint16)
    mant = rng.integers(0, 128, size=shape, dtype=np.uint16)
    return (sign << 15) | (exp << 7) | mant


def scale_of(HS):
    return 1.0 if HS >= 256 else HS ** -0.5


def toolchain():
    """the `hipcc --version` text of the compiler mila_amd.build uses ('' when it cannot be run)"""
    from mila_amd import build
    try:
        return subprocess.run([build.HIPCC, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return ""


def _history_len(row):
    return max(max(row.lengths, default=HOOK_POSITION + 1), ring_case(row)[2])


@functools.lru_cache(maxsize=2)
def _history(row_name):
    """K and V of every position of a row's history, [B, T, NKV, HS] bf16 bits on the device (the append entries' source order): |K| < 0.5, |V| < 1"""
    from gpu_util import dev_u16
    row = ALL_ROWS[row_name]
    shape = (row.B, _history_len(row), row.NKV, row.HS)
    return dev_u16(bf16_pattern("history-k/" + row_name, shape, 120, 125)), dev_u16(bf16_pattern("history-v/" + row_name, shape, 120, 126))


def _query(case, row):
    from gpu_util import dev_u16
    return dev_u16(bf16_pattern("query/" + case, (row.B, row.NH * row.HS), 121, 126))


def _cache16(row, cap, first, end):
    """a bf16 cache of `cap` rows holding positions [first, end) of the history (kv_write_bf16), NaN in every other row"""
    import torch
    from mila_amd import capi
    hk, hv = _history(row.name)
    K = torch.full((row.B, row.NKV, cap, row.HS), NAN_BITS, dtype=torch.int16, device="cuda")
    V = torch.full((row.B, row.NKV, cap, row.HS), NAN_BITS, dtype=torch.int16, device="cuda")
    if end > first:
        capi.call("kv_write_bf16", K, V, hk[:, first:end].contiguous(), hv[:, first:end].contiguous(), row.B, end - first, row.NKV, row.HS, first, cap)
    return K, V


def _cache8(row, cap, first, end):
    """the same rows through kv_write_fp8: e4m3 bytes and row scales; byte 0x7F and a NaN scale in every other row"""
    import torch
    from mila_amd import capi
    hk, hv = _history(row.name)
    K8 = torch.full((row.B, row.NKV, cap, row.HS), POISON8, dtype=torch.uint8, device="cuda")
    V8 = torch.full((row.B, row.NKV, cap, row.HS), POISON8, dtype=torch.uint8, device="cuda")
    Ks = torch.full((row.B, row.NKV, cap), float("nan"), dtype=torch.float32, device="cuda")
    Vs = torch.full((row.B, row.NKV, cap), float("nan"), dtype=torch.float32, device="cuda")
    capi.call("kv_write_fp8", K8, V8, Ks, Vs, hk[:, first:end].contiguous(), hv[:, first:end].contiguous(), row.B, end - first, row.NKV, row.HS, first, cap)
    return K8, V8, Ks, Vs


def _scratch(row):
    import torch
    from mila_amd import capi
    nbytes = capi.load().mila_cdna4_attn_decode_scratch_bytes(row.B, row.NH, row.HS)
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), C.c_size_t(nbytes)


def _band_first(length, window):
    return max(0, length - window) if window > 0 else 0


# ---- the launches -----------------------------------------------------------------------------------------------------------------------------------------------
def _decode(case, cache, row, cap, length, window, devpos=False):
    """Y of attn_decode_<cache>[_devpos] at `length` keys over positions [band start, length) of the history in a cache of `cap` rows"""
    from gpu_util import dev_i32, empty_u16
    from mila_amd import capi
    first = _band_first(length, window)
    arrays = _cache16(row, cap, first, length) if cache == "bf16" else _cache8(row, cap, first, length)
    Y = empty_u16(row.B, row.NH * row.HS)
    scratch, nbytes = _scratch(row)
    entry = "attn_decode_bf16" if cache == "bf16" else "attn_decode_kvfp8"
    head = (Y, _query(case, row)) + tuple(arrays) + (scratch, nbytes, row.B, row.NH, row.NKV, row.HS, cap)
    if devpos:
        max_len = max(length, capi.load().mila_cdna4_attn_decode_band_bucket(length, cap))      # the upper end of the length's bucket: what a graph is captured for
        capi.call(entry + "_devpos", *head, dev_i32([length - 1]), max_len, window, scale_of(row.HS))
    else:
        capi.call(entry, *head, length, window, scale_of(row.HS))
    return [Y]


@functools.lru_cache(maxsize=None)
def _rope_cache(HS, max_seq=4608):
    from gpu_util import empty_f32
    from mila_amd import capi
    cos, sin = empty_f32(max_seq, HS // 2), empty_f32(max_seq, HS // 2)
    capi.call("rope_build_cache", cos, sin, max_seq, HS, 1e4, 0)
    return cos, sin


class _FusedArgs(C.Structure):      # mila_fused_attn_args (csrc/internal.h)
    _fields_ = ([(n, C.c_void_p) for n in ("Y", "Kc", "Vc", "q_raw", "k_raw", "v_raw", "qw", "kw", "vw", "cos_cache", "sin_cache", "scratch")] +
                [("scratch_bytes", C.c_size_t), ("tickets", C.c_void_p), ("ticket_count", C.c_size_t),
                 ("warm_a", C.c_void_p), ("warm_a_bytes", C.c_size_t), ("warm_a_blocks", C.c_int),
                 ("warm_b", C.c_void_p), ("warm_b_bytes", C.c_size_t), ("warm_b_blocks", C.c_int), ("warm_b_pair_offset", C.c_size_t)] +
                [(n, C.c_int) for n in ("NH", "NKV", "HS", "capacity", "position")] +
                [("position_dev", C.c_void_p), ("window", C.c_int), ("scale", C.c_float), ("eps", C.c_float)])


def _fused(case, row, window, cap, pos, hook=None, kv_shared=False):
    """one fused launch at position `pos` over positions [band start, pos) of the history: Y (the partials under hook 'partials') and the appended K / V rows"""
    import torch
    from gpu_util import dev_u16, empty_u16
    from mila_amd import capi
    B, NH, NKV, HS = row.B, row.NH, row.NKV, row.HS
    K, V = _cache16(row, cap, _band_first(pos + 1, window), pos)
    qn, kn = NH * HS, NKV * HS
    packed = qn + 2 * kn + 24                               # (the row stride need not be the sum of the parts)
    rows = dev_u16(bf16_pattern("raw/" + case, (B, packed), 121, 127))
    q_raw, k_raw = rows[0, 0:], rows[0, qn:]
    v_raw = k_raw if kv_shared else rows[0, qn + kn:]
    qw, kw = dev_u16(bf16_pattern("qw/" + case, (HS,), 126, 127)), dev_u16(bf16_pattern("kw/" + case, (HS,), 126, 127))
    cos, sin = _rope_cache(HS)
    scratch, nbytes = _scratch(row)
    Y = empty_u16(B, NH * HS)
    scale = HS ** -0.5                                      # (the normed rows have unit rms: HS ** -0.5 keeps the scores of order 1 at every head size)
    tail = (NH, NKV, HS, cap, pos, None, window, scale, EPS)
    out = [Y]
    if hook is None and B == 1:
        capi.call("fused_attn_decode_bf16", Y, K, V, q_raw, k_raw, v_raw, qw, kw, None, cos, sin, scratch, nbytes, *tail)
    elif hook is None:
        capi.call("fused_attn_decode_batch_bf16", Y, K, V, q_raw, k_raw, v_raw, C.c_int64(packed), qw, kw, None, cos, sin, scratch, nbytes, B, *tail)
    elif hook == "onepass":
        nt = capi.load().mila_cdna4_attn_decode_ticket_count(1, NH)
        tickets = torch.zeros(nt, dtype=torch.int32, device="cuda")
        capi.call("fused_attn_decode_onepass_bf16", Y, K, V, q_raw, k_raw, v_raw, qw, kw, None, cos, sin, scratch, nbytes, tickets, C.c_size_t(nt), *tail)
    elif hook == "partials":
        plan = capi.attn_decode_plan(B, NH, NKV, HS, cap, window, pos + 1, fused=True, hooks=True)
        assert plan["splits"] > 1
        capi.call("fused_attn_decode_partials_bf16", K, V, q_raw, k_raw, v_raw, qw, kw, None, cos, sin, scratch, nbytes, *tail)
        out = [scratch[:plan["partial_floats"] * 4]]       # O | M | L | pad per (head, split); the pad keeps the zeros the scratch was handed out with
    else:
        warm = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        ptr = lambda t: t.data_ptr()
        a = _FusedArgs(ptr(Y), ptr(K), ptr(V), ptr(q_raw), ptr(k_raw), ptr(v_raw), ptr(qw), ptr(kw), None, ptr(cos), ptr(sin), ptr(scratch), nbytes.value, None, 0,
                       ptr(warm), 1 << 19, 3, ptr(warm) + (1 << 19), 1 << 19, 2, 1 << 18, NH, NKV, HS, cap, pos, None, window, scale, EPS)
        capi.call("fused_attn_decode_ex", C.byref(a))
    return out + [K[:, :, pos % cap], V[:, :, pos % cap]]


def _fused_position(row, kind):
    from test_attn_decode_classes_gpu import _fused_positions
    return next((w, cap, pos) for w, cap, pos, k in _fused_positions(row) if k == kind)


def _outputs(case):
    from mila_amd import capi
    what = _BY_CASE[case]
    if what[0] in ("decode", "devpos"):
        row = ALL_ROWS[what[2]]
        return _decode(case, what[1], row, row.capacity, what[3], row.window, devpos=what[0] == "devpos")
    if what[0] == "gh512":
        capi.tune(*GH512_TUNING)
        try:
            return _decode(case, "bf16", GH512_ROW, GH512_ROW.capacity, what[1], GH512_ROW.window)
        finally:
            capi.tune_reset()
    if what[0] == "ring":
        row = BY_NAME[what[2]]
        window, cap, length = ring_case(row)
        return _decode(case, what[1], row, cap, length, window)
    if what[0] == "fused":
        row = BY_NAME[what[1]]
        return _fused(case, row, *_fused_position(row, what[2]))
    row = HOOK_ROWS[what[2]]
    return _fused(case, row, row.window, row.capacity, HOOK_POSITION, hook=what[1], kv_shared=what[2] == "global")


def run(case):
    """run one case on the GPU: the SHA-256 (hex) of its outputs' bytes, in order"""
    import torch
    outs = _outputs(case)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()
