"""The launch-index classes of the split-K decode kernels (attn_decode_kernel in csrc/attention.hip, attn_decode_kvfp8_kernel in csrc/attention_kvfp8.hip) as a table of
shapes: one row per class of (heads per workgroup, workgroups per KV head, batch rows, split count) that plan_decode can produce and that the Gemma / Llama / GPT-2
geometries of tests/test_attention_gpu.py do not reach.  tests/test_attn_decode_classes_cpu.py holds every row to the plan it names (so a later change of a plan rule
cannot empty a class silently), tests/test_attn_decode_classes_gpu.py runs every row at every length against the float64 oracle.

A plain module: no pytest settings, no fixtures."""
import collections

Row = collections.namedtuple("Row", "name B NH NKV HS capacity window lengths plan")

FORM = "attn_decode"      # the wave-per-position kernel; the fp8 cache's plan names the same class FORM_KVFP8
FORM_KVFP8 = "attn_decode_kvfp8"


def _plan(gh, hgroups, splits):
    return dict(heads_per_group=gh, head_groups=hgroups, splits=splits, form=FORM)


def class_lengths(capacity, window, splits, extra=()):
    """the live lengths a row runs at.  1; splits - 1, splits, splits + 1 (the chunk is 1 and the trailing splits are empty); 64 splits - 1, 64 splits, 64 splits + 1
    (every split exactly full, and one key either side); the capacity; on a windowed row window - 1, window, window + 1 and one length beyond twice the window (the
    cache is then a ring where that exceeds the capacity) and the largest multiple of the split count inside the window (64 splits may exceed the window: this one
    fills every split exactly).  An unwindowed row cannot hold more than its capacity: longer lengths are dropped."""
    want = {1, splits - 1, splits, splits + 1, 64 * splits - 1, 64 * splits, 64 * splits + 1, capacity} | set(extra)
    if window > 0:
        want |= {window - 1, window, window + 1, 2 * window + 37, window // splits * splits}
    return tuple(sorted(n for n in want if n >= 1 and (window > 0 or n <= capacity)))


def _row(name, B, NH, NKV, HS, capacity, window, gh, hgroups, splits, extra=()):
    return Row(name, B, NH, NKV, HS, capacity, window, class_lengths(capacity, window, splits, extra), _plan(gh, hgroups, splits))


ROWS = [
    #    name              B  NH NKV  HS   cap  window | gh hgroups splits
    _row("gs8_hs128",      1, 16,  2, 128, 2048,    0,   4,  2, 32),
    _row("gs32_hs64",      1, 32,  1,  64, 2048,    0,   4,  8, 32),
    _row("gs16_hs256",     1, 16,  1, 256, 2048,    0,   4,  4, 32),
    _row("gs8_hs256_w150", 1, 16,  2, 256, 2048,  150,   4,  2,  3),
    _row("gs1_hs512",      1,  2,  2, 512, 2048,    0,   1,  1, 32),
    _row("gs4_hs512",      1,  8,  2, 512, 2048,    0,   2,  2, 32),
    _row("gs32_hs512",     1, 32,  1, 512, 2048,    0,   2, 16, 16),      # 16 heads on one KV head, but a band below 8192 keys: the scalar form; capped by the workgroup budget
    _row("batch3_local",   3, 16,  8, 256, 2048, 1024,   2,  1, 10),      # capped; a chunk of 103 keys is no multiple of the 8 waves
    _row("batch2_global",  2, 16,  1, 512, 2048,    0,   2,  8, 16),
    _row("batch2_gs8",     2, 16,  2, 128, 2048,    0,   4,  2, 32),
    _row("unsplit_long",   9, 64, 16,  64,  600,    0,   4,  1,  1, extra=(600,)),      # the workgroup budget leaves one split: the direct-write path over 600 keys
    _row("splits2",        1,  8,  2, 128, 2048,  100,   4,  1,  2),
    _row("splits17",       1,  8,  2, 128, 2048, 1050,   4,  1, 17),
    _row("splits33",       1,  8,  2, 128, 4096, 2100,   4,  1, 33),
    _row("splits64",       1,  8,  2, 128, 8192,    0,   4,  1, 64, extra=(4096, 4097, 8192)),      # kMaxSplits, in the 4096-key bucket and in the 8192-key one
]
BY_NAME = {r.name: r for r in ROWS}

# HS 512 with four heads per workgroup: the <512, 4> instantiation runs only under this tuning, and only on the bf16 cache (the fp8 entry reports MILA_E_UNSUPPORTED)
GH512_TUNING = ("attn.heads_per_group_512", 4)
GH512_ROW = _row("gs16_hs512_gh4", 1, 16, 1, 512, 2048, 0, 4, 4, 32)

RING_ROWS = ("gs32_hs64", "gs8_hs128", "gs4_hs512", "batch3_local")      # ring equals unbounded
RING_WINDOW = 200                                                        # the window a ring case gives a row that has none
FUSED_ROWS = tuple(r.name for r in ROWS if r.plan["head_groups"] > 1 and r.HS < 512) + ("batch3_local",)      # the fused prologue's hg == 0 rule


def ring_case(row):
    """(window, ring capacity, live length): a ring of window + 3 rows under a history that wraps it twice"""
    window = row.window or RING_WINDOW
    cap = window + 3
    return window, cap, 2 * cap + 41
