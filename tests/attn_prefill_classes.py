"""The kernel-form, batch and loop classes of prefill attention (csrc/attention_prefill.hip: flash_prefill_kernel, flash_prefill_kernel_s1, flash_prefill_pp_kernel) as a
table of shapes: one row per instantiation the default flash.form reaches -- the register-staged kernel at HS 64 / 128, the LDS-DMA kernel at HS 256 / 512, each with
4, 2 and 1 heads per workgroup --, each once unwindowed and once under a window that is no multiple of 16, with batches of 2 and 3 in every kernel group.  A row runs
SCHEDULES -- lists of (pos_offset, chunk) launches over one history -- chosen so that the workgroups of every row take every key-tile count from 1 to 8, hence every
lean-loop pair count of the double-buffered kernels, a ragged last query tile, a chunk shorter than, equal to and longer than a workgroup's query rows, and a wrapped ring.
tests/test_attn_prefill_classes_cpu.py holds every row to the plan it names (capi.attn_prefill_plan) and the table to the classes it is there for;
tests/test_attn_prefill_classes_gpu.py runs every launch against the float64 oracle.

A plain module: no pytest settings, no fixtures."""
import collections

Row = collections.namedtuple("Row", "name B NH NKV HS window scale plan")

KEYS_PER_TILE = 32      # csrc/attention_tiles.h: kKeysPerTile
NUM_CU = 256            # csrc/common.h: kNumCU -- the heavy / light work list deals workgroup ids in rounds of this many
FORMS = (9, 10, 11, 2, 1)      # the flash.form tunings beside the default 8 (csrc/attention_prefill.hip: plan_prefill)


def _plan(form, HB, DS, NW):
    return dict(form=form, HB=HB, DS=DS, NW=NW, QROWS=16 * (NW // (HB * DS)))


def _row(name, B, NH, NKV, HS, window, scale, form, HB, DS, NW):
    return Row(name, B, NH, NKV, HS, window, 1.0 if scale == 1 else HS ** -0.5, _plan(form, HB, DS, NW))


RS, DMA = "flash", "flash_dma"
ROWS = [
    #    name               B NH NKV  HS  window scale (1: 1.0, 0: HS ** -0.5) | form HB DS NW
    _row("rs64_hb4",        1, 8, 2,  64,   0, 0, RS, 4, 1, 4),
    _row("rs64_hb4_w75",    2, 4, 1,  64,  75, 1, RS, 4, 1, 4),
    _row("rs64_hb2",        1, 6, 3,  64,   0, 1, RS, 2, 1, 4),      # three head blocks per KV-head triple: an odd n_hblk
    _row("rs64_hb2_w100",   1, 4, 2,  64, 100, 0, RS, 2, 1, 4),
    _row("rs64_hb1",        3, 3, 3,  64,   0, 0, RS, 1, 1, 4),
    _row("rs64_hb1_w129",   1, 3, 3,  64, 129, 1, RS, 1, 1, 4),
    _row("rs128_hb4",       1, 4, 1, 128,   0, 1, RS, 4, 1, 4),
    _row("rs128_hb4_w100",  1, 8, 2, 128, 100, 0, RS, 4, 1, 4),
    _row("rs128_hb2",       2, 4, 2, 128,   0, 0, RS, 2, 1, 4),
    _row("rs128_hb2_w129",  1, 6, 3, 128, 129, 1, RS, 2, 1, 4),
    _row("rs128_hb1",       1, 2, 2, 128,   0, 1, RS, 1, 1, 4),
    _row("rs128_hb1_w75",   1, 3, 3, 128,  75, 0, RS, 1, 1, 4),
    _row("dma256_hb4",      1, 8, 2, 256,   0, 1, DMA, 4, 1, 4),
    _row("dma256_hb4_w75",  2, 4, 1, 256,  75, 0, DMA, 4, 1, 4),
    _row("dma256_hb2",      1, 6, 3, 256,   0, 0, DMA, 2, 1, 4),
    _row("dma256_hb2_w100", 1, 4, 2, 256, 100, 1, DMA, 2, 1, 4),
    _row("dma256_hb1",      3, 3, 3, 256,   0, 1, DMA, 1, 1, 4),
    _row("dma256_hb1_w129", 1, 2, 2, 256, 129, 0, DMA, 1, 1, 4),
    _row("dma512_hb4",      2, 4, 1, 512,   0, 1, DMA, 4, 2, 8),
    _row("dma512_hb4_w100", 1, 8, 2, 512, 100, 0, DMA, 4, 2, 8),
    _row("dma512_hb2",      1, 4, 2, 512,   0, 0, DMA, 2, 2, 4),
    _row("dma512_hb2_w75",  1, 6, 3, 512,  75, 1, DMA, 2, 2, 4),
    _row("dma512_hb1",      1, 3, 3, 512,   0, 0, DMA, 1, 2, 4),
    _row("dma512_hb1_w129", 2, 3, 3, 512, 129, 1, DMA, 1, 2, 4),
]
BY_NAME = {r.name: r for r in ROWS}
# (One head per workgroup is the plan of an odd group size.  The rows have GS 1: the decode entry, which every row's last from_zero position is also held to, takes
# group sizes 1, 2, 4, ... 32 only.)

# The heavy / light work list (item = bid / 256 odd ? n_items - 1 - k : k) with a last round of 256 workgroup ids that is only partly filled: 260 items are one full
# round and 4 ids of an odd one, 520 two full rounds and 8 ids of an even one.  More heads than the class rows have, so that the chunks stay short; a window keeps
# the work per row small.  One launch of PARTIAL_T rows from position 0.
PARTIAL_T = 2070
PARTIAL_ROWS = [
    (_row("partial_rs128_2rounds",  1,  8, 4, 128, 75, 0, RS, 2, 1, 4), 260),      # 65 query tiles of 32 rows x 4 head blocks
    (_row("partial_dma256_3rounds", 1, 16, 4, 256, 75, 1, DMA, 4, 1, 4), 520),     # 130 query tiles of 16 rows x 4 head blocks
]

FROM_ZERO_T = 229               # 229 % 16, % 32 and % 64 are all non-zero; the last workgroup of every row has 8 key tiles when unwindowed
HISTORY = 96                    # cached positions in front of the behind_history chunks
BEHIND_CHUNKS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
SHORT_CHUNKS = (20, 45, 31)     # from position 0: 1 key tile for every workgroup shape, then 3 for the 64-row ones (which from_zero gives even counts only)
RING_CHUNK = 40


def _back_to_back(start, chunks):
    out = []
    for c in chunks:
        out.append((start, c))
        start += c
    return out


def ring_capacity(row):
    return row.window + RING_CHUNK - 1


def schedule(row, name):
    """the (pos_offset, chunk) launches of a schedule.  from_zero: one chunk of 229 rows.  short_start: three short chunks from position 0.  behind_history: 96 cached
    positions, then chunks of 1 .. 65 rows back to back (>= 4 key tiles in every workgroup of an unwindowed row).  ring (windowed rows): chunks of 40 rows into a cache
    of window + 39 rows until the history is three capacities long."""
    if name == "from_zero":
        return [(0, FROM_ZERO_T)]
    if name == "short_start":
        return _back_to_back(0, SHORT_CHUNKS)
    if name == "behind_history":
        return _back_to_back(HISTORY, BEHIND_CHUNKS)
    if name == "ring":
        assert row.window > 0
        n = -(-3 * ring_capacity(row) // RING_CHUNK)
        return _back_to_back(0, (RING_CHUNK,) * n)
    raise KeyError(name)


def schedules_of(row):
    return ("from_zero", "short_start", "behind_history") + (("ring",) if row.window else ())


def history_len(row):
    return max(p + c for s in schedules_of(row) for p, c in schedule(row, s))


# ---- the kernels' index arithmetic, restated (attention_prefill.hip: "key range needed by the workgroup") ----
def workgroups(QROWS, pos_offset, chunk, window):
    """(q0, rows, kt0, ntiles) of every query tile of a launch: its first row, its row count (QROWS but for a ragged last tile), the tile-aligned first key and the
    number of 32-key tiles it walks"""
    out = []
    for q0 in range(0, chunk, QROWS):
        rows = min(QROWS, chunk - q0)
        pos_first, pos_last = pos_offset + q0, pos_offset + q0 + rows - 1
        kmin = max(0, pos_first - window + 1) if window > 0 else 0
        kt0 = kmin & ~(KEYS_PER_TILE - 1)
        out.append((q0, rows, kt0, (pos_last - kt0) // KEYS_PER_TILE + 1))
    return out


def lean_pairs(ntiles):
    """tile pairs a double-buffered kernel runs in its lean loop (MODE 0: for (t = 0; t + 4 <= ntiles; t += 2)) on an unwrapped cache"""
    return max(0, (ntiles - 2) // 2)


def double_buffered(HS, plan):
    """flash_prefill_kernel_s1's DB: the 8-wave form and every HS <= 256 form keep two [K | V] tile pairs and have the lean loop"""
    return plan["form"] == "flash_dma" and (plan["NW"] == 8 or HS <= 256)


def poison_floor(pos_offset, window):
    """cache rows below this one may hold NaN during a launch: the kernels read (masked) the tile-aligned rows below the first key of a band"""
    return (max(0, pos_offset - window + 1) if window > 0 else 0) & ~(KEYS_PER_TILE - 1)


# ---- spiked keys of from_zero: K rows set to half a query, so that one head's running maximum jumps late in its band ----
SPIKE_QROWS = (FROM_ZERO_T - 1, 200)
SPIKE_GAIN = 0.5


def spikes(row):
    """[(key position, query row, head)]: key <- SPIKE_GAIN x q[query row, head].  The key sits in the LAST tile of the lean loop of the query row's workgroup where
    that loop runs and the row sees the tile (10 and 23 keys from its end), else 58 keys behind the row: inside every window of the table."""
    out = []
    for qrow, head, back in zip(SPIKE_QROWS, (row.NH - 1, 0), (10, 23)):
        Q = row.plan["QROWS"]
        q0, _, kt0, ntiles = workgroups(Q, 0, FROM_ZERO_T, row.window)[qrow // Q]
        key = kt0 + 2 * KEYS_PER_TILE * lean_pairs(ntiles) - back
        if lean_pairs(ntiles) == 0 or (row.window > 0 and key < qrow - row.window + 1):
            key = qrow - 58
        out.append((key, qrow, head))
    return out


def spike_in_lean_loop(row, key, qrow):
    Q = row.plan["QROWS"]
    _, _, kt0, ntiles = workgroups(Q, 0, FROM_ZERO_T, row.window)[qrow // Q]
    return kt0 <= key < kt0 + 2 * KEYS_PER_TILE * lean_pairs(ntiles)


def partial_sample_rows(QROWS, T=PARTIAL_T):
    """the rows a partial_round launch is checked on: every row of the first three and the last three query tiles, plus every 37th row"""
    n = -(-T // QROWS)
    tiles = [0, 1, 2, n - 3, n - 2, n - 1]
    rows = {r for t in tiles for r in range(t * QROWS, min(T, (t + 1) * QROWS))} | set(range(0, T, 37))
    return sorted(rows)
