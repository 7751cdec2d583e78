"""Decode attention over the FP8 KV cache (attn_decode_kvfp8, csrc/attention_kvfp8.hip) against the bf16 cache (attn_decode_bf16) on the same box in the same
process, at Gemma's two layer geometries:
    local   NH 16, NKV 8, HS 256, window 1024, len 2048
    global  NH 16, NKV 1, HS 512, unwindowed, len 2048 / 8192 / 16384 / 32768      (from 8192 keys on both caches run their matrix-core forms)
Three legs: attn_decode_bf16, attn_decode_kvfp8 as planned, and attn_decode_kvfp8 under attn.kvfp8_mfma_decode 0 (the wave-per-position kernel at every length: what the
fp8 cache ran before it had a matrix-core form) -- the tuning is set before that leg's pass and reset after it.
Method: a pair of HIP events around every launch (attention + combine), the launches of a pass walking a ROTATION of cache copies whose total size exceeds the
256 MiB Infinity Cache, so every launch streams its K / V from HBM.  The entries are warmed up, then timed in alternating passes; the figure is the median over all
timed launches (passes x copies), the minimum beside it, and the spread of the per-pass medians (what a difference between two legs has to exceed).  Both caches hold the same random K / V (the fp8 one through kv_write_fp8).  Bytes are the live band's: band x NKV x 2 x HS x 2 for bf16,
band x NKV x 2 x (HS + 4) for fp8.
    python tools/bench_attn_kvfp8.py [--passes 15] [--out FILE]  ->  one JSON line per case"""
import os
os.environ.setdefault("MILA_CDNA4_TUNING", "1")      # (only for last_form: which kernel form served each entry)
import argparse
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mila_amd import capi  # noqa: E402

CASES = [
    # name, NH, NKV, HS, window, len
    ("gemma_local", 16, 8, 256, 1024, 2048),
    ("gemma_global", 16, 1, 512, 0, 2048),
    ("gemma_global", 16, 1, 512, 0, 8192),
    ("gemma_global", 16, 1, 512, 0, 16384),
    ("gemma_global", 16, 1, 512, 0, 32768),
]
ROTATION_BYTES = 320 << 20      # > the 256 MiB Infinity Cache


def bench(name, NH, NKV, HS, window, length, passes):
    lib = capi.load()
    cap, B = length, 1
    band = min(window, length) if window > 0 else length
    bytes16, bytes8 = band * NKV * 2 * HS * 2, band * NKV * 2 * (HS + 4)
    cache16, cache8 = cap * NKV * 2 * HS * 2, cap * NKV * 2 * (HS + 4)
    n16, n8 = -(-ROTATION_BYTES // cache16) + 1, -(-ROTATION_BYTES // cache8) + 1
    gen = torch.Generator(device="cuda").manual_seed(length + HS)
    rnd = lambda shape, amp: (torch.rand(shape, device="cuda", generator=gen) * 2 - 1).mul_(amp).to(torch.bfloat16).view(torch.int16)
    q = rnd((B, NH * HS), 1.0)
    sets16, sets8 = [], []
    for i in range(max(n16, n8)):
        k, v = rnd((B, cap, NKV, HS), 0.5), rnd((B, cap, NKV, HS), 1.0)      # [B, T, NKV, HS]: the append entries' source order
        if i < n16:
            Kc, Vc = torch.empty((B, NKV, cap, HS), dtype=torch.int16, device="cuda"), torch.empty((B, NKV, cap, HS), dtype=torch.int16, device="cuda")
            capi.call("kv_write_bf16", Kc, Vc, k, v, B, cap, NKV, HS, 0, cap)
            sets16.append((Kc, Vc))
        if i < n8:
            K8, V8 = torch.empty((B, NKV, cap, HS), dtype=torch.uint8, device="cuda"), torch.empty((B, NKV, cap, HS), dtype=torch.uint8, device="cuda")
            Ks, Vs = torch.empty((B, NKV, cap), dtype=torch.float32, device="cuda"), torch.empty((B, NKV, cap), dtype=torch.float32, device="cuda")
            capi.call("kv_write_fp8", K8, V8, Ks, Vs, k, v, B, cap, NKV, HS, 0, cap)
            sets8.append((K8, V8, Ks, Vs))
        del k, v
    nb = lib.mila_cdna4_attn_decode_scratch_bytes(B, NH, HS)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    Y16, Y8 = torch.empty((B, NH * HS), dtype=torch.int16, device="cuda"), torch.empty((B, NH * HS), dtype=torch.int16, device="cuda")
    run16 = lambda s: capi.call("attn_decode_bf16", Y16, q, s[0], s[1], scratch, C.c_size_t(nb), B, NH, NKV, HS, cap, length, window, 1.0)
    run8 = lambda s: capi.call("attn_decode_kvfp8", Y8, q, s[0], s[1], s[2], s[3], scratch, C.c_size_t(nb), B, NH, NKV, HS, cap, length, window, 1.0)

    def scalar_leg(fn):
        """fn() under attn.kvfp8_mfma_decode 0"""
        capi.tune("attn.kvfp8_mfma_decode", 0)
        try:
            return fn()
        finally:
            capi.tune_reset()

    capi.last_form()
    run16(sets16[0])
    form16 = "+".join(capi.last_form())
    run8(sets8[0])
    form8 = "+".join(capi.last_form())
    scalar_leg(lambda: run8(sets8[0]))
    form8s = "+".join(capi.last_form())
    torch.cuda.synchronize()
    # the two caches hold the same K / V up to the fp8 rounding: the outputs must agree to that rounding (a faster, different answer is no answer)
    diff = (Y16.view(torch.bfloat16).float() - Y8.view(torch.bfloat16).float()).abs().max().item()

    def one_pass(run, sets):
        """one launch per cache copy, each between its own pair of events (the host's time between two launches is not in the figure): microseconds per launch"""
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in sets]
        for (e0, e1), s in zip(ev, sets):
            e0.record()
            run(s)
            e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]

    for _ in range(3):      # warm-up: code objects, clocks, both rotations
        one_pass(run16, sets16)
        one_pass(run8, sets8)
        scalar_leg(lambda: one_pass(run8, sets8))
    t16, t8, t8s = [], [], []      # one list of launches per pass
    for _ in range(passes):
        t16.append(one_pass(run16, sets16))
        t8.append(one_pass(run8, sets8))
        t8s.append(scalar_leg(lambda: one_pass(run8, sets8)))
    flat = lambda t: [x for p in t for x in p]
    med = lambda t: statistics.median(flat(t))
    spread = lambda t: round(max(statistics.median(p) for p in t) - min(statistics.median(p) for p in t), 2)      # between the passes' own medians
    m16, m8, m8s = med(t16), med(t8), med(t8s)
    return {"case": name, "NH": NH, "NKV": NKV, "HS": HS, "window": window, "len": length, "band": band,
            "bf16_form": form16, "fp8_form": form8, "fp8_scalar_form": form8s,
            "bf16_us": round(m16, 2), "bf16_min_us": round(min(flat(t16)), 2), "bf16_pass_spread_us": spread(t16),
            "fp8_us": round(m8, 2), "fp8_min_us": round(min(flat(t8)), 2), "fp8_pass_spread_us": spread(t8),
            "fp8_scalar_us": round(m8s, 2), "fp8_scalar_min_us": round(min(flat(t8s)), 2), "fp8_scalar_pass_spread_us": spread(t8s),
            "fp8_over_bf16": round(m8 / m16, 3), "fp8_scalar_over_bf16": round(m8s / m16, 3), "fp8_over_fp8_scalar": round(m8 / m8s, 3),
            "pass_medians_us": {"bf16": [round(statistics.median(p), 2) for p in t16], "fp8": [round(statistics.median(p), 2) for p in t8],
                                "fp8_scalar": [round(statistics.median(p), 2) for p in t8s]},
            "bf16_band_bytes": bytes16, "fp8_band_bytes": bytes8,
            "bf16_GBps": round(bytes16 / m16 / 1e3, 1), "fp8_GBps": round(bytes8 / m8 / 1e3, 1),
            "copies": [len(sets16), len(sets8)], "passes": passes, "max_abs_output_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_kvfp8: no GPU -- a timing needs the MI355X")
    for case in CASES:
        row = bench(*case, passes=a.passes)
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
