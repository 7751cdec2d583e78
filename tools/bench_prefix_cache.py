"""What the prefix cache of serveRequests buys and costs on the full-size model (profiles/r19_prefix_cache.md).
  workload    16 greedy requests that share a PREFIX-token header and end in distinct 32-token tails, 32 new tokens each, through GemmaModel.serve_requests_prefix with
              the cache on (cold at the start of every pass) and off, alternated inside one process, PASSES passes after a warm-up each: wall-clock tokens/s with the
              spread, prefill_tokens and the admission milliseconds.  The arithmetic part is asserted: the same steps on both sides, 16 x (PREFIX + 32) prefilled
              tokens with the cache off, (PREFIX + 32) + 15 x 32 with it on.
  off         the cache-off side once more through the flag-less serve_requests (the entry the build before this one has: run the tool there with --package-root for
              the comparison across builds).
  fork        one fork of 64 and of 2048 positions between HIP events on caches of the model's shapes, kv_rows_fork_layers_bf16 (one launch for all 48 layers)
              against kv_rows_fork_bf16 once per layer.
  break-even  per L in 1, 16, 64, 256: a request of L shared + 32 own tokens, admitted by fork + tail prefill against its whole prefill, host milliseconds.
usage: python tools/bench_prefix_cache.py [--package-root DIR] [--prefix N] [--only workload|fork|breakeven] [bf16 fp8 fp4]"""
import json
import os
import sys
import time

args = sys.argv[1:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option(name, default):
    if name in args:
        i = args.index(name)
        value = args[i + 1]
        del args[i:i + 2]
        return value
    return default


root = os.path.abspath(option("--package-root", root))
PREFIX = int(option("--prefix", 1024))
only = option("--only", None)
policies = [a for a in args if not a.startswith("--")] or ["bf16"]
sys.path.insert(0, root)
import numpy as np  # noqa: E402

from mila_amd import host  # noqa: E402

R, CONTEXT, TAIL, NEW, N, PASSES = 4, 4096, 32, 32, 16, 5
UNUSED = [262143]
HAS_CACHE = hasattr(host.GemmaModel, "serve_requests_prefix")


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def admission(stats):
    return sum(stats["admission_ms"].values())


for policy in policies:
    rng = np.random.default_rng(0)
    header = rng.integers(0, 1000, PREFIX).tolist()
    # tails that split from the header's continuation AND from one another at their first token (ids 1000 .. : never in a header)
    reqs = [dict(prompt=header + [1000 + i] + rng.integers(0, 1000, TAIL - 1).tolist(), max_new_tokens=NEW, stop_tokens=UNUSED) for i in range(N)]
    if only in (None, "workload", "breakeven"):
        m = host.GemmaModel.synthetic(policy, None, context=CONTEXT, prefill_chunk=2048, seed=1234, max_batch=R)

        def run(mode):
            if mode == "flagless":
                t0 = time.perf_counter()
                rows, stats = m.serve_requests(reqs)
            else:
                m.clear_prefix_cache()
                t0 = time.perf_counter()
                rows, stats = m.serve_requests_prefix(reqs, prefix_cache=(mode == "on"))
            dt = time.perf_counter() - t0
            assert sum(len(r[0]) for r in rows) == N * NEW, mode
            return dt, rows, stats

    if only in (None, "workload"):
        modes = ["on", "off", "flagless"] if HAS_CACHE else ["flagless"]
        first = {mode: run(mode) for mode in modes}      # warm-up: graph captures, scratch growth
        rate, adm, last = {k: [] for k in modes}, {k: [] for k in modes}, {}
        for _ in range(PASSES):
            for mode in modes:
                dt, rows, stats = run(mode)
                rate[mode].append(N * NEW / dt)
                adm[mode].append(admission(stats))
                last[mode] = stats
        whole = N * (PREFIX + TAIL)
        assert last["flagless"]["prefill_tokens"] == whole and last["flagless"]["prefills"] == N, last["flagless"]
        if HAS_CACHE:
            on, off = last["on"], last["off"]
            assert off["prefill_tokens"] == whole and on["prefill_tokens"] == (PREFIX + TAIL) + (N - 1) * TAIL, (on, off)
            assert on["steps"] == off["steps"] == last["flagless"]["steps"] and on["prefills"] == N and on["prefix_forks"] + on["prefix_in_place"] == N - 1, (on, off)
            assert on["reused_tokens"] == [0] + [PREFIX] * (N - 1), on
            # greedy requests: the tokens may differ in bits-of-a-tie only where a suffix prefill's GEMM form differs; report, do not assert
            same = sum(a[0] == b[0] for a, b in zip(first["on"][1], first["off"][1]))
        for mode in modes:
            st = last[mode]
            print(json.dumps({"policy": policy, "what": "workload", "prefix": PREFIX, "mode": mode, "tok_s": spread(rate[mode]), "admission_ms": spread(adm[mode]),
                              "prefill_tokens": st["prefill_tokens"], "steps": st["steps"], "prefill_ms_last": round(st["admission_ms"]["prefill"], 3),
                              "fork_ms_last": round(st["admission_ms"]["fork"], 3), "prefix_forks": st.get("prefix_forks"), "prefix_in_place": st.get("prefix_in_place")}), flush=True)
        if HAS_CACHE:
            r_on, r_off = spread(rate["on"]), spread(rate["off"])
            print(json.dumps({"policy": policy, "what": "workload, on against off", "prefix": PREFIX, "ratio_of_medians": round(r_on["median"] / r_off["median"], 3),
                              "beyond_the_off_spread": r_on["min"] > r_off["max"], "requests_with_the_same_tokens": same}), flush=True)

    if only in (None, "breakeven") and HAS_CACHE and policy == "bf16":
        filler = dict(prompt=[7, 8, 9], max_new_tokens=1, stop_tokens=UNUSED)
        donor = dict(prompt=header[:512], max_new_tokens=1, stop_tokens=UNUSED)
        for L in (1, 16, 64, 256):
            q = dict(prompt=header[:L] + [1000] + rng.integers(0, 1000, TAIL - 1).tolist(), max_new_tokens=1, stop_tokens=UNUSED)
            cost = {"reuse": [], "whole": []}
            for p in range(PASSES + 1):
                m.clear_prefix_cache()
                m.serve_requests_prefix([filler, donor])      # the donor in row 1: the request enters row 0 and forks
                _, st = m.serve_requests_prefix([q])
                assert st["reused_tokens"] == [L] and st["donor_row"] == [1] and st["prefix_forks"] == 1 and st["prefill_tokens"] == TAIL, st
                _, sw = m.serve_requests_prefix([q], prefix_cache=False)
                assert sw["prefill_tokens"] == L + TAIL, sw
                if p:
                    cost["reuse"].append(st["admission_ms"]["prefill"] + st["admission_ms"]["fork"])
                    cost["whole"].append(sw["admission_ms"]["prefill"])
            a, b = spread(cost["reuse"]), spread(cost["whole"])
            print(json.dumps({"policy": policy, "what": "break-even: fork + tail prefill against the whole prefill, host ms", "L": L, "tail": TAIL, "fork_and_tail_ms": a,
                              "whole_ms": b, "reuse_wins_beyond_the_spread": a["max"] < b["min"]}), flush=True)
    if only in (None, "workload", "breakeven"):
        m.close()

    if only in (None, "fork") and HAS_CACHE and policy == "bf16":
        # the two device entries on caches of the model's shapes (no model needed): 40 local layers of 8 heads x 256, 8 global ones of 1 head x 512, four rows
        import torch
        from mila_amd import capi
        kinds = [(1, 512) if (i + 1) % 6 == 0 else (8, 256) for i in range(48)]
        caches = [(torch.zeros((R, nkv, CONTEXT, hs), dtype=torch.int16, device="cuda"), torch.zeros((R, nkv, CONTEXT, hs), dtype=torch.int16, device="cuda")) for nkv, hs in kinds]
        table = (capi.KvForkLayer * len(kinds))()
        for i, ((nkv, hs), (K, V)) in enumerate(zip(kinds, caches)):
            table[i].K, table[i].V, table[i].NKV, table[i].capacity, table[i].HS = K.data_ptr(), V.data_ptr(), nkv, CONTEXT, hs

        def one_launch(length):
            capi.call("kv_rows_fork_layers_bf16", table, len(kinds), R, 0, 0b0010, length)

        def per_layer(length):
            for (nkv, hs), (K, V) in zip(kinds, caches):
                capi.call("kv_rows_fork_bf16", K, V, R, nkv, CONTEXT, hs, 0, 0b0010, length)

        def timed(fn, length, reps):
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(length)
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1))
            return out

        for length in (64, 2048):
            out = {}
            for name, fn in (("one_launch", one_launch), ("per_layer", per_layer)):
                timed(fn, length, 3)
                out[name] = spread(timed(fn, length, 20))
            print(json.dumps({"policy": policy, "what": "one fork into one row, 48 layers, HIP-event ms, 20 repetitions", "positions": length, **out,
                              "one_launch_faster_beyond_the_spread": out["one_launch"]["max"] < out["per_layer"]["min"]}), flush=True)
        del caches
