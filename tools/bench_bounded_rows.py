"""The bounded sliding-window KV cache under batched rows (bounded_local_kv_rows) against the flat bf16 rows model, on the Gemma-4 12B geometry, prefill chunk 2048
(ring capacity 3071).  One JSON line per measurement; nothing here is part of the product path.
  (default)   per weight policy: both rows models in ONE process at max_seq = the largest context + slack; per context one shared prefill + fork into four rows; the
              step time (time_decode_rows: graph replays between two events) of B = 2 and 4 rows, the two models ALTERNATED --repeats times; with each model's resident
              KV bytes (derived from the capacities) and device_state_bytes (reported by the model).
  --memory    no step: both models built at --contexts' largest entry, KV bytes and device_state_bytes only (a 32 848-position flat model is 45 GB of KV).
  --fork      one fork into one row at 64, 2048 and 32 768 positions between two events: the band entry on a ring layer table against the whole-prefix entry on a flat
              one (the 12B layer table, two rows).
  --prefix    the workload of tools/bench_prefix_cache.py (16 greedy requests sharing a 1024-token header, 32-token tails, 32 new tokens, four rows) through
              serve_requests_prefix on both models, alternated: tokens/s, prefill tokens, fork milliseconds."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mila_amd import capi, host  # noqa: E402

G = host.GEMMA4_12B
CHUNK = 2048
RING_CAPACITY = G["window"] + CHUNK - 1


def layer(i):
    glob = (i + 1) % G["sliding_window_pattern"] == 0
    return glob, (G["num_global_kv_heads"], G["global_head_dim"]) if glob else (G["num_kv_heads"], G["head_dim"])


def kv_bytes(rows, max_seq, ring):
    """resident KV bytes from the configuration: per layer 2 (K, V) x NKV x capacity x HS x 2 bytes, the ring's capacity on a sliding-window layer of a ring model"""
    total = 0
    for i in range(G["num_layers"]):
        glob, (nkv, hs) = layer(i)
        total += rows * 2 * nkv * (min(max_seq, RING_CAPACITY) if ring and not glob else max_seq) * hs * 2
    return total


def build(policy, kind, max_seq):
    return host.Gemma(policy, None, max_seq=max_seq, max_prefill=CHUNK, seed=1234, max_batch=4, **(dict(bounded_local_kv_rows=True) if kind == "ring" else {}))


def memory(a):
    max_seq = max(int(c) for c in a.contexts.split(","))
    for kind in ("flat", "ring"):
        g = build(a.policies.split(",")[0], kind, max_seq)
        try:
            st = g.memory_stats()
            print(json.dumps({"what": "memory", "kind": kind, "max_seq": max_seq, "rows": 4, "kv_bytes_derived": kv_bytes(4, max_seq, kind == "ring"),
                              "device_state_bytes": st["actual"]["device_state_bytes"], "required_device_state_bytes": st["required"]["device_state_bytes"]}), flush=True)
        finally:
            g.close()


def steps(a):
    contexts = [int(c) for c in a.contexts.split(",")]
    max_seq = max(contexts) + a.warmup + a.steps + 8      # (every timing starts again from the context: the same positions are rewritten)
    for policy in a.policies.split(","):
        models = {kind: build(policy, kind, max_seq) for kind in ("flat", "ring")}
        try:
            for ctx in contexts:
                tokens = np.random.default_rng(0).integers(0, G["vocab_size"], ctx)
                for g in models.values():
                    for b in range(4):
                        g.reset_row(b)
                    g.prefill_row(0, tokens)      # one prefill, shared: every row holds a real history of ctx tokens
                    g.fork_row(0, 0b1110, ctx)
                for B in (int(v) for v in a.rows.split(",")):
                    ms = {kind: [] for kind in models}
                    for _ in range(a.repeats):
                        for kind, g in models.items():      # alternated: flat, ring, flat, ring ...
                            ms[kind].append(g.time_decode_rows(B, ctx, a.steps, a.warmup)["device_ms_per_step"])
                    for kind, g in models.items():
                        print(json.dumps({"what": "rows_step", "policy": policy, "kind": kind, "context": ctx, "B": B, "ms_per_step": [round(v, 4) for v in ms[kind]],
                                          "median_ms_per_step": round(statistics.median(ms[kind]), 4), "kv_bytes_derived": kv_bytes(4, max_seq, kind == "ring"),
                                          "device_state_bytes": g.memory_stats()["actual"]["device_state_bytes"]}), flush=True)
                    print(json.dumps({"what": "rows_step, ring against flat", "policy": policy, "context": ctx, "B": B,
                                      "ratio_of_medians": round(statistics.median(ms["ring"]) / statistics.median(ms["flat"]), 4),
                                      "ring_inside_the_flat_spread": min(ms["flat"]) <= statistics.median(ms["ring"]) <= max(ms["flat"])}), flush=True)
        finally:
            for g in models.values():
                g.close()


def fork(a):
    import torch
    rows, n, flat_cap = 2, G["num_layers"], 32768 + 80
    for kind in ("band", "whole"):
        keep = []
        table = (capi.KvForkLayerBand * n)() if kind == "band" else (capi.KvForkLayer * n)()
        for i in range(n):
            glob, (nkv, hs) = layer(i)
            cap = RING_CAPACITY if kind == "band" and not glob else flat_cap
            K, V = (torch.zeros((rows, nkv, cap, hs), dtype=torch.int16, device="cuda") for _ in range(2))
            keep += [K, V]
            table[i].K, table[i].V, table[i].NKV, table[i].capacity, table[i].HS = K.data_ptr(), V.data_ptr(), nkv, cap, hs
            if kind == "band":
                table[i].window = 0 if glob else G["window"]
        entry = "kv_rows_fork_layers_band_bf16" if kind == "band" else "kv_rows_fork_layers_bf16"
        for length in (64, 2048, 32768):
            us = []
            for i in range(a.repeats + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                capi.call(entry, table, n, rows, 0, 0b0010, length)
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    us.append(e0.elapsed_time(e1) * 1000.0)
            copied = sum(2 * layer(i)[1][0] * (min(length, G["window"]) if kind == "band" and not layer(i)[0] else length) * layer(i)[1][1] * 2 for i in range(n))
            print(json.dumps({"what": "fork_one_row", "kind": kind, "len": length, "us": [round(v, 1) for v in us], "median_us": round(statistics.median(us), 1),
                              "bytes_copied": copied}), flush=True)
        del keep
        torch.cuda.empty_cache()


def prefix(a):
    R, CONTEXT, PREFIX, TAIL, NEW, N = 4, 4096, 1024, 32, 32, 16
    rng = np.random.default_rng(0)
    header = rng.integers(0, 1000, PREFIX).tolist()
    reqs = [dict(prompt=header + [1000 + i] + rng.integers(0, 1000, TAIL - 1).tolist(), max_new_tokens=NEW, stop_tokens=[262143]) for i in range(N)]
    for policy in a.policies.split(","):
        models = {kind: host.GemmaModel.synthetic(policy, None, context=CONTEXT, prefill_chunk=CHUNK, seed=1234, max_batch=R,
                                                  **(dict(bounded_local_kv_rows=True) if kind == "ring" else {})) for kind in ("flat", "ring")}
        try:
            def run(m):
                m.clear_prefix_cache()
                t0 = time.perf_counter()
                rows, stats = m.serve_requests_prefix(reqs)
                dt = time.perf_counter() - t0
                assert sum(len(r[0]) for r in rows) == N * NEW
                return dt, rows, stats
            first = {kind: run(m) for kind, m in models.items()}      # warm-up: graph captures, scratch growth
            rate, last = {k: [] for k in models}, {}
            for _ in range(a.repeats):
                for kind, m in models.items():
                    dt, _, last[kind] = run(m)
                    rate[kind].append(N * NEW / dt)
            same = sum(x[0] == y[0] for x, y in zip(first["flat"][1], first["ring"][1]))
            for kind, st in last.items():
                print(json.dumps({"what": "prefix workload", "policy": policy, "kind": kind, "tok_s": [round(v, 1) for v in rate[kind]], "median_tok_s": round(statistics.median(rate[kind]), 1),
                                  "prefill_tokens": st["prefill_tokens"], "reused_tokens": st["reused_tokens"], "prefix_forks": st["prefix_forks"], "prefix_in_place": st["prefix_in_place"],
                                  "fork_ms": round(st["admission_ms"]["fork"], 3), "prefill_ms": round(st["admission_ms"]["prefill"], 3), "requests_with_the_flat_tokens": same}), flush=True)
        finally:
            for m in models.values():
                m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="bf16")
    ap.add_argument("--contexts", default="2048,32768")
    ap.add_argument("--rows", default="2,4")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--fork", action="store_true")
    ap.add_argument("--prefix", action="store_true")
    a = ap.parse_args()
    if a.memory:
        return memory(a)
    if a.fork:
        return fork(a)
    if a.prefix:
        return prefix(a)
    return steps(a)


if __name__ == "__main__":
    main()
