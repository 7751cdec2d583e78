"""The FP8 KV cache under batched rows against the bf16 rows step, on the Gemma-4 12B geometry: step time (time_decode_rows: graph replays between two events, the
median of --repeats) of B = 2 and 4 rows at each --contexts entry, per weight policy and KV kind, with the model's resident KV bytes; the one-row kv_fp8 graph step
(--one-row); and one fork of a prefix into one row (--fork: the two kv_rows_fork_layers entries on caches of the 12B layer table, between two events on the caller's
stream).  One JSON line per measurement.  --kv bf16 uses nothing newer than max_batch, so the same file measures a commit from before kv_fp8_rows existed.  Not part
of the product path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mila_amd import capi, host  # noqa: E402

G = host.GEMMA4_12B


def kv_bytes(rows, capacity, fp8):
    """resident KV bytes from the configuration: per layer 2 x NKV x capacity x (HS + 4 | 2 HS)"""
    total = 0
    for i in range(G["num_layers"]):
        glob = (i + 1) % G["sliding_window_pattern"] == 0
        nkv, hs = (G["num_global_kv_heads"], G["global_head_dim"]) if glob else (G["num_kv_heads"], G["head_dim"])
        total += rows * 2 * nkv * capacity * ((hs + 4) if fp8 else 2 * hs)
    return total


def steps(a):
    contexts = [int(c) for c in a.contexts.split(",")]
    max_seq = max(contexts) + a.warmup + a.steps + 8
    for policy in a.policies.split(","):
        for kv in a.kv.split(","):
            kw = dict(kv_fp8_rows=True) if kv == "fp8" else {}
            g = host.Gemma(policy, None, max_seq=max_seq, max_prefill=2048, seed=1234, max_batch=4, **kw)
            try:
                rng = np.random.default_rng(0)
                for ctx in contexts:
                    for b in range(4):
                        g.reset_row(b)
                    g.prefill_row(0, rng.integers(0, g.vocab, ctx))      # one prefill, shared: every row holds a real history of ctx tokens
                    g.fork_row(0, 0b1110, ctx)
                    for B in (int(v) for v in a.rows.split(",")):
                        ms = [g.time_decode_rows(B, ctx, a.steps, a.warmup)["device_ms_per_step"] for _ in range(a.repeats)]
                        print(json.dumps({"what": "rows_step", "policy": policy, "kv": kv, "context": ctx, "B": B, "ms_per_step": [round(v, 4) for v in ms],
                                          "median_ms_per_step": round(statistics.median(ms), 4), "kv_bytes_resident": kv_bytes(4, max_seq, kv == "fp8"),
                                          "device_state_bytes": g.memory_stats()["actual"]["device_state_bytes"]}), flush=True)
            finally:
                g.close()


def one_row(a):
    ctx = int(a.contexts.split(",")[0])
    for policy in a.policies.split(","):
        g = host.Gemma(policy, None, max_seq=ctx + a.warmup + a.steps + 8, max_prefill=2048, seed=1234, kv_fp8=True)
        try:
            g.prefill(np.random.default_rng(0).integers(0, g.vocab, ctx))
            ms = [g.time_decode(ctx, a.steps, a.warmup, "graph")["device_ms_per_step"] for _ in range(a.repeats)]
            print(json.dumps({"what": "one_row_kv_fp8_step", "policy": policy, "context": ctx, "ms_per_step": [round(v, 4) for v in ms],
                              "median_ms_per_step": round(statistics.median(ms), 4)}), flush=True)
        finally:
            g.close()


def fork(a):
    import torch
    lib = capi.load()
    cap, rows = 2112, 4
    kinds = ["bf16"] + (["fp8"] if hasattr(lib, "mila_cdna4_kv_rows_fork_layers_kvfp8") else [])
    for kind in kinds:
        keep, n = [], G["num_layers"]
        table = (capi.KvForkLayer * n)() if kind == "bf16" else (capi.KvForkLayerFp8 * n)()
        for i in range(n):
            glob = (i + 1) % G["sliding_window_pattern"] == 0
            nkv, hs = (G["num_global_kv_heads"], G["global_head_dim"]) if glob else (G["num_kv_heads"], G["head_dim"])
            if kind == "bf16":
                K, V = (torch.zeros((rows, nkv, cap, hs), dtype=torch.int16, device="cuda") for _ in range(2))
                keep += [K, V]
                table[i].K, table[i].V = K.data_ptr(), V.data_ptr()
            else:
                K, V = (torch.zeros((rows, nkv, cap, hs), dtype=torch.uint8, device="cuda") for _ in range(2))
                Ks, Vs = (torch.zeros((rows, nkv, cap), dtype=torch.float32, device="cuda") for _ in range(2))
                keep += [K, V, Ks, Vs]
                table[i].K8, table[i].V8, table[i].Ks, table[i].Vs = K.data_ptr(), V.data_ptr(), Ks.data_ptr(), Vs.data_ptr()
            table[i].NKV, table[i].capacity, table[i].HS, table[i].reserved = nkv, cap, hs, 0
        entry = "kv_rows_fork_layers_bf16" if kind == "bf16" else "kv_rows_fork_layers_kvfp8"
        for length in (64, 2048):
            us = []
            for i in range(a.repeats + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                capi.call(entry, table, n, rows, 0, 0b0010, length)
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    us.append(e0.elapsed_time(e1) * 1000.0)
            copied = kv_bytes(1, length, kind == "fp8")
            print(json.dumps({"what": "fork_one_row", "kv": kind, "len": length, "us": [round(v, 1) for v in us], "median_us": round(statistics.median(us), 1),
                              "bytes_copied": copied}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="bf16,fp8,fp4")
    ap.add_argument("--kv", default="bf16,fp8", help="KV kinds of the rows models: bf16, fp8 (kv_fp8_rows)")
    ap.add_argument("--contexts", default="2048,32768")
    ap.add_argument("--rows", default="2,4")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--one-row", action="store_true", help="the one-row kv_fp8 graph step instead")
    ap.add_argument("--fork", action="store_true", help="one fork into one row at 64 and 2048 positions instead")
    a = ap.parse_args()
    if a.fork:
        return fork(a)
    if a.one_row:
        return one_row(a)
    return steps(a)


if __name__ == "__main__":
    main()
