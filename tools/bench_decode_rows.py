"""Aggregate decode tok/s of the Gemma-4 12B model for B = 1 .. 4 sequences per step, per weight policy: context 2048 in every row (each row prefilled with its own
2048-token prompt), 128 timed greedy graph replays, the median of three.  B = 1 is the one-sequence graph path (mila_gemma_time_decode) of the same model, from the same
tool.  Prints one JSON line per (policy, B) and a closing line that says, per policy, whether the B = 2 aggregate exceeds B = 1.  Not part of the product path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mila_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="bf16,fp8,fp4")
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=4)
    a = ap.parse_args()
    verdict = {}
    for policy in a.policies.split(","):
        g = host.Gemma(policy, None, max_seq=a.context + a.warmup + a.steps + 8, max_prefill=a.context, seed=1234, max_batch=a.max_batch)
        rng = np.random.default_rng(0)
        for b in range(a.max_batch):
            g.prefill_row(b, rng.integers(0, g.vocab, a.context))
        agg = {}
        for B in range(1, a.max_batch + 1):
            ms = []
            for _ in range(a.repeats):
                t = g.time_decode(a.context, a.steps, a.warmup, "graph") if B == 1 else g.time_decode_rows(B, a.context, a.steps, a.warmup)
                ms.append(t["device_ms_per_step"])
            med = statistics.median(ms)
            agg[B] = B * 1000.0 / med
            print(json.dumps({"policy": policy, "B": B, "ms_per_step": [round(v, 4) for v in ms], "median_ms_per_step": round(med, 4), "aggregate_tok_s": round(agg[B], 1),
                              "vs_B1": round(agg[B] / agg[1], 3), "context": a.context, "steps": a.steps}), flush=True)
        verdict[policy] = {"B2_exceeds_B1": agg.get(2, 0) > agg[1], "best_B": max(agg, key=agg.get)}
        g.close()
    print(json.dumps({"rows_worth_dispatching": verdict}), flush=True)


if __name__ == "__main__":
    main()
