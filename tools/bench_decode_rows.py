"""Aggregate decode tok/s of the Gemma-4 12B model for B = 1 .. 4 sequences per step, per weight policy: context 2048 in every row (each row prefilled with its own
2048-token prompt), 128 timed greedy graph replays, the median of three.  B = 1 is the one-sequence graph path (mila_gemma_time_decode) of the same model, from the same
tool.  Prints one JSON line per (policy, B) and a closing line that says, per policy, whether the B = 2 aggregate exceeds B = 1.
--stochastic: the step time of a stochastic GemmaModel.generate_batch at B = 2 .. max-batch instead -- (wall time of a batch of --steps tokens per row minus that of one
token per row) / (steps - 1), per repeat and as a median, at --temperature / --top-k / --top-p (default: Gemma's 1.0 / 64 / 0.95); it uses nothing but generate_batch,
so the same file measures a commit from before the sampler moved into the rows graph.
--logprobs N: the same measurements with token log-probabilities (top N) in every step.  Not part of the product path."""
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
    ap.add_argument("--stochastic", action="store_true")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=64)
    ap.add_argument("--top-p", type=float, default=0.95)
    ap.add_argument("--logprobs", type=int, default=None, help="token log-probabilities (top N, 0 .. 20) in every step")
    ap.add_argument("--min-p", type=float, default=0.0, help="sampling filter: min-p (stochastic steps)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, help="sampling filter: repetition penalty (every row gets a token table marked with its prompt)")
    ap.add_argument("--presence-penalty", type=float, default=0.0)
    ap.add_argument("--frequency-penalty", type=float, default=0.0)
    a = ap.parse_args()
    a.filters = dict(min_p=a.min_p, repetition_penalty=a.repetition_penalty, presence_penalty=a.presence_penalty, frequency_penalty=a.frequency_penalty)
    if a.stochastic:
        return stochastic(a)
    verdict = {}
    for policy in a.policies.split(","):
        g = host.Gemma(policy, None, max_seq=a.context + a.warmup + a.steps + 8, max_prefill=a.context, seed=1234, max_batch=a.max_batch)
        rng = np.random.default_rng(0)
        for b in range(a.max_batch):
            prompt = rng.integers(0, g.vocab, a.context)
            g.prefill_row(b, prompt)
            if host._filters(**a.filters)[1:] != host._filters()[1:]:
                g.set_token_table(b, prompt)
        g.set_sampling_filters(**a.filters)      # the greedy steps below: argmax of the adjusted logits when a penalty is set
        g.set_step_logprobs(a.logprobs)
        agg = {}
        for B in range(1, a.max_batch + 1):
            ms = []
            for _ in range(a.repeats):
                t = g.time_decode(a.context, a.steps, a.warmup, "graph") if B == 1 else g.time_decode_rows(B, a.context, a.steps, a.warmup)
                ms.append(t["device_ms_per_step"])
            med = statistics.median(ms)
            agg[B] = B * 1000.0 / med
            print(json.dumps({"policy": policy, "B": B, "ms_per_step": [round(v, 4) for v in ms], "median_ms_per_step": round(med, 4), "aggregate_tok_s": round(agg[B], 1),
                              "vs_B1": round(agg[B] / agg[1], 3), "context": a.context, "steps": a.steps, "logprobs": a.logprobs, "filters": a.filters}), flush=True)
        verdict[policy] = {"B2_exceeds_B1": agg.get(2, 0) > agg[1], "best_B": max(agg, key=agg.get)}
        g.close()
    print(json.dumps({"rows_worth_dispatching": verdict}), flush=True)


def stochastic(a):
    import time
    req = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, stop_tokens=[262143])
    for policy in a.policies.split(","):
        m = host.GemmaModel.synthetic(policy, None, context=a.context + a.steps + 8, prefill_chunk=min(a.context, 2048), seed=1234, max_batch=a.max_batch)
        rng = np.random.default_rng(0)
        prompts = [rng.integers(0, 1000, a.context).tolist() for _ in range(a.max_batch)]
        for B in range(2, a.max_batch + 1):
            def run(n, seed):
                t0 = time.perf_counter()
                got = m.generate_batch(prompts[:B], max_new_tokens=n, seed=seed, logprobs=a.logprobs, **req, **a.filters)
                return time.perf_counter() - t0, min(len(g[0]) for g in got)
            run(a.warmup + 1, 1)
            ms = []
            for i in range(a.repeats):
                t1, _ = run(1, 10 + i)
                tn, shortest = run(a.steps, 10 + i)
                assert shortest == a.steps, "a row stopped early: the step time would be of a shrinking batch"
                ms.append(1000.0 * (tn - t1) / (a.steps - 1))
            med = statistics.median(ms)
            print(json.dumps({"policy": policy, "mode": "stochastic generate_batch", "B": B, "ms_per_step": [round(v, 4) for v in ms], "median_ms_per_step": round(med, 4),
                              "spread_us": round(1000 * (max(ms) - min(ms)), 1), "aggregate_tok_s": round(B * 1000.0 / med, 1), "context": a.context, "steps": a.steps,
                              "sampling": [a.temperature, a.top_k, a.top_p], "logprobs": a.logprobs, "filters": a.filters}), flush=True)
        m.close()


if __name__ == "__main__":
    main()
