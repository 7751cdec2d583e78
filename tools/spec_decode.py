"""Speculative greedy decode of the Gemma-4 12B model at context 2048, per weight policy: what a chain step (T = 2 .. 4 consecutive positions of one sequence) costs
against the one-row graph step and against the independent-rows step at the same T (time_decode_rows, the yardstick), and what generate() makes of it -- tokens per
step and tok/s with the default drafter (prompt lookup) on a repetitive prompt, and with a full-acceptance hint (the ceiling).  Prints one JSON line per policy.
Not part of the product path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mila_amd import host  # noqa: E402


def _median(f, repeats):
    return statistics.median(f()["device_ms_per_step"] for _ in range(repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="bf16,fp8,fp4")
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--draft-tokens", type=int, default=3)
    ap.add_argument("--config", default=None, help="JSON geometry (default: Gemma-4 12B)")
    a = ap.parse_args()
    cfg = json.loads(a.config) if a.config else None
    K = a.draft_tokens
    max_seq = a.context + (a.steps + a.warmup) * (K + 1) + 8
    for policy in a.policies.split(","):
        out = {"policy": policy, "context": a.context, "steps": a.steps, "draft_tokens": K}
        rng = np.random.default_rng(0)
        prompt = rng.integers(0, 1000, a.context)
        # the yardstick: one row, and T independent rows, on a max_batch model
        g = host.Gemma(policy, cfg, max_seq=max_seq, max_prefill=a.context, seed=1234, max_batch=K + 1)
        for b in range(K + 1):
            g.prefill_row(b, prompt)
        out["one_row_ms"] = round(_median(lambda: g.time_decode(a.context, a.steps, a.warmup, "graph"), a.repeats), 4)
        out["rows_ms"] = {T: round(_median(lambda: g.time_decode_rows(T, a.context, a.steps, a.warmup), a.repeats), 4) for T in range(2, K + 2)}
        g.close()
        # the chain step on a draft_tokens model (the drafts are whatever the token words hold: the step's cost does not depend on what it accepts)
        g = host.Gemma(policy, cfg, max_seq=max_seq, max_prefill=a.context, seed=1234, draft_tokens=K)
        g.prefill(prompt)
        out["chain_ms"] = {T: round(_median(lambda: g.time_decode_chain(T, a.context, a.steps, a.warmup), a.repeats), 4) for T in range(2, K + 2)}
        out["chain_graph_nodes"] = g.chain_graph_info()["nodes"]
        g.close()
        out["chain_over_rows_us"] = {T: round(1000 * (out["chain_ms"][T] - out["rows_ms"][T]), 1) for T in out["chain_ms"]}
        out["chain_over_one_row"] = {T: round(out["chain_ms"][T] / out["one_row_ms"], 3) for T in out["chain_ms"]}
        # tokens per step at which a T-row chain step pays for itself: chain_ms / one_row_ms tokens; as an acceptance rate of the T - 1 drafts
        out["break_even_acceptance"] = {T: round((out["chain_ms"][T] / out["one_row_ms"] - 1) / (T - 1), 3) for T in out["chain_ms"]}
        # generate(): a repetitive prompt (a 16-token phrase over and over), the default drafter and the ceiling
        phrase = rng.integers(0, 1000, 16).tolist()
        rep = (phrase * (a.context // 16 + 1))[:a.context - a.new_tokens - 8]
        m = host.GemmaModel.synthetic(policy, cfg, context=a.context, prefill_chunk=min(a.context, 2048), seed=1234, draft_tokens=K)

        def timed(n, hint=None):
            t0 = time.perf_counter()
            toks, status, _ = m.generate(rep, max_new_tokens=n, stop_tokens=[cfg["vocab_size"] - 1 if cfg else 262143], draft_hint=hint)
            return toks, time.perf_counter() - t0, m.speculation_stats()

        timed(2)                                   # the prompt's prefill; every later request reuses it but for the last position
        _, t_first, _ = timed(1)                   # prefill of the last position + the first token
        for name, hint in (("default_drafter", None), ("full_acceptance_hint", True)):
            if hint:
                hint = timed(a.new_tokens)[0]      # the same request's own output
            toks, t, st = timed(a.new_tokens, hint)
            steps = max(st["steps"], 1)
            out[name] = {"tokens": len(toks), "steps": st["steps"], "chain_steps": st["chain_steps"], "drafted": st["drafted"], "accepted": st["accepted"],
                         "tokens_per_step": round((len(toks) - 1) / steps, 3), "tok_s": round((len(toks) - 1) / max(t - t_first, 1e-9), 1),
                         "acceptance": round(st["accepted"] / max(st["drafted"], 1), 3)}
        m.close()
        out["one_row_tok_s"] = round(1000.0 / out["one_row_ms"], 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
