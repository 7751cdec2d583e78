"""Speculative greedy decode of the Gemma-4 12B model at context 2048, per weight policy: what a chain step (T = 2 .. 4 consecutive positions of one sequence) costs
against the one-row graph step and against the independent-rows step at the same T (time_decode_rows, the yardstick), and what generate() makes of it -- tokens per
step and tok/s with the default drafter (prompt lookup) on a repetitive prompt, and with a full-acceptance hint (the ceiling).  Prints one JSON line per policy.
--stochastic: the same for speculative SAMPLING (GenerateParams::speculative_sampling) at --temperature / --top-k / --top-p (default: Gemma's 1.0 / 64 / 0.95) -- the
chain step with the sampling tail against the greedy chain step and against the one-row stochastic graph step, and generate() against the plain stochastic generate()
of the same model.  --baseline-only stops after the one-row figures (they need nothing this mode added).
--logprobs N: every step and every request with token log-probabilities (top N, 0 .. 20) on.
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
    ap.add_argument("--stochastic", action="store_true")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=64)
    ap.add_argument("--top-p", type=float, default=0.95)
    ap.add_argument("--logprobs", type=int, default=None, help="token log-probabilities (top N, 0 .. 20) in every step and request")
    a = ap.parse_args()
    if a.stochastic:
        return stochastic(a)
    cfg = json.loads(a.config) if a.config else None
    K = a.draft_tokens
    max_seq = a.context + (a.steps + a.warmup) * (K + 1) + 8
    for policy in a.policies.split(","):
        out = {"policy": policy, "context": a.context, "steps": a.steps, "draft_tokens": K, "logprobs": a.logprobs}
        rng = np.random.default_rng(0)
        prompt = rng.integers(0, 1000, a.context)
        # the yardstick: one row, and T independent rows, on a max_batch model
        g = host.Gemma(policy, cfg, max_seq=max_seq, max_prefill=a.context, seed=1234, max_batch=K + 1)
        for b in range(K + 1):
            g.prefill_row(b, prompt)
        g.set_step_logprobs(a.logprobs)
        out["one_row_ms"] = round(_median(lambda: g.time_decode(a.context, a.steps, a.warmup, "graph"), a.repeats), 4)
        out["rows_ms"] = {T: round(_median(lambda: g.time_decode_rows(T, a.context, a.steps, a.warmup), a.repeats), 4) for T in range(2, K + 2)}
        g.close()
        # the chain step on a draft_tokens model (the drafts are whatever the token words hold: the step's cost does not depend on what it accepts)
        g = host.Gemma(policy, cfg, max_seq=max_seq, max_prefill=a.context, seed=1234, draft_tokens=K)
        g.prefill(prompt)
        g.set_step_logprobs(a.logprobs)
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
            toks = m.generate(rep, max_new_tokens=n, stop_tokens=[cfg["vocab_size"] - 1 if cfg else 262143], draft_hint=hint, logprobs=a.logprobs)[0]
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


def stochastic(a):
    cfg = json.loads(a.config) if a.config else None
    K = a.draft_tokens
    setting = (a.temperature, a.top_k, a.top_p)
    req = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    max_seq = a.context + (a.steps + a.warmup) * (K + 1) + 8
    for policy in a.policies.split(","):
        out = {"policy": policy, "mode": "stochastic", "context": a.context, "steps": a.steps, "draft_tokens": K, "sampling": setting}
        rng = np.random.default_rng(0)
        prompt = rng.integers(0, 1000, a.context)
        stop = [cfg["vocab_size"] - 1 if cfg else 262143]
        phrase = rng.integers(0, 1000, 16).tolist()
        rep = (phrase * (a.context // 16 + 1))[:a.context - a.new_tokens - 8]
        # the one-row stochastic graph step, through the plain generate() of a plain model: (time of n tokens - time of 1) / (n - 1), the median of `repeats`
        m = host.GemmaModel.synthetic(policy, cfg, context=a.context, prefill_chunk=min(a.context, 2048), seed=1234)

        def plain(n, seed):
            t0 = time.perf_counter()
            toks = m.generate(rep, max_new_tokens=n, stop_tokens=stop, seed=seed, logprobs=a.logprobs, **req)[0]
            return toks, time.perf_counter() - t0

        plain(2, 1)
        rates = []
        for i in range(a.repeats):
            _, t1 = plain(1, 10 + i)
            toks, tn = plain(a.new_tokens, 10 + i)
            rates.append((len(toks) - 1) / max(tn - t1, 1e-9))
        m.close()
        out["one_row_stochastic_tok_s"] = round(statistics.median(rates), 1)
        out["one_row_stochastic_tok_s_runs"] = [round(r, 1) for r in rates]
        out["one_row_stochastic_ms"] = round(1000.0 / statistics.median(rates), 4)
        if a.baseline_only:
            print(json.dumps(out), flush=True)
            continue
        # the chain step: greedy tail, then the sampling tail (the drafts are whatever the token words hold: the step's cost does not depend on what it accepts)
        g = host.Gemma(policy, cfg, max_seq=max_seq, max_prefill=a.context, seed=1234, draft_tokens=K)
        g.prefill(prompt)
        g.set_step_logprobs(a.logprobs)
        out["one_row_greedy_ms"] = round(_median(lambda: g.time_decode(a.context, a.steps, a.warmup, "graph"), a.repeats), 4)
        out["chain_greedy_ms"] = {T: round(_median(lambda: g.time_decode_chain(T, a.context, a.steps, a.warmup), a.repeats), 4) for T in range(2, K + 2)}
        greedy_nodes = g.chain_graph_info()["nodes"]
        g.set_step_sampling("chain", setting, [0.5] * (K + 1))
        out["chain_stochastic_ms"] = {T: round(_median(lambda: g.time_decode_chain(T, a.context, a.steps, a.warmup), a.repeats), 4) for T in range(2, K + 2)}
        out["chain_graph_nodes"] = {"greedy": greedy_nodes, "stochastic": g.chain_graph_info()["nodes"]}
        g.close()
        out["stochastic_over_greedy_chain_us"] = {T: round(1000 * (out["chain_stochastic_ms"][T] - out["chain_greedy_ms"][T]), 1) for T in out["chain_greedy_ms"]}
        out["chain_over_one_row_stochastic"] = {T: round(out["chain_stochastic_ms"][T] / out["one_row_stochastic_ms"], 3) for T in out["chain_stochastic_ms"]}
        out["break_even_acceptance"] = {T: round((out["chain_stochastic_ms"][T] / out["one_row_stochastic_ms"] - 1) / (T - 1), 3) for T in out["chain_stochastic_ms"]}
        # generate() with speculative_sampling: the default drafter on the repetitive prompt, and the ceiling (hint = the same request's own output)
        m = host.GemmaModel.synthetic(policy, cfg, context=a.context, prefill_chunk=min(a.context, 2048), seed=1234, draft_tokens=K)

        def timed(n, hint=None, seed=10):
            t0 = time.perf_counter()
            toks = m.generate(rep, max_new_tokens=n, stop_tokens=stop, seed=seed, draft_hint=hint, speculative_sampling=True, logprobs=a.logprobs, **req)[0]
            return toks, time.perf_counter() - t0, m.speculation_stats()

        timed(2)
        _, t_first, _ = timed(1)
        for name, hint in (("default_drafter", None), ("full_acceptance_hint", True)):
            if hint:
                hint = timed(a.new_tokens)[0]
            toks, t, st = timed(a.new_tokens, hint)
            steps = max(st["steps"], 1)
            tok_s = (len(toks) - 1) / max(t - t_first, 1e-9)
            out[name] = {"tokens": len(toks), "steps": st["steps"], "chain_steps": st["chain_steps"], "drafted": st["drafted"], "accepted": st["accepted"],
                         "tokens_per_step": round((len(toks) - 1) / steps, 3), "tok_s": round(tok_s, 1), "vs_one_row_stochastic": round(tok_s / out["one_row_stochastic_tok_s"], 3),
                         "acceptance": round(st["accepted"] / max(st["drafted"], 1), 3)}
        m.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
