"""What the request queue buys and costs on the full-size model (profiles/r18_request_queue.md): a queue of 16 greedy requests with 64-token prompts and the
max_new_tokens of MAX_NEW below through GemmaModel.serve_requests, against the same requests through generate_requests in arrival-order groups of four (the path
without a queue), alternated inside one process, PASSES passes after a warm-up each, wall-clock tokens/s with the spread; beside it the step counts the scheduling rule
predicts for both, the host milliseconds of an admission split into setters, prefill and first sample, and one fork against the prefill it replaces at prompt lengths
64 and 2048.
usage: python tools/bench_request_queue.py [--package-root DIR] [bf16 fp8 fp4]"""
import json
import os
import sys
import time

args = sys.argv[1:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package-root" in args:
    root = os.path.abspath(args[args.index("--package-root") + 1])
    del args[args.index("--package-root"):args.index("--package-root") + 2]
policies = [a for a in args if not a.startswith("--")] or ["bf16"]
sys.path.insert(0, root)
import numpy as np  # noqa: E402

from mila_amd import host  # noqa: E402

R, CONTEXT, PROMPT, PASSES = 4, 4096, 64, 5
MAX_NEW = [8, 96, 16, 64, 24, 128, 8, 48, 32, 112, 12, 80, 20, 56, 8, 100]      # the fixed mixed list: 812 tokens
UNUSED = [262143]


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


for policy in policies:
    m = host.GemmaModel.synthetic(policy, None, context=CONTEXT, prefill_chunk=2048, seed=1234, max_batch=R)
    rng = np.random.default_rng(0)
    reqs = [dict(prompt=rng.integers(0, 1000, PROMPT).tolist(), max_new_tokens=n, stop_tokens=UNUSED) for n in MAX_NEW]
    tokens = sum(MAX_NEW)

    def queued():
        t0 = time.perf_counter()
        rows, stats = m.serve_requests(reqs)
        return time.perf_counter() - t0, sum(len(r[0]) for r in rows), stats

    def grouped():
        t0 = time.perf_counter()
        n = 0
        for g in range(0, len(reqs), R):
            n += sum(len(r[0]) for r in m.generate_requests(reqs[g:g + R]))
        return time.perf_counter() - t0, n, None

    queued(), grouped()      # warm-up: graph captures, scratch growth
    rate = {"queue": [], "groups": []}
    stats = None
    for _ in range(PASSES):
        for name, fn in (("queue", queued), ("groups", grouped)):
            dt, n, st = fn()
            assert n == tokens, (name, n)
            rate[name].append(n / dt)
            stats = st or stats
    group_steps = sum(max(MAX_NEW[g:g + R]) - 1 for g in range(0, len(MAX_NEW), R))
    adm = stats["admission_ms"]
    print(json.dumps({"policy": policy, "what": "throughput", "tokens": tokens, "queue_tok_s": spread(rate["queue"]), "groups_tok_s": spread(rate["groups"]),
                      "ratio_of_medians": round(spread(rate["queue"])["median"] / spread(rate["groups"])["median"], 3), "queue_steps": stats["steps"], "group_steps": group_steps,
                      "step_ratio": round(group_steps / stats["steps"], 3), "captures_last_pass": stats["captures"]}), flush=True)
    print(json.dumps({"policy": policy, "what": "admission, host ms per admission (last pass, 16 admissions of a 64-token prompt)",
                      "setters": round(adm["setters"] / 16, 3), "prefill": round(adm["prefill"] / 16, 3), "first_sample": round(adm["first_sample"] / 16, 3)}), flush=True)
    for length in (64, 2048):
        prompt = rng.integers(0, 1000, length).tolist()
        pair = [dict(prompt=prompt, max_new_tokens=2, stop_tokens=UNUSED, n=2)]
        m.serve_requests(pair)
        pf, fk = [], []
        for _ in range(PASSES):
            _, st = m.serve_requests(pair)
            assert (st["prefills"], st["forks"]) == (1, 1), st
            pf.append(st["admission_ms"]["prefill"])
            fk.append(st["admission_ms"]["fork"])
        print(json.dumps({"policy": policy, "what": "one fork against the prefill it replaces, host ms", "prompt": length, "prefill_ms": spread(pf), "fork_ms": spread(fk)}), flush=True)
    m.close()
