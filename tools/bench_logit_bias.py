"""What a bias table costs per decode step on the full-size model (profiles/r14_logit_bias.md): the one-row decode-ahead GemmaModel.generate(), greedy and stochastic, and
the four-row stochastic rows graph, each with the bias off and on, alternated inside one process, three passes; and the wall time of a request with a min_tokens restore
against the same request without one.
usage: python tools/bench_logit_bias.py [bf16 fp8 fp4]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mila_amd import host  # noqa: E402

CONTEXT, PROMPT, NEW, PASSES, V = 4096, 2048, 128, 3, 262144
rng = np.random.default_rng(0)
prompt = rng.integers(2, V, PROMPT).tolist()
UNUSED = [V - 1]
# the bias of the "on" setting: 4096 finite values of both signs and 64 bans -- the table is dense on the device whatever the request lists
ids = rng.choice(V - 1, size=4096 + 64, replace=False)
BIAS = dict(logit_bias={int(i): float(v) for i, v in zip(ids[:4096], rng.standard_normal(4096) * 2.0)}, banned_tokens=[int(i) for i in ids[4096:]])
STOCHASTIC = dict(temperature=0.8, top_k=64, top_p=0.95, seed=1)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def fmt(xs):
    return " / ".join("%.4f" % x for x in xs)


for policy in sys.argv[1:] or ["bf16"]:
    m = host.GemmaModel.synthetic(policy, None, context=CONTEXT, prefill_chunk=2048, seed=1234)
    m.generate(prompt, max_new_tokens=8, stop_tokens=UNUSED)

    def per_token(**kw):
        """ms per token of the decode-ahead loop: the difference of two lengths on a fully reused prompt (prefill, table upload and first sample cancel)"""
        def timed(n):
            t = time.perf_counter()
            out = m.generate(prompt, max_new_tokens=n, stop_tokens=UNUSED, **kw)[0]
            assert len(out) == n
            return time.perf_counter() - t
        timed(9)                                  # untimed: the capture for this setting
        a, b = timed(NEW // 2 + 1), timed(NEW + 1)
        return (b - a) * 1e3 / (NEW // 2)

    runs = {}
    for p in range(PASSES):
        for name, kw in (("greedy off", {}), ("greedy bias", BIAS), ("stochastic off", STOCHASTIC), ("stochastic bias", dict(STOCHASTIC, **BIAS))):
            runs.setdefault(name, []).append(per_token(**kw))
    for kind in ("greedy", "stochastic"):
        off, on = runs[kind + " off"], runs[kind + " bias"]
        print("%s one-row %s generate(), ms per token: off %s (median %.4f) | bias %s (median %.4f) | %+.1f us" % (policy, kind, fmt(off), med(off), fmt(on), med(on),
                                                                                                                (med(on) - med(off)) * 1e3), flush=True)

    # the min_tokens restore: the same biased request with the stop token held back for 32 samples (one staged upload at the start, one small launch before sample 32)
    # against the request that bans it throughout
    def request(**kw):
        t = time.perf_counter()
        out = m.generate(prompt, max_new_tokens=NEW + 1, **kw)[0]
        assert len(out) == NEW + 1
        return (time.perf_counter() - t) * 1e3
    S = 12345
    held, banned = [], []
    for p in range(PASSES + 1):
        b = request(stop_tokens=UNUSED, logit_bias=BIAS["logit_bias"], banned_tokens=BIAS["banned_tokens"] + [S, V - 1])
        h = request(stop_tokens=[S, V - 1], logit_bias=BIAS["logit_bias"], banned_tokens=BIAS["banned_tokens"] + [S], min_tokens=32)
        if p:                                     # (the first pass captures)
            banned.append(b)
            held.append(h)
    print("%s greedy request of %d tokens, wall ms: stop token banned %s (median %.3f) | held back by min_tokens=32, then restored %s (median %.3f) | %+.1f us per request" % (
        policy, NEW + 1, fmt(banned), med(banned), fmt(held), med(held), (med(held) - med(banned)) * 1e3), flush=True)
    m.close()

    g = host.Gemma(policy, None, max_seq=CONTEXT, max_prefill=1, seed=1234, max_batch=4)
    g.set_step_sampling("rows", (0.8, 64, 0.95), [0.11, 0.42, 0.63, 0.94])
    rows = {"off": [], "bias": []}
    for p in range(PASSES):
        for name in ("off", "bias"):
            g.set_token_bias(BIAS["logit_bias"] | {t: float("-inf") for t in BIAS["banned_tokens"]} if name == "bias" else None)
            rows[name].append(g.time_decode_rows(4, 2048, steps=64, warmup=8, greedy=False)["device_ms_per_step"])
    print("%s four-row stochastic rows graph, device ms per step: off %s (median %.4f) | bias (one shared table) %s (median %.4f) | %+.1f us" % (
        policy, fmt(rows["off"]), med(rows["off"]), fmt(rows["bias"]), med(rows["bias"]), (med(rows["bias"]) - med(rows["off"])) * 1e3), flush=True)
    g.close()
