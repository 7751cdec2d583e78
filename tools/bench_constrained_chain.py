"""What constrained speculative decode costs and gains on the full-size model (profiles/r16_constrained_chain.md), context 2048.
(a) the chain step of T = 2 and 4 rows, replayed from its graph: unconstrained, under a bias table, and under an automaton over that table (chain_compose in front, the
    biased tail, chain_step behind), alternated, three passes; beside it the one-row captured step.
(b) GemmaModel.generate() end to end on a draft_tokens = 3 model: an automaton with forced runs (free, forced, forced, forced, repeating) and one without a forced
    state, each with speculate_constrained off and on, greedy and stochastic: ms per token from the difference of two lengths on a fully reused prompt, and the
    speculative loop's counters.
usage: python tools/bench_constrained_chain.py [bf16 fp8 fp4]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mila_amd import host  # noqa: E402

CONTEXT, PROMPT, NEW, PASSES, V = 2048, 1024, 128, 3, 262144
S, C_ = 300, 7
rng = np.random.default_rng(0)
prompt = rng.integers(2, V, PROMPT).tolist()
UNUSED = [V - 1]
ids = rng.choice(V - 1, size=4096 + 64, replace=False)
BIAS = {int(i): float(v) for i, v in zip(ids[:4096], rng.standard_normal(4096) * 2.0)}
BIAS.update({int(i): float("-inf") for i in ids[4096:]})
STOCHASTIC = dict(temperature=0.8, top_k=64, top_p=0.95, seed=1)
# r15's automaton: 300 states over 7 classes, a third of the transitions forbidden, no state without an allowed class -- and no forced state
class_of = rng.integers(0, C_, size=V).astype(np.uint16)
nxt = rng.integers(0, S, size=(S, C_)).astype(np.uint16)
nxt[rng.random((S, C_)) < 0.33] = 0xFFFF
for s in range(S):
    if (nxt[s] != 0xFFFF).sum() < 1:
        nxt[s, s % C_] = (s + 1) % S
UNFORCED = host.TokenAutomaton(class_of, nxt)
# free, forced, forced, forced, repeating
forced_cls = np.zeros(V, dtype=np.uint16)
forced_cls[[40, 500, 77]] = [1, 2, 3]
forced_nxt = np.full((4, 4), 0xFFFF, dtype=np.uint16)
forced_nxt[0, 0] = 1
for i in range(3):
    forced_nxt[i + 1, i + 1] = (i + 2) % 4
FORCED = host.TokenAutomaton(forced_cls, forced_nxt)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def fmt(xs):
    return " / ".join("%.4f" % x for x in xs)


def chain_steps(policy):
    g = host.Gemma(policy, None, max_seq=CONTEXT, max_prefill=1, seed=1234, draft_tokens=3)
    settings = (("unconstrained", lambda: (g.set_token_bias(None), g.set_token_automaton(None))), ("bias", lambda: (g.set_token_bias(BIAS), g.set_token_automaton(None))),
                ("bias + automaton", lambda: (g.set_token_bias(BIAS), g.set_token_automaton(UNFORCED))))
    runs = {}
    for p in range(PASSES):
        for name, setup in settings:
            setup()
            for T in (2, 4):
                runs.setdefault((name, T), []).append(g.time_decode_chain(T, PROMPT, 64, 8)["device_ms_per_step"])
        g.set_token_bias(None)
        g.set_token_automaton(None)
        runs.setdefault(("one row", 1), []).append(g.time_decode(PROMPT, 64, 8)["device_ms_per_step"])
    for (name, T), xs in runs.items():
        print("%s chain step, greedy, device ms per step: %-18s T=%d  %s (median %.4f, spread %.1f us)" % (policy, name, T, fmt(xs), med(xs), (max(xs) - min(xs)) * 1e3), flush=True)
    g.close()


def end_to_end(policy):
    m = host.GemmaModel.synthetic(policy, None, context=CONTEXT, prefill_chunk=1024, seed=1234, draft_tokens=3)
    m.generate(prompt, max_new_tokens=8, stop_tokens=UNUSED)

    def per_token(**kw):
        def timed(n):
            t = time.perf_counter()
            out = m.generate(prompt, max_new_tokens=n, stop_tokens=UNUSED, **kw)[0]
            assert len(out) == n
            return time.perf_counter() - t, m.speculation_stats_forced()
        timed(9)                                  # untimed: the captures for this setting
        (a, _), (b, st) = timed(NEW // 2 + 1), timed(NEW + 1)
        return (b - a) * 1e3 / (NEW // 2), st

    settings = []
    for kind, base in (("greedy", {}), ("stochastic", dict(STOCHASTIC, speculative_sampling=True))):
        for name, a in (("forced runs", FORCED), ("no forced state", UNFORCED)):
            for flag in (False, True):
                settings.append(("%s, %s, flag %s" % (kind, name, "on" if flag else "off"), dict(base, automaton=a, speculate_constrained=flag)))
    runs, stats = {}, {}
    for p in range(PASSES):
        for name, kw in settings:
            ms, st = per_token(**kw)
            runs.setdefault(name, []).append(ms)
            stats[name] = st
    for name, xs in runs.items():
        print("%s generate(): %-44s ms per token %s (median %.4f = %.1f tok/s, spread %.1f us) | 129 tokens: %s" % (
            policy, name, fmt(xs), med(xs), 1e3 / med(xs), (max(xs) - min(xs)) * 1e3, stats[name]), flush=True)
    m.close()


for policy in sys.argv[1:] or ["bf16"]:
    chain_steps(policy)
    end_to_end(policy)
