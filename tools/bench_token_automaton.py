"""What the token automaton's step costs per decode token on the full-size model (profiles/r15_token_automaton.md): the one-row decode-ahead GemmaModel.generate(),
greedy and stochastic, for a biased request, the same request constrained by an automaton (the effective table composed over the same bias table) and an automaton
alone, alternated inside one process, three passes.  Beside them, from chains of launches replayed from a graph (tools/bench_fixed_cost.py: time_chain): the fixed cost
of one dependent launch (advance_position, one thread) and the step kernel itself at the model's vocabulary.
usage: python tools/bench_token_automaton.py [bf16 fp8 fp4]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fixed_cost import time_chain  # noqa: E402
from mila_amd import capi, host  # noqa: E402

CONTEXT, PROMPT, NEW, PASSES, V = 4096, 2048, 128, 3, 262144
S, C_ = 300, 7
rng = np.random.default_rng(0)
prompt = rng.integers(2, V, PROMPT).tolist()
UNUSED = [V - 1]
# the bias of r14's "on" setting: 4096 finite values of both signs and 64 bans
ids = rng.choice(V - 1, size=4096 + 64, replace=False)
BIAS = dict(logit_bias={int(i): float(v) for i, v in zip(ids[:4096], rng.standard_normal(4096) * 2.0)}, banned_tokens=[int(i) for i in ids[4096:]])
STOCHASTIC = dict(temperature=0.8, top_k=64, top_p=0.95, seed=1)
# 300 states over 7 classes, a third of the transitions forbidden, no state without an allowed class; the banned ids are spread over all classes, so no dead end
class_of = rng.integers(0, C_, size=V).astype(np.uint16)
nxt = rng.integers(0, S, size=(S, C_)).astype(np.uint16)
nxt[rng.random((S, C_)) < 0.33] = 0xFFFF
for s in range(S):
    if (nxt[s] == 0xFFFF).all():
        nxt[s, s % C_] = (s + 1) % S
AUTOMATON = host.TokenAutomaton(class_of, nxt)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def fmt(xs):
    return " / ".join("%.4f" % x for x in xs)


def kernel_chains():
    """us per launch inside a replayed chain of 64: the one-thread launch, and the step kernel over a bias table at the model's vocabulary"""
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    fixed = time_chain(lambda i: capi.call("advance_position", pos))
    cls_dev = torch.from_numpy(class_of.view(np.int16)).cuda()
    nxt_dev = torch.from_numpy(nxt.view(np.int16)).cuda()
    base = torch.randn(V, device="cuda")
    eff = torch.empty(V, device="cuda")
    state, ticket, tok = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
    tok.fill_(17)
    step = time_chain(lambda i: capi.token_automaton_step(eff, base, cls_dev, nxt_dev, state, tok, ticket))
    step_nobase = time_chain(lambda i: capi.token_automaton_step(eff, None, cls_dev, nxt_dev, state, tok, ticket))
    print("chains of 64 launches replayed from a graph, us per launch: advance_position (one thread) %.2f | token_automaton_step over a bias table %.2f | without a base %.2f"
          % (fixed, step, step_nobase), flush=True)


for policy in sys.argv[1:] or ["bf16"]:
    kernel_chains()
    m = host.GemmaModel.synthetic(policy, None, context=CONTEXT, prefill_chunk=2048, seed=1234)
    m.generate(prompt, max_new_tokens=8, stop_tokens=UNUSED)

    def per_token(**kw):
        """ms per token of the decode-ahead loop: the difference of two lengths on a fully reused prompt (prefill, uploads, validation and first sample cancel)"""
        def timed(n):
            t = time.perf_counter()
            out = m.generate(prompt, max_new_tokens=n, stop_tokens=UNUSED, **kw)[0]
            assert len(out) == n
            return time.perf_counter() - t
        timed(9)                                  # untimed: the capture for this setting
        a, b = timed(NEW // 2 + 1), timed(NEW + 1)
        return (b - a) * 1e3 / (NEW // 2)

    settings = (("greedy bias", BIAS), ("greedy bias + automaton", dict(BIAS, automaton=AUTOMATON)), ("greedy automaton", dict(automaton=AUTOMATON)),
                ("stochastic bias", dict(STOCHASTIC, **BIAS)), ("stochastic bias + automaton", dict(STOCHASTIC, automaton=AUTOMATON, **BIAS)),
                ("stochastic automaton", dict(STOCHASTIC, automaton=AUTOMATON)))
    runs = {}
    for p in range(PASSES):
        for name, kw in settings:
            runs.setdefault(name, []).append(per_token(**kw))
    for kind in ("greedy", "stochastic"):
        off = runs[kind + " bias"]
        print("%s one-row %s generate(), ms per token: bias %s (median %.4f, spread %.1f us)" % (policy, kind, fmt(off), med(off), (max(off) - min(off)) * 1e3), flush=True)
        for name in (" bias + automaton", " automaton"):
            on = runs[kind + name]
            print("    %s%s %s (median %.4f) | %+.1f us against bias" % (kind, name, fmt(on), med(on), (med(on) - med(off)) * 1e3), flush=True)
    m.close()
