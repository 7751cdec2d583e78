"""What row requests cost per four-row decode step on the full-size model (profiles/r17_row_requests.md): the shared-parameter rows graph (greedy, and stochastic at
Gemma's sampling defaults) against the requests step with four identical stochastic requests, with two greedy and two stochastic rows, and with four automata, every
setting alternated inside one process, PASSES passes, device ms per step at context 2048.
usage: python tools/bench_row_requests.py [--baseline-only] [--package-root DIR] [bf16 fp8 fp4]
--baseline-only: the shared-parameter settings alone (they need nothing this feature added, so the same file times an older build); --package-root: where mila_amd is."""
import json
import os
import sys

args = sys.argv[1:]
baseline_only = "--baseline-only" in args
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package-root" in args:
    root = os.path.abspath(args[args.index("--package-root") + 1])
    del args[args.index("--package-root"):args.index("--package-root") + 2]
policies = [a for a in args if not a.startswith("--")] or ["bf16"]
sys.path.insert(0, root)
import numpy as np  # noqa: E402

from mila_amd import host  # noqa: E402

MAX_SEQ, CONTEXT, STEPS, WARMUP, PASSES, V = 4096, 2048, 64, 8, 5, 262144
DEFAULTS = (1.0, 64, 0.95)      # Gemma's sampling defaults
DRAWS = [0.11, 0.42, 0.63, 0.94]
STOCHASTIC = dict(temperature=DEFAULTS[0], top_k=DEFAULTS[1], top_p=DEFAULTS[2])


def automaton(seed):
    """300 states over 7 classes, a third of the transitions forbidden, no state without an allowed class (the image of profiles/r15_token_automaton.md)"""
    rng = np.random.default_rng(seed)
    class_of = rng.integers(0, 7, size=V).astype(np.uint16)
    nxt = rng.integers(0, 300, size=(300, 7)).astype(np.uint16)
    nxt[rng.random((300, 7)) < 1.0 / 3.0] = host.TokenAutomaton.FORBIDDEN
    for s in range(300):
        if (nxt[s] == host.TokenAutomaton.FORBIDDEN).all():
            nxt[s, rng.integers(7)] = rng.integers(300)
    return host.TokenAutomaton(class_of, nxt)


for policy in policies:
    g = host.Gemma(policy, None, max_seq=MAX_SEQ, max_prefill=1, seed=1234, max_batch=4)

    def shared_greedy():
        g.set_step_sampling("rows", None)
        return True

    def shared_stochastic():
        g.set_step_sampling("rows", DEFAULTS, DRAWS)
        return False

    settings = {"shared greedy": shared_greedy, "shared stochastic": shared_stochastic}
    if not baseline_only:
        def requests(rows, automata=False):
            def install():
                for b in range(4):
                    g.set_row_token_automaton(b, automaton(b) if automata else None)
                g.set_rows_requests(rows, DRAWS)
                return False
            return install

        def clear(fn):
            def run():
                g.set_rows_requests(None)
                return fn()
            return run

        settings = {k: clear(v) for k, v in settings.items()}
        settings["requests: 4 stochastic"] = requests([STOCHASTIC] * 4)
        settings["requests: 2 greedy + 2 stochastic"] = requests([dict(temperature=0.0), STOCHASTIC, dict(temperature=0.0), STOCHASTIC])
        settings["requests: 4 greedy"] = requests([dict(temperature=0.0)] * 4)
        settings["requests: 4 stochastic + 4 automata"] = requests([STOCHASTIC] * 4, automata=True)
    ms = {k: [] for k in settings}
    nodes = {}
    for _ in range(PASSES):
        for name, install in settings.items():
            greedy = install()
            ms[name].append(g.time_decode_rows(4, CONTEXT, steps=STEPS, warmup=WARMUP, greedy=greedy)["device_ms_per_step"])
            nodes[name] = g.rows_graph_info()["nodes"]
    for name in settings:
        xs = sorted(ms[name])
        print(json.dumps({"policy": policy, "setting": name, "device_ms_per_step": [round(v, 4) for v in ms[name]], "median": round(xs[len(xs) // 2], 4),
                          "spread_us": round((xs[-1] - xs[0]) * 1e3, 1), "nodes": nodes[name], "context": CONTEXT, "steps": STEPS, "root": os.path.basename(root)}), flush=True)
    g.close()
