"""Writes tests/golden/generate_batch_stochastic.json: tokens and finish reasons of stochastic GemmaModel.generate_batch for fixed prompts, seeds and parameters.

The committed file was recorded with this script on the commit BEFORE the stochastic sampler moved into the rows graph, where every active row was sampled by a
one-row radix call of its own after each replay.  tests/test_gemma_rows_sampling_gpu.py asserts that the in-graph sampler gives exactly these tokens.

    python tests/golden/record_generate_batch_stochastic.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONTEXT = 24
SEED = 7
SETTINGS = [dict(temperature=0.9, top_k=12, top_p=0.9), dict(temperature=1.0, top_k=64, top_p=0.95), dict(temperature=1.3, top_k=0, top_p=1.0)]


def cases():
    from test_gemma_rows_gpu import NEW_PROMPT, PROMPTS
    long = (PROMPTS[2] + NEW_PROMPT + [7])[:21]            # hits the context limit of 24
    out = []
    for policy in ("bf16", "fp8", "fp4"):
        for i, s in enumerate(SETTINGS):
            out.append(dict(policy=policy, prompts=[PROMPTS[0], PROMPTS[1], NEW_PROMPT], seed=31 + i, max_new_tokens=8, stop_tokens=[1], **s))
        out.append(dict(policy=policy, prompts=[PROMPTS[0], PROMPTS[1], long, NEW_PROMPT], seed=40, max_new_tokens=6, stop_tokens=None, **SETTINGS[0]))      # stop: chosen below
        out.append(dict(policy=policy, prompts=[PROMPTS[1], PROMPTS[0]], seed=77, max_new_tokens=10, stop_tokens=[1], **SETTINGS[1]))
        out.append(dict(policy=policy, prompts=[PROMPTS[1]], seed=5, max_new_tokens=7, stop_tokens=[1], **SETTINGS[0]))
    return out


def run(model, case):
    kw = {k: case[k] for k in ("max_new_tokens", "stop_tokens", "temperature", "top_k", "top_p", "seed")}
    return [[toks, status] for toks, status in model.generate_batch(case["prompts"], **kw)]


def main(path):
    from mila_amd import host
    from test_gemma_host_gpu import SMALL
    models, recorded = {}, []
    try:
        for case in cases():
            if case["policy"] not in models:
                models[case["policy"]] = host.GemmaModel.synthetic(case["policy"], SMALL, context=CONTEXT, prefill_chunk=16, seed=SEED, max_batch=4)
            m = models[case["policy"]]
            if case["stop_tokens"] is None:
                # the third token row 0 emits in the free run ends that row: rows retire at different steps of one batch
                free = run(m, dict(case, stop_tokens=[1]))
                case["stop_tokens"] = [free[0][0][2]]
            case["want"] = run(m, case)
            recorded.append(case)
    finally:
        for m in models.values():
            m.close()
    with open(path, "w") as f:
        json.dump(dict(context=CONTEXT, model_seed=SEED, geometry="SMALL", cases=recorded), f, indent=1)
        f.write("\n")
    print("wrote %d cases to %s" % (len(recorded), path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "generate_batch_stochastic.json"))
