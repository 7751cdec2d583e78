"""Parity fixtures of the decode-attention plan (csrc/attention.hip: DecodePlan), recorded from a build one trusts -- the commit BEFORE an edit of the plan rules --
and asserted by tests/test_attn_decode_plan_cpu.py and tests/test_attention_gpu.py against the build under test.  Needs only entry points whose signatures never
changed, plus the tuning / last_form hooks of csrc/internal.h.

  python tools/attn_decode_plan_fixtures.py queries [out.json]   no GPU: attn_decode_split_count over the SWEEP and attn_decode_scratch_bytes over its (B, NH, HS),
                                                                 at the defaults and under each of TUNINGS -> tests/golden/attn_decode_plan_queries.json
  python tools/attn_decode_plan_fixtures.py bits [out.json]      on a GPU: attn_decode_bf16, fused_attn_decode_bf16 (B > 1: fused_attn_decode_batch_bf16) and
                                                                 mha_decode_bf16 on seeded inputs, per case mila_cdna4_last_form, the sha256 of the output bits and the sha256 of
                                                                 the scratch (zeroed before the call: the split partials, so the split count), at the
                                                                 defaults and under each case's own tunings -> tests/golden/attn_decode_plan_bits.json

queries layout: {"sweep": {axis: values}, "default": {"splits": [...], "scratch": [...]}, "tuned": {"name=value": {the same | "same"}}}: `splits` in sweep_cases()
order, `scratch` in scratch_cases() order.  split_count is called with a trailing len_hint of 0 (the capacity): a build from before that argument ignores it.
bits layout: {"setting": {"NH,NKV,HS,capacity,window,position,B": {entry: [forms, sha256 of Y, sha256 of the scratch]}}}; an entry that does not serve a case (the fused form at a head size
other than 64, 128, 256 or 512, MHA on a windowed case or on the 16-on-1 long-context geometry) is left out.  mha_decode_bf16 runs NH heads of HS on a cache of its own."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

os.environ.setdefault("MILA_CDNA4_TUNING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mila_amd import capi  # noqa: E402

SWEEP = {"B": [1, 2, 4], "heads": [[8, 8], [8, 2], [16, 8], [16, 1], [32, 1], [12, 12]], "HS": [64, 128, 256, 512, 96],
         "capacity": [64, 512, 4096, 4097, 8192, 8300, 12000, 32768], "window": [0, 128, 1024]}
TUNINGS = [("attn.positions_per_split", 16), ("attn.positions_per_split", 128), ("attn.max_workgroups", 64), ("attn.max_workgroups", 512),
           ("attn.heads_per_group_512", 4), ("attn.mfma_decode", 0), ("attn.mfma_min_band", 4096)]

# bits mode: (geometries (NH, NKV, HS), capacity, windows, positions, batch sizes, settings)
BIT_GROUPS = [
    ([(8, 2, 64), (8, 2, 128), (8, 8, 256), (4, 2, 512), (6, 6, 96)], 512, [0, 128], [0, 63, 64, 300, 511], [1, 2], ["default"]),       # the scalar kernel (96: generic)
    ([(4, 1, 256)], 8300, [0], [4095, 4096], [1], ["default", "attn.positions_per_split=128"]),                                       # either side of a bucket edge
    ([(16, 1, 512)], 8300, [0], [4095, 4096, 8299], [1], ["default"]),                                                                 # the matrix-core decode
]


def sweep_cases(sweep=SWEEP):
    return [(B, NH, NKV, HS, cap, w) for B, (NH, NKV), HS, cap, w in itertools.product(sweep["B"], sweep["heads"], sweep["HS"], sweep["capacity"], sweep["window"])]


def scratch_cases(sweep=SWEEP):
    return [(B, NH, HS) for B, NH, HS in itertools.product(sweep["B"], sorted({h[0] for h in sweep["heads"]}), sweep["HS"])]


def apply_setting(setting):
    capi.tune_reset()
    if setting != "default":
        name, value = setting.split("=")
        capi.tune(name, int(value))


def record_queries():
    lib = capi.load()
    data = {"sweep": SWEEP, "tuned": {}}
    for setting in ["default"] + ["%s=%d" % t for t in TUNINGS]:
        apply_setting(setting)
        got = {"splits": [int(lib.mila_cdna4_attn_decode_split_count(*c, 0)) for c in sweep_cases()],
               "scratch": [int(lib.mila_cdna4_attn_decode_scratch_bytes(*c)) for c in scratch_cases()]}
        if setting == "default":
            data["default"] = got
        else:
            data["tuned"][setting] = {k: ("same" if v == data["default"][k] else v) for k, v in got.items()}
    capi.tune_reset()
    return data


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------------------------
def bit_cases():
    """[(setting, (NH, NKV, HS, capacity, window, position, B))], grouped by geometry so that run_bit_case's inputs are built once per geometry"""
    out = []
    for geoms, cap, windows, positions, batches, settings in BIT_GROUPS:
        for (NH, NKV, HS), setting, w, pos, B in itertools.product(geoms, settings, windows, positions, batches):
            out.append((setting, (NH, NKV, HS, cap, w, pos, B)))
    return out


def case_key(case):
    return ",".join(str(v) for v in case)


_inputs = {}


def _geometry_inputs(NH, NKV, HS, cap, B):
    """seeded device inputs of one geometry (kept for the next case of the same geometry only): bf16 values by truncation of uniform floats"""
    import numpy as np
    import torch
    key = (NH, NKV, HS, cap, B)
    if key not in _inputs:
        _inputs.clear()
        rng = np.random.default_rng(NH * 1000003 + NKV * 10007 + HS * 101 + cap)

        def bf(shape, scale=1.0):
            f = rng.uniform(-1, 1, shape).astype(np.float32) * np.float32(scale)
            return torch.from_numpy((f.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).cuda()
        d = {"K": bf((B, NKV, cap, HS), 0.5), "V": bf((B, NKV, cap, HS)), "Q": bf((B, NH * HS)), "raw": bf((B, (NH + 2 * NKV) * HS), 2.0)}
        d["qw"], d["kw"] = bf((HS,)), bf((HS,))
        if HS in (64, 128, 256, 512):
            d["cos"] = torch.empty((cap, HS // 2), dtype=torch.float32, device="cuda")
            d["sin"] = torch.empty_like(d["cos"])
            capi.call("rope_build_cache", d["cos"], d["sin"], cap, HS, 1e4, 0)
        if NH // NKV < 16:
            d["mK"], d["mV"], d["QKV"] = bf((B, NH, cap, HS), 0.5), bf((B, NH, cap, HS)), bf((B, 3 * NH * HS))
        nbytes = int(capi.load().mila_cdna4_attn_decode_scratch_bytes(B, NH, HS))
        d["nbytes"], d["scratch"] = nbytes, torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        _inputs[key] = d
    return _inputs[key]


def run_bit_case(case):
    """{entry: [forms, sha256 of the output bits, sha256 of the scratch]} of one case under the current tuning"""
    import torch
    NH, NKV, HS, cap, window, pos, B = case
    with_mha = window == 0 and NH // NKV < 16
    d = _geometry_inputs(NH, NKV, HS, cap, max(B for g in BIT_GROUPS if g[1] == cap for B in g[4]))
    nb, scratch = C.c_size_t(d["nbytes"]), d["scratch"]

    def fresh():
        scratch.zero_()
        capi.last_form()
        return torch.full((B, NH * HS), 0x7fc0, dtype=torch.int16, device="cuda")

    def done(Y):
        torch.cuda.synchronize()
        return ["+".join(capi.last_form())] + [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (Y, scratch)]
    out = {}
    Y = fresh()
    capi.call("attn_decode_bf16", Y, d["Q"][:B], d["K"][:B], d["V"][:B], scratch, nb, B, NH, NKV, HS, cap, pos + 1, window, 1.0)
    out["attn_decode_bf16"] = done(Y)
    if HS in (64, 128, 256, 512):
        Y = fresh()
        K, V, raw = d["K"][:B].clone(), d["V"][:B].clone(), d["raw"]
        q_raw, k_raw, v_raw = raw[0], raw[0, NH * HS:], raw[0, (NH + NKV) * HS:]
        if B == 1:
            capi.call("fused_attn_decode_bf16", Y, K, V, q_raw, k_raw, v_raw, d["qw"], d["kw"], None, d["cos"], d["sin"], scratch, nb, NH, NKV, HS, cap, pos, None,
                      window, 1.0, 1e-6)
            out["fused_attn_decode_bf16"] = done(Y)
        else:
            capi.call("fused_attn_decode_batch_bf16", Y, K, V, q_raw, k_raw, v_raw, C.c_int64(raw.shape[1]), d["qw"], d["kw"], None, d["cos"], d["sin"], scratch, nb,
                      B, NH, NKV, HS, cap, pos, None, window, 1.0, 1e-6)
            out["fused_attn_decode_batch_bf16"] = done(Y)
    if with_mha:
        Y = fresh()
        capi.call("mha_decode_bf16", Y, d["QKV"][:B], d["mK"][:B].clone(), d["mV"][:B].clone(), scratch, nb, B, NH * HS, NH, cap, pos)
        out["mha_decode_bf16"] = done(Y)
    return out


def record_bits():
    data = {}
    for setting, case in bit_cases():
        apply_setting(setting)
        data.setdefault(setting, {})[case_key(case)] = run_bit_case(case)
    capi.tune_reset()
    return data


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode not in ("queries", "bits"):
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "attn_decode_plan_%s.json" % mode)
    data = record_queries() if mode == "queries" else record_bits()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(data, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
