"""Parity fixtures of the prefill GEMM dispatch (csrc/gemm_plan.hip), recorded from a build one trusts -- the commit BEFORE an edit of the plan rules -- and
asserted by tests/test_gemm_plan_cpu.py against the build under test.  Needs only the exported ABI and the tuning / last_form hooks of csrc/internal.h.

  python tools/gemm_plan_fixtures.py queries [out.json]     no GPU: the six size / applicability queries over SHAPES x ROWS, at the defaults and under each of TUNINGS
                                                            -> tests/golden/gemm_plan_queries.json
  python tools/gemm_plan_fixtures.py forms [out.json]       on a GPU: the six entry points on zero-filled operands, mila_cdna4_last_form of every call, at the defaults
                                                            and under each of FORM_TUNINGS -> tests/golden/gemm_plan_forms.json

Layout of both files: {"rows": ROWS, "default": {"K,N": {name: row}}, "tuned": {"name=value": {"K,N": {name: row | "same"}}}} -- "same": the tuned row equals the
default one.  A query row is the list of values in ROWS order (0 / 1 answers as one string of digits); a forms row is {"form+form": [M, ...]} with the calls the
entry does not serve (gemm_geglu_* outside its applicable shapes, an odd N for F = N / 2) left out.  The GeGLU entries take the (K, N) of the [gate | up] weight: F = N / 2."""
import ctypes as C
import json
import os
import sys

os.environ.setdefault("MILA_CDNA4_TUNING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mila_amd import capi  # noqa: E402

SHAPES = [(3840, 8192), (3840, 8704), (4096, 3840), (8192, 3840), (3840, 30720), (15360, 3840),      # Gemma 4
          (768, 2304), (768, 768), (768, 3072), (3072, 768), (768, 50257),                           # GPT-2
          (1280, 5120), (2560, 5120), (192, 250), (384, 3840)]                                       # odd shapes of the test suite
ROWS = [1, 2, 16, 17, 32, 33, 64, 65, 255, 256, 257, 300, 511, 512, 513, 576, 1000, 1041, 2047, 2048, 2049, 2112, 2113, 2303, 2304, 4095, 4096, 8192]
TUNINGS = [("gemm.splitk", 0), ("gemm.colsplit", 0), ("gemm.bf16_skinny", 0), ("gemm.fewrow", 0), ("gemm.force128", 1), ("gemm.schedule", 2), ("gemm.schedule", 3),
           ("gemm_fp8.big_rule", 0), ("gemm_fp8.big_rule", 1), ("gemm_fp8.big_rule", 2), ("gemm_fp8.tail_form", 1), ("gemm.ldsdma_loose_tiles", 0),
           ("gemm.skinny_ahead_rows", 16), ("gemm.splitk_min_rows", 17)]
FORM_TUNINGS = [("gemm.schedule", 2), ("gemm_fp8.tail_form", 1), ("gemm_fp8.tail_form", 2), ("gemm_fp8.big_rule", 0)]
QUERIES = ["gemm_workspace_bytes", "gemm_fp8_workspace_bytes", "gemm_staging_bytes", "gemm_geglu_applicable", "gemm_geglu_preferred", "gemm_geglu_w4a8_applicable"]
ENTRIES = ["gemm_bf16", "gemm_bf16_ws", "gemm_geglu_bf16", "gemm_fp8_scaled", "gemm_fp8_scaled_ws", "gemm_geglu_fp8_scaled"]


def query_rows(K, N):
    """{query: row} of one shape; the three GeGLU answers are about F = N / 2 (0 for an odd N)"""
    lib = capi.load()
    out = {}
    for q in QUERIES:
        fn = getattr(lib, "mila_cdna4_" + q)
        if "geglu" in q:
            out[q] = "".join(str(int(fn(M, K, N // 2)) if N % 2 == 0 else 0) for M in ROWS)
        else:
            out[q] = [int(fn(M, K, N)) for M in ROWS]
    return out


def form_rows(K, N, buf):
    """{entry: {forms: [M, ...]}} of one shape: every entry on zero-filled operands"""
    lib = capi.load()
    Y, X, W, xs, ws1, ws = buf
    out = {e: {} for e in ENTRIES}
    for M in ROWS:
        F = N // 2
        wsb = int(lib.mila_cdna4_gemm_workspace_bytes(M, K, N))
        wsf = int(lib.mila_cdna4_gemm_fp8_workspace_bytes(M, K, N))
        assert max(wsb, wsf) <= ws.numel(), "workspace buffer too small: %d" % max(wsb, wsf)
        calls = [("gemm_bf16", (Y, X, W, None, M, K, N)),
                 ("gemm_bf16_ws", (Y, X, W, None, M, K, N, 0, ws, C.c_size_t(wsb))),
                 ("gemm_fp8_scaled", (Y, X, W, xs, ws1, None, M, K, N)),
                 ("gemm_fp8_scaled_ws", (Y, X, W, xs, ws1, None, M, K, N, ws, C.c_size_t(wsf)))]
        if N % 2 == 0 and lib.mila_cdna4_gemm_geglu_applicable(M, K, F):
            calls.append(("gemm_geglu_bf16", (Y, X, W, M, K, F)))
        if N % 2 == 0 and lib.mila_cdna4_gemm_geglu_w4a8_applicable(M, K, F):
            calls.append(("gemm_geglu_fp8_scaled", (Y, X, W, xs, ws1, M, K, F)))
        for name, args in calls:
            capi.last_form()
            capi.call(name, *args)
            out[name].setdefault("+".join(capi.last_form()), []).append(M)
    return out


def sweep(tunings, one_shape):
    data = {"rows": ROWS, "default": {}, "tuned": {}}
    capi.tune_reset()
    for K, N in SHAPES:
        data["default"]["%d,%d" % (K, N)] = one_shape(K, N)
    for name, value in tunings:
        capi.tune_reset()
        capi.tune(name, value)
        t = data["tuned"]["%s=%d" % (name, value)] = {}
        for K, N in SHAPES:
            base, got = data["default"]["%d,%d" % (K, N)], one_shape(K, N)
            t["%d,%d" % (K, N)] = {k: ("same" if v == base[k] else v) for k, v in got.items()}
    capi.tune_reset()
    return data


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "queries":
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "gemm_plan_queries.json")
        data = sweep(TUNINGS, query_rows)
    elif mode == "forms":
        import torch
        out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "gemm_plan_forms.json")
        mx, mk, mn = max(ROWS), max(k for k, _ in SHAPES), max(n for _, n in SHAPES)
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")      # noqa: E731
        buf = (z(2 * mx * mn), z(2 * mx * mk), z(2 * max(k * n for k, n in SHAPES)), z(4 * mx), z(16), z(64 << 20))

        def one_shape(K, N):
            rows = form_rows(K, N, buf)
            torch.cuda.synchronize()
            return rows
        data = sweep(FORM_TUNINGS, one_shape)
    else:
        sys.exit(__doc__)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(data, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
