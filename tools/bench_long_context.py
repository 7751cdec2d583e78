"""The reference's published regime beside the headline (Mila/Docs/Discussions/DecodePerformanceCampaign.md:113-117, CHANGELOG.md:235-236:
decode at a 32K-token context, a 22.5K-token chunked prefill): three policies, chunked prefill through the KV caches (bounded ring on the sliding-window layers
optional), then graph-replayed decode at the end of the context.
    python tools/bench_long_context.py [--context 32768] [--prefill-tokens 22528] [--policies bf16,fp8,fp4] [--bounded 0|1] [--kv-fp8]
--kv-fp8: the FP8 KV cache (PerChannelKvFp8<>, GemmaConfig::kv_fp8) on every layer; the resident KV bytes are reported either way."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mila_amd import host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--context", type=int, default=32768)
ap.add_argument("--prefill-tokens", type=int, default=22528)
ap.add_argument("--chunk", type=int, default=2048)
ap.add_argument("--policies", default="bf16,fp8,fp4")
ap.add_argument("--bounded", type=int, default=0)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--kv-fp8", action="store_true")
a = ap.parse_args()
HBM = 8000.0
out = {}
for pol in a.policies.split(","):
    cfg = dict(host.GEMMA4_12B, bounded_local_kv=a.bounded)
    m = host.Gemma(pol, cfg, max_seq=a.context + a.steps + 16, max_prefill=a.chunk, seed=1234, kv_fp8=a.kv_fp8)
    r = {}
    cap = a.context + a.steps + 16
    local_cap = min(cap, cfg["window"] + a.chunk - 1) if a.bounded else cap
    kv = 0
    for i in range(cfg["num_layers"]):
        g = (i + 1) % cfg["sliding_window_pattern"] == 0
        hs, nkv, rows = (cfg["global_head_dim"], cfg["num_global_kv_heads"], cap) if g else (cfg["head_dim"], cfg["num_kv_heads"], local_cap)
        kv += 2 * nkv * rows * ((hs + 4) if a.kv_fp8 else 2 * hs)
    r["resident_kv_GB"] = round(kv / 1e9, 3)
    ms = m.time_prefill_chunked(a.prefill_tokens)
    r["chunked_prefill_%d_ms" % a.prefill_tokens] = round(ms, 2)
    r["chunked_prefill_tok_s"] = round(a.prefill_tokens / ms * 1e3, 1)
    ms = m.time_prefill_chunked(a.context)                      # fills the caches to the context length
    r["chunked_prefill_%d_ms" % a.context] = round(ms, 2)
    info = m.info(a.context)
    t = m.time_decode(a.context, a.steps, 8, "graph")
    r["decode_ms_per_token"] = round(t["wall_ms_per_step"], 4)
    r["decode_tok_s"] = round(1e3 / t["wall_ms_per_step"], 2)
    r["bytes_per_token_GB"] = round(info["decode_bytes_per_token"] / 1e9, 3)
    r["whole_token_frac_of_8TBps"] = round(info["decode_bytes_per_token"] / (t["wall_ms_per_step"] * 1e-3) / 1e9 / HBM, 4)
    out[pol] = r
    print(pol, json.dumps(r), flush=True)
    m.close()
print(json.dumps({"context": a.context, "prefill_tokens": a.prefill_tokens, "chunk": a.chunk, "bounded_local_kv": a.bounded, "kv_fp8": int(a.kv_fp8), "policies": out}))
