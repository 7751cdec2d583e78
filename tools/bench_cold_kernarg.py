"""What a launch pays for a COLD kernel-argument fetch: a graph of 64 dependent near-empty matvec launches (K 4096, N 256, one weight matrix per node), replayed
hot (back to back) and cold (an untimed read-only pass over 1 GiB between replays, so that the nodes' kernarg slots -- and everything else -- have left every cache),
events around each replay, microseconds per launch.  Sibling of bench_fixed_cost.py, whose chains are always hot.  Not part of the product path.

Two or more BUILDS of the library in one process on one box, interleaved (tools/experiments/ab_prev_lib.py does the same for GEMMs):
    python tools/bench_cold_kernarg.py preload=mila_amd/lib/libmila_cdna4.so plain=tools/experiments/_build/plain/libmila_cdna4.so
prints one JSON line per (build, mode) and a last line with the cold differences against the first build."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, NODES, PASSES, REPS = 4096, 256, 64, 6, 12
FLUSH_BYTES = 1 << 30


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def main():
    specs = sys.argv[1:] or ["current=mila_amd/lib/libmila_cdna4.so"]
    libs = {}
    for s in specs:
        name, path = s.split("=", 1)
        libs[name] = C.CDLL(os.path.join(ROOT, path) if not os.path.isabs(path) else path)
    first = next(iter(libs.values()))
    Ws = [torch.randint(-30000, 30000, (N, K), dtype=torch.int16, device="cuda") for _ in range(NODES)]
    x = torch.randn(K, device="cuda").to(torch.bfloat16).view(torch.int16)
    y = torch.empty(N, dtype=torch.int16, device="cuda")
    flush_src = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device="cuda")
    sink = torch.zeros(4096, dtype=torch.float32, device="cuda")

    graphs = {}
    for name, lib in libs.items():
        def launch(i, lib=lib):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert lib.mila_cdna4_matvec_bf16(P(y), P(x), P(Ws[i]), None, K, N, st) == 0
        for _ in range(3):
            launch(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(NODES):
                launch(i)
        g.replay()
        torch.cuda.synchronize()
        graphs[name] = g

    def flush():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert first.mila_cdna4_stream_read(P(sink), P(flush_src), C.c_size_t(FLUSH_BYTES), st) == 0

    def replay_us(g, cold):
        out = []
        for _ in range(REPS):
            if cold:
                flush()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / NODES)
        return out

    samples = {(n, m): [] for n in libs for m in ("hot", "cold")}      # per pass: the median of REPS replays
    names = list(libs)
    for rnd in range(PASSES):
        for name in (names if rnd % 2 == 0 else names[::-1]):
            for mode in ("hot", "cold"):
                replay_us(graphs[name], mode == "cold")[:2]             # settle after the switch of graph / mode
                samples[(name, mode)].append(statistics.median(replay_us(graphs[name], mode == "cold")))
    res = {}
    for (name, mode), v in samples.items():
        res[(name, mode)] = statistics.median(v)
        print(json.dumps({"build": name, "mode": mode, "us_per_launch_median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                          "passes": [round(t, 3) for t in v]}), flush=True)
    base = names[0]
    for other in names[1:]:
        print(json.dumps({"cold_us_per_launch": {base: round(res[(base, "cold")], 3), other: round(res[(other, "cold")], 3)},
                          "difference_us": round(res[(other, "cold")] - res[(base, "cold")], 3),
                          "spread_of_repeats_us": round(max(max(samples[(n, "cold")]) - min(samples[(n, "cold")]) for n in (base, other)), 3)}), flush=True)


if __name__ == "__main__":
    main()
