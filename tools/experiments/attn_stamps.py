"""Launch -> first K/V request and launch -> first score of the fused decode-attention kernel, in shader cycles, from diagnostic libraries built by attn_stamps.sh
(lane 0 of workgroup (0, 0, 0) stamps its first instruction, the issue of its first K/V row loads and the first score of its first group): Gemma's sliding-window and global layer shapes at position 2100, position read from device memory, hot
(launches back to back) and cold (an untimed 1 GiB read-only pass before every launch, as the weight stream leaves the caches in a decode step).
    python tools/experiments/attn_stamps.py after=<lib> before=<lib>"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FLUSH_BYTES = 1 << 30


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def main():
    libs = {}
    for s in sys.argv[1:]:
        name, path = s.split("=", 1)
        lib = C.CDLL(path if os.path.isabs(path) else os.path.join(ROOT, path))
        lib.mila_cdna4_attn_decode_scratch_bytes.restype = C.c_size_t
        libs[name] = lib
    flush_src = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device="cuda")
    sink = torch.zeros(4096, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos, cap, max_seq = 2100, 4096, 4096
    for shape, NH, NKV, HS, window in (("sliding-window", 16, 8, 256, 1024), ("global", 16, 1, 512, 0)):
        def bf(*dims):
            return (torch.rand(dims, device="cuda") - 0.5).to(torch.bfloat16).view(torch.int16)
        Kc, Vc = bf(1, NKV, cap, HS), bf(1, NKV, cap, HS)
        q, k, v, qw, kw = bf(NH * HS), bf(NKV * HS), bf(NKV * HS), bf(HS), bf(HS)
        cos, sin = torch.rand((max_seq, HS // 2), device="cuda"), torch.rand((max_seq, HS // 2), device="cuda")
        Y = torch.empty(NH * HS, dtype=torch.int16, device="cuda")
        pd = torch.tensor([pos], dtype=torch.int32, device="cuda")
        for name, lib in libs.items():
            nbytes = lib.mila_cdna4_attn_decode_scratch_bytes(1, NH, HS)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

            def launch():
                rc = lib.mila_cdna4_fused_attn_decode_bf16(P(Y), P(Kc), P(Vc), P(q), P(k), P(v), P(qw), P(kw), None, P(cos), P(sin), P(scratch), C.c_size_t(nbytes), NH, NKV, HS,
                                                           cap, 0, P(pd), window, C.c_float(1.0), C.c_float(1e-6), st)
                assert rc == 0, rc

            def read():
                torch.cuda.synchronize()
                out = (C.c_ulonglong * 3)()
                assert lib.mila_dbg_attn_stamps(out) == 0
                return out[0], out[1], out[2]
            for mode in ("hot", "cold"):
                per_pass, per_pass_score = [], []
                for _ in range(5):
                    for _ in range(3):
                        launch()
                    c0, n0, s0 = read()
                    for _ in range(20):
                        if mode == "cold":
                            assert lib.mila_cdna4_stream_read(P(sink), P(flush_src), C.c_size_t(FLUSH_BYTES), st) == 0
                        launch()
                    c1, n1, s1 = read()
                    per_pass.append((c1 - c0) / (n1 - n0))
                    per_pass_score.append((s1 - s0) / (n1 - n0))
                print(json.dumps({"shape": shape, "build": name, "mode": mode, "cycles_launch_to_first_kv_request": round(sorted(per_pass)[2]),
                                  "cycles_launch_to_first_score": round(sorted(per_pass_score)[2]),
                                  "passes": [round(x) for x in per_pass], "passes_score": [round(x) for x in per_pass_score]}), flush=True)


if __name__ == "__main__":
    main()
