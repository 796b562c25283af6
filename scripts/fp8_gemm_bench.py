"""Kernel time and achieved weight GB/s of the FP8 projection (samd_gemm_skinny_f8) against the fp16 one (samd_gemm_skinny) on the same
shapes: every Vicuna-7B and Llama-3-8B projection at 16 and 64 rows, split-K as the runner chooses (samd_gemm_splits).  Each shape streams
COPIES distinct matrices in turn (> 1 GB together), so that no launch finds its weights in the Infinity Cache -- as in a forward, where
layer l + 1's matrices are hundreds of MB away from layer l's.  Prints one JSON line per (shape, rows) and a summary.

    python scripts/fp8_gemm_bench.py [--reps 20]
Times are per launch from event pairs around a replayed graph of the launches; kernel-only times: run it under `rocprofv3 --kernel-trace --stats -- python scripts/fp8_gemm_bench.py`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam-decoding_amd"))

import torch

from samd_hip import _ptr, check, current_stream, lib
from samd_hip import fp8 as F8

SHAPES = {
    "vicuna-7b": dict(qkv=(12288, 4096), o=(4096, 4096), gate_up=(22016, 4096), down=(4096, 11008)),
    "llama3-8b": dict(qkv=(6144, 4096), o=(4096, 4096), gate_up=(28672, 4096), down=(4096, 14336)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stream-bytes", type=float, default=1.5e9, help="bytes of distinct matrices each measurement cycles through")
    args = ap.parse_args()
    L, st = lib(), current_stream()
    rows_out = []
    for model, projs in SHAPES.items():
        for name, (N, K) in projs.items():
            copies = max(2, int(args.stream_bytes // (2 * N * K)))
            w16, w8 = [], []
            for i in range(copies):
                W = (torch.randn((N, K), device="cuda") * 0.02).half()
                p16 = torch.empty_like(W)
                check(L.samd_gemm_pack_weights(_ptr(W), _ptr(p16), N, K, st))
                q, s = F8.quantize_rows(W)
                p8 = torch.empty((N * K,), dtype=torch.uint8, device="cuda")
                check(L.samd_gemm_pack_f8(_ptr(q), _ptr(p8), N, K, st))
                w16.append(p16)
                w8.append((p8, s))
                del W, q
            for R in (16, 64):
                sp = L.samd_gemm_splits(N, K, R)
                A = torch.randn((R, K), device="cuda").half()
                out = torch.empty((R, N), device="cuda", dtype=torch.float16)
                part = torch.empty((sp, R, N), device="cuda", dtype=torch.float32)
                res = {}
                for fmt in ("fp16", "fp8"):
                    def launch(i):
                        st = current_stream()
                        if fmt == "fp16":
                            check(L.samd_gemm_skinny(_ptr(A), _ptr(w16[i]), R, N, K, sp, _ptr(part), _ptr(out), 0, st))
                        else:
                            check(L.samd_gemm_skinny_f8(_ptr(A), _ptr(w8[i][0]), _ptr(w8[i][1]), R, N, K, sp, _ptr(part), _ptr(out), 0, st))
                    for i in range(copies):
                        launch(i)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()               # the launches replayed as one graph: no host gaps between kernels
                    with torch.cuda.graph(g):
                        for i in range(copies):
                            launch(i)
                    g.replay()
                    torch.cuda.synchronize()
                    best = float("inf")
                    for _ in range(args.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        g.replay()
                        e1.record()
                        e1.synchronize()
                        best = min(best, e0.elapsed_time(e1) * 1e3 / copies)
                    del g
                    wbytes = N * K * (2 if fmt == "fp16" else 1) + (0 if fmt == "fp16" else 4 * N)
                    res[fmt] = dict(us=round(best, 2), weight_gbps=round(wbytes / (best * 1e-6) / 1e9, 1))
                line = dict(model=model, proj=name, N=N, K=K, rows=R, splits=sp, fp16=res["fp16"], fp8=res["fp8"],
                            gbps_ratio=round(res["fp8"]["weight_gbps"] / res["fp16"]["weight_gbps"], 3),
                            speedup=round(res["fp16"]["us"] / res["fp8"]["us"], 3))
                print(json.dumps(line), flush=True)
                rows_out.append(line)
            del w16, w8
            torch.cuda.empty_cache()
    print(json.dumps(dict(summary=dict(min_gbps_ratio=min(r["gbps_ratio"] for r in rows_out),
                                       mean_speedup=round(sum(r["speedup"] for r in rows_out) / len(rows_out), 3)))))


if __name__ == "__main__":
    main()
