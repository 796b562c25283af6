"""Kernel time and achieved weight GB/s of the MXFP4 projection (samd_gemm_skinny_f4) against the FP8 one (samd_gemm_skinny_f8) and the fp16
one (samd_gemm_skinny) on the same shapes: every Vicuna-7B and Llama-3-8B projection at 16 / 32 / 48 / 64 rows, split-K as the runner
chooses (samd_gemm_splits).  Each shape streams COPIES distinct matrices in turn (> 1 GB together in fp16), so that no launch finds its
weights in the Infinity Cache -- as in a forward, where layer l + 1's matrices are hundreds of MB away from layer l's.  All three kernels
are timed in the same process, from the one library.  Prints one JSON line per (shape, rows) and a summary.

    python scripts/fp4_gemm_bench.py [--reps 20] [--rows 16,32,48,64] [--formats fp16,fp8,mxfp4]
Times are per launch from event pairs around a replayed graph of the launches: `us` is the best of the repetitions, `spread_us` the distance
from the best to the median repetition -- the run-to-run margin a comparison between two formats has to clear."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam-decoding_amd"))

import torch

from samd_hip import _ptr, check, current_stream, lib
from samd_hip import fp8 as F8
from samd_hip import mxfp4 as MX

SHAPES = {
    "vicuna-7b": dict(qkv=(12288, 4096), o=(4096, 4096), gate_up=(22016, 4096), down=(4096, 11008)),
    "llama3-8b": dict(qkv=(6144, 4096), o=(4096, 4096), gate_up=(28672, 4096), down=(4096, 14336)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="16,32,48,64")
    ap.add_argument("--formats", default="fp16,fp8,mxfp4")
    ap.add_argument("--stream-bytes", type=float, default=1.5e9, help="fp16 bytes of distinct matrices each measurement cycles through")
    args = ap.parse_args()
    formats = args.formats.split(",")
    L = lib()
    rows_out = []
    for model, projs in SHAPES.items():
        for name, (N, K) in projs.items():
            copies = max(2, int(args.stream_bytes // (2 * N * K)))
            w = {f: [] for f in formats}
            for i in range(copies):
                st = current_stream()
                W = (torch.randn((N, K), device="cuda") * 0.02).half()
                if "fp16" in w:
                    p16 = torch.empty_like(W)
                    check(L.samd_gemm_pack_weights(_ptr(W), _ptr(p16), N, K, st))
                    w["fp16"].append(p16)
                if "fp8" in w:
                    q, s = F8.quantize_rows(W)
                    p8 = torch.empty((N * K,), dtype=torch.uint8, device="cuda")
                    check(L.samd_gemm_pack_f8(_ptr(q), _ptr(p8), N, K, st))
                    w["fp8"].append((p8, s))
                if "mxfp4" in w:
                    q, e8 = MX.quantize_blocks(W, torch.float16)
                    p4 = torch.empty((MX.packed_bytes(N, K),), dtype=torch.uint8, device="cuda")
                    check(L.samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(p4), N, K, st))
                    w["mxfp4"].append(p4)
                torch.cuda.synchronize()
                del W, q
            wbytes = dict(fp16=2 * N * K, fp8=N * K + 4 * N, mxfp4=MX.packed_bytes(N, K))
            for R in (int(r) for r in args.rows.split(",")):
                sp = L.samd_gemm_splits(N, K, R)
                A = torch.randn((R, K), device="cuda").half()
                out = torch.empty((R, N), device="cuda", dtype=torch.float16)
                part = torch.empty((sp, R, N), device="cuda", dtype=torch.float32)
                res = {}
                for fmt in formats:
                    def launch(i):
                        st = current_stream()
                        if fmt == "fp16":
                            check(L.samd_gemm_skinny(_ptr(A), _ptr(w[fmt][i]), R, N, K, sp, _ptr(part), _ptr(out), 0, st))
                        elif fmt == "fp8":
                            check(L.samd_gemm_skinny_f8(_ptr(A), _ptr(w[fmt][i][0]), _ptr(w[fmt][i][1]), R, N, K, sp, _ptr(part), _ptr(out), 0, st))
                        else:
                            check(L.samd_gemm_skinny_f4(_ptr(A), _ptr(w[fmt][i]), R, N, K, sp, _ptr(part), _ptr(out), 0, st))
                    for i in range(copies):
                        launch(i)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()               # the launches replayed as one graph: no host gaps between kernels
                    with torch.cuda.graph(g):
                        for i in range(copies):
                            launch(i)
                    g.replay()
                    torch.cuda.synchronize()
                    times = []
                    for _ in range(args.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        g.replay()
                        e1.record()
                        e1.synchronize()
                        times.append(e0.elapsed_time(e1) * 1e3 / copies)
                    del g
                    best = min(times)
                    res[fmt] = dict(us=round(best, 2), spread_us=round(statistics.median(times) - best, 2),
                                    weight_gbps=round(wbytes[fmt] / (best * 1e-6) / 1e9, 1))
                line = dict(model=model, proj=name, N=N, K=K, rows=R, splits=sp, **res)
                if "fp8" in res and "mxfp4" in res:
                    line["f4_over_f8_us"] = round(res["mxfp4"]["us"] / res["fp8"]["us"], 3)
                    line["f4_not_slower"] = res["mxfp4"]["us"] <= res["fp8"]["us"] + max(res["mxfp4"]["spread_us"], res["fp8"]["spread_us"])
                print(json.dumps(line), flush=True)
                rows_out.append(line)
            del w
            torch.cuda.empty_cache()
    both = [r for r in rows_out if "f4_over_f8_us" in r]
    if both:
        print(json.dumps(dict(summary={f"rows{R}": dict(max_f4_over_f8_us=max(r["f4_over_f8_us"] for r in both if r["rows"] == R),
                                                        all_not_slower=all(r["f4_not_slower"] for r in both if r["rows"] == R))
                                       for R in sorted({r["rows"] for r in both})})))


if __name__ == "__main__":
    main()
