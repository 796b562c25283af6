"""Kernel time and achieved weight GB/s of the INT8 projection (samd_gemm_skinny_i8: GPTQ 8-bit codes, group scales and zero points) against
the model-dtype one (samd_gemm_skinny), the per-row FP8 one (samd_gemm_skinny_f8) and the INT4 one (samd_gemm_skinny_i4) on the same shapes: every
Vicuna-7B and Llama-3-8B projection at 16 and 64 rows (--rows), in fp16 and bf16 (--dtypes), split-K as the runner chooses
(samd_gemm_splits).  Each shape streams COPIES distinct matrices in turn (> 1 GB together in the model dtype), so that no launch finds its
weights in the Infinity Cache -- as in a forward, where layer l + 1's matrices are hundreds of MB away from layer l's.  All kernels are timed
in the same process, from the one library.  Prints one JSON line per (dtype, shape, rows) and a summary.

    python scripts/int8_gemm_bench.py [--reps 20] [--rows 16,64] [--dtypes fp16,bf16] [--formats dense,fp8,int4,int8]   (dense = the model dtype, samd_gemm_skinny)
Times are per launch from event pairs around a replayed graph of the launches: `us` is the best of the repetitions, `spread_us` the distance
from the best to the median repetition -- the run-to-run margin a comparison between two formats or dtypes has to clear."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam-decoding_amd"))

import torch

from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import fp8 as F8
from samd_hip import int4 as I4
from samd_hip import int8 as I8

SHAPES = {
    "vicuna-7b": dict(qkv=(12288, 4096), o=(4096, 4096), gate_up=(22016, 4096), down=(4096, 11008)),
    "llama3-8b": dict(qkv=(6144, 4096), o=(4096, 4096), gate_up=(28672, 4096), down=(4096, 14336)),
}
DTYPES = dict(fp16=torch.float16, bf16=torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="16,64")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--formats", default="dense,fp8,int4,int8")
    ap.add_argument("--models", default=",".join(SHAPES))
    ap.add_argument("--stream-bytes", type=float, default=1.5e9, help="model-dtype bytes of distinct matrices each measurement cycles through")
    args = ap.parse_args()
    formats = args.formats.split(",")
    L = lib()
    rows_out = []
    for dname in args.dtypes.split(","):
        dtype = DTYPES[dname]
        dt = torch_dtype_code(dtype)
        for model in args.models.split(","):
            for name, (N, K) in SHAPES[model].items():
                copies = max(2, int(args.stream_bytes // (2 * N * K)))
                w = {f: [] for f in formats}
                for i in range(copies):
                    st = current_stream()
                    W = (torch.randn((N, K), device="cuda") * 0.02).to(dtype)
                    if "dense" in w:
                        p16 = torch.empty_like(W)
                        check(L.samd_gemm_pack_weights(_ptr(W), _ptr(p16), N, K, st))
                        w["dense"].append(p16)
                    if "fp8" in w:
                        q, s = F8.quantize_rows(W)
                        p8 = torch.empty((N * K,), dtype=torch.uint8, device="cuda")
                        check(L.samd_gemm_pack_f8(_ptr(q), _ptr(p8), N, K, st))
                        w["fp8"].append((p8, s))
                    if "int4" in w:
                        q, z, s = I4.quantize_groups(W, dtype)
                        pi = torch.empty((I4.packed_bytes(N, K),), dtype=torch.uint8, device="cuda")
                        check(L.samd_gemm_pack_i4(_ptr(q), _ptr(z), _ptr(s), _ptr(pi), N, K, dt, st))
                        w["int4"].append(pi)
                    if "int8" in w:
                        q, z, s = I8.quantize_groups(W, dtype)
                        pi = torch.empty((I8.packed_bytes(N, K),), dtype=torch.uint8, device="cuda")
                        check(L.samd_gemm_pack_i8(_ptr(q), _ptr(z), _ptr(s), _ptr(pi), N, K, dt, st))
                        w["int8"].append(pi)
                    torch.cuda.synchronize()
                    del W
                wbytes = dict(dense=2 * N * K, fp8=N * K + 4 * N, int4=I4.packed_bytes(N, K), int8=I8.packed_bytes(N, K))
                for R in (int(r) for r in args.rows.split(",")):
                    sp = L.samd_gemm_splits(N, K, R)
                    A = torch.randn((R, K), device="cuda").to(dtype)
                    out = torch.empty((R, N), device="cuda", dtype=dtype)
                    part = torch.empty((sp, R, N), device="cuda", dtype=torch.float32)
                    res = {}
                    for fmt in formats:
                        def launch(i):
                            st = current_stream()
                            if fmt == "dense":
                                check(L.samd_gemm_skinny(_ptr(A), _ptr(w[fmt][i]), R, N, K, sp, _ptr(part), _ptr(out), dt, st))
                            elif fmt == "fp8":
                                check(L.samd_gemm_skinny_f8(_ptr(A), _ptr(w[fmt][i][0]), _ptr(w[fmt][i][1]), R, N, K, sp, _ptr(part), _ptr(out), dt, st))
                            elif fmt == "int8":
                                check(L.samd_gemm_skinny_i8(_ptr(A), _ptr(w[fmt][i]), R, N, K, sp, _ptr(part), _ptr(out), dt, st))
                            else:
                                check(L.samd_gemm_skinny_i4(_ptr(A), _ptr(w[fmt][i]), R, N, K, sp, _ptr(part), _ptr(out), dt, st))
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
                    line = dict(dtype=dname, model=model, proj=name, N=N, K=K, rows=R, splits=sp, **res)
                    if "int8" in res:
                        for other in ("dense", "fp8", "int4"):
                            if other in res:
                                line[f"i8_over_{other}_us"] = round(res["int8"]["us"] / res[other]["us"], 3)
                                line[f"i8_slower_than_{other}_beyond_spread"] = res["int8"]["us"] - res[other]["us"] > max(res["int8"]["spread_us"], res[other]["spread_us"])
                    print(json.dumps(line), flush=True)
                    rows_out.append(line)
                del w
                torch.cuda.empty_cache()
    # the summary: per dtype and row count, the best and the worst ratio against each format; bf16 against fp16 per shape (is the conversion binding?)
    summary = {}
    for dname in sorted({r["dtype"] for r in rows_out}):
        for R in sorted({r["rows"] for r in rows_out}):
            sel = [r for r in rows_out if r["dtype"] == dname and r["rows"] == R]
            summary[f"{dname}_rows{R}"] = {k: [min(r[k] for r in sel), max(r[k] for r in sel)] for k in ("i8_over_dense_us", "i8_over_fp8_us", "i8_over_int4_us")
                                           if all(k in r for r in sel) and sel}
    by = {(r["dtype"], r["model"], r["proj"], r["rows"]): r for r in rows_out if "int8" in r}
    bf_over = []
    for (dname, model, proj, R), r in by.items():
        o = by.get(("fp16", model, proj, R))
        if dname == "bf16" and o is not None:
            bf_over.append(dict(model=model, proj=proj, rows=R, bf16_over_fp16_us=round(r["int8"]["us"] / o["int8"]["us"], 3),
                                beyond_spread=r["int8"]["us"] - o["int8"]["us"] > max(r["int8"]["spread_us"], o["int8"]["spread_us"])))
    print(json.dumps(dict(summary=summary, int8_bf16_over_fp16=bf_over)))


if __name__ == "__main__":
    main()
