"""Launch time of the dense block-scaled FP8 projection (samd_gemm_skinny_f8b) against its two yardsticks of the same build: the model-dtype
launch (samd_gemm_skinny) and the per-row FP8 launch (samd_gemm_skinny_f8: the same 1-byte stream, 4 bytes per output row of scales where the
block format has 4 bytes per 16 Ki weights).  Shapes: Qwen3-8B's four projections at 16 / 32 / 48 / 64 rows, fp16 and bf16, split-K as the
runner chooses (samd_gemm_splits).  The method is that of profiles/moe_experts_fp8.md: each format's launch is captured ONCE as a hipGraph over
COPIES distinct weight sets (>= 1 GB of FP8 codes together, so that no launch finds its weights in the Infinity Cache -- as in a forward, where
layer l + 1's matrices are hundreds of MB away from layer l's), replayed three times as a warm-up, and then the three graphs are replayed
ALTERNATELY (model dtype, per-row FP8, block FP8, model dtype, ...), --reps single replays each, every replay between two hipEvents.  Figures are
microseconds per launch (replay time / COPIES): the median, and the 10th - 90th percentile of the single replays as the spread.

    python scripts/fp8b_gemm_bench.py [--reps 30] [--dtypes f16,bf16] [--rows 16,32,48,64] [--md]
Prints one JSON line per (dtype, projection, rows); --md appends the rows of the tables of profiles/fp8b128_gemm.md."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam-decoding_amd"))

import torch

from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import fp8 as F8

SHAPES = dict(qkv=(6144, 4096), o=(4096, 4096), gate_up=(24576, 4096), down=(4096, 12288))          # Qwen3-8B
DTYPES = dict(f16=torch.float16, bf16=torch.bfloat16)
FORMATS = ("model", "fp8_row", "fp8_block")


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(p / 100 * (len(xs) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--rows", default="16,32,48,64")
    ap.add_argument("--stream-bytes", type=float, default=1.0e9, help="bytes of distinct FP8 codes each graph cycles through")
    ap.add_argument("--md", action="store_true")
    args = ap.parse_args()
    L = lib()
    lines = []
    for dname in args.dtypes.split(","):
        dtype = DTYPES[dname]
        dt = torch_dtype_code(dtype)
        for pname, (N, K) in SHAPES.items():
            copies = max(4, int(-(-args.stream_bytes // (N * K))))
            sets = []
            for i in range(copies):
                W = (torch.randn((N, K), device="cuda") * 0.02).to(dtype)
                p16 = torch.empty_like(W)
                check(L.samd_gemm_pack_weights(_ptr(W), _ptr(p16), N, K, current_stream()))
                qr, sr = F8.quantize_rows(W)
                pr = torch.empty((N * K,), dtype=torch.uint8, device="cuda")
                check(L.samd_gemm_pack_f8(_ptr(qr), _ptr(pr), N, K, current_stream()))
                qb, sb = F8.quantize_blocks(W)
                pb = torch.empty((N * K,), dtype=torch.uint8, device="cuda")
                check(L.samd_gemm_pack_f8(_ptr(qb), _ptr(pb), N, K, current_stream()))
                sets.append((p16, (pr, sr), (pb, sb)))
                del W, qr, qb
            torch.cuda.synchronize()
            for R in (int(x) for x in args.rows.split(",")):
                sp = L.samd_gemm_splits(N, K, R)
                A = torch.randn((R, K), device="cuda").to(dtype)
                out = torch.empty((R, N), device="cuda", dtype=dtype)
                part = torch.empty((max(sp, 1), R, N), device="cuda", dtype=torch.float32)

                def launch(fmt, i):
                    st = current_stream()
                    p16, (pr, sr), (pb, sb) = sets[i]
                    if fmt == "model":
                        check(L.samd_gemm_skinny(_ptr(A), _ptr(p16), R, N, K, sp, _ptr(part), _ptr(out), dt, st))
                    elif fmt == "fp8_row":
                        check(L.samd_gemm_skinny_f8(_ptr(A), _ptr(pr), _ptr(sr), R, N, K, sp, _ptr(part), _ptr(out), dt, st))
                    else:
                        check(L.samd_gemm_skinny_f8b(_ptr(A), _ptr(pb), _ptr(sb), R, N, K, sp, _ptr(part), _ptr(out), dt, st))
                graphs = {}
                for fmt in FORMATS:
                    for i in range(copies):
                        launch(fmt, i)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for i in range(copies):
                            launch(fmt, i)
                    for _ in range(3):
                        g.replay()
                    torch.cuda.synchronize()
                    graphs[fmt] = g
                times = {fmt: [] for fmt in FORMATS}
                for _ in range(args.reps):
                    for fmt in FORMATS:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        graphs[fmt].replay()
                        e1.record()
                        e1.synchronize()
                        times[fmt].append(e0.elapsed_time(e1) * 1e3 / copies)
                del graphs
                res = {fmt: dict(us=round(pct(t, 50), 2), p10=round(pct(t, 10), 2), p90=round(pct(t, 90), 2)) for fmt, t in times.items()}
                line = dict(dtype=dname, proj=pname, N=N, K=K, rows=R, splits=sp, copies=copies, **res,
                            block_over_row=round(res["fp8_block"]["us"] / res["fp8_row"]["us"], 3),
                            block_over_model=round(res["fp8_block"]["us"] / res["model"]["us"], 3),
                            row_over_model=round(res["fp8_row"]["us"] / res["model"]["us"], 3))
                print(json.dumps(line), flush=True)
                lines.append(line)
            del sets
            torch.cuda.empty_cache()
    if args.md:
        f = lambda r: f"{r['us']:.2f} ({r['p10']:.2f} - {r['p90']:.2f})"
        for dname in args.dtypes.split(","):
            print(f"\n## {dname}\n")
            print("| projection (N x K) | rows | splits | model dtype us (p10 - p90) | per-row FP8 us (p10 - p90) | block FP8 us (p10 - p90) | block / per-row | block / model | per-row / model |")
            print("|---|---|---|---|---|---|---|---|---|")
            for l in lines:
                if l["dtype"] == dname:
                    print(f"| {l['proj']} ({l['N']} x {l['K']}) | {l['rows']} | {l['splits']} | {f(l['model'])} | {f(l['fp8_row'])} | {f(l['fp8_block'])} | "
                          f"{l['block_over_row']:.2f} | {l['block_over_model']:.2f} | {l['row_over_model']:.2f} |")


if __name__ == "__main__":
    main()
