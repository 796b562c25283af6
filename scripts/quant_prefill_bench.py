"""quant_prefill_bench.py -- the one-pass prefill of a quantised dense runner (each projection unpacked on the device into a scratch matrix,
then the library product) against the 64-row chunked prefill through the streaming kernels.  Runners: --layers (4) random-init layers at
Vicuna-7B and Llama-3-8B geometry, weight_format fp8, fp8b128, mxfp4, int4g128, int8g128, fp16 and bf16; prompts of 128 .. 4096 tokens.

  arms     "new": this build; per prompt length the one-pass prefill (SAMD_QUANT_PREFILL_MIN_ROWS=128 forces it at every length) and its own
           chunked prefill (SAMD_PREFILL=chunked) ALTERNATE in one process after a warm-up, every prefill between a host clock and a device
           synchronise.  "parent" (--parent-lib: libsamd_hip.so built from the parent commit, loaded through SAMD_HIP_LIB): the chunked
           prefill of that library in a process of its own, started right after the "new" one of the same configuration -- THE YARDSTICK.
           The parent library lacks the samd_gemm_unpack_* entry points, so that process drops them from the binding table before the library
           is loaded; it cannot take the one-pass path.  The chunked prefill runs the same kernels in both libraries: new-chunked against
           parent-chunked is the process-to-process spread.
  unpack   one more one-pass prefill per length with device events around every samd_gemm_unpack_* launch: their share of the prefill and
           (bytes read + bytes written) / time.
Each figure is the median and the 10th - 90th percentile of whole prefill() calls, in milliseconds; one JSON line per (configuration, arm,
form, length).  Every child process runs under its own time limit and nothing more is started after one that failed.  No device setting is
touched.

  measure  python scripts/quant_prefill_bench.py --parent-lib PATH [--models vicuna-7b,llama-3-8b] [--configs fp16:int4g128,...] --out DIR
  report   python scripts/quant_prefill_bench.py --report DIR/a.json,DIR/b.json [--md FILE]
           (profiles/quant_prefill.md holds the output of this step on profiles/quant_prefill_*.json between its method and its reasons)
           the table, and the switch-over: the smallest measured length from which, at that length and every longer one, in every format and
           dtype, one-pass <= parent-chunked * (1 + s), s = |new-chunked - parent-chunked| / parent-chunked of the same cell (the two
           chunked columns' own spread)."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sam-decoding_amd")]

MODELS = {
    "vicuna-7b": dict(hidden_size=4096, intermediate_size=11008, num_attention_heads=32, num_key_value_heads=32, vocab_size=32000,
                      max_position_embeddings=8192, rms_norm_eps=1e-5),
    "llama-3-8b": dict(hidden_size=4096, intermediate_size=14336, num_attention_heads=32, num_key_value_heads=8, vocab_size=128256,
                       max_position_embeddings=8192, rms_norm_eps=1e-5, rope_theta=5e5),
}
FORMATS = ("fp8", "fp8b128", "mxfp4", "int4g128", "int8g128")
LENGTHS = (128, 192, 256, 512, 1024, 2048, 4096)
CONFIGS = tuple(f"{d}:{f}" for f in FORMATS for d in ("fp16", "bf16"))
CHILD_LIMIT = 300                                                # seconds per child process
UNPACK = ("samd_gemm_unpack_f8", "samd_gemm_unpack_f8b", "samd_gemm_unpack_f4", "samd_gemm_unpack_i4", "samd_gemm_unpack_i8")
PACKED_BYTES_PER_WEIGHT = {"fp8": 1.0, "fp8b128": 1.0, "mxfp4": 17 / 32, "int4g128": 17 / 32, "int8g128": 33 / 32}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def child(a):
    arm, (dt_name, fmt) = a.child, a.config.split(":")
    import samd_hip
    if arm == "parent":
        for name in UNPACK:
            samd_hip._PROTOS.pop(name, None)                     # the parent library does not export them; its chunked prefill needs none
        os.environ["SAMD_PREFILL"] = "chunked"
    os.environ["SAMD_QUANT_PREFILL_MIN_ROWS"] = "128"
    import numpy as np
    import torch
    from samd_hip.llama import LlamaRunner
    dtype = dict(bf16=torch.bfloat16, fp16=torch.float16)[dt_name]
    cfg = dict(MODELS[a.model], num_hidden_layers=a.layers)
    runner = LlamaRunner.random_init(cfg, max(a.lengths) + 64, dtype, seed=1, std=0.02, weight_format=fmt)
    assert runner.weight_format == fmt and runner.row_major_released
    weights = sum(t.shape[0] * t.shape[1] for l in runner.w["layers"] for k, t in l.items() if k in ("wqkv", "wo", "wgu", "wdown"))

    def prefill(ids, mode):
        os.environ["SAMD_PREFILL"] = mode
        sess = samd_hip.Session(runner.max_len)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.prefill(sess, ids)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    modes = ("chunked",) if arm == "parent" else ("wide", "chunked")
    for N in a.lengths:
        ids = torch.tensor([np.random.default_rng(N).integers(3, cfg["vocab_size"], N).tolist()], device="cuda")
        reps = a.reps if N <= 1024 else max(3, a.reps // 2)
        for m in modes:                                          # warm-up: code objects, library handles, buffers of this length
            prefill(ids, m), prefill(ids, m)
        times = {m: [] for m in modes}
        for _ in range(reps):
            for m in modes:
                times[m].append(prefill(ids, m))
        for m in modes:
            rec = dict(model=a.model, config=a.config, arm=arm, form="one_pass" if m == "wide" else "chunked", tokens=N, reps=reps,
                       median_ms=round(pct(times[m], 0.5), 3), p10_ms=round(pct(times[m], 0.1), 3), p90_ms=round(pct(times[m], 0.9), 3))
            if m == "wide":
                assert "quant_prefill_scratch" in runner.memory_report(), "the one-pass form did not run"
                rec.update(unpack_share(runner, torch, ids, prefill, weights * (PACKED_BYTES_PER_WEIGHT[fmt] + 2)))
            print("RESULT " + json.dumps(rec), flush=True)


def unpack_share(runner, torch, ids, prefill, nbytes):
    """one more one-pass prefill with device events around every unpack launch"""
    spans, orig = [], runner._pf_weight

    def timed(li, key):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(li, key)
        e1.record()
        spans.append((e0, e1))
        return out
    runner._pf_weight = timed
    try:
        total = prefill(ids, "wide")
    finally:
        del runner._pf_weight
    ms = sum(e0.elapsed_time(e1) for e0, e1 in spans)
    return dict(unpack_ms=round(ms, 3), unpack_share=round(ms / total, 3), unpack_gb_s=round(nbytes / ms / 1e6, 1))


def switch_over(results):
    """(the smallest measured length from which every cell holds at it and at every longer length, or None; the cells that fail, by length)"""
    cells = {}
    for r in results:
        cells.setdefault((r["model"], r["config"], r["tokens"]), {})[(r["arm"], r["form"])] = r
    lengths = sorted({k[2] for k in cells})
    fails = {N: [] for N in lengths}
    for (model, config, N), c in sorted(cells.items()):
        w, own, par = c.get(("new", "one_pass")), c.get(("new", "chunked")), c.get(("parent", "chunked"))
        if not (w and own and par):
            fails[N].append((model, config, "not measured"))
            continue
        spread = abs(own["median_ms"] - par["median_ms"]) / par["median_ms"]
        if w["median_ms"] > par["median_ms"] * (1 + spread):
            fails[N].append((model, config, f"{w['median_ms']:.2f} > {par['median_ms']:.2f} * (1 + {spread:.3f})"))
    ok_from = None
    for N in reversed(lengths):
        if fails[N]:
            break
        ok_from = N
    return ok_from, fails


def report(results, md):
    cell = lambda r: f"{r['median_ms']:.2f} ({r['p10_ms']:.2f} - {r['p90_ms']:.2f})" if r else "-"
    lines = ["| model | dtype:format | tokens | one-pass ms | chunked ms (this build) | chunked ms (parent library) | parent / one-pass | unpack share | unpack GB/s |",
             "|---|---|---|---|---|---|---|---|---|"]
    keys = sorted({(r["model"], r["config"]) for r in results}, key=lambda k: (k[0], k[1].split(":")[1], k[1]))
    for model, config in keys:
        for N in sorted({r["tokens"] for r in results}):
            get = lambda arm, form: next((r for r in results if (r["model"], r["config"], r["arm"], r["form"], r["tokens"]) == (model, config, arm, form, N)), None)
            w, c, p = get("new", "one_pass"), get("new", "chunked"), get("parent", "chunked")
            if w:
                base = p or c
                lines.append(f"| {model} | {config} | {N} | {cell(w)} | {cell(c)} | {cell(p)} | {base['median_ms'] / w['median_ms']:.2f} | "
                             f"{w['unpack_share']:.2f} | {w['unpack_gb_s']:.0f} |")
    ok_from, fails = switch_over(results)
    lines += ["", f"Switch-over by the rule of scripts/quant_prefill_bench.py: {ok_from if ok_from is not None else 'no measured length qualifies'}."]
    for N, bad in sorted(fails.items()):
        if bad:
            lines.append(f"- {N} tokens fails in {len(bad)} cells: " + "; ".join(f"{m} {c} ({why})" for m, c, why in bad[:6]) + (" ..." if len(bad) > 6 else ""))
    text = "\n".join(lines) + "\n"
    print(text)
    if md:
        with open(md, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("new", "parent"))
    ap.add_argument("--model", default="vicuna-7b")
    ap.add_argument("--config", default=CONFIGS[0])
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--parent-lib")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--lengths", type=lambda s: tuple(int(x) for x in s.split(",")), default=LENGTHS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--report", default=None, help="comma-separated JSON files of earlier runs: print (and with --md write) the table and the switch-over")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.report:
        return report([r for p in a.report.split(",") for r in json.load(open(p))], a.md)
    results = []
    for model in a.models.split(","):
        for config in a.configs.split(","):
            for arm in ("new", "parent") if a.parent_lib else ("new",):
                env = dict(os.environ)
                env.pop("SAMD_PREFILL", None)
                env.pop("SAMD_WEIGHT_FORMAT", None)
                if arm == "parent":
                    env["SAMD_HIP_LIB"] = os.path.abspath(a.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--model", model, "--config", config, "--layers", str(a.layers),
                       "--lengths", ",".join(map(str, a.lengths)), "--reps", str(a.reps)]
                print("==", model, config, arm, flush=True)
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT)] + cmd, env=env, capture_output=True, text=True)
                for line in p.stdout.splitlines():
                    if line.startswith("RESULT "):
                        results.append(json.loads(line[7:]))
                        print(line[7:], flush=True)
                if a.out:                                        # after every child: a later failure keeps what was measured
                    os.makedirs(a.out, exist_ok=True)
                    with open(os.path.join(a.out, "quant_prefill_bench_" + "_".join(a.models.split(",")) + ".json"), "w") as f:
                        json.dump(results, f, indent=1)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-4000:], sep="\n")
                    raise SystemExit(f"{model} {config} {arm}: exit {p.returncode}; nothing more is started")
    report(results, a.md)


if __name__ == "__main__":
    main()
