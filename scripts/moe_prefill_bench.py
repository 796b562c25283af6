"""moe_prefill_bench.py -- the one-pass prefill of a mixture-of-experts runner against the chunked prefill, on Qwen3-30B-A3B geometry (hidden 2048,
moe_intermediate 768, 128 experts, top-8, 32 / 4 heads) with --layers (4) random-init layers, prompts of 128 .. 4096 tokens, the four expert
formats in bf16 and the model dtype also in fp16.

  arms     "new": this build; per prompt length the one-pass prefill and its own chunked prefill (SAMD_PREFILL=chunked) ALTERNATE in one process
           after a warm-up, every prefill between a host clock and a device synchronise.  "parent" (--parent-lib: libsamd_hip.so built from
           the parent commit, loaded through SAMD_HIP_LIB as scripts/ab_lib.sh does): the chunked prefill of that library in a process of
           its own, started right after the "new" one of the same configuration.  The parent library lacks the samd_moe_wide_* entry points,
           so that process drops them from the binding table before the library is loaded; it cannot take the one-pass path.
           The chunked prefill runs the same kernels in both libraries: new-chunked against parent-chunked is the process-to-process spread.
  share    one more one-pass prefill per length with device events around MoeWideBuffers.route / lists / experts: the share of the prefill
           spent in the sparse layers' wide launches.
  bytes    from the routing of that prefill (route_log): the expert bytes the chunked form streams (per 64-row chunk and layer, the distinct
           experts it touches) and the one-pass form's lower and upper count (per super-chunk and layer: every touched expert once; once per
           64-entry tile if no tile found its expert's weights in a cache).
Reports median and p10 - p90 in milliseconds, one JSON line per (configuration, arm, length), and a markdown table at the end.
Every child process runs under its own time limit and nothing more is started after one that failed.
usage: python scripts/moe_prefill_bench.py [--parent-lib PATH] [--layers 4] [--lengths 128,256,...] [--configs bf16:none,bf16:mxfp4,...] [--reps 7] [--out DIR]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sam-decoding_amd")]

A3B = dict(model_type="qwen3_moe", hidden_size=2048, intermediate_size=6144, moe_intermediate_size=768, num_attention_heads=32, num_key_value_heads=4,
           head_dim=128, vocab_size=151936, max_position_embeddings=40960, rms_norm_eps=1e-6, rope_theta=1e6, num_experts=128, num_experts_per_tok=8,
           norm_topk_prob=True, decoder_sparse_step=1, mlp_only_layers=[])
LENGTHS = (128, 256, 512, 1024, 2048, 4096)
CONFIGS = ("bf16:none", "bf16:mxfp4", "bf16:int4g128", "bf16:fp8b128", "fp16:none")
CHILD_LIMIT = 300                                                # seconds per child process


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def child(a):
    arm, (dt_name, fmt) = a.child, a.config.split(":")
    if arm == "parent":
        import samd_hip
        for name in [n for n in samd_hip._PROTOS if n.startswith("samd_moe_wide_")]:
            del samd_hip._PROTOS[name]                           # the parent library does not export them; its chunked prefill needs none
        os.environ["SAMD_PREFILL"] = "chunked"
    import numpy as np
    import torch
    import samd_hip
    from samd_hip import moe as MOE
    from samd_hip.llama import LlamaRunner
    dtype = dict(bf16=torch.bfloat16, fp16=torch.float16)[dt_name]
    cfg = dict(A3B, num_hidden_layers=a.layers)
    runner = LlamaRunner.random_init(cfg, max(a.lengths) + 64, dtype, seed=1, std=0.02, expert_format=None if fmt == "none" else fmt)
    per_expert = sum(l[k].numel() * l[k].element_size() for l in runner.wp["layers"] for k in ("moe_gu", "moe_down")) / (a.layers * cfg["num_experts"])

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
        for m in modes:                                          # warm-up: code objects, buffers of this length
            prefill(ids, m), prefill(ids, m)
        times = {m: [] for m in modes}
        for _ in range(reps):
            for m in modes:
                times[m].append(prefill(ids, m))
        for m in modes:
            rec = dict(config=a.config, arm=arm, form="one_pass" if m == "wide" else "chunked", tokens=N, reps=reps, median_ms=round(pct(times[m], 0.5), 3),
                       p10_ms=round(pct(times[m], 0.1), 3), p90_ms=round(pct(times[m], 0.9), 3))
            if m == "wide":
                rec.update(share_and_bytes(runner, MOE, torch, ids, N, per_expert, prefill))
            print("RESULT " + json.dumps(rec), flush=True)


def share_and_bytes(runner, MOE, torch, ids, N, per_expert, prefill):
    """one more one-pass prefill with device events around the wide launches and the routing logged"""
    spans, orig = [], {}

    def timed(name):
        fn = orig[name] = getattr(MOE.MoeWideBuffers, name)

        def wrapper(self, *args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(self, *args, **kw)
            e1.record()
            spans.append((e0, e1))
            return out
        setattr(MOE.MoeWideBuffers, name, wrapper)
    for name in ("route", "lists", "experts"):
        timed(name)
    runner.route_log = []
    try:
        total = prefill(ids, "wide")
    finally:
        for name, fn in orig.items():
            setattr(MOE.MoeWideBuffers, name, fn)
    log, runner.route_log = runner.route_log, None
    wide_ms = sum(e0.elapsed_time(e1) for e0, e1 in spans)
    chunked = lower = upper = 0
    for _, n, idx, _ in log:
        idx = idx[:n].cpu()
        counts = torch.bincount(idx.flatten(), minlength=runner.shape.n_experts)
        lower += int((counts > 0).sum())
        upper += int(((counts + 63) // 64).sum())
        chunked += sum(int(idx[c0:c0 + 64].unique().numel()) for c0 in range(0, n, 64))
    gb = lambda experts: round(experts * per_expert / 1e9, 3)
    return dict(wide_launch_share=round(wide_ms / total, 3), expert_gb_chunked=gb(chunked), expert_gb_one_pass_min=gb(lower), expert_gb_one_pass_max=gb(upper))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("new", "parent"))
    ap.add_argument("--config", default=CONFIGS[0])
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--parent-lib")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--lengths", type=lambda s: tuple(int(x) for x in s.split(",")), default=LENGTHS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    results = []
    for config in a.configs.split(","):
        for arm in ("new", "parent") if a.parent_lib else ("new",):
            env = dict(os.environ)
            env.pop("SAMD_PREFILL", None)
            if arm == "parent":
                env["SAMD_HIP_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--config", config, "--layers", str(a.layers),
                   "--lengths", ",".join(map(str, a.lengths)), "--reps", str(a.reps)]
            print("==", config, arm, flush=True)
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT)] + cmd, env=env, capture_output=True, text=True)
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    results.append(json.loads(line[7:]))
                    print(line[7:], flush=True)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:], sep="\n")
                raise SystemExit(f"{config} {arm}: exit {p.returncode}; nothing more is started")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "moe_prefill_bench.json"), "w") as f:
            json.dump(results, f, indent=1)
    cell = lambda r: f"{r['median_ms']:.2f} ({r['p10_ms']:.2f} - {r['p90_ms']:.2f})" if r else "-"
    print("\n| experts | tokens | one-pass ms | chunked ms (this build) | chunked ms (parent library) | parent / one-pass | wide launches' share | expert GB chunked | expert GB one-pass (min - max) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for config in a.configs.split(","):
        for N in a.lengths:
            get = lambda arm, form: next((r for r in results if (r["config"], r["arm"], r["form"], r["tokens"]) == (config, arm, form, N)), None)
            w, c, p = get("new", "one_pass"), get("new", "chunked"), get("parent", "chunked")
            if w:
                base = p or c
                print(f"| {config} | {N} | {cell(w)} | {cell(c)} | {cell(p)} | {base['median_ms'] / w['median_ms']:.2f} | {w['wide_launch_share']:.2f} | "
                      f"{w['expert_gb_chunked']:.2f} | {w['expert_gb_one_pass_min']:.2f} - {w['expert_gb_one_pass_max']:.2f} |")


if __name__ == "__main__":
    main()
