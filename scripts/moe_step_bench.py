"""moe_step_bench.py -- what the mixture-of-experts path costs on Qwen3-30B-A3B geometry (hidden 2048, moe_intermediate 768, 128 experts, top-8),
random-init weights, per row bucket 1 / 8 / 16 / 64.

  experts  per bucket: distinct experts touched per layer, bytes streamed by the three launches (route, gate|up + SiLU, down + combine) divided
           by their graph-replay time, and beside it the SAME number of bytes streamed by the dense samd_gemm_pairs_silu + samd_gemm_skinny on
           an MLP of equal weight size, in the same process -- the yardstick (never the new kernels against themselves).  --layers distinct
           weight sets are visited per replay so that no replay finds its weights in the Infinity Cache.
  step     graph-replay time of one verify forward per bucket for a --depth layer Qwen3-30B-A3B stack, and its ratio to the 1-row
           (autoregressive) step.

  formats  (--expert-format mxfp4, step "experts") the MXFP4 expert launches against the model-dtype ones of the same build on the same routing:
           gate|up + SiLU, down + combine and the whole three-call layer, each captured once over --layers weight sets and replayed ALTERNATELY
           (model dtype, mxfp4, model dtype, ...), every single replay between two hipEvents after a warm-up; median, 10th / 90th percentile and
           the achieved weight rate (bytes of the experts touched over the median of the two expert launches).  With --step step the forward is
           built with expert_format="mxfp4".  --expert-format int4g128 adds the INT4 (AWQ / GPTQ) expert launches as a third graph in the
           same alternation: model dtype and MXFP4, both untouched by the INT4 kernels, are its yardsticks in the same run.  --dtype picks
           the model dtype (bf16 or fp16) of this step.  --expert-format fp8b128 does the same for the block-scaled FP8 expert launches
           (e4m3fn codes, one fp32 scale per 128 x 128 block): model dtype and MXFP4 are the yardsticks, never the new code against itself.
           --expert-format int8g128 times the INT8 (GPTQ) expert launches beside the model-dtype and the block-scaled FP8 ones (the other
           8-bit format), in the same alternation.

Without --step every step runs as a child process of its own under its own time limit, and nothing more is started after a step that failed.
--buckets 1 keeps a profiler's per-kernel statistics to one bucket: rocprofv3 --kernel-trace --stats -- python scripts/moe_step_bench.py --step experts --buckets 1
usage: python scripts/moe_step_bench.py [--step experts|step] [--reps 30] [--layers 4] [--depth 12] [--buckets 1,8,16,64] [--expert-format none|mxfp4|int4g128|fp8b128|int8g128] [--dtype bf16|fp16]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sam-decoding_amd")]

A3B = dict(model_type="qwen3_moe", hidden_size=2048, intermediate_size=6144, moe_intermediate_size=768, num_attention_heads=32, num_key_value_heads=4,
           head_dim=128, vocab_size=151936, max_position_embeddings=40960, rms_norm_eps=1e-6, rope_theta=1e6, num_experts=128, num_experts_per_tok=8,
           norm_topk_prob=True, decoder_sparse_step=1, mlp_only_layers=[])
BUCKETS = (1, 8, 16, 64)
STEP_LIMITS = {"experts": 420, "step": 420}        # seconds per child process


def replay_us(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def step_experts(a):
    import torch
    import samd_hip
    from samd_hip import moe as MOE, _ptr, check, current_stream, lib
    H, I, E, k = A3B["hidden_size"], A3B["moe_intermediate_size"], A3B["num_experts"], A3B["num_experts_per_tok"]
    dt, L = torch.bfloat16, lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: (torch.randn(s, generator=g, device="cuda") * 0.02).to(dt)
    sets = []
    for _ in range(a.layers):
        sets.append((rnd(E, H) * 50, *MOE.pack_experts(rnd(E, 2 * I, H), rnd(E, H, I))))
    for n in a.buckets:
        RP = max(16, n)
        h = torch.randn((RP, H), generator=g, device="cuda").to(dt)
        d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        bufs = [MOE.MoeBuffers(RP, H, I, E, k, dt, samd_hip.BF16, "cuda") for _ in sets]

        def moe():
            for (router, pgu, pd), b in zip(sets, bufs):
                b.route(h, router, d_n, True)
                b.experts(h, pgu, pd, d_n)
        t_moe = replay_us(moe, a.reps) / a.layers
        active = [b.routing_state()[0] for b in bufs]
        # the three calls on their own (each over all the weight sets, so the weights stay cold); lists = the second kernel of the route call
        L_ = lib()
        parts = dict(
            route=lambda: [b.route(h, r, d_n, True) for (r, _, _), b in zip(sets, bufs)],
            lists=lambda: [b.lists(d_n) for b in bufs],
            gate_up=lambda: [check(L_.samd_moe_gate_up_silu(_ptr(h), _ptr(pgu), _ptr(b.ws), RP, H, I, E, k, _ptr(b.act), samd_hip.BF16, current_stream()))
                             for (_, pgu, _), b in zip(sets, bufs)],
            down_combine=lambda: [check(L_.samd_moe_down_combine(_ptr(b.act), _ptr(pd), _ptr(b.topk_idx), _ptr(b.topk_w), _ptr(d_n), _ptr(b.ws), RP, H, I, E, k,
                                                                 _ptr(b.out), samd_hip.BF16, current_stream())) for (_, _, pd), b in zip(sets, bufs)])
        part_us = {name: round(replay_us(fn, a.reps) / a.layers, 1) for name, fn in parts.items()}
        act_mean = sum(active) / len(active)
        nbytes = act_mean * 3 * H * I * 2
        # the dense yardstick: one MLP whose gate|up and down matrices hold as many bytes (intermediate = active experts x 768, a multiple of 128)
        Id = int(round(act_mean)) * I
        dense = []
        for _ in sets:
            wgu, wd = rnd(2 * Id, H), rnd(H, Id)
            pgu, pdn = torch.empty_like(wgu), torch.empty_like(wd)
            check(L.samd_gemm_pack_groups(_ptr(wgu), _ptr(pgu), 2 * Id, H, current_stream()))
            check(L.samd_gemm_pack_weights(_ptr(wd), _ptr(pdn), H, Id, current_stream()))
            dense.append((pgu, pdn))
            del wgu, wd
        act = torch.zeros((RP, Id), dtype=dt, device="cuda")
        out = torch.zeros((RP, H), dtype=dt, device="cuda")
        sp = L.samd_gemm_splits(H, Id, RP)
        part = torch.zeros(max(sp * RP * H, 1), dtype=torch.float32, device="cuda")

        def mlp():
            for pgu, pdn in dense:
                check(L.samd_gemm_pairs_silu(_ptr(h), _ptr(pgu), RP, Id, H, _ptr(act), samd_hip.BF16, current_stream()))
                check(L.samd_gemm_skinny(_ptr(act), _ptr(pdn), RP, H, Id, sp, _ptr(part), _ptr(out), samd_hip.BF16, current_stream()))
        t_dense = replay_us(mlp, a.reps) / a.layers
        print(json.dumps(dict(step="experts", rows=n, bucket=RP, experts_touched=active, mbytes=round(nbytes / 1e6, 1), moe_us=round(t_moe, 1), calls_us=part_us,
                              moe_tb_s=round(nbytes / t_moe / 1e6, 3), dense_us=round(t_dense, 1), dense_tb_s=round(nbytes / t_dense / 1e6, 3),
                              moe_over_dense=round(t_moe / t_dense, 2))), flush=True)
        del dense, bufs, act, out, part
        torch.cuda.empty_cache()


def step_formats(a):
    import torch
    import samd_hip
    from samd_hip import moe as MOE, _ptr, check, current_stream, lib
    H, I, E, k = A3B["hidden_size"], A3B["moe_intermediate_size"], A3B["num_experts"], A3B["num_experts_per_tok"]
    dt, BF = (torch.float16, samd_hip.F16) if a.dtype == "fp16" else (torch.bfloat16, samd_hip.BF16)
    L = lib()
    fmts = ("model", "fp8b128", "int8g128") if a.expert_format == "int8g128" else \
        ("model", "mxfp4") + ((a.expert_format,) if a.expert_format in ("int4g128", "fp8b128") else ())
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: (torch.randn(s, generator=g, device="cuda") * 0.02).to(dt)
    sets = []
    for _ in range(a.layers):
        router, gu, dn = rnd(E, H) * 50, rnd(E, 2 * I, H), rnd(E, H, I)
        packed = {"model": MOE.pack_experts(gu, dn)}
        if "mxfp4" in fmts:
            packed["mxfp4"] = MOE.pack_experts_mxfp4(*MOE.quantize_experts(gu, dn, dt))
        if "int8g128" in fmts:
            packed["int8g128"] = MOE.pack_experts_int8(*MOE.quantize_experts_int8(gu, dn, dt), dt)
        if "int4g128" in fmts:
            packed["int4g128"] = MOE.pack_experts_int4(*MOE.quantize_experts_int4(gu, dn, dt), dt)
        if "fp8b128" in fmts:
            packed["fp8b128"] = MOE.pack_experts_fp8(*MOE.quantize_experts_fp8(gu, dn))
        sets.append((router, packed))
        del gu, dn
    per_expert = {"model": 3 * H * I * 2, "mxfp4": 3 * H * I // 2 + 3 * H * I // 32, "int4g128": 3 * H * I // 2 + 3 * H * I // 32,
                  "fp8b128": 3 * H * I + 3 * (H // 64) * (I // 128) * 4,     # codes + the packed table: one fp32 per (64 rows, 128 k)
                  "int8g128": 3 * H * I + 3 * H * I // 32}
    gate_up_fn = {"model": L.samd_moe_gate_up_silu, "mxfp4": L.samd_moe_gate_up_silu_f4, "int4g128": L.samd_moe_gate_up_silu_i4,
                  "fp8b128": L.samd_moe_gate_up_silu_f8, "int8g128": L.samd_moe_gate_up_silu_i8}
    down_fn = {"model": L.samd_moe_down_combine, "mxfp4": L.samd_moe_down_combine_f4, "int4g128": L.samd_moe_down_combine_i4,
               "fp8b128": L.samd_moe_down_combine_f8, "int8g128": L.samd_moe_down_combine_i8}

    def graph(fn):
        fn(); torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        for _ in range(3):                                       # warm-up replays
            gr.replay()
        torch.cuda.synchronize()
        return gr

    def alternate(graphs, reps):
        """single replays of the graphs in turn, each between two events -> {name: sorted us per layer}"""
        ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for name in graphs}
        for r in range(reps):
            for name, gr in graphs.items():
                ev[name][r][0].record(); gr.replay(); ev[name][r][1].record()
        torch.cuda.synchronize()
        return {name: sorted(e0.elapsed_time(e1) * 1e3 / a.layers for e0, e1 in ev[name]) for name in graphs}

    for n in a.buckets:
        RP = max(16, n)
        h = torch.randn((RP, H), generator=g, device="cuda").to(dt)
        d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
        bufs = [MOE.MoeBuffers(RP, H, I, E, k, dt, BF, "cuda") for _ in sets]
        for (router, _), b in zip(sets, bufs):
            b.route(h, router, d_n, True)
        torch.cuda.synchronize()
        active = [b.routing_state()[0] for b in bufs]
        act_mean = sum(active) / len(active)
        st = current_stream

        def gate_up(fmt):
            for (_, packed), b in zip(sets, bufs):
                check(gate_up_fn[fmt](_ptr(h), _ptr(packed[fmt][0]), _ptr(b.ws), RP, H, I, E, k, _ptr(b.act), BF, st()))

        def down(fmt):
            for (_, packed), b in zip(sets, bufs):
                check(down_fn[fmt](_ptr(b.act), _ptr(packed[fmt][1]), _ptr(b.topk_idx), _ptr(b.topk_w), _ptr(d_n), _ptr(b.ws), RP, H, I, E, k,
                                   _ptr(b.out), BF, st()))

        def layer(fmt):
            for (router, packed), b in zip(sets, bufs):
                b.route(h, router, d_n, True)
                b.experts(h, *packed[fmt], d_n, expert_format=None if fmt == "model" else fmt)
        out = dict(step="formats", dtype=a.dtype, rows=n, bucket=RP, experts_touched=active, reps=a.reps, layers=a.layers)
        med = {}
        for what, fn in (("gate_up", gate_up), ("down_combine", down), ("layer", layer)):
            times = alternate({fmt: graph(lambda fmt=fmt: fn(fmt)) for fmt in fmts}, a.reps)
            for fmt, t in times.items():
                med[what, fmt] = t[len(t) // 2]
                out[f"{what}_{fmt}_us"] = dict(median=round(t[len(t) // 2], 2), p10=round(t[len(t) // 10], 2), p90=round(t[(9 * len(t)) // 10], 2),
                                               min=round(t[0], 2), max=round(t[-1], 2))
            for fmt in fmts[1:]:
                out[f"{what}_{fmt}_over_model"] = round(med[what, fmt] / med[what, "model"], 3)
        for fmt in fmts:
            nbytes = act_mean * per_expert[fmt]
            out[f"{fmt}_mbytes"] = round(nbytes / 1e6, 2)
            out[f"{fmt}_weight_tb_s"] = round(nbytes / (med["gate_up", fmt] + med["down_combine", fmt]) / 1e6, 3)
        print(json.dumps(out), flush=True)
        del bufs
        torch.cuda.empty_cache()


def step_forward(a):
    import torch
    import samd_hip
    from samd_hip.llama import LlamaRunner
    runner = LlamaRunner.random_init(dict(A3B, num_hidden_layers=a.depth), 2048, torch.float16 if a.dtype == "fp16" else torch.bfloat16, seed=0,
                                     expert_format=None if a.expert_format == "none" else a.expert_format)
    sess = samd_hip.Session(4096)
    sess.reset()
    res, touched = {}, {}
    for n in a.buckets:
        toks = torch.arange(5, 5 + n, dtype=torch.int32, device="cuda"); par = torch.arange(-1, n - 1, dtype=torch.int32, device="cuda")
        sess.set_draft(toks, par, n)
        sess.set_cache_length(800)
        R = runner.bucket(n)
        runner.warm(R)
        runner.route_log = []
        runner.verify(sess, R); torch.cuda.synchronize()
        touched[n] = round(sum(len(set(e[2][:e[1]].flatten().tolist())) for e in runner.route_log) / max(len(runner.route_log), 1), 1)
        runner.route_log = None
        res[n] = round(replay_us(lambda: runner.verify(sess, R), a.reps) / 1e3, 4)
    print(json.dumps(dict(step="step", dtype=a.dtype, depth=a.depth, expert_format=runner.expert_format, step_ms=res, experts_touched_per_layer=touched,
                          ratio_to_1_row={n: round(res[n] / res[1], 3) for n in a.buckets if 1 in res})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("experts", "step"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--buckets", default=",".join(map(str, BUCKETS)), help="row counts, comma separated")
    ap.add_argument("--expert-format", default="none", choices=("none", "mxfp4", "int4g128", "fp8b128", "int8g128"),
                    help="mxfp4: the MXFP4 expert kernels against the model-dtype ones; int4g128 / fp8b128: the INT4 / block-scaled FP8 ones against both; "
                         "int8g128: the INT8 ones against the model-dtype and FP8 ones")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"), help="model dtype of the formats and step measurements")
    a = ap.parse_args()
    a.buckets = tuple(int(b) for b in a.buckets.split(","))
    if a.step == "experts":
        return step_formats(a) if a.expert_format != "none" else step_experts(a)
    if a.step == "step":
        return step_forward(a)
    for name, limit in STEP_LIMITS.items():        # a fresh process per step, each under its own limit; a failure ends the run
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--layers", str(a.layers),
               "--depth", str(a.depth), "--buckets", ",".join(map(str, a.buckets)), "--expert-format", a.expert_format, "--dtype", a.dtype]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"step {name} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
