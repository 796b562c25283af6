"""qwen_step_bench.py -- graph-replay time of one verify forward per row bucket (L = 800 cached keys) for random-init Llama-3-8B, Qwen2.5-7B and
Qwen3-8B (and Vicuna-7B: --models vicuna-7b) at full depth, in fp16 and with FP8, MXFP4, INT4 or INT8 projections (--formats fp16,fp8,mxfp4,int4g128,int8g128).  Qwen runs the eight-launch layer with samd_rope_kv_write_epi (q|k|v bias / q-k
norm); Llama-3-8B is the yardstick.   usage: python scripts/qwen_step_bench.py [--reps 30] [--models llama3-8b,qwen2.5-7b,qwen3-8b]"""
import argparse, gc, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sam-decoding_amd")]
import torch
import bench, samd_hip
from samd_hip.llama import LlamaRunner

MODELS = {
    "llama3-8b": dict(bench.LLAMA3_8B),
    "vicuna-7b": dict(bench.VICUNA_7B),
    "qwen2.5-7b": dict(model_type="qwen2", hidden_size=3584, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28,
                       num_key_value_heads=4, head_dim=128, vocab_size=152064, max_position_embeddings=32768, rms_norm_eps=1e-6, rope_theta=1e6),
    "qwen3-8b": dict(model_type="qwen3", hidden_size=4096, intermediate_size=12288, num_hidden_layers=36, num_attention_heads=32,
                     num_key_value_heads=8, head_dim=128, vocab_size=151936, max_position_embeddings=40960, rms_norm_eps=1e-6, rope_theta=1e6),
}


def step_ms(runner, sess, n, reps):
    toks = torch.arange(5, 5 + n, dtype=torch.int32, device="cuda"); par = torch.arange(-1, n - 1, dtype=torch.int32, device="cuda")
    sess.set_draft(toks, par, n)
    sess.set_cache_length(800)
    R = runner.bucket(n)
    runner.warm(R)
    runner.verify(sess, R); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        runner.verify(sess, R)
    g.replay(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    mean = (time.perf_counter() - t0) / reps * 1e3
    each = []                                                 # the same replays one by one: their spread is the margin between two formats
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); e1.synchronize()
        each.append(e0.elapsed_time(e1))
    return R, mean, max(each) - min(each)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--models", default="llama3-8b,qwen2.5-7b,qwen3-8b")
    ap.add_argument("--formats", default="fp16,fp8")
    a = ap.parse_args()
    for name in a.models.split(","):
        for fmt in a.formats.split(","):
            if fmt not in ("fp16", "fp8", "mxfp4", "int4g128", "int8g128"):
                raise SystemExit(f"--formats: unknown format {fmt!r} (fp16, fp8, mxfp4, int4g128, int8g128)")
            runner = LlamaRunner.random_init(MODELS[name], 2048, torch.float16, seed=0, weight_format=fmt if fmt != "fp16" else None)
            sess = samd_hip.Session(4096)
            sess.reset()
            sizes = (1, 8, 16, 32, 48, 64) + ((128,) if runner.max_draft_rows() >= 128 else ())
            runs = [step_ms(runner, sess, n, a.reps) for n in sizes]
            res = {R: round(ms, 4) for R, ms, _ in runs}
            spread = {R: round(sp, 4) for R, _, sp in runs}
            print(json.dumps(dict(model=name, format=fmt, epilogue=runner.qkv_epilogue, step_ms=res, spread_ms=spread,
                                  resident_weight_bytes=runner.memory_report()["total"])), flush=True)
            del runner, sess
            gc.collect(); torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
