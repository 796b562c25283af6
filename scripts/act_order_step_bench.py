"""act_order_step_bench.py -- what the act-order tables cost a verify step: graph-replay time of one forward at 8 and 64 rows (L = 800 cached
keys) of ONE random-init INT4 (or INT8) runner at Vicuna-7B geometry, full depth, first in plain K order and then with random permutation
tables on every layer (the two norms and the KV-split merge store through them; the weights are random either way, so the same packed
buffers serve both).  The two forms alternate --rounds times in one process; each figure is the mean of --reps replays and comes with the
spread of single replays.   usage: python scripts/act_order_step_bench.py [--format int4g128] [--model vicuna-7b] [--reps 50] [--rounds 3]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sam-decoding_amd"), os.path.join(ROOT, "scripts")]
import torch
import samd_hip
from samd_hip.llama import LlamaRunner
from qwen_step_bench import MODELS, step_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", default="int4g128", choices=("int4g128", "int8g128"))
    ap.add_argument("--model", default="vicuna-7b", choices=sorted(MODELS))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    runner = LlamaRunner.random_init(MODELS[a.model], 2048, torch.float16, seed=0, weight_format=a.format)
    s, g = runner.shape, torch.Generator().manual_seed(0)
    table = lambda n: torch.randperm(n, generator=g).to(torch.int32).cuda()
    tables = [runner._act_order_tables(dict(perm_attn=table(s.hidden), perm_o=table(s.heads * s.head_dim), perm_mlp=table(s.hidden)), li)
              for li in range(s.layers)]
    sess = samd_hip.Session(4096)
    sess.reset()
    for rnd in range(a.rounds):
        for form, perms in (("plain", [None] * s.layers), ("act-order", tables)):
            runner.perms, runner.act_order = perms, [p is not None for p in perms]
            runs = [step_ms(runner, sess, n, a.reps) for n in (8, 64)]
            print(json.dumps(dict(model=a.model, format=a.format, form=form, round=rnd, step_ms={R: round(ms, 4) for R, ms, _ in runs},
                                  spread_ms={R: round(sp, 4) for R, _, sp in runs})), flush=True)


if __name__ == "__main__":
    main()
