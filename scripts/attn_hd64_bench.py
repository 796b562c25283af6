"""attn_hd64_bench.py -- samd_tree_attention (split launch + merge) per call, 32 query / 8 KV heads, fp16, row-major cache: head_dim 64
(k_tree_attention_gqa64) beside head_dim 128 (k_tree_attention) in the same process, alternating, three repeats.  32 calls on 32 layers'
caches in one hipGraph, 50 replays per measurement (device events); the table of profiles/attention_hd64.md.
usage: python scripts/attn_hd64_bench.py"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sam-decoding_amd")]
import torch
import samd_hip
from samd_hip import _ptr, check, current_stream, lib
from bench import hip_time_ms

H, Hkv, layers, max_len = 32, 8, 32, 4096
Lib = lib()


def make(D, R, L0):
    n = R - 3
    kv = torch.randn((layers, 2, Hkv, max_len, D), device="cuda").half()
    q = torch.randn((R, H, D), device="cuda").half()
    out = torch.zeros((R, H, D), device="cuda", dtype=torch.float16)
    mask = torch.tensor([(1 << (i + 1)) - 1 if i < 63 else -1 for i in range(64)], dtype=torch.int64, device="cuda")
    d_L = torch.tensor([L0], dtype=torch.int32, device="cuda")
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    ws = torch.zeros(Lib.samd_tree_attention_workspace(R, H, D), dtype=torch.uint8, device="cuda")
    keep = (kv, q, out, mask, d_L, d_n, ws)

    def fn():
        st = current_stream()
        for li in range(layers):
            check(Lib.samd_tree_attention(_ptr(q), _ptr(kv[li, 0]), _ptr(kv[li, 1]), _ptr(out), samd_hip.F16, R, H, Hkv, D, max_len, _ptr(mask),
                                          _ptr(d_L), _ptr(d_n), 1.0 / math.sqrt(D), _ptr(ws), ws.numel(), st))
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g, keep


for L0 in (512, 2048):
    for R in (8, 16, 64):
        graphs = {D: make(D, R, L0) for D in (64, 128)}
        times = {64: [], 128: []}
        for rep in range(3):
            for D in (64, 128):
                times[D].append(hip_time_ms(graphs[D][0].replay, 50) * 1e3 / layers)
        print(f"R={R} n={R - 3} L={L0}: " + "  ".join(f"D={D} " + "/".join(f"{t:.2f}" for t in times[D]) + " us" for D in (64, 128)), flush=True)
