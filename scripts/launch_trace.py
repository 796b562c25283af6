#!/usr/bin/env python3
"""Which library calls does a forward make, and with which arguments?  A development aid for changes to the host side of the runner that
must leave every launch as it is (profiles/runner_formats.md): run it on two trees and diff the two files.

    python scripts/launch_trace.py --out trace.txt        # one line per library call of every traced forward
    python scripts/launch_trace.py --time                 # the eager 70-token chunked prefill, ms per call, three runners (one JSON line)

samd_hip.llama.lib and samd_hip.moe.lib are replaced by a recorder around the real library.  A line is the function name and its arguments:
integers and floats as they are, None as 0, a struct argument as its type name, a pointer as the index of that address's first appearance
within the forward.  torch.mm calls are outside the trace.

The model is the smallest at which the dispatch can still go wrong: hidden 256, 2 heads of 128, 2 KV heads, intermediate 256, vocab 256,
2 layers, max_cache_len 512, fp16; its mixture-of-experts variant has mlp_only_layers [0], 4 experts, top-k 2, moe_intermediate_size 256
(layer 0 dense, layer 1 sparse).  Runners (random_init): the model dtype with SAMD_QKV_FUSED=force (so that the norm-fold form exists),
every weight_format, every expert_format including None.  Forwards: the second call of forward_rows at buckets 1, 8, 32 and 64, a 70-token
chunked prefill, and the one-pass prefill at 256 tokens (dense) or 128 tokens (mixture of experts)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sam-decoding_amd"))

import torch  # noqa: E402

import samd_hip  # noqa: E402
from samd_hip import llama as LL, moe as MOE  # noqa: E402

DENSE_CFG = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, head_dim=128, intermediate_size=256, vocab_size=256,
                 num_hidden_layers=2, max_position_embeddings=512, rms_norm_eps=1e-6)
MOE_CFG = dict(DENSE_CFG, model_type="qwen3_moe", mlp_only_layers=[0], num_experts=4, num_experts_per_tok=2, moe_intermediate_size=256,
               norm_topk_prob=True, decoder_sparse_step=1)
MAX_LEN = 512


class Recorder:
    """the library, with every call written down while `lines` is a list"""

    def __init__(self, real):
        self._real, self.lines, self._seen = real, None, {}

    def start(self):
        self.lines, self._seen = [], {}

    def stop(self):
        lines, self.lines = self.lines, None
        return lines

    def _arg(self, a):
        if a is None:
            return "0"
        if isinstance(a, (int, float)):
            return repr(a)
        if isinstance(a, C.c_void_p):
            return "0" if not a.value else f"p{self._seen.setdefault(a.value, len(self._seen))}"
        if hasattr(a, "_obj"):                                   # ctypes.byref(struct)
            return type(a._obj).__name__
        return type(a).__name__

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            if self.lines is not None:
                self.lines.append(" ".join([name] + [self._arg(a) for a in args]))
            return fn(*args)
        return call


def runners():
    """(label, constructor): built one at a time, so that only one runner's buffers live"""
    def model_dtype():
        os.environ["SAMD_QKV_FUSED"] = "force"                   # (read at construction only)
        try:
            return LL.LlamaRunner.random_init(DENSE_CFG, MAX_LEN, torch.float16)
        finally:
            del os.environ["SAMD_QKV_FUSED"]
    yield "dense/model-dtype", model_dtype
    for fmt in LL.QUANT_FORMATS:
        yield f"dense/{fmt}", lambda fmt=fmt: LL.LlamaRunner.random_init(DENSE_CFG, MAX_LEN, torch.float16, weight_format=fmt)
    for fmt in MOE.EXPERT_FORMATS_SERVED:
        yield f"moe/{fmt}", lambda fmt=fmt: LL.LlamaRunner.random_init(MOE_CFG, MAX_LEN, torch.float16, expert_format=fmt)


def prompt(n):
    return (torch.arange(n, dtype=torch.int64) * 7 + 3) % DENSE_CFG["vocab_size"]


def trace(out_path):
    rec = Recorder(samd_hip.lib())
    LL.lib = MOE.lib = lambda: rec
    out = []
    for label, make in runners():
        runner = make()
        session = samd_hip.Session(MAX_LEN)
        scratch_L = torch.zeros(1, dtype=torch.int32, device=runner.device)
        for R in (1, 8, 32, 64):
            runner.pf_n.fill_(R)
            for traced in (False, True):
                if traced:
                    rec.start()
                runner.forward_rows(R, runner.pf_tokens, runner.pf_relpos, runner.pf_mask, scratch_L, runner.pf_n)
            out += [f"== {label} forward_rows {R}"] + rec.stop()
        for n in (70, 128 if runner.shape.moe else 256):
            rec.start()
            runner.prefill(session, prompt(n))
            out += [f"== {label} prefill {n}"] + rec.stop()
        torch.cuda.synchronize()
        del runner, session
    with open(out_path, "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"{len(out)} lines -> {out_path}")


def timing(calls=50, warmup=5):
    res = {}
    for label, make in runners():
        if label not in ("dense/model-dtype", "dense/int4g128", "moe/int8g128"):
            continue
        runner, ids = make(), prompt(70)
        session = samd_hip.Session(MAX_LEN)
        for _ in range(warmup):
            runner.prefill(session, ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            runner.prefill(session, ids)
        torch.cuda.synchronize()
        res[label] = round((time.perf_counter() - t0) * 1e3 / calls, 4)
        del runner, session
    print(json.dumps(dict(prefill70_ms=res)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="launch_trace.txt")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    timing() if a.time else trace(a.out)
