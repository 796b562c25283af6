#!/usr/bin/env python3
"""What does LlamaRunner.from_hf answer for every module the CPU tests hand it?  A development aid for changes to the checkpoint import
(samd_hip/hf_import.py) that must leave every acceptance, refusal and imported tensor as it is (profiles/hf_import.md): run it on two trees
and compare the files.  The sibling of scripts/launch_trace.py, and like it without a GPU.

    python scripts/import_trace.py --out trace.txt                   # run the CPU tests below in-process, one record per from_hf call
    python scripts/import_trace.py --check PARENT PARENT2 THIS       # the three conditions below, over three such files
    python scripts/import_trace.py --time                            # from_hf up to the constructor, ms per call, two modules (one JSON line)

The tests run through pytest.main with a plugin of this script (no conftest, no setting changes); LlamaRunner.from_hf and
LlamaRunner.__init__ are wrapped.  A record is: the test's node id; every positional and keyword argument as its repr (object addresses
blanked); if the call raises, the exception's class and its message in full; if the constructor is reached, its arguments (the shape as
its fields) and, for every tensor of the weights dict, key path, dtype, shape, device type and the SHA-256 of its bytes (`meta` for a meta
tensor).  The plugin seeds torch, numpy and random before every test, so that modules built without a seed are the same in every run.  The
file ends with the counts: tests by outcome, from_hf calls, constructor entries.

--check states what "the same answer for every input we have" means, and exits non-zero unless all of it holds:
  1. PARENT and PARENT2, two runs of the parent commit, are equal: the trace is reproducible.  (If they are not, something unseeded
     reaches from_hf: seed it in the plugin here, not in a conftest.)
  2. THIS holds at least as many from_hf calls and constructor entries as PARENT: a tree that reaches fewer is not compared.
  3. PARENT and THIS are equal: calls, their order, messages in full, keys, dtypes, shapes and hashes.

--time builds two modules from the tests' own helpers -- the 4-layer Qwen3-MoE module of test_moe_cpu.qwen3_moe(mlp_only_layers=[1]) as an
INT4 checkpoint with INT4 attention (test_moe_int4_cpu.to_int4_moe_checkpoint, gptq_v2, bf16), and the same architecture with every layer
dense and all seven projections 8-bit GPTQ modules (test_moe_int8_cpu.to_int8_moe_checkpoint) -- and times from_hf(..., device="cpu") up to
the constructor's first statement: one untimed call, then the mean of --calls calls."""
import argparse
import hashlib
import inspect
import json
import os
import random
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "sam-decoding_amd"), ROOT):
    sys.path.insert(0, p)

TESTS = ("test_moe_cpu.py", "test_moe_fp8_cpu.py", "test_moe_int4_cpu.py", "test_moe_int8_cpu.py", "test_moe_mxfp4_cpu.py", "test_qwen_cpu.py",
         "test_fp8b128_cpu.py", "test_formats_cpu.py", "test_fp8_weights_cpu.py", "test_int4_weights_cpu.py", "test_int8_weights_cpu.py",
         "test_mxfp4_weights_cpu.py", "test_eagle2_cpu.py")
COUNTS = re.compile(r"^# from_hf calls (\d+), constructor entries (\d+)$", re.M)


def _text(x):
    return re.sub(r" at 0x[0-9a-f]+", " at 0x", repr(x)).replace("\n", "\\n")


def _tensors(x, path=""):
    """(key path, tensor) of every tensor inside nested dicts / lists / tuples, in the containers' own order"""
    import torch
    if isinstance(x, torch.Tensor):
        yield path, x
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _tensors(v, f"{path}.{k}" if path else str(k))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _tensors(v, f"{path}.{i}" if path else str(i))


def _digest(t):
    import torch
    if t.device.type == "meta":
        return "meta"
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


class Tracer:
    """the pytest plugin and the two wrappers"""

    def __init__(self):
        self.lines, self.node, self.depth = [], "<collection>", 0
        self.calls = self.ctors = 0
        self.outcomes = {}

    def pytest_runtest_setup(self, item):
        import numpy
        import torch
        self.node = item.nodeid
        torch.manual_seed(0)
        numpy.random.seed(0)
        random.seed(0)

    def pytest_runtest_logreport(self, report):
        if report.when == "call" or report.outcome != "passed":
            self.outcomes[report.outcome] = self.outcomes.get(report.outcome, 0) + 1

    def install(self):
        from samd_hip.llama import LlamaRunner
        from_hf, init = LlamaRunner.__dict__["from_hf"].__func__, LlamaRunner.__init__
        sig = inspect.signature(init)
        tr = self

        def traced_from_hf(cls, *a, **kw):
            tr.calls += 1
            tr.lines.append(f"from_hf {tr.node}")
            tr.lines += [f"  arg {_text(x)}" for x in a] + [f"  kw {k}={_text(v)}" for k, v in kw.items()]
            tr.depth += 1
            try:
                runner = from_hf(cls, *a, **kw)
            except BaseException as e:
                tr.lines.append(f"  raises {type(e).__module__}.{type(e).__qualname__}: " + str(e).replace("\n", "\\n"))
                raise
            finally:
                tr.depth -= 1
            tr.lines.append(f"  returns {type(runner).__name__}")
            return runner

        def traced_init(self, *a, **kw):
            if tr.depth:
                tr.ctors += 1
                got = sig.bind(self, *a, **kw).arguments
                tr.lines.append("  constructor")
                for k, v in got.items():
                    if k == "shape":
                        tr.lines.append(f"    shape {_text(sorted(vars(v).items()))}")
                    elif k == "kw" or k == "kwargs":
                        tr.lines += [f"    {kk}={_text(vv)}" for kk, vv in v.items()]
                    elif k not in ("self", "weights"):
                        tr.lines.append(f"    {k}={_text(v)}")
                for path, t in _tensors(got["weights"]):
                    tr.lines.append(f"    {path} {t.dtype} {tuple(t.shape)} {t.device.type} {_digest(t)}")
            return init(self, *a, **kw)
        LlamaRunner.from_hf, LlamaRunner.__init__ = classmethod(traced_from_hf), traced_init


def trace(out_path):
    import pytest
    tr = Tracer()
    tr.install()
    os.chdir(ROOT)
    rc = pytest.main(["-q", "-p", "no:cacheprovider", "--rootdir", ROOT] + [os.path.join("tests", t) for t in TESTS], plugins=[tr])
    tr.lines.append("# tests " + ", ".join(f"{k} {v}" for k, v in sorted(tr.outcomes.items())))
    tr.lines.append(f"# from_hf calls {tr.calls}, constructor entries {tr.ctors}")
    with open(out_path, "w") as f:
        f.write("\n".join(tr.lines) + "\n")
    print(f"{len(tr.lines)} lines, {tr.calls} from_hf calls, {tr.ctors} constructor entries, tests {tr.outcomes} -> {out_path}")
    return int(rc)


def check(parent, parent2, this):
    text = {p: open(p).read() for p in (parent, parent2, this)}
    counts = {p: tuple(int(x) for x in COUNTS.search(text[p]).groups()) for p in text}
    print(f"parent: {counts[parent][0]} from_hf calls, {counts[parent][1]} constructor entries; this tree: {counts[this][0]}, {counts[this][1]}")
    if text[parent] != text[parent2]:
        print("FAIL 1: two runs of the parent differ -- the trace is not reproducible; seed what differs in this script's plugin")
        return 1
    if counts[this][0] < counts[parent][0] or counts[this][1] < counts[parent][1]:
        print("FAIL 2: this tree reaches fewer from_hf calls or constructor entries than the parent; not compared")
        return 1
    if text[parent] != text[this]:
        a, b = text[parent].split("\n"), text[this].split("\n")
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"FAIL 3: parent and this tree differ, first at line {first + 1}:\n  parent: {a[first][:300] if first < len(a) else '<end>'}\n"
              f"  this:   {b[first][:300] if first < len(b) else '<end>'}")
        return 1
    print(f"ok: parent == parent2 == this tree, {len(text[parent].splitlines())} lines")
    return 0


def timing(calls):
    import torch
    from samd_hip.llama import LlamaRunner
    from test_moe_cpu import qwen3_moe
    from test_moe_int4_cpu import to_int4_moe_checkpoint
    from test_moe_int8_cpu import to_int8_moe_checkpoint

    class Reached(Exception):
        pass

    def stop(self, *a, **kw):
        raise Reached
    LlamaRunner.__init__ = stop
    torch.manual_seed(0)
    modules = {"moe/int4g128 experts + attention": to_int4_moe_checkpoint(qwen3_moe(mlp_only_layers=[1])[1], torch.bfloat16, "gptq_v2", attention=True),
               "dense/int8g128": to_int8_moe_checkpoint(qwen3_moe(mlp_only_layers=[0, 1, 2, 3])[1], torch.bfloat16, v2=True, attention=True)}
    res = {}
    for label, ck in modules.items():
        for i in range(calls + 1):
            if i == 1:
                t0 = time.perf_counter()
            try:
                LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
            except Reached:
                continue
            raise SystemExit(f"{label}: from_hf returned without reaching the constructor")
        res[label] = round((time.perf_counter() - t0) * 1e3 / calls, 2)
    print(json.dumps(dict(from_hf_to_constructor_ms=res)))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="import_trace.txt")
    ap.add_argument("--check", nargs=3, metavar=("PARENT", "PARENT2", "THIS"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    sys.exit(check(*a.check) if a.check else timing(a.calls) if a.time else trace(a.out))
