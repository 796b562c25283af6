"""The one-pass prefill of a mixture-of-experts runner (LlamaRunner._prefill_moe: layer-major, one wide route / lists / gate|up / down + combine
per sparse layer and super-chunk) against the chunked prefill (SAMD_PREFILL=chunked: 64 rows through all layers at a time) of the SAME runner.

Everything is compared by equality: the returned logits, session.start_token, K and V of every layer, the logits of an 8-node verify step
behind the prompt, the sequence of on_chunk calls (count, n, tokens, logits and hidden states), and the routing itself.  route_log must
hold exactly one entry per sparse layer and super-chunk with n_rows = the super-chunk's rows (one per 64-row chunk on the chunked path).

TINY geometry of tests/test_gpu_moe_runner.py (3 layers, E = 8, k = 2, stacks "sparse" and "mixed", max_cache_len 512) through random_init;
experts in the model dtype, mxfp4, int4g128 and fp8b128 (quantised on load); fp16 and bf16; prompts of 128 (the switch-over: two full
tiles), 130 and 300 tokens, 300 once more with SAMD_MOE_PREFILL_ROWS=128 (super-chunks 128 + 128 + 44).  One case at Qwen3-30B-A3B's
geometry (2 layers, E = 128, k = 8, bf16, prompt 300)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import moe as MOE
from samd_hip.llama import LlamaRunner
from test_gpu_moe_runner import A3B, TINY

T = 64
FORMATS = [None, "mxfp4", "int4g128", "fp8b128"]
# (prompt length, SAMD_MOE_PREFILL_ROWS or None)
PLAN = [(128, None), (130, None), (300, None), (300, 128)]


def start_token(sess):
    torch.cuda.synchronize()
    out = C.c_int32(-1)
    rc = C.CDLL("libamdhip64.so").hipMemcpy(C.byref(out), C.c_void_p(sess.device_views()["start_token"]), C.c_size_t(4), 2)    # device to host
    assert rc == 0
    return out.value


def run(runner, prompt, monkeypatch, mode, rows=None):
    """one prefill + one 8-node verify step on a cleared cache; everything the comparison needs, cloned"""
    monkeypatch.setenv("SAMD_PREFILL", mode)
    if rows is None:
        monkeypatch.delenv(MOE.PREFILL_ROWS_ENV, raising=False)
    else:
        monkeypatch.setenv(MOE.PREFILL_ROWS_ENV, str(rows))
    runner.kv.zero_()
    runner.route_log = []
    sess = samd_hip.Session(runner.max_len)
    calls = []
    logits = runner.prefill(sess, torch.tensor([prompt], device="cuda"),
                            lambda tok, lg, n, hid: calls.append((n, tok[:n].clone(), lg[:n].clone(), hid[:n].clone()))).clone()
    torch.cuda.synchronize()
    out = dict(logits=logits, start=start_token(sess), kv=runner.kv.clone(), calls=calls, log=runner.route_log, cache_length=sess.get_cache_length(),
               hidden=runner.hidden_rows(T).clone())
    runner.route_log = None
    rng = np.random.default_rng(len(prompt))
    dev = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()
    n = 8
    sess.set_draft(dev(rng.integers(3, 1000, n).tolist()), dev([-1] + [int(rng.integers(0, i)) for i in range(1, n)]), n, type_=1)
    out["verify"] = runner.verify(sess, runner.bucket(n))["logits"][:n].clone()
    # the same without on_chunk: only the last slice runs the head
    runner.kv.zero_()
    sess2 = samd_hip.Session(runner.max_len)
    out["logits_plain"] = runner.prefill(sess2, torch.tensor([prompt], device="cuda")).clone()
    out["start_plain"], out["kv_plain"] = start_token(sess2), runner.kv.clone()
    torch.cuda.synchronize()
    return out


def compare(runner, N, rows, monkeypatch, label):
    prompt = np.random.default_rng(N).integers(3, runner.shape.vocab, N).tolist()
    want = run(runner, prompt, monkeypatch, "chunked")
    got = run(runner, prompt, monkeypatch, "wide", rows)
    sparse = [li for li, sp in enumerate(runner.shape.sparse) if sp]
    cap = rows or MOE.WIDE_MAX_ROWS
    supers = [min(cap, N - s0) for s0 in range(0, N, cap)]
    # route_log: one entry per sparse layer and super-chunk, in the order they ran, with the super-chunk's rows
    assert [(e[0], e[1]) for e in got["log"]] == [(li, r) for r in supers for li in sparse], label
    assert [(e[0], e[1]) for e in want["log"]] == [(li, min(T, N - c0)) for c0 in range(0, N, T) for li in sparse], label
    for li in sparse:                                             # the routing itself, row by row
        for j in (2, 3):
            a, b = (torch.cat([e[j][:e[1]] for e in o["log"] if e[0] == li]) for o in (got, want))
            assert torch.equal(a, b), (label, li, "topk_idx" if j == 2 else "topk_w")
    assert got["cache_length"] == want["cache_length"] == N
    assert torch.equal(got["logits"], want["logits"]) and torch.equal(got["logits_plain"], want["logits"]), label
    assert got["start"] == want["start"] == got["start_plain"] == want["start_plain"] and 0 <= want["start"] < runner.shape.vocab, label
    assert torch.equal(got["kv"], want["kv"]) and torch.equal(got["kv_plain"], want["kv"]), label
    assert bool(want["kv"][:, :, :, :N].float().abs().sum() > 0)
    assert torch.equal(got["verify"], want["verify"]), label
    n_last = N - T * ((N - 1) // T)                               # hidden_rows(64): the last chunk's states (its real rows)
    assert torch.equal(got["hidden"][:n_last], want["hidden"][:n_last]), label
    assert len(got["calls"]) == len(want["calls"]) == -(-N // T), label
    for c, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a[0] == b[0] == min(T, N - T * c), (label, c)
        assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), (label, c, "on_chunk's tokens, logits or hidden states")


def tiny(stack, dtype, fmt, **kw):
    cfg = dict(TINY, model_type="qwen3_moe", norm_topk_prob=True, **(dict(mlp_only_layers=[1]) if stack == "mixed" else {}), **kw)
    return LlamaRunner.random_init(cfg, 512, dtype, seed=5, std=0.05, expert_format=fmt)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("stack", ["sparse", "mixed"])
def test_one_pass_prefill_equals_the_chunked_prefill(stack, fmt, dtype, monkeypatch):
    runner = tiny(stack, dtype, fmt)
    assert runner.shape.sparse == ([True, False, True] if stack == "mixed" else [True] * 3) and runner.expert_format == fmt
    for N, rows in PLAN:
        compare(runner, N, rows, monkeypatch, f"{stack} {fmt} {dtype} N={N} rows={rows}")
    assert runner.row_major_released, "no row-major copy comes back"


def test_last_layer_dense_runs_the_head_inside_the_last_stretch(monkeypatch):
    """mlp_only_layers = [2]: the stack ends in a dense MLP, whose split-K partials are folded by the final norm of the same stretch"""
    cfg = dict(TINY, model_type="qwen3_moe", norm_topk_prob=True, mlp_only_layers=[2])
    runner = LlamaRunner.random_init(cfg, 512, torch.bfloat16, seed=6, std=0.05)
    assert runner.shape.sparse == [True, True, False]
    compare(runner, 200, None, monkeypatch, "dense last layer")
    compare(runner, 200, 128, monkeypatch, "dense last layer, two super-chunks")


def test_short_prompts_and_the_chunked_mode_keep_one_entry_per_chunk(monkeypatch):
    runner = tiny("sparse", torch.bfloat16, None)
    monkeypatch.delenv("SAMD_PREFILL", raising=False)
    for N, mode in ((127, None), (300, "chunked")):
        if mode:
            monkeypatch.setenv("SAMD_PREFILL", mode)
        runner.route_log = []
        runner.prefill(samd_hip.Session(512), torch.tensor([np.random.default_rng(1).integers(3, 1000, N).tolist()], device="cuda"))
        torch.cuda.synchronize()
        assert [(e[0], e[1]) for e in runner.route_log] == [(li, min(T, N - c0)) for c0 in range(0, N, T) for li in range(3)], (N, mode)
    runner.route_log = None


def test_a_rejected_super_chunk_size_raises_before_any_launch(monkeypatch):
    runner = tiny("sparse", torch.bfloat16, None)
    monkeypatch.setenv(MOE.PREFILL_ROWS_ENV, "100")
    with pytest.raises(samd_hip.SamdError, match="multiple of 64"):
        runner.prefill(samd_hip.Session(512), torch.arange(3, 203, device="cuda")[None])


def test_a3b_geometry_two_layers(monkeypatch):
    cfg = dict(TINY, **A3B, model_type="qwen3_moe")
    runner = LlamaRunner.random_init(cfg, 512, torch.bfloat16, seed=3, std=0.02)
    assert runner.shape.n_experts == 128 and runner.shape.top_k == 8 and runner.shape.sparse == [True, True]
    compare(runner, 300, None, monkeypatch, "qwen3-30b-a3b geometry")
    del runner
    torch.cuda.empty_cache()
