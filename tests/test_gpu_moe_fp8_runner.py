"""Qwen3-MoE with block-scaled FP8 experts (expert_format="fp8b128") on LlamaRunner against HuggingFace in fp32 on the same GPU, under
replayed routing: the machinery and the margins of test_gpu_moe_runner.py, unchanged.

The runner is built first and quantises the module's expert tensors on load; the HF module's expert tensors are then overwritten with
dequantize_blocks(quantize_blocks(.)) of the same values -- one (q, s) on both sides, nothing is quantised twice.  Quantisation error is
then no part of the comparison, only the kernels' arithmetic is.  Router, attention, dense MLP layers, embedding and lm_head are in the model
dtype in both.  A block-scaled FP8 checkpoint -- transformers' fused FP8Experts or per-expert FP8Linear modules -- must give the bits of the
quantise-on-load runner, and one whose attention is block-scaled FP8 too the bits of the same module with its attention dequantised by hand."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import samd_hip
from samd_hip import fp8 as F8
from samd_hip import moe as MOE
from samd_hip.llama import LlamaRunner
from test_gpu_lm_shapes import hf_low_precision_twin
from test_gpu_moe_mxfp4_runner import logits_of
from test_gpu_moe_runner import A3B, PLAN, TINY, Replay, _near_tie, compare, hf_moe
from test_moe_fp8_cpu import ATTN, PROJ, to_fp8_moe_checkpoint

KEYS = ("experts_gu", "experts_gu_sinv", "experts_down", "experts_down_sinv")
FMT = "fp8b128"


def packed_bytes(s):
    return s.n_experts * F8.packed_block_bytes(2 * s.moe_inter, s.hidden), s.n_experts * F8.packed_block_bytes(s.hidden, s.moe_inter)


def requantise(lm, dtype):
    """the expert tensors of every sparse layer <- dequantize(quantize(.)) of the values a `dtype` runner saw, held in the module's own dtype"""
    with torch.no_grad():
        for lyr in lm.model.layers:
            ex = getattr(lyr.mlp, "experts", None)
            if ex is None:
                continue
            gu, dn = MOE.quantize_experts_fp8(ex.gate_up_proj.to(dtype), ex.down_proj.to(dtype))
            ex.gate_up_proj.copy_(MOE.dequantize_experts_fp8(*gu))
            ex.down_proj.copy_(MOE.dequantize_experts_fp8(*dn))
    return lm


def build8(cfg_kw, seed, dtype, std=0.05):
    lm = hf_moe(cfg_kw, seed, std)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype, expert_format=FMT)      # quantises the module's own values ...
    assert runner.expert_format == FMT and runner.weight_format is None
    requantise(lm, dtype)                                        # ... which the module then holds dequantised: one (q, s) on both sides
    lm_low = hf_low_precision_twin(lm, dtype)
    replay = Replay(runner)
    replay.patch(lm, "fp32"), replay.patch(lm_low, "low")
    return lm, lm_low, runner, replay


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("stack", ["sparse", "mixed"])
def test_tiny_qwen3_moe_with_fp8_experts_matches_hf_under_replayed_routing(dtype, stack):
    kw = dict(norm_topk_prob=True, **(dict(mlp_only_layers=[1]) if stack == "mixed" else {}))
    lm, lm_low, runner, replay = build8(kw, seed=14, dtype=dtype)
    s = runner.shape
    assert s.sparse == ([True, False, True] if stack == "mixed" else [True] * 3)
    assert runner.row_major_released and runner.max_draft_rows() == 64
    # the memory report: the bytes actually held, the format, nothing of the experts row-major
    rep = runner.memory_report()
    gu, down = packed_bytes(s)
    assert rep["expert_format"] == FMT and "weight_format" not in rep
    assert (rep["packed_moe_gu"], rep["packed_moe_down"]) == (sum(s.sparse) * gu, sum(s.sparse) * down)
    for l, lp, sp in zip(runner.w["layers"], runner.wp["layers"], s.sparse):
        if sp:
            assert all(l[k].device.type == "meta" for k in KEYS)
            assert l["experts_gu"].dtype == torch.float8_e4m3fn and tuple(l["experts_gu_sinv"].shape) == (s.n_experts, 2 * s.moe_inter // 128, s.hidden // 128)
            assert lp["moe_gu"].dtype == torch.uint8 and lp["moe_gu"].numel() == gu and lp["moe_down"].numel() == down
        else:
            assert lp["wgu"] is not None and lp["wgu"].dtype == dtype        # a dense layer of a mixed stack stays in the model dtype
    plain = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype)
    plain_rep = plain.memory_report()
    assert runner.weight_bytes() < plain.weight_bytes() and rep["total"] < plain_rep["total"]
    assert 0.50 < rep["packed_moe_gu"] / plain_rep["packed_moe_gu"] < 0.51           # 8 bits + 4 bytes per (64, 128) instead of 16 bits
    # one expert more: its codes and its block scales, in the format's own bytes
    per_expert = 3 * s.hidden * s.moe_inter + 3 * (s.hidden // 128) * (s.moe_inter // 128) * 4
    assert runner.weight_bytes(experts=3) - runner.weight_bytes(experts=2) == sum(s.sparse) * per_expert
    del plain
    for prompt_len, n in PLAN:
        compare(lm, lm_low, runner, replay, prompt_len, n, TINY["vocab_size"], seed=prompt_len + n, label=f"fp8 experts {stack} {dtype}")


def test_a3b_geometry_two_layers_with_fp8_experts_matches_hf():
    lm, lm_low, runner, replay = build8(A3B, seed=3, dtype=torch.bfloat16, std=0.02)
    gu, down = packed_bytes(runner.shape)
    rep = runner.memory_report()
    assert (rep["packed_moe_gu"], rep["packed_moe_down"]) == (2 * gu, 2 * down)
    for prompt_len, n in ((70, 16), (70, 1)):
        compare(lm, lm_low, runner, replay, prompt_len, n, A3B["vocab_size"], seed=n, label="fp8 experts qwen3-30b-a3b")
    del runner, lm, lm_low, replay
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype,form", [(torch.float16, "per_expert"), (torch.bfloat16, "fused")])
def test_a_prequantised_module_gives_the_logits_of_the_quantise_on_load_runner(dtype, form):
    """transformers' FP8Experts, or per-expert FP8Linear modules (mlp.experts.{e}.gate_proj.weight + weight_scale_inv), quantised from the
    values the on-load runner saw: loaded with NO extra argument, the same packed experts, so the same bits at prefill and on an 11-node
    tree at 16 rows"""
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=21)
    on_load = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype, expert_format=FMT)
    want = logits_of(on_load)
    ck = to_fp8_moe_checkpoint(lm, dtype, form)
    ex = ck.model.layers[0].mlp.experts
    if form == "fused":
        assert type(ex).__name__ == "FP8Experts" and ex.gate_up_proj.dtype == torch.float8_e4m3fn and ex.gate_up_proj_scale_inv.dtype == torch.float32
    else:
        assert not hasattr(ex, "gate_up_proj") and ex[0].gate_proj.weight.dtype == torch.float8_e4m3fn
    imported = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert imported.expert_format == FMT and imported.weight_format is None
    assert imported.memory_report() == on_load.memory_report()
    for lp, lq in zip(imported.wp["layers"], on_load.wp["layers"]):
        if "moe_gu" in lp:
            assert torch.equal(lp["moe_gu"], lq["moe_gu"]) and torch.equal(lp["moe_down"], lq["moe_down"])
    got = logits_of(imported)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(samd_hip.SamdError, match="block-scaled FP8 expert tensors"):
        LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype, expert_format="mxfp4")


def test_fp8_attention_of_a_moe_module_equals_the_same_attention_dequantised_by_hand():
    """the block-scaled FP8 attention and dense-MLP projections of a module with FP8 experts are dequantised once at import: the logits are
    those of the same module with these projections replaced by plain Linears holding rne_dtype(fl32(float(q) * s))"""
    dtype = torch.bfloat16
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=22)
    ck = to_fp8_moe_checkpoint(lm, dtype, "fused", attention=True)
    assert ck.model.layers[1].mlp.gate_proj.weight.dtype == torch.float8_e4m3fn and ck.model.layers[0].self_attn.q_proj.weight_scale_inv.dim() == 2
    runner = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert runner.expert_format == FMT and runner.weight_format is None
    assert all(lp["wo"] is not None and lp["wo"].dtype == dtype for lp in runner.wp["layers"])
    hand = copy.deepcopy(ck)
    for lyr in hand.model.layers:
        where = [(lyr.self_attn, p) for p in ATTN] + [(lyr.mlp, p) for p in PROJ if hasattr(lyr.mlp, p)]
        for own, p in where:
            mod = getattr(own, p)
            q, s = mod.weight.detach(), mod.weight_scale_inv.detach()
            w = (q.float() * s.repeat_interleave(128, 0).repeat_interleave(128, 1)).to(dtype)
            lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False)
            lin.weight = torch.nn.Parameter(w.float(), requires_grad=False)
            setattr(own, p, lin)
    by_hand = LlamaRunner.from_hf(hand, max_cache_len=512, dtype=dtype)
    assert by_hand.expert_format == FMT
    want, got = logits_of(by_hand), logits_of(runner)
    assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert runner.memory_report() == by_hand.memory_report()


@pytest.mark.parametrize("R,n", [(16, 5), (64, 41)])
def test_graph_replay_equals_the_eager_forward_with_fp8_experts(R, n):
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=9)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.bfloat16, expert_format=FMT)
    rng = np.random.default_rng(4)
    sess = samd_hip.Session(512)
    runner.prefill(sess, torch.tensor([rng.integers(3, 1024, 90).tolist()], device="cuda"))
    dev = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()
    sess.set_draft(dev(rng.integers(3, 1024, n).tolist()), dev([-1] + [int(rng.integers(0, i)) for i in range(1, n)]), n, type_=1)
    eager = runner.verify(sess, R)["logits"][:n].clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eager).all()) and bool(eager.abs().max() > 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        runner.verify(sess, R)
    runner._buffers(R)["logits"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(runner._buffers(R)["logits"][:n], eager)


def test_random_init_takes_fp8b128_and_the_rejections_hold_on_the_gpu():
    cfg = dict(TINY, model_type="qwen3_moe", decoder_sparse_step=2, norm_topk_prob=True)
    r = LlamaRunner.random_init(cfg, 256, torch.float16, expert_format=FMT)
    assert r.expert_format == FMT and r.wp["layers"][1]["moe_gu"].dtype == torch.uint8 and r.wp["layers"][0]["wgu"].dtype == torch.float16
    sess = samd_hip.Session(256)
    assert bool(torch.isfinite(r.prefill(sess, torch.arange(3, 103, device="cuda")[None])).all())
    with pytest.raises(samd_hip.SamdError, match="mixture-of-experts"):         # weight_format keeps its rejection
        LlamaRunner.random_init(cfg, 256, torch.float16, expert_format=FMT, weight_format="fp8")
    with pytest.raises(samd_hip.SamdError, match="without mixture-of-experts"):
        LlamaRunner.random_init(dict(TINY, model_type="qwen3"), 256, torch.float16, expert_format=FMT)
    with pytest.raises(samd_hip.SamdError, match="expected one of"):
        LlamaRunner.random_init(cfg, 256, torch.float16, expert_format="fp8")


def test_generate_speculative_equals_autoregressive_with_fp8_experts(monkeypatch):
    """test_gpu_moe_runner's generation test with SAMD_EXPERT_FORMAT=fp8b128 (SamdModel cannot pass the argument), 96 new tokens:
    speculative decoding stays lossless against the same runner's autoregressive decoding, up to the near-tie allowance of that test; with
    graphs (the hipGraph path) and without"""
    import samd_sam_only as SO
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", FMT)
    lm = hf_moe(dict(vocab_size=512, norm_topk_prob=True, mlp_only_layers=[0]), seed=3, std=0.08).half()
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 70).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=96, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]
    assert ar._runner.expert_format == FMT
    probe = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.float16)
    assert probe.expert_format == FMT

    def same(seq, after=8):
        m = min(len(seq), len(seq_ar))
        diff = [i for i in range(m) if seq[i] != seq_ar[i]]
        assert not diff or (diff[0] > len(prompt) + after and _near_tie(probe, seq[:diff[0]], seq[diff[0]], seq_ar[diff[0]])), diff[:3]
    docs = [seq_ar[len(prompt):]] + [rng.integers(3, 512, 50).tolist() for _ in range(4)] + [[i] for i in range(512)]
    cfg = SO.SamdConfig(max_predicts=16, alpha=4.0, len_bias=0)
    spec = SO.SamdModel(cfg, lm, SO.DraftModel(cfg, sam_static=SO.build_sam(docs, 2), device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    for use_graphs in (True, False):
        spec.set_cache(gcfg)
        spec.engine.use_graphs = use_graphs
        out = spec.generate(ids, generation_config=gcfg)
        assert out.decode_steps < out.decode_tokens, "drafts were never accepted"
        same(out.output_ids[0])
    assert spec._runner.expert_format == FMT
