"""Qwen3-MoE with MXFP4 experts (expert_format="mxfp4") on LlamaRunner against HuggingFace in fp32 on the same GPU, under replayed routing:
the machinery and the margins of test_gpu_moe_runner.py, unchanged.

The HF module's expert tensors are overwritten with dequantize(quantize(.)) first.  Quantising is idempotent on its own output, so the runner
(which quantises on load) multiplies by exactly the weights the HF modules hold: quantisation error is no part of the comparison, only the
kernels' arithmetic is.  Router, attention, dense MLP layers, embedding and lm_head are in the model dtype in both."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import samd_hip
from samd_hip import moe as MOE
from samd_hip import mxfp4 as MX
from samd_hip.llama import LlamaRunner
from test_gpu_lm_shapes import hf_low_precision_twin
from test_gpu_moe_runner import A3B, PLAN, TINY, Replay, _near_tie, compare, hf_moe
from test_moe_mxfp4_cpu import quantise_module


def requantise(lm, dtype):
    """the expert tensors of every sparse layer <- dequantize(quantize(.)), values of `dtype` held in the module's own dtype"""
    with torch.no_grad():
        for lyr in lm.model.layers:
            ex = getattr(lyr.mlp, "experts", None)
            if ex is None:
                continue
            q_gu, e8_gu, q_down, e8_down = MOE.quantize_experts(ex.gate_up_proj.to(dtype), ex.down_proj.to(dtype), dtype)
            ex.gate_up_proj.copy_(MOE.dequantize_experts(q_gu, e8_gu))
            ex.down_proj.copy_(MOE.dequantize_experts(q_down, e8_down))
    return lm


def build4(cfg_kw, seed, dtype, std=0.05):
    lm = requantise(hf_moe(cfg_kw, seed, std), dtype)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype, expert_format="mxfp4")
    assert runner.expert_format == "mxfp4" and runner.weight_format is None
    lm_low = hf_low_precision_twin(lm, dtype)
    replay = Replay(runner)
    replay.patch(lm, "fp32"), replay.patch(lm_low, "low")
    return lm, lm_low, runner, replay


def packed_bytes(s):
    E, I, H = s.n_experts, s.moe_inter, s.hidden
    return E * 2 * I * H // 2 + E * 2 * I * H // 32, E * H * I // 2 + E * H * I // 32


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("stack", ["sparse", "mixed"])
def test_tiny_qwen3_moe_with_4bit_experts_matches_hf_under_replayed_routing(dtype, stack):
    kw = dict(norm_topk_prob=True, **(dict(mlp_only_layers=[1]) if stack == "mixed" else {}))
    lm, lm_low, runner, replay = build4(kw, seed=14, dtype=dtype)
    s = runner.shape
    assert s.sparse == ([True, False, True] if stack == "mixed" else [True] * 3)
    assert runner.row_major_released and runner.max_draft_rows() == 64
    # the memory report: the bytes actually held, the format, nothing of the experts row-major
    rep = runner.memory_report()
    gu, down = packed_bytes(s)
    assert rep["expert_format"] == "mxfp4" and "weight_format" not in rep
    assert (rep["packed_moe_gu"], rep["packed_moe_down"]) == (sum(s.sparse) * gu, sum(s.sparse) * down)
    for l, lp, sp in zip(runner.w["layers"], runner.wp["layers"], s.sparse):
        if sp:
            assert all(l[k].device.type == "meta" for k in ("experts_gu", "experts_gu_scale", "experts_down", "experts_down_scale"))
            assert lp["moe_gu"].dtype == torch.uint8 and lp["moe_gu"].numel() == gu and lp["moe_down"].numel() == down
        else:
            assert lp["wgu"] is not None and lp["wgu"].dtype == dtype        # a dense layer of a mixed stack stays in the model dtype
    # a step streams the 4-bit experts: top_k of them per sparse layer at one row
    assert runner.weight_bytes() < LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype).weight_bytes()
    for prompt_len, n in PLAN:
        compare(lm, lm_low, runner, replay, prompt_len, n, TINY["vocab_size"], seed=prompt_len + n, label=f"mxfp4 experts {stack} {dtype}")


def test_a_default_runner_reports_no_expert_format_and_the_old_bytes():
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=14)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.bfloat16)
    rep = runner.memory_report()
    assert runner.expert_format is None and rep["expert_format"] is None
    assert rep["packed_moe_gu"] == 2 * rep["packed_moe_down"] == 2 * 8 * 2 * 256 * 512 * 2
    assert all(lp["moe_gu"].dtype == torch.bfloat16 for lp in runner.wp["layers"] if "moe_gu" in lp)


def test_a3b_geometry_two_layers_with_4bit_experts_matches_hf():
    lm, lm_low, runner, replay = build4(A3B, seed=3, dtype=torch.bfloat16, std=0.02)
    gu, down = packed_bytes(runner.shape)
    rep = runner.memory_report()
    assert (rep["packed_moe_gu"], rep["packed_moe_down"]) == (2 * gu, 2 * down)
    for prompt_len, n in ((70, 16), (70, 1)):
        compare(lm, lm_low, runner, replay, prompt_len, n, A3B["vocab_size"], seed=n, label="mxfp4 experts qwen3-30b-a3b")
    del runner, lm, lm_low, replay
    torch.cuda.empty_cache()


def logits_of(runner, seed=4, n=11):
    rng = np.random.default_rng(seed)
    sess = samd_hip.Session(512)
    last = runner.prefill(sess, torch.tensor([rng.integers(3, 1024, 90).tolist()], device="cuda")).clone()
    dev = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()
    sess.set_draft(dev(rng.integers(3, 1024, n).tolist()), dev([-1] + [int(rng.integers(0, i)) for i in range(1, n)]), n, type_=1)
    tree = runner.verify(sess, 16)["logits"][:n].clone()
    torch.cuda.synchronize()
    return last, tree


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_prequantised_module_gives_the_logits_of_the_quantise_on_load_runner(dtype):
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=21)
    on_load = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype, expert_format="mxfp4")
    want = logits_of(on_load)
    with torch.no_grad():                                        # (quantise the values the runner saw: the module's, rounded to the dtype)
        for lyr in lm.model.layers:
            if hasattr(lyr.mlp, "experts"):
                lyr.mlp.experts.gate_up_proj.copy_(lyr.mlp.experts.gate_up_proj.to(dtype))
                lyr.mlp.experts.down_proj.copy_(lyr.mlp.experts.down_proj.to(dtype))
    quantise_module(lm, dtype, scales_as="buffer")
    assert lm.model.layers[0].mlp.experts.gate_up_proj.dtype == torch.uint8
    imported = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype)
    assert imported.expert_format == "mxfp4" and imported.memory_report() == on_load.memory_report()
    got = logits_of(imported)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if MX._F4 is not None and MX._E8 is not None:                # the same bytes under torch's own 4-bit / e8m0 dtypes
        for lyr in lm.model.layers:
            ex = getattr(lyr.mlp, "experts", None)
            if ex is not None:
                ex.gate_up_proj = torch.nn.Parameter(ex.gate_up_proj.data.view(MX._F4), requires_grad=False)
                ex.down_proj = torch.nn.Parameter(ex.down_proj.data.view(MX._F4), requires_grad=False)
                ex.gate_up_proj_scale, ex.down_proj_scale = ex.gate_up_proj_scale.view(MX._E8), ex.down_proj_scale.view(MX._E8)
        typed = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype)
        got = logits_of(typed)
        assert typed.expert_format == "mxfp4" and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("R,n", [(16, 5), (64, 41)])
def test_graph_replay_equals_the_eager_forward_with_4bit_experts(R, n):
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=9)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.bfloat16, expert_format="mxfp4")
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


def test_random_init_takes_expert_format_and_the_rejections_hold_on_the_gpu():
    cfg = dict(TINY, model_type="qwen3_moe", decoder_sparse_step=2, norm_topk_prob=True)
    r = LlamaRunner.random_init(cfg, 256, torch.float16, expert_format="mxfp4")
    assert r.expert_format == "mxfp4" and r.wp["layers"][1]["moe_gu"].dtype == torch.uint8 and r.wp["layers"][0]["wgu"].dtype == torch.float16
    sess = samd_hip.Session(256)
    assert bool(torch.isfinite(r.prefill(sess, torch.arange(3, 103, device="cuda")[None])).all())
    with pytest.raises(samd_hip.SamdError, match="expected one of"):
        LlamaRunner.random_init(cfg, 256, torch.float16, expert_format="fp8")
    with pytest.raises(samd_hip.SamdError, match="mixture-of-experts"):         # weight_format keeps its rejection
        LlamaRunner.random_init(cfg, 256, torch.float16, expert_format="mxfp4", weight_format="mxfp4")
    dense = dict(TINY, model_type="qwen3")
    with pytest.raises(samd_hip.SamdError, match="without mixture-of-experts"):
        LlamaRunner.random_init(dense, 256, torch.float16, expert_format="mxfp4")


def test_generate_speculative_equals_autoregressive_with_4bit_experts(monkeypatch):
    """test_gpu_moe_runner's generation test with SAMD_EXPERT_FORMAT=mxfp4 (SamdModel cannot pass the argument): speculative decoding stays
    lossless against the same runner's autoregressive decoding, up to the near-tie allowance of that test"""
    import samd_sam_only as SO
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "mxfp4")
    lm = hf_moe(dict(vocab_size=512, norm_topk_prob=True, mlp_only_layers=[0]), seed=3, std=0.08).half()
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 70).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=64, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]
    assert ar._runner.expert_format == "mxfp4"
    probe = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.float16)
    assert probe.expert_format == "mxfp4"

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
    assert spec._runner.expert_format == "mxfp4"
