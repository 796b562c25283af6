"""Qwen3-MoE with INT8 (GPTQ) experts (expert_format="int8g128") on LlamaRunner against HuggingFace in fp32 on the same GPU, under replayed
routing: the machinery and the margins of test_gpu_moe_runner.py, unchanged (test_gpu_moe_int4_runner.py carried over).

The checkpoint under test is a GPTQ-Int8 mixture-of-experts module (tests/test_moe_int8_cpu.py: per-expert 8-bit GPTQ modules, 8-bit attention
and dense-layer MLP projections too), loaded with no argument.  Its HF twin holds dequantize(.) of the SAME (q, z, s) -- the experts' and
the other projections' -- so one (q, z, s) is shared between runner and twin, quantisation error is no part of the comparison and only the
kernels' arithmetic is.  Quantise-on-load, the environment variable, generation with drafts, the one-pass prefill and the memory report
follow."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import samd_hip
from samd_hip import int8 as I8
from samd_hip import moe as MOE
from samd_hip.llama import LlamaRunner
from test_gpu_lm_shapes import hf_low_precision_twin
from test_gpu_moe_mxfp4_runner import logits_of
from test_gpu_moe_prefill import compare as prefill_compare
from test_gpu_moe_runner import PLAN, TINY, Replay, _near_tie, compare, hf_moe
from test_moe_int8_cpu import ATTN, DKEYS, GKEYS, to_int8_moe_checkpoint


def packed_bytes(s):
    E, I, H = s.n_experts, s.moe_inter, s.hidden
    return E * 2 * I * H * 33 // 32, E * H * I * 33 // 32


def dequantised_twin(lm, ck, dtype):
    """`lm` (fp32, fused experts) with every weight the checkpoint `ck` quantised replaced by rne_dtype((q - z) * s) of ck's own (q, z, s),
    s rounded once to `dtype`: what the runner built from ck multiplies by"""
    qcfg = ck.config.quantization_config

    def deq(mod, name):
        q, z, s = I8.linear_int8(mod, name, config=qcfg)
        return I8.dequantize_groups(q, z, I8.as_scales(s, dtype, name))
    twin = copy.deepcopy(lm)
    with torch.no_grad():
        for tl, cl in zip(twin.model.layers, ck.model.layers):
            for p in ATTN:
                if I8.is_int8_module(getattr(cl.self_attn, p), qcfg):
                    getattr(tl.self_attn, p).weight.copy_(deq(getattr(cl.self_attn, p), p))
            ex = getattr(tl.mlp, "experts", None)
            if ex is None:
                for p in MOE.INT4_EXPERT_PROJECTIONS:
                    if I8.is_int8_module(getattr(cl.mlp, p), qcfg):
                        getattr(tl.mlp, p).weight.copy_(deq(getattr(cl.mlp, p), p))
                continue
            for e in range(len(cl.mlp.experts)):
                g, u, d = (deq(getattr(cl.mlp.experts[e], p), p) for p in MOE.INT4_EXPERT_PROJECTIONS)
                ex.gate_up_proj[e].copy_(torch.cat([g, u]))
                ex.down_proj[e].copy_(d)
    return twin


def build8(cfg_kw, seed, dtype, std=0.05, v2=True):
    lm = hf_moe(cfg_kw, seed, std)
    ck = to_int8_moe_checkpoint(lm, dtype, v2=v2, attention=True)
    runner = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)         # no argument: the module's 8-bit experts decide
    assert runner.expert_format == "int8g128" and runner.weight_format is None
    twin = dequantised_twin(lm, ck, dtype)
    lm_low = hf_low_precision_twin(twin, dtype)
    replay = Replay(runner)
    replay.patch(twin, "fp32"), replay.patch(lm_low, "low")
    return twin, lm_low, runner, replay, ck


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("stack", ["sparse", "mixed"])
def test_a_gptq_int8_moe_module_loads_by_itself_and_matches_hf_under_replayed_routing(dtype, stack):
    kw = dict(norm_topk_prob=True, **(dict(mlp_only_layers=[1]) if stack == "mixed" else {}))
    lm, lm_low, runner, replay, ck = build8(kw, seed=14, dtype=dtype, v2=stack == "mixed")
    s = runner.shape
    assert s.sparse == ([True, False, True] if stack == "mixed" else [True] * 3)
    assert runner.row_major_released and runner.max_draft_rows() == 64
    # the memory report: the bytes actually held (E N K 33 / 32), the format, nothing of the experts row-major
    rep = runner.memory_report()
    gu, down = packed_bytes(s)
    assert (gu, down) == (s.n_experts * I8.packed_bytes(2 * s.moe_inter, s.hidden), s.n_experts * I8.packed_bytes(s.hidden, s.moe_inter))
    assert rep["expert_format"] == "int8g128" and "weight_format" not in rep
    assert (rep["packed_moe_gu"], rep["packed_moe_down"]) == (sum(s.sparse) * gu, sum(s.sparse) * down)
    for l, lp, sp in zip(runner.w["layers"], runner.wp["layers"], s.sparse):
        if sp:
            assert all(l[k].device.type == "meta" for k in GKEYS + DKEYS)
            assert lp["moe_gu"].dtype == torch.uint8 and lp["moe_gu"].numel() == gu and lp["moe_down"].numel() == down
            assert lp["moe_gu"].expert_format == lp["moe_down"].expert_format == "int8g128"
        else:
            assert lp["wgu"] is not None and lp["wgu"].dtype == dtype        # a dense layer's 8-bit MLP: dequantised at import, model dtype
        assert lp["wo"] is not None and lp["wo"].dtype == dtype              # and so is the 8-bit attention
    plain = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype, expert_format=None)
    n_sparse = sum(s.sparse)
    # weight_bytes counts the packed bytes: top_k of E experts per sparse layer at 33 / 32 bytes per weight instead of 2
    per_expert = 3 * s.hidden * s.moe_inter
    assert plain.weight_bytes() - runner.weight_bytes() == n_sparse * s.top_k * (per_expert * 2 - per_expert * 33 // 32)
    assert rep["total"] < plain.memory_report()["total"]
    del plain
    for prompt_len, n in PLAN:
        compare(lm, lm_low, runner, replay, prompt_len, n, TINY["vocab_size"], seed=prompt_len + n, label=f"int8 experts {stack} {dtype}")


@pytest.mark.parametrize("dtype,v2", [(torch.float16, False), (torch.bfloat16, True)])
def test_the_checkpoint_gives_the_bits_of_the_quantise_on_load_runner(dtype, v2):
    """per-expert 8-bit GPTQ modules quantised from the values the on-load runner saw ("gptq" and "gptq_v2" zero points): the same packed
    experts, so the same bits at prefill and on an 11-node tree at 16 rows; expert_format="int8g128" on a plain module is that runner"""
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=21)
    on_load = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype, expert_format="int8g128")
    assert on_load.expert_format == "int8g128" and on_load.weight_format is None
    want = logits_of(on_load)
    ck = to_int8_moe_checkpoint(lm, dtype, v2=v2)
    assert not hasattr(ck.model.layers[0].mlp.experts, "gate_up_proj") and ck.model.layers[0].mlp.experts[0].gate_proj.qweight.dtype == torch.int32
    imported = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert imported.expert_format == "int8g128" and imported.weight_format is None
    assert imported.memory_report() == on_load.memory_report() and imported.weight_bytes() == on_load.weight_bytes()
    for lp, lq in zip(imported.wp["layers"], on_load.wp["layers"]):
        if "moe_gu" in lp:
            assert torch.equal(lp["moe_gu"], lq["moe_gu"]) and torch.equal(lp["moe_down"], lq["moe_down"])
    got = logits_of(imported)
    assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for explicit in (None, "int4g128"):
        with pytest.raises(samd_hip.SamdError, match="INT8 .* expert tensors"):
            LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype, expert_format=explicit)


def test_random_init_and_the_constructor_take_int8g128_and_the_rejections_hold_on_the_gpu():
    cfg = dict(TINY, model_type="qwen3_moe", decoder_sparse_step=2, norm_topk_prob=True)
    r = LlamaRunner.random_init(cfg, 256, torch.float16, expert_format="int8g128")
    assert r.expert_format == "int8g128" and r.wp["layers"][1]["moe_gu"].dtype == torch.uint8 and r.wp["layers"][0]["wgu"].dtype == torch.float16
    assert r.memory_report()["packed_moe_gu"] == packed_bytes(r.shape)[0]
    sess = samd_hip.Session(256)
    assert bool(torch.isfinite(r.prefill(sess, torch.arange(3, 103, device="cuda")[None])).all())
    with pytest.raises(samd_hip.SamdError, match="mixture-of-experts"):         # weight_format keeps its rejection
        LlamaRunner.random_init(cfg, 256, torch.float16, expert_format="int8g128", weight_format="int8g128")
    with pytest.raises(samd_hip.SamdError, match="without mixture-of-experts"):
        LlamaRunner.random_init(dict(TINY, model_type="qwen3"), 256, torch.float16, expert_format="int8g128")


@pytest.mark.parametrize("R,n", [(16, 5), (64, 41)])
def test_graph_replay_equals_the_eager_forward_with_int8_experts(R, n):
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=9)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.bfloat16, expert_format="int8g128")
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


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_one_pass_prefill_stores_the_bits_of_the_chunked_prefill_with_int8_experts(dtype, monkeypatch):
    """130 tokens (two tiles and a bit) and 200, the latter also in two super-chunks: K / V, logits, start token, the verify step behind"""
    cfg = dict(TINY, model_type="qwen3_moe", norm_topk_prob=True, mlp_only_layers=[1])
    runner = LlamaRunner.random_init(cfg, 512, dtype, seed=5, std=0.05, expert_format="int8g128")
    assert runner.expert_format == "int8g128"
    for N, rows in ((130, None), (200, None), (200, 128)):
        prefill_compare(runner, N, rows, monkeypatch, f"int8 experts {dtype} N={N} rows={rows}")
    assert runner.row_major_released


def test_generate_speculative_equals_autoregressive_with_int8_experts(monkeypatch):
    """test_gpu_moe_runner's generation test with SAMD_EXPERT_FORMAT=int8g128 (SamdModel cannot pass the argument), 96 new tokens:
    speculative decoding stays lossless against the same runner's autoregressive decoding, up to the near-tie allowance of that test; with
    graphs (the hipGraph path) and without"""
    import samd_sam_only as SO
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "int8g128")
    lm = hf_moe(dict(vocab_size=512, norm_topk_prob=True, mlp_only_layers=[0]), seed=3, std=0.08).half()
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 70).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=96, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]
    assert ar._runner.expert_format == "int8g128"
    probe = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.float16)
    assert probe.expert_format == "int8g128"

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
    assert spec._runner.expert_format == "int8g128"
