"""Qwen2 / Qwen2.5 (q|k|v bias) and Qwen3 (per-head q / k RMSNorm) on LlamaRunner, against HuggingFace in fp32 on the same GPU, with the
yardstick of test_gpu_lm_shapes.py: our error <= 1.5x HF low precision's own error (+ 0.02), and our arg-max == fp32's on every row whose
top-2 gap exceeds twice the larger error.  No checkpoint: random weights, with the biases and q / k norm weights drawn far from HF's
defaults (zero bias and unit norm weights would hide a missing or misplaced epilogue)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import samd_hip
from samd_hip import SamdError
from samd_hip.llama import LlamaRunner
from test_gpu_lm_shapes import hf_low_precision_twin, tree_mask_4d, verify_against_hf

TINY = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=6, num_key_value_heads=2, head_dim=128,
            vocab_size=1024, max_position_embeddings=2048, rms_norm_eps=1e-6)
REAL = {   # two layers of the real geometries: GQA 7, the 152k vocabulary, a q width != hidden
    "qwen2.5-7b": ("qwen2", dict(hidden_size=3584, intermediate_size=18944, num_attention_heads=28, num_key_value_heads=4, vocab_size=152064)),
    "qwen3-8b": ("qwen3", dict(hidden_size=4096, intermediate_size=12288, num_attention_heads=32, num_key_value_heads=8, vocab_size=151936)),
    "qwen3-32b": ("qwen3", dict(hidden_size=5120, intermediate_size=25600, num_attention_heads=64, num_key_value_heads=8, vocab_size=151936)),
}


def hf_qwen(kind, cfg_kw, seed, std=0.05, tie=False):
    from transformers import Qwen2Config, Qwen2ForCausalLM, Qwen3Config, Qwen3ForCausalLM
    Cfg, M = (Qwen2Config, Qwen2ForCausalLM) if kind == "qwen2" else (Qwen3Config, Qwen3ForCausalLM)
    cfg = Cfg(**dict(dict(TINY, head_dim=128), **cfg_kw), tie_word_embeddings=tie, rope_parameters=dict(rope_type="default", rope_theta=1e6))
    cfg._attn_implementation = "eager"
    torch.manual_seed(seed)
    with torch.device("cuda"):
        lm = M(cfg)
    lm = lm.float().eval()
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g, device="cuda") * std)
            elif name.endswith(("q_norm.weight", "k_norm.weight")):
                mag = 0.5 + 1.5 * torch.rand(p.shape, generator=g, device="cuda")
                p.copy_(mag * torch.where(torch.rand(p.shape, generator=g, device="cuda") < 0.5, -1.0, 1.0))
            elif name.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g, device="cuda") * 0.5)
            else:
                p.copy_(1 + 0.05 * torch.randn(p.shape, generator=g, device="cuda"))
    return lm


def compare(lm, lm_low, runner, prompt_len, n, vocab, seed, label):
    from transformers import DynamicCache
    e_pre, e_tree = verify_against_hf(lm, runner, prompt_len, n, vocab, tol=None, seed=seed)
    c = verify_against_hf.last
    dtype = next(lm_low.parameters()).dtype
    with torch.no_grad():
        cache = DynamicCache()
        ids = torch.tensor([c["prompt"]], device="cuda")
        last_low = lm_low(input_ids=ids, past_key_values=cache, use_cache=True, logits_to_keep=1).logits[0, -1].float()
        tree_low = lm_low(input_ids=torch.tensor([c["toks"]], device="cuda"), position_ids=torch.tensor([[prompt_len + x for x in c["depth"]]], device="cuda"),
                          attention_mask=tree_mask_4d(c["anc"], prompt_len, n).to(dtype), past_key_values=cache, use_cache=True).logits[0].float()
    hf_pre, hf_tree = (c["ref_last"] - last_low).abs().max().item(), (c["want"] - tree_low).abs().max().item()
    print(f"{label} L={prompt_len} n={n}: ours {e_pre:.4f} / {e_tree:.4f}, HF low precision {hf_pre:.4f} / {hf_tree:.4f}")
    assert e_pre <= 1.5 * hf_pre + 0.02 and e_tree <= 1.5 * hf_tree + 0.02, (label, n, e_pre, hf_pre, e_tree, hf_tree)
    top2 = c["want"].topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * max(e_tree, hf_tree) + 1e-3
    assert bool((c["argmax"] == c["want"].argmax(-1))[decided].all()), label


def env(monkeypatch, **kv):
    for k, v in kv.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# (prompt length, draft nodes): 70 = chunked prefill, 300 / 1100 = the wide prefill; every row bucket 1 .. 128
PLAN = [(70, 1), (300, 8), (70, 16), (300, 32), (1100, 48), (70, 64), (300, 128)]


@pytest.mark.parametrize("kind,tie", [("qwen2", False), ("qwen3", False), ("qwen3", True)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("attention,v_layout", [("split", "t"), ("split", "rows"), ("split3", "t"), ("split3", "rows")])
def test_tiny_qwen_matches_hf(monkeypatch, kind, tie, dtype, attention, v_layout):
    env(monkeypatch, SAMD_V_LAYOUT=v_layout)
    lm = hf_qwen(kind, {}, seed=11 + tie, tie=tie)
    runner = LlamaRunner.from_hf(lm, max_cache_len=1280, dtype=dtype, attention=attention)
    assert runner.qkv_epilogue and not runner.norm_fold and all(l["wqkv64"] is None for l in runner.wp["layers"])
    assert runner.v_transposed == (v_layout == "t")
    lm_low = hf_low_precision_twin(lm, dtype)
    for prompt_len, n in PLAN:
        compare(lm, lm_low, runner, prompt_len, n, TINY["vocab_size"], seed=prompt_len + n, label=f"{kind} tie={tie} {dtype} {attention} V={v_layout}")


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
@pytest.mark.parametrize("v_layout", ["t", "rows"])
def test_sdpa_prefill_matches_hf(monkeypatch, kind, v_layout):
    """SAMD_PREFILL_ATTENTION=sdpa reads V straight from the q|k|v product (V^T cache) or from the cache: the bias must be in both"""
    env(monkeypatch, SAMD_V_LAYOUT=v_layout, SAMD_PREFILL_ATTENTION="sdpa")
    lm = hf_qwen(kind, {}, seed=5)
    runner = LlamaRunner.from_hf(lm, max_cache_len=1280, dtype=torch.bfloat16)
    lm_low = hf_low_precision_twin(lm, torch.bfloat16)
    for prompt_len, n in ((300, 16), (1100, 64)):
        compare(lm, lm_low, runner, prompt_len, n, TINY["vocab_size"], seed=n, label=f"{kind} sdpa V={v_layout}")


@pytest.mark.parametrize("name", list(REAL))
def test_real_geometry_two_layers_matches_hf(name):
    kind, kw = REAL[name]
    lm = hf_qwen(kind, dict(kw, num_hidden_layers=2), seed=3, std=0.02)
    runner = LlamaRunner.from_hf(lm, max_cache_len=1280, dtype=torch.bfloat16)
    lm_low = hf_low_precision_twin(lm, torch.bfloat16)
    for prompt_len, n in ((300, 48), (70, 16)):
        compare(lm, lm_low, runner, prompt_len, n, kw["vocab_size"], seed=n, label=name)
    del runner, lm, lm_low
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fp8_runner_matches_hf_on_dequantised_weights(kind, dtype):
    from test_gpu_fp8_runner import to_fp8_checkpoint
    lm = hf_qwen(kind, {}, seed=21)
    ck = to_fp8_checkpoint(lm, dtype)                     # lm now holds the dequantised projections; biases / norms stay in lm and ck
    runner = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert runner.weight_format == "fp8" and runner.qkv_epilogue
    lm_low = hf_low_precision_twin(lm, dtype)
    for prompt_len, n in ((70, 1), (70, 16), (130, 64)):
        compare(lm, lm_low, runner, prompt_len, n, TINY["vocab_size"], seed=n, label=f"fp8 {kind} {dtype}")


def test_fused_forms_stay_off_and_other_attention_modes_raise(monkeypatch):
    env(monkeypatch, SAMD_QKV_FUSED="force")
    lm = hf_qwen("qwen3", {}, seed=2)
    runner = LlamaRunner.from_hf(lm, max_cache_len=256, dtype=torch.float16)
    assert all(l["wqkv64"] is None for l in runner.wp["layers"]) and not runner.norm_fold
    assert runner.memory_report()["qkv_epilogue"] == 2 * 2 * 128 * 2
    for mode in ("split2", "block"):
        with pytest.raises(SamdError, match=mode):
            LlamaRunner.from_hf(lm, max_cache_len=256, dtype=torch.float16, attention=mode)
    r2 = LlamaRunner.random_init(dict(TINY, model_type="qwen2"), 256, torch.float16)
    assert r2.qkv_epilogue and r2.w["layers"][0]["bqkv"].abs().max().item() > 0.5


def _near_tie(lm, prefix, a, b, eps=5e-2):
    with torch.no_grad():
        lg = lm(input_ids=torch.tensor([prefix], device="cuda")).logits[0, -1]
    return abs(lg[a].item() - lg[b].item()) < eps


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
def test_generate_speculative_equals_autoregressive(kind):
    import samd as S
    import samd_sam_only as SO
    lm = hf_qwen(kind, dict(vocab_size=512), seed=3, std=0.08).half()
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 70).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=64, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]

    def same(seq, after=8):
        m = min(len(seq), len(seq_ar))
        diff = [i for i in range(m) if seq[i] != seq_ar[i]]
        assert not diff or (diff[0] > len(prompt) + after and _near_tie(lm, seq[:diff[0]], seq[diff[0]], seq_ar[diff[0]])), diff[:3]
    docs = [seq_ar[len(prompt):]] + [rng.integers(3, 512, 50).tolist() for _ in range(4)] + [[i] for i in range(512)]
    cfg = SO.SamdConfig(max_predicts=16, alpha=4.0, len_bias=0)
    spec = SO.SamdModel(cfg, lm, SO.DraftModel(cfg, sam_static=SO.build_sam(docs, 2), device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    for use_graphs in (True, False):
        spec.set_cache(gcfg)
        spec.engine.use_graphs = use_graphs
        out = spec.generate(ids, generation_config=gcfg)
        assert out.decode_steps < out.decode_tokens, "drafts were never accepted"
        same(out.output_ids[0])
    spec.gen_config = gcfg
    got = list(prompt)
    for new_ids, _ in spec._run_granular(ids, gcfg, 24):
        got.extend(new_ids)
    same(got)
    # Token Recycle (the full variant's tree drafts): lossless as well
    tcfg = S.SamdConfig(n_predicts=12, len_threshold=3, len_bias=0)
    tr = S.SamdModel(tcfg, lm, S.DraftModel(tcfg, sam_static=SO.build_sam(docs, 2), lm=lm, device="cuda"), eos_token_id=2, dtype=torch.float16,
                     device="cuda")
    out = tr.generate(ids, generation_config=gcfg)
    same(out.output_ids[0])
    # one sampled run completes
    g = SO.SamdGenerationConfig(max_new_tokens=24, max_cache_len=512, greedy=False, temperature=0.8, top_p=0.9)
    out = spec.generate(ids, generation_config=g)
    assert len(out.output_ids[0]) > len(prompt)
