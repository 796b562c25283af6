"""LlamaRunner with FP8 (OCP e4m3fn) projections: parity with HuggingFace fp32 on the dequantised weights (the yardstick of
test_gpu_lm_shapes.py: within 1.5x of HF low precision's own error), the checkpoint importer against quantising on load (bit-equal logits),
losslessness of speculative decoding against the same FP8 runner's greedy output, and the memory accounting."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import samd_hip
from samd_hip import fp8 as F8
from samd_hip.llama import LlamaRunner
from test_gpu_lm_shapes import hf_llama, hf_low_precision_twin, tree_mask_4d, verify_against_hf

PROJ = (("self_attn", "q_proj"), ("self_attn", "k_proj"), ("self_attn", "v_proj"), ("self_attn", "o_proj"), ("mlp", "gate_proj"), ("mlp", "up_proj"),
        ("mlp", "down_proj"))


def linears(lm):
    for lyr in lm.model.layers:
        for a, b in PROJ:
            yield getattr(getattr(lyr, a), b)


def to_fp8_checkpoint(lm, dtype, scale_kind="row"):
    """(an FP8 checkpoint of lm: every projection float8_e4m3fn + weight_scale, quantised from its `dtype` weights;
        lm itself with those projections replaced by float(q) * scale)"""
    ck = copy.deepcopy(lm)
    for lin, lin_ref in zip(linears(ck), linears(lm)):
        q, s = F8.quantize_rows(lin.weight.detach().to(dtype))
        lin.weight = torch.nn.Parameter(q, requires_grad=False)
        lin.register_buffer("weight_scale", s[:, None].clone() if scale_kind == "row1" else s.clone())
        with torch.no_grad():
            lin_ref.weight.copy_(F8.dequantize_rows(q, s))
    return ck


def tiny_cfg(kv_heads):
    return dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=kv_heads, vocab_size=1024,
                max_position_embeddings=512, rms_norm_eps=1e-5, head_dim=128)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_fp8_runner_matches_hf_on_dequantised_weights(dtype, kv_heads):
    lm = hf_llama(tiny_cfg(kv_heads), seed=21 + kv_heads, std=0.05)
    ck = to_fp8_checkpoint(lm, dtype)                    # lm now holds the dequantised weights (fp32)
    runner = LlamaRunner.from_hf(ck, max_cache_len=256, dtype=dtype)
    assert runner.weight_format == "fp8" and not runner.norm_fold and runner.max_draft_rows() == 64
    lm_low = hf_low_precision_twin(lm, dtype)
    for n in (1, 8, 16, 32, 48, 64):
        e_pre, e_tree = verify_against_hf(lm, runner, 70, n, 1024, tol=None, seed=n)
        c = verify_against_hf.last
        from transformers import DynamicCache
        with torch.no_grad():
            cache = DynamicCache()
            ids = torch.tensor([c["prompt"]], device="cuda")
            last_low = lm_low(input_ids=ids, past_key_values=cache, use_cache=True, logits_to_keep=1).logits[0, -1].float()
            tree_low = lm_low(input_ids=torch.tensor([c["toks"]], device="cuda"), position_ids=torch.tensor([[70 + x for x in c["depth"]]], device="cuda"),
                              attention_mask=tree_mask_4d(c["anc"], 70, n).to(dtype), past_key_values=cache, use_cache=True).logits[0].float()
        hf_pre, hf_tree = (c["ref_last"] - last_low).abs().max().item(), (c["want"] - tree_low).abs().max().item()
        print(f"fp8 {dtype} kv {kv_heads} n={n}: ours {e_pre:.4f} / {e_tree:.4f}, HF low precision {hf_pre:.4f} / {hf_tree:.4f}")
        assert e_pre <= 1.5 * hf_pre + 0.02 and e_tree <= 1.5 * hf_tree + 0.02, (n, e_pre, hf_pre, e_tree, hf_tree)
        top2 = c["want"].topk(2, dim=-1).values
        decided = (top2[:, 0] - top2[:, 1]) > 2 * max(e_tree, hf_tree) + 1e-3
        assert bool((c["argmax"] == c["want"].argmax(-1))[decided].all())


@pytest.mark.parametrize("scale_kind", ["row", "row1"])
def test_checkpoint_import_equals_quantising_on_load(scale_kind):
    """from_hf on a module with float8_e4m3fn weights + weight_scale == a runner that quantises the same fp16 module on load: bit-equal logits"""
    lm = hf_llama(tiny_cfg(2), seed=5, std=0.05).half()
    a = LlamaRunner.from_hf(lm, max_cache_len=256, dtype=torch.float16, weight_format="fp8")
    b = LlamaRunner.from_hf(to_fp8_checkpoint(lm, torch.float16, scale_kind), max_cache_len=256, dtype=torch.float16)
    assert a.weight_format == b.weight_format == "fp8"
    rng = np.random.default_rng(3)
    prompt = torch.tensor([rng.integers(3, 1024, 150).tolist()], device="cuda")
    drafts = [torch.tensor(rng.integers(3, 1024, n), dtype=torch.int32, device="cuda") for n in (5, 40)]
    outs = []
    for r in (a, b):
        sess = samd_hip.Session(512)
        res = [r.prefill(sess, prompt).clone()]
        for toks in drafts:                              # sequence drafts on the 8- and 48-row buckets
            n = toks.numel()
            res.append(r.forward_tokens(sess, toks, torch.arange(n, dtype=torch.int32, device="cuda"), r.pf_mask, n, 150).clone())
        outs.append(res)
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_weight_format_errors_and_env():
    from samd_hip import SamdError
    lm = hf_llama(tiny_cfg(2), seed=6, std=0.05)
    ck = to_fp8_checkpoint(lm, torch.float16)
    with pytest.raises(SamdError, match="float8_e4m3fn projections"):
        LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16, weight_format="fp16")
    with pytest.raises(SamdError, match="weight_format"):
        LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="int4")
    lin = ck.model.layers[1].mlp.up_proj
    lin.weight = torch.nn.Parameter(torch.zeros(lin.weight.shape), requires_grad=False)
    with pytest.raises(SamdError, match="mix of FP8"):
        LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16)
    assert LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="fp16").weight_format is None


def test_memory_accounting():
    cfg = dict(hidden_size=1024, intermediate_size=2816, num_hidden_layers=4, num_attention_heads=8, num_key_value_heads=8, vocab_size=1024,
               max_position_embeddings=512, rms_norm_eps=1e-5)
    r16 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2)
    b16 = r16.weight_bytes()
    proj = sum(t.numel() for l in r16.w["layers"] for k, t in l.items() if k in F8.PROJECTIONS)
    rows = sum(t.shape[0] for l in r16.w["layers"] for k, t in l.items() if k in F8.PROJECTIONS)
    del r16
    torch.cuda.empty_cache()
    r8 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2, weight_format="fp8")
    rep = r8.memory_report()
    assert rep["weight_format"] == "fp8"
    assert sum(rep["packed_" + k + "_f8"] for k in F8.PROJECTIONS) == proj and rep["fp8_scales"] == 4 * rows
    assert all(rep.get("packed_" + k, 0) == 0 for k in ("wqkv", "wqkv64", "wo", "wo_g", "wgu", "wdown", "wdown_g"))
    assert all(t.device.type == "meta" for l in r8.w["layers"] for k, t in l.items() if k in F8.PROJECTIONS)   # no model-dtype projection left
    want_row_major = sum(t.numel() * 2 for t in (r8.w["embed"], r8.w["lm_head"])) + sum(l[k].numel() * 2 for l in r8.w["layers"] for k in ("ln1", "ln2"))
    assert rep["row_major"] == want_row_major
    assert r8.weight_bytes() == b16 - proj + 4 * rows
    assert 0.49 < r8.weight_bytes() / b16 < 0.53
    assert r8.max_draft_rows() == 64 and r8.tune_prefill() == {} and r8.release_row_major()


def _ar_and_spec(lm, monkeypatch):
    import samd_sam_only as SO
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "fp8")
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 40).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=96, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    out_ar = ar.generate(ids, generation_config=gcfg)
    return SO, rng, prompt, ids, gcfg, out_ar.output_ids[0]


def _dequantised_tiny(seed):
    from test_gpu_llama import tiny_llama
    lm = tiny_llama(2, seed=seed)
    to_fp8_checkpoint(lm, torch.float16)                 # lm keeps float(q) * scale: HF's near-tie check then sees (almost) the FP8 model
    return lm


def _near_tie(lm, prefix, a, b, eps=5e-2):
    with torch.no_grad():
        lg = lm(input_ids=torch.tensor([prefix], device="cuda")).logits[0, -1]
    return abs(lg[a].item() - lg[b].item()) < eps


def test_fp8_speculative_equals_autoregressive(monkeypatch):
    """evaluation/equal.py's criterion with FP8 weights: SAM-drafted decoding == the greedy output of the same FP8 runner (graphs on and off,
    and the granular prefill / decode form); only a near-tie may split them"""
    lm = _dequantised_tiny(3)
    SO, rng, prompt, ids, gcfg, seq_ar = _ar_and_spec(lm, monkeypatch)
    docs = [seq_ar[len(prompt):]] + [rng.integers(3, 512, 50).tolist() for _ in range(4)] + [[i] for i in range(512)]
    cfg = SO.SamdConfig(max_predicts=16, alpha=4.0, len_bias=0)
    draft = SO.DraftModel(cfg, sam_static=SO.build_sam(docs, 2), device="cuda")
    spec = SO.SamdModel(cfg, lm, draft, eos_token_id=2, dtype=torch.float16, device="cuda")
    for use_graphs in (True, False):
        spec.set_cache(gcfg)
        spec.engine.use_graphs = use_graphs
        out = spec.generate(ids, generation_config=gcfg)
        assert spec._runner.weight_format == "fp8"
        seq = out.output_ids[0]
        assert out.decode_steps < out.decode_tokens, "drafts were never accepted"
        m = min(len(seq), len(seq_ar))
        diff = [i for i in range(m) if seq[i] != seq_ar[i]]
        if diff:
            i = diff[0]
            assert i > len(prompt) + 8 and _near_tie(lm, seq[:i], seq[i], seq_ar[i]), f"diverged at {i}"
    spec.gen_config = gcfg
    got = list(prompt)
    for new_ids, _ in spec._run_granular(ids, gcfg, 24):
        got.extend(new_ids)
    m = min(len(got), len(seq_ar))
    diff = [i for i in range(m) if got[i] != seq_ar[i]]
    assert not diff or _near_tie(lm, got[:diff[0]], got[diff[0]], seq_ar[diff[0]])


def test_fp8_token_recycle_is_lossless(monkeypatch):
    import samd as S
    lm = _dequantised_tiny(9)
    SO, rng, prompt, ids, gcfg, seq_ar = _ar_and_spec(lm, monkeypatch)
    cfg = S.SamdConfig(n_predicts=16, len_threshold=4, len_bias=0, tree_method="token_recycle")
    draft = S.DraftModel(cfg, lm=lm, device="cuda")
    model = S.SamdModel(cfg, lm, draft, eos_token_id=2, dtype=torch.float16, device="cuda")
    for rep in range(2):
        out = model.generate(ids, generation_config=gcfg)
        seq = out.output_ids[0]
        m = min(len(seq), len(seq_ar))
        diff = [i for i in range(m) if seq[i] != seq_ar[i]]
        assert not diff or (diff[0] > len(prompt) + 4 and _near_tie(lm, seq[:diff[0]], seq[diff[0]], seq_ar[diff[0]])), diff[:3]
    assert out.decode_steps < out.decode_tokens, "Token Recycle never got a draft accepted on a repeated request"
