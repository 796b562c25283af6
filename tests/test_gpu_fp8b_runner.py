"""LlamaRunner with dense block-scaled FP8 projections (weight_format "fp8b128": e4m3fn codes + one fp32 scale per 128 x 128 block): parity
with HuggingFace fp32 on the dequantised weights (the yardstick of test_gpu_fp8_runner.py: within 1.5x of HF low precision's own error), the
checkpoint importer (transformers' own FP8Linear modules) against quantising on load (bit-equal logits), losslessness of speculative decoding
against the same runner's greedy output, and the memory accounting."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import samd_hip
from samd_hip import fp8 as F8
from samd_hip.llama import LlamaRunner
from test_gpu_fp8_runner import PROJ, tiny_cfg
from test_gpu_lm_shapes import hf_llama, hf_low_precision_twin, tree_mask_4d, verify_against_hf

QCFG = dict(quant_method="fp8", activation_scheme="dynamic", weight_block_size=[128, 128])


def to_block_checkpoint(lm, dtype):
    """(a block-scaled FP8 checkpoint of lm: every projection a transformers FP8Linear -- float8_e4m3fn weight + fp32 weight_scale_inv per
        128 x 128 block -- quantised from its `dtype` weights, config.quantization_config set;  lm itself with those projections replaced by
        fl32(float(q) * s))"""
    from transformers.integrations.finegrained_fp8 import FP8Linear
    ck = copy.deepcopy(lm)
    for lyr, lyr_ref in zip(ck.model.layers, lm.model.layers):
        for a, b in PROJ:
            ref = getattr(getattr(lyr_ref, a), b)
            q, s = F8.quantize_blocks(ref.weight.detach().to(dtype))
            lin = FP8Linear(ref.in_features, ref.out_features, block_size=(128, 128)).to(ref.weight.device)
            lin.weight.data, lin.weight_scale_inv.data = q, s
            setattr(getattr(lyr, a), b, lin)
            with torch.no_grad():
                ref.weight.copy_(F8.dequantize_blocks(q, s))
    ck.config.quantization_config = dict(QCFG)
    return ck


def check_parity(lm, lm_low, runner, dtype, prompt_len, n, vocab, label):
    """test_fp8_runner_matches_hf_on_dequantised_weights' criterion: <= 1.5 x HF low precision's own error + 0.02, arg-max equal on decided nodes"""
    from transformers import DynamicCache
    e_pre, e_tree = verify_against_hf(lm, runner, prompt_len, n, vocab, tol=None, seed=n)
    c = verify_against_hf.last
    with torch.no_grad():
        cache = DynamicCache()
        ids = torch.tensor([c["prompt"]], device="cuda")
        last_low = lm_low(input_ids=ids, past_key_values=cache, use_cache=True, logits_to_keep=1).logits[0, -1].float()
        tree_low = lm_low(input_ids=torch.tensor([c["toks"]], device="cuda"), position_ids=torch.tensor([[prompt_len + x for x in c["depth"]]], device="cuda"),
                          attention_mask=tree_mask_4d(c["anc"], prompt_len, n).to(dtype), past_key_values=cache, use_cache=True).logits[0].float()
    hf_pre, hf_tree = (c["ref_last"] - last_low).abs().max().item(), (c["want"] - tree_low).abs().max().item()
    print(f"{label} n={n}: ours {e_pre:.4f} / {e_tree:.4f}, HF low precision {hf_pre:.4f} / {hf_tree:.4f}")
    assert e_pre <= 1.5 * hf_pre + 0.02 and e_tree <= 1.5 * hf_tree + 0.02, (n, e_pre, hf_pre, e_tree, hf_tree)
    top2 = c["want"].topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * max(e_tree, hf_tree) + 1e-3
    assert bool((c["argmax"] == c["want"].argmax(-1))[decided].all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_fp8b_runner_matches_hf_on_dequantised_weights(dtype, kv_heads):
    lm = hf_llama(tiny_cfg(kv_heads), seed=21 + kv_heads, std=0.05)
    ck = to_block_checkpoint(lm, dtype)                  # lm now holds the dequantised weights (fp32)
    runner = LlamaRunner.from_hf(ck, max_cache_len=256, dtype=dtype)
    assert runner.weight_format == "fp8b128" and not runner.norm_fold and runner.max_draft_rows() == 64
    lm_low = hf_low_precision_twin(lm, dtype)
    for n in (1, 8, 16, 32, 48, 64):
        check_parity(lm, lm_low, runner, dtype, 70, n, 1024, f"fp8b128 {dtype} kv {kv_heads}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fp8b_qwen3_runner_matches_hf_on_dequantised_weights(dtype):
    """q / k norm: the projection's partials go through samd_rope_kv_write_epi, as for per-row FP8"""
    from test_gpu_qwen import TINY, hf_qwen
    lm = hf_qwen("qwen3", {}, seed=21)
    ck = to_block_checkpoint(lm, dtype)
    runner = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert runner.weight_format == "fp8b128" and runner.qkv_epilogue
    lm_low = hf_low_precision_twin(lm, dtype)
    for prompt_len, n in ((70, 1), (70, 16), (130, 64)):
        check_parity(lm, lm_low, runner, dtype, prompt_len, n, TINY["vocab_size"], f"fp8b128 qwen3 {dtype}")


def test_checkpoint_import_equals_quantising_on_load():
    """from_hf, with no argument, on a module of FP8Linears (weight + weight_scale_inv) == a runner that quantises the same fp16 module on load:
    bit-equal logits at the prefill, the 8-row bucket and the 48-row bucket"""
    lm = hf_llama(tiny_cfg(2), seed=5, std=0.05).half()
    a = LlamaRunner.from_hf(lm, max_cache_len=256, dtype=torch.float16, weight_format="fp8b128")
    b = LlamaRunner.from_hf(to_block_checkpoint(copy.deepcopy(lm), torch.float16), max_cache_len=256, dtype=torch.float16)
    assert a.weight_format == b.weight_format == "fp8b128"
    for x, y in zip(a.wp["layers"], b.wp["layers"]):                     # the same codes and the same tables
        for k in F8.PROJECTIONS:
            assert torch.equal(x[k + "_f8b"][0].view(torch.uint8), y[k + "_f8b"][0].view(torch.uint8)) and torch.equal(x[k + "_f8b"][1], y[k + "_f8b"][1])
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
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_weight_format_errors_on_the_device():
    from samd_hip import SamdError
    lm = hf_llama(tiny_cfg(2), seed=6, std=0.05)
    ck = to_block_checkpoint(copy.deepcopy(lm), torch.float16)
    with pytest.raises(SamdError, match="block-scaled FP8 projections"):
        LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16, weight_format="fp8")
    with pytest.raises(SamdError, match="native_gemm=False is not available with weight_format 'fp8b128'"):
        LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16, native_gemm=False)
    # a raw weights dict: the _sinv keys make the runner "fp8b128"; a bad table is rejected by projection
    cfg = dict(tiny_cfg(2))
    r = LlamaRunner.random_init(cfg, 128, torch.float16, seed=1)
    w = dict(r.w, layers=[dict(l) for l in r.w["layers"]])
    for l in w["layers"]:
        for k in F8.PROJECTIONS:
            l[k], l[k + "_sinv"] = F8.quantize_blocks(l[k])
    shape = r.shape
    del r
    ok = LlamaRunner(shape, dict(w, layers=[dict(l) for l in w["layers"]]), 128, torch.float16, "cuda")
    assert ok.weight_format == "fp8b128" and ok.memory_report()["weight_format"] == "fp8b128"
    bad = dict(w, layers=[dict(l) for l in w["layers"]])
    bad["layers"][1]["wdown_sinv"] = bad["layers"][1]["wdown_sinv"][:, :-1].contiguous()
    with pytest.raises(SamdError, match="block-scaled FP8 projection wdown: weight_scale_inv of shape"):
        LlamaRunner(shape, bad, 128, torch.float16, "cuda")
    with pytest.raises(SamdError, match="pass None or 'fp8b128'"):
        LlamaRunner(shape, dict(w, layers=[dict(l) for l in w["layers"]]), 128, torch.float16, "cuda", weight_format="fp8")


def test_shapes_the_kernel_cannot_run_raise_by_projection():
    from samd_hip import SamdError
    cfg = dict(tiny_cfg(2), intermediate_size=1088)                      # 8.5 blocks: gate|up would straddle
    with pytest.raises(SamdError, match="intermediate_size 1088 is not a multiple of 128"):
        LlamaRunner.random_init(cfg, 128, torch.float16, seed=1, weight_format="fp8b128")
    cfg = dict(tiny_cfg(2), intermediate_size=384)                       # the down projection's K
    with pytest.raises(SamdError, match=r"projection wdown of layer 0, shape \(512, 384\)"):
        LlamaRunner.random_init(cfg, 128, torch.float16, seed=1, weight_format="fp8b128")


def test_memory_accounting():
    cfg = dict(hidden_size=1024, intermediate_size=2816, num_hidden_layers=4, num_attention_heads=8, num_key_value_heads=8, vocab_size=1024,
               max_position_embeddings=512, rms_norm_eps=1e-5)
    r16 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2)
    b16 = r16.weight_bytes()
    proj = sum(t.numel() for l in r16.w["layers"] for k, t in l.items() if k in F8.PROJECTIONS)
    blocks = sum((t.shape[0] // 128) * (t.shape[1] // 128) for l in r16.w["layers"] for k, t in l.items() if k in F8.PROJECTIONS)
    assert blocks * 128 * 128 == proj
    del r16
    torch.cuda.empty_cache()
    r8 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2, weight_format="fp8b128")
    rep = r8.memory_report()
    assert rep["weight_format"] == "fp8b128"
    assert sum(rep["packed_" + k + "_f8b"] for k in F8.PROJECTIONS) == proj and rep["fp8_block_scales"] == 4 * blocks
    assert proj + 4 * blocks == sum(F8.block_scaled_bytes(*t.shape) for l in r8.w["layers"] for k, t in l.items() if k in F8.PROJECTIONS)
    assert all(rep.get("packed_" + k, 0) == 0 for k in ("wqkv", "wqkv64", "wo", "wo_g", "wgu", "wdown", "wdown_g"))
    assert all(t.device.type == "meta" for l in r8.w["layers"] for k, t in l.items() if k in F8.PROJECTIONS)   # no model-dtype projection left
    want_row_major = sum(t.numel() * 2 for t in (r8.w["embed"], r8.w["lm_head"])) + sum(l[k].numel() * 2 for l in r8.w["layers"] for k in ("ln1", "ln2"))
    assert rep["row_major"] == want_row_major
    assert r8.weight_bytes() == b16 - proj + 4 * blocks
    assert r8.max_draft_rows() == 64 and r8.tune_prefill() == {} and r8.release_row_major()


def _near_tie(lm, prefix, a, b, eps=5e-2):
    with torch.no_grad():
        lg = lm(input_ids=torch.tensor([prefix], device="cuda")).logits[0, -1]
    return abs(lg[a].item() - lg[b].item()) < eps


def test_fp8b_speculative_equals_autoregressive(monkeypatch):
    """evaluation/equal.py's criterion with block-scaled FP8 weights, reached through SAMD_WEIGHT_FORMAT as SamdModel and bench.py reach it:
    SAM-drafted decoding == the greedy output of the same runner (graphs on and off); only a near-tie may split them"""
    import samd_sam_only as SO
    from test_gpu_llama import tiny_llama
    lm = tiny_llama(2, seed=3)
    to_block_checkpoint(lm, torch.float16)               # lm keeps fl32(float(q) * s): HF's near-tie check then sees (almost) the FP8 model
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "fp8b128")
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 40).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=96, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]
    assert ar._runner.weight_format == "fp8b128"
    docs = [seq_ar[len(prompt):]] + [rng.integers(3, 512, 50).tolist() for _ in range(4)] + [[i] for i in range(512)]
    cfg = SO.SamdConfig(max_predicts=16, alpha=4.0, len_bias=0)
    draft = SO.DraftModel(cfg, sam_static=SO.build_sam(docs, 2), device="cuda")
    spec = SO.SamdModel(cfg, lm, draft, eos_token_id=2, dtype=torch.float16, device="cuda")
    for use_graphs in (True, False):
        spec.set_cache(gcfg)
        spec.engine.use_graphs = use_graphs
        out = spec.generate(ids, generation_config=gcfg)
        assert spec._runner.weight_format == "fp8b128"
        seq = out.output_ids[0]
        assert out.decode_steps < out.decode_tokens, "drafts were never accepted"
        m = min(len(seq), len(seq_ar))
        diff = [i for i in range(m) if seq[i] != seq_ar[i]]
        if diff:
            i = diff[0]
            assert i > len(prompt) + 8 and _near_tie(lm, seq[:i], seq[i], seq_ar[i]), f"diverged at {i}"
