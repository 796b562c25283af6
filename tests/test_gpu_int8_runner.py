"""LlamaRunner with INT8 (GPTQ 8-bit: one code per byte, group scales and 8-bit zero points) projections: parity with HuggingFace fp32 on the
dequantised weights (the yardstick of test_gpu_lm_shapes.py: within 1.5x of HF low precision's own error), the GPTQ importer (v1, v2)
against quantising on load (equal packed buffers, bit-equal logits), Qwen2 / Qwen3 shapes, format errors and the env knob, the memory
accounting, and losslessness of speculative decoding against the same INT8 runner's greedy output."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import samd_hip
from samd_hip import SamdError
from samd_hip import int8 as I8
from samd_hip.llama import LlamaRunner
from test_gpu_fp8_runner import PROJ, tiny_cfg
from test_gpu_int4_runner import to_int4_checkpoint
from test_gpu_lm_shapes import hf_llama, hf_low_precision_twin
from test_gpu_mxfp4_runner import _near_tie, parity
from test_int8_weights_cpu import GPTQ8_CFG, GPTQ8V2_CFG, gptq8_module

CONFIGS = {"gptq": GPTQ8_CFG, "gptq_v2": GPTQ8V2_CFG}


def to_int8_checkpoint(lm, dtype, layout="gptq", dequantise_into_lm=True):
    """(an 8-bit GPTQ checkpoint of lm in `layout` ("gptq": v1, stores z - 1; "gptq_v2"): every projection replaced by a module with int32
        qweight / qzeros and fp16 scales, quantised from its `dtype` weights per group of 128, and config.quantization_config set; lm
        itself with those projections replaced by the dequantised weights).  The scales are quantize_groups' in `dtype`, stored as fp16 as
        a checkpoint stores them (exact for these magnitudes), so that the import's one rounding to a bf16 runner's dtype gives them back."""
    ck = copy.deepcopy(lm)
    for lyr, lyr_ref in zip(ck.model.layers, lm.model.layers):
        for a, b in PROJ:
            lin = getattr(getattr(lyr_ref, a), b)
            q, z, s = I8.quantize_groups(lin.weight.detach().to(dtype), dtype)
            s16 = s.to(torch.float16)
            assert torch.equal(s16.to(dtype), s)
            q, z, s16 = q.cpu(), z.cpu(), s16.cpu()
            bias = getattr(lin, "bias", None)
            bias = None if bias is None else torch.nn.Parameter(bias.detach().clone(), requires_grad=False)
            if layout == "gptq":
                assert int(z.min()) >= 1                      # (a v1 checkpoint stores z - 1; Gaussian groups of 128 straddle zero)
            mod = gptq8_module(q, z, s16, v2=layout == "gptq_v2", bias=bias)
            setattr(getattr(lyr, a), b, mod.to(lin.weight.device))
            if dequantise_into_lm:
                with torch.no_grad():
                    lin.weight.copy_(I8.dequantize_groups(q.to(s.device), z.to(s.device), s))
    ck.config.quantization_config = dict(CONFIGS[layout])
    return ck


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_int8_runner_matches_hf_on_dequantised_weights(dtype, kv_heads):
    lm = hf_llama(tiny_cfg(kv_heads), seed=21 + kv_heads, std=0.05)
    ck = to_int8_checkpoint(lm, dtype, "gptq" if kv_heads == 4 else "gptq_v2")     # lm now holds the dequantised weights (fp32)
    runner = LlamaRunner.from_hf(ck, max_cache_len=256, dtype=dtype)
    assert runner.weight_format == "int8g128" and not runner.norm_fold and runner.max_draft_rows() == 64
    lm_low = hf_low_precision_twin(lm, dtype)
    for n in (1, 8, 16, 32, 48, 64):
        # a bucket's rows may all be near-ties (the 1-row bucket has one row): up to three prompts per bucket, EVERY one held to the error
        # bound and the arg-max check, and at least one with decided rows, so the arg-max check did not pass empty
        shares = []
        for seed in (n, n + 100, n + 200):
            shares.append(parity(lm, lm_low, runner, 70, n, 1024, seed=seed, label=f"int8 {dtype} kv {kv_heads}"))
            if shares[-1] > 0:
                break
        assert max(shares) > 0, (n, shares)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_checkpoint_import_equals_quantising_on_load(dtype):
    """from_hf on 8-bit GPTQ modules (v1 and v2) built from the same (q, z, s), with no format argument, and a runner that quantises the
    same module on load: equal packed buffers, bit-equal logits at prefill and on 5- and 40-node drafts"""
    lm = hf_llama(tiny_cfg(2), seed=5, std=0.05).to(dtype)
    runners = [LlamaRunner.from_hf(lm, max_cache_len=256, dtype=dtype, weight_format="int8g128")]
    for layout in ("gptq", "gptq_v2"):
        runners.append(LlamaRunner.from_hf(to_int8_checkpoint(lm, dtype, layout, dequantise_into_lm=False), max_cache_len=256, dtype=dtype))
    assert all(r.weight_format == "int8g128" for r in runners)
    for r in runners[1:]:
        for la, lb in zip(runners[0].wp["layers"], r.wp["layers"]):
            for k in I8.PROJECTIONS:
                assert torch.equal(la[k + "_i8"], lb[k + "_i8"])
    rng = np.random.default_rng(3)
    prompt = torch.tensor([rng.integers(3, 1024, 150).tolist()], device="cuda")
    drafts = [torch.tensor(rng.integers(3, 1024, n), dtype=torch.int32, device="cuda") for n in (5, 40)]
    outs = []
    for r in runners:
        sess = samd_hip.Session(512)
        res = [r.prefill(sess, prompt).clone()]
        for toks in drafts:                              # sequence drafts on the 8- and 48-row buckets
            n = toks.numel()
            res.append(r.forward_tokens(sess, toks, torch.arange(n, dtype=torch.int32, device="cuda"), r.pf_mask, n, 150).clone())
        outs.append(res)
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.isfinite(x.float()).all() and torch.equal(x, y)


@pytest.mark.parametrize("kind,layout", [("qwen2", "gptq"), ("qwen3", "gptq_v2")])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_qwen_shapes_match_hf_on_dequantised_weights(kind, layout, dtype):
    from test_gpu_qwen import TINY, hf_qwen
    lm = hf_qwen(kind, {}, seed=21)
    ck = to_int8_checkpoint(lm, dtype, layout)           # lm now holds the dequantised projections; biases / norms stay in lm and ck
    runner = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert runner.weight_format == "int8g128" and runner.qkv_epilogue
    lm_low = hf_low_precision_twin(lm, dtype)
    shares = [parity(lm, lm_low, runner, prompt_len, n, TINY["vocab_size"], seed=n, label=f"int8 {kind} {dtype}")
              for prompt_len, n in ((70, 1), (70, 16), (130, 64))]
    assert shares[1] > 0 and shares[2] > 0, shares       # (the 1-row bucket's single row may be a near-tie)


def test_weight_format_errors_and_env(monkeypatch):
    lm = hf_llama(tiny_cfg(2), seed=6, std=0.05)
    make = lambda layout="gptq": to_int8_checkpoint(lm, torch.float16, layout, dequantise_into_lm=False)
    ck = make()
    assert LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16).weight_format == "int8g128"
    # another format against an 8-bit checkpoint
    for fmt in ("fp16", "fp8", "mxfp4", "int4g128", "fp8b128"):
        with pytest.raises(SamdError, match="INT8 \\(GPTQ\\) projections"):
            LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16, weight_format=fmt)
    with pytest.raises(SamdError, match="'int8g128'"):                   # the unknown-format error lists every value
        LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="int3")
    with pytest.raises(SamdError, match="native_gemm=False is not available with weight_format 'int8g128'"):
        LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="int8g128", native_gemm=False)
    # a scale whose 255-fold overflows fp16: the message names bf16, and a bf16 runner takes the same checkpoint
    far = make()
    far.model.layers[0].mlp.down_proj.scales[1, 3] = 300.0
    with pytest.raises(SamdError, match="bfloat16"):
        LlamaRunner.from_hf(far, max_cache_len=128, dtype=torch.float16)
    assert LlamaRunner.from_hf(far, max_cache_len=128, dtype=torch.bfloat16).weight_format == "int8g128"
    # a mix of 8-bit and plain projections, and of 8-bit and 4-bit ones (no config: the widths are read off the modules' shapes)
    mixed = make()
    old = lm.model.layers[1].mlp.up_proj
    mixed.model.layers[1].mlp.up_proj = torch.nn.Linear(old.in_features, old.out_features, bias=False, device="cuda")
    with pytest.raises(SamdError, match="mix of INT8"):
        LlamaRunner.from_hf(mixed, max_cache_len=128, dtype=torch.float16)
    mixed4 = make()
    ck4 = to_int4_checkpoint(lm, torch.float16, "gptq", dequantise_into_lm=False)
    mixed4.model.layers[1].mlp.up_proj = ck4.model.layers[1].mlp.up_proj
    mixed4.config.quantization_config = dict(quant_method="gptq", group_size=128, desc_act=False)
    with pytest.raises(SamdError, match="mix of INT8 and other projections \\(\\d+ of \\d+ are INT8; e.g. layers.1.mlp.up_proj"):
        LlamaRunner.from_hf(mixed4, max_cache_len=128, dtype=torch.float16)
    # a bias on o_proj / down_proj raises, as for every other format
    for a, b, msg in (("self_attn", "o_proj", "o_proj bias"), ("mlp", "down_proj", "MLP projection biases")):
        biased = make()
        mod = getattr(getattr(biased.model.layers[0], a), b)
        mod.bias = torch.nn.Parameter(torch.zeros(mod.out_features, device="cuda"), requires_grad=False)
        with pytest.raises(SamdError, match=msg):
            LlamaRunner.from_hf(biased, max_cache_len=128, dtype=torch.float16)
    # what the importer rejects reaches the caller of from_hf: act-order, a v1 zero point of 255
    act = make()
    act.model.layers[0].self_attn.q_proj.g_idx = act.model.layers[0].self_attn.q_proj.g_idx.flip(0).contiguous()
    with pytest.raises(SamdError, match="layers.0.q_proj: act-order"):
        LlamaRunner.from_hf(act, max_cache_len=128, dtype=torch.float16)
    z255 = make()
    z255.model.layers[1].self_attn.k_proj.qzeros[0, 0] |= 0xFF
    with pytest.raises(SamdError, match="layers.1.k_proj: a stored zero point of 255"):
        LlamaRunner.from_hf(z255, max_cache_len=128, dtype=torch.float16)
    # the environment selects the format for callers that cannot pass one; an explicit argument wins
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "int8g128")
    assert LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16).weight_format == "int8g128"
    assert LlamaRunner.random_init(tiny_cfg(2), 128, torch.float16).weight_format == "int8g128"
    assert LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="fp16").weight_format is None
    monkeypatch.delenv("SAMD_WEIGHT_FORMAT")
    assert LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16).weight_format is None


def test_mixture_of_experts_rejects_int8():
    """weight_format 'int8g128' against a module with sparse layers, and a module whose experts are 8-bit GPTQ modules: each raises by message"""
    from samd_hip import moe as MOE
    from test_gpu_moe_runner import hf_moe
    from test_moe_int4_cpu import to_int4_moe_checkpoint
    with pytest.raises(SamdError, match="mixture-of-experts models are not available with weight_format 'int8g128'"):
        MOE.reject_unsupported("int8g128")
    lm = hf_moe(dict(norm_topk_prob=True), 3)
    with pytest.raises(SamdError, match="mixture-of-experts models are not available with weight_format 'int8g128'"):
        LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="int8g128")
    # 8-bit experts: the 4-bit mixture-of-experts checkpoint of the INT4 test with one expert projection swapped for an 8-bit module
    ck = to_int4_moe_checkpoint(lm, torch.float16, "gptq")
    sparse = next(i for i, lyr in enumerate(ck.model.layers) if hasattr(lyr.mlp, "experts"))
    old = ck.model.layers[sparse].mlp.experts[0].down_proj
    K, N = old.in_features, old.out_features
    q, z, s = I8.quantize_groups(torch.randn((N, K)) * 0.05, torch.float16)
    ck.model.layers[sparse].mlp.experts[0].down_proj = gptq8_module(q, z.clamp_min(1), s).to(old.qweight.device)
    ck.config.quantization_config = dict(quant_method="gptq", group_size=128, desc_act=False)
    with pytest.raises(SamdError, match=f"layers.{sparse}.mlp.experts.0.down_proj: an 8-bit GPTQ module in a mixture-of-experts model"):
        LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16)


def test_memory_accounting():
    cfg = dict(hidden_size=1024, intermediate_size=2816, num_hidden_layers=4, num_attention_heads=8, num_key_value_heads=8, vocab_size=1024,
               max_position_embeddings=512, rms_norm_eps=1e-5)
    r16 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2)
    b16 = r16.weight_bytes()
    proj = sum(t.numel() for l in r16.w["layers"] for k, t in l.items() if k in I8.PROJECTIONS)
    del r16
    torch.cuda.empty_cache()
    r8 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2, weight_format="int8g128")
    rep = r8.memory_report()
    assert rep["weight_format"] == "int8g128"
    assert sum(rep["packed_" + k + "_i8"] for k in I8.PROJECTIONS) == proj and rep["int8_group_data"] == proj // 32
    assert all(rep.get("packed_" + k, 0) == 0 for k in ("wqkv", "wqkv64", "wo", "wo_g", "wgu", "wdown", "wdown_g"))
    assert all(t.device.type == "meta" for l in r8.w["layers"] for k, t in l.items() if k in I8.PROJECTIONS)   # no model-dtype projection left
    assert not any(k.endswith("_z8") or k.endswith("_s8") for l in r8.w["layers"] for k in l)                  # nor an unpacked (q, z, s)
    want_row_major = sum(t.numel() * 2 for t in (r8.w["embed"], r8.w["lm_head"])) + sum(l[k].numel() * 2 for l in r8.w["layers"] for k in ("ln1", "ln2"))
    assert rep["row_major"] == want_row_major
    assert r8.weight_bytes() == b16 - 2 * proj + proj + proj // 32 and r8.weight_bytes() < b16
    assert r8.max_draft_rows() == 64 and r8.tune_prefill() == {} and r8.row_major_released and r8.release_row_major()


def _dequantised_tiny(seed):
    """a tiny model whose projections hold dequantised INT8 weights: HF's forward on it is the near-tie oracle for the runner that quantises
    it on load"""
    from test_gpu_llama import tiny_llama
    lm = tiny_llama(2, seed=seed)
    for lyr in lm.model.layers:
        for a, b in PROJ:
            lin = getattr(getattr(lyr, a), b)
            with torch.no_grad():
                lin.weight.copy_(I8.dequantize_groups(*I8.quantize_groups(lin.weight.detach().to(torch.float16), torch.float16)))
    return lm


def test_int8_speculative_equals_autoregressive(monkeypatch):
    """evaluation/equal.py's criterion with INT8 weights: SAM-drafted decoding through SamdModel / DecodeEngine == the greedy output of the
    same INT8 runner, token for token (graphs on and off)"""
    import samd_sam_only as SO
    lm = _dequantised_tiny(3)
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "int8g128")
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 40).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=96, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]
    assert ar._runner.weight_format == "int8g128"
    docs = [seq_ar[len(prompt):]] + [rng.integers(3, 512, 50).tolist() for _ in range(4)] + [[i] for i in range(512)]
    cfg = SO.SamdConfig(max_predicts=16, alpha=4.0, len_bias=0)
    draft = SO.DraftModel(cfg, sam_static=SO.build_sam(docs, 2), device="cuda")
    spec = SO.SamdModel(cfg, lm, draft, eos_token_id=2, dtype=torch.float16, device="cuda")
    for use_graphs in (True, False):
        spec.set_cache(gcfg)
        spec.engine.use_graphs = use_graphs
        out = spec.generate(ids, generation_config=gcfg)
        assert spec._runner.weight_format == "int8g128"
        seq = out.output_ids[0]
        assert out.decode_steps < out.decode_tokens, "drafts were never accepted"
        m = min(len(seq), len(seq_ar))
        diff = [i for i in range(m) if seq[i] != seq_ar[i]]
        if diff:                                             # (printed for the reader of a failure: was it a near-tie of the two buckets' sums?)
            i = diff[0]
            print(f"graphs {use_graphs}: diverged at {i} of {m}; near-tie: {_near_tie(lm, seq[:i], seq[i], seq_ar[i])}")
        assert m >= len(prompt) + 90 and not diff, diff[:3]  # exactly the INT8 runner's own greedy tokens
