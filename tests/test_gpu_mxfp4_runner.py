"""LlamaRunner with MXFP4 (e2m1 + e8m0 block scale) projections: parity with HuggingFace fp32 on the dequantised weights (the yardstick of
test_gpu_lm_shapes.py: within 1.5x of HF low precision's own error), the checkpoint importer in both accepted forms against quantising on
load (bit-equal logits), Qwen2 / Qwen3 shapes, losslessness of speculative decoding against the same MXFP4 runner's greedy output, and the
memory accounting."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import samd_hip
from samd_hip import SamdError
from samd_hip import mxfp4 as MX
from samd_hip.llama import LlamaRunner
from test_gpu_fp8_runner import linears, tiny_cfg
from test_gpu_lm_shapes import hf_llama, hf_low_precision_twin, tree_mask_4d, verify_against_hf


def to_mxfp4_checkpoint(lm, dtype, form="fp4"):
    """(an MXFP4 checkpoint of lm: every projection's weight as packed e2m1 bytes + an e8m0 weight_scale, quantised from its `dtype` weights
        -- form "fp4": float4_e2m1fn_x2 + float8_e8m0fnu, "u8": uint8 + uint8; lm itself with those projections replaced by the dequantised
        weights)"""
    ck = copy.deepcopy(lm)
    for lin, lin_ref in zip(linears(ck), linears(lm)):
        q, e8 = MX.quantize_blocks(lin.weight.detach().to(dtype), dtype)
        lin.weight = torch.nn.Parameter(q.view(torch.float4_e2m1fn_x2) if form == "fp4" else q, requires_grad=False)
        lin.register_buffer("weight_scale", e8.view(torch.float8_e8m0fnu) if form == "fp4" else e8.clone())
        with torch.no_grad():
            lin_ref.weight.copy_(MX.dequantize_blocks(q, e8))
    return ck


def parity(lm, lm_low, runner, prompt_len, n, vocab, seed, label):
    """verify_against_hf + HF low precision's own error on the same case; returns the decided share of the tree rows"""
    from transformers import DynamicCache
    dtype = next(lm_low.parameters()).dtype
    e_pre, e_tree = verify_against_hf(lm, runner, prompt_len, n, vocab, tol=None, seed=seed)
    c = verify_against_hf.last
    with torch.no_grad():
        cache = DynamicCache()
        ids = torch.tensor([c["prompt"]], device="cuda")
        last_low = lm_low(input_ids=ids, past_key_values=cache, use_cache=True, logits_to_keep=1).logits[0, -1].float()
        tree_low = lm_low(input_ids=torch.tensor([c["toks"]], device="cuda"),
                          position_ids=torch.tensor([[prompt_len + x for x in c["depth"]]], device="cuda"),
                          attention_mask=tree_mask_4d(c["anc"], prompt_len, n).to(dtype), past_key_values=cache, use_cache=True).logits[0].float()
    hf_pre, hf_tree = (c["ref_last"] - last_low).abs().max().item(), (c["want"] - tree_low).abs().max().item()
    top2 = c["want"].topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * max(e_tree, hf_tree) + 1e-3
    share = decided.float().mean().item()
    print(f"{label} L={prompt_len} n={n}: ours {e_pre:.4f} / {e_tree:.4f}, HF low precision {hf_pre:.4f} / {hf_tree:.4f}, decided {share:.2f}")
    assert e_pre <= 1.5 * hf_pre + 0.02 and e_tree <= 1.5 * hf_tree + 0.02, (label, n, e_pre, hf_pre, e_tree, hf_tree)
    assert bool((c["argmax"] == c["want"].argmax(-1))[decided].all()), label
    return share


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_mxfp4_runner_matches_hf_on_dequantised_weights(dtype, kv_heads):
    lm = hf_llama(tiny_cfg(kv_heads), seed=21 + kv_heads, std=0.05)
    ck = to_mxfp4_checkpoint(lm, dtype)                  # lm now holds the dequantised weights (fp32)
    runner = LlamaRunner.from_hf(ck, max_cache_len=256, dtype=dtype)
    assert runner.weight_format == "mxfp4" and not runner.norm_fold and runner.max_draft_rows() == 64
    lm_low = hf_low_precision_twin(lm, dtype)
    for n in (1, 8, 16, 32, 48, 64):
        # a bucket's rows may all be near-ties (the 1-row bucket has one row): up to three prompts per bucket, EVERY one held to the error
        # bound and the arg-max check, and at least one with decided rows, so the arg-max check did not pass empty
        shares = []
        for seed in (n, n + 100, n + 200):
            shares.append(parity(lm, lm_low, runner, 70, n, 1024, seed=seed, label=f"mxfp4 {dtype} kv {kv_heads}"))
            if shares[-1] > 0:
                break
        assert max(shares) > 0, (n, shares)


@pytest.mark.parametrize("form", ["fp4", "u8"])
def test_checkpoint_import_equals_quantising_on_load(form):
    """from_hf on a module with packed e2m1 weights + e8m0 weight_scale == a runner that quantises the same fp16 module on load: bit-equal logits"""
    lm = hf_llama(tiny_cfg(2), seed=5, std=0.05).half()
    a = LlamaRunner.from_hf(lm, max_cache_len=256, dtype=torch.float16, weight_format="mxfp4")
    b = LlamaRunner.from_hf(to_mxfp4_checkpoint(lm, torch.float16, form), max_cache_len=256, dtype=torch.float16)
    assert a.weight_format == b.weight_format == "mxfp4"
    for la, lb in zip(a.wp["layers"], b.wp["layers"]):
        for k in MX.PROJECTIONS:
            assert torch.equal(la[k + "_f4"], lb[k + "_f4"])
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
        assert torch.isfinite(x.float()).all() and torch.equal(x, y)


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_qwen_shapes_match_hf_on_dequantised_weights(kind, dtype):
    from test_gpu_qwen import TINY, hf_qwen
    lm = hf_qwen(kind, {}, seed=21)
    ck = to_mxfp4_checkpoint(lm, dtype)                  # lm now holds the dequantised projections; biases / norms stay in lm and ck
    runner = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert runner.weight_format == "mxfp4" and runner.qkv_epilogue
    lm_low = hf_low_precision_twin(lm, dtype)
    shares = [parity(lm, lm_low, runner, prompt_len, n, TINY["vocab_size"], seed=n, label=f"mxfp4 {kind} {dtype}")
              for prompt_len, n in ((70, 1), (70, 16), (130, 64))]
    assert shares[1] > 0 and shares[2] > 0, shares       # (the 1-row bucket's single row may be a near-tie)


def test_weight_format_errors_and_env(monkeypatch):
    lm = hf_llama(tiny_cfg(2), seed=6, std=0.05)
    make = lambda: to_mxfp4_checkpoint(copy.deepcopy(lm), torch.float16)     # (a fresh one each time: nothing here copies 4-bit tensors)
    ck = make()
    with pytest.raises(SamdError, match="MXFP4 projections"):
        LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16, weight_format="fp16")
    with pytest.raises(SamdError, match="MXFP4 projections"):
        LlamaRunner.from_hf(ck, max_cache_len=128, dtype=torch.float16, weight_format="fp8")
    with pytest.raises(SamdError, match="'fp8', 'mxfp4'"):              # the unknown-format error lists all three values
        LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="int4")
    with pytest.raises(SamdError, match="native_gemm=False"):
        LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="mxfp4", native_gemm=False)
    # an exponent outside fp16's exact range: the message names bf16, and a bf16 runner takes the same checkpoint
    far = make()
    s = far.model.layers[0].mlp.down_proj.weight_scale.view(torch.uint8).clone()
    s[3, 1] = 127 + 40
    far.model.layers[0].mlp.down_proj.weight_scale = s.view(torch.float8_e8m0fnu)
    with pytest.raises(SamdError, match="bfloat16"):
        LlamaRunner.from_hf(far, max_cache_len=128, dtype=torch.float16)
    assert LlamaRunner.from_hf(far, max_cache_len=128, dtype=torch.bfloat16).weight_format == "mxfp4"
    # a mix of MXFP4 and other projections; a 4-bit lm_head
    mixed = make()
    lin = mixed.model.layers[1].mlp.up_proj
    lin.weight = torch.nn.Parameter(torch.zeros((lin.out_features, lin.in_features), device="cuda"), requires_grad=False)
    with pytest.raises(SamdError, match="mix of MXFP4"):
        LlamaRunner.from_hf(mixed, max_cache_len=128, dtype=torch.float16)
    head4 = make()
    head4.lm_head.weight = torch.nn.Parameter(torch.zeros((1024, 256), dtype=torch.uint8, device="cuda"), requires_grad=False)
    with pytest.raises(SamdError, match="lm_head"):
        LlamaRunner.from_hf(head4, max_cache_len=128, dtype=torch.float16)
    # the environment selects the format for callers that cannot pass one; an explicit argument wins
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "mxfp4")
    assert LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16).weight_format == "mxfp4"
    assert LlamaRunner.random_init(tiny_cfg(2), 128, torch.float16).weight_format == "mxfp4"
    assert LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16, weight_format="fp16").weight_format is None
    monkeypatch.delenv("SAMD_WEIGHT_FORMAT")
    assert LlamaRunner.from_hf(lm, max_cache_len=128, dtype=torch.float16).weight_format is None


def test_memory_accounting():
    cfg = dict(hidden_size=1024, intermediate_size=2816, num_hidden_layers=4, num_attention_heads=8, num_key_value_heads=8, vocab_size=1024,
               max_position_embeddings=512, rms_norm_eps=1e-5)
    r16 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2)
    b16 = r16.weight_bytes()
    proj = sum(t.numel() for l in r16.w["layers"] for k, t in l.items() if k in MX.PROJECTIONS)
    del r16
    torch.cuda.empty_cache()
    r4 = LlamaRunner.random_init(cfg, 256, torch.float16, seed=2, weight_format="mxfp4")
    rep = r4.memory_report()
    assert rep["weight_format"] == "mxfp4"
    assert sum(rep["packed_" + k + "_f4"] for k in MX.PROJECTIONS) == proj // 2 and rep["mxfp4_scales"] == proj // 32
    assert all(rep.get("packed_" + k, 0) == 0 for k in ("wqkv", "wqkv64", "wo", "wo_g", "wgu", "wdown", "wdown_g"))
    assert all(t.device.type == "meta" for l in r4.w["layers"] for k, t in l.items() if k in MX.PROJECTIONS)   # no model-dtype projection left
    want_row_major = sum(t.numel() * 2 for t in (r4.w["embed"], r4.w["lm_head"])) + sum(l[k].numel() * 2 for l in r4.w["layers"] for k in ("ln1", "ln2"))
    assert rep["row_major"] == want_row_major
    assert r4.weight_bytes() == b16 - 2 * proj + proj // 2 + proj // 32
    assert r4.max_draft_rows() == 64 and r4.tune_prefill() == {} and r4.row_major_released and r4.release_row_major()


def _ar_and_spec(lm, monkeypatch):
    import samd_sam_only as SO
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "mxfp4")
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
    to_mxfp4_checkpoint(lm, torch.float16)               # lm keeps the dequantised weights: quantising them again on load gives the same model
    return lm


def _near_tie(lm, prefix, a, b, eps=5e-2):
    with torch.no_grad():
        lg = lm(input_ids=torch.tensor([prefix], device="cuda")).logits[0, -1]
    return abs(lg[a].item() - lg[b].item()) < eps


def test_mxfp4_speculative_equals_autoregressive(monkeypatch):
    """evaluation/equal.py's criterion with MXFP4 weights: SAM-drafted decoding == the greedy output of the same MXFP4 runner (graphs on and
    off, and the granular prefill / decode form); only a near-tie may split them, and only past len(prompt) + 8"""
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
        assert spec._runner.weight_format == "mxfp4"
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
    assert not diff or (diff[0] > len(prompt) + 8 and _near_tie(lm, got[:diff[0]], got[diff[0]], seq_ar[diff[0]]))


def test_mxfp4_token_recycle_is_lossless(monkeypatch):
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
        assert not diff or (diff[0] > len(prompt) + 8 and _near_tie(lm, seq[:diff[0]], seq[diff[0]], seq_ar[diff[0]])), diff[:3]
    assert out.decode_steps < out.decode_tokens, "Token Recycle never got a draft accepted on a repeated request"
