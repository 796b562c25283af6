"""Qwen3-MoE on LlamaRunner against HuggingFace in fp32 on the same GPU, under REPLAYED routing.

Free-running low-precision routing is no yardstick: HF's own bf16 twin routes 5 % (E = 8, k = 2) to 37 % (E = 128, k = 8) of the rows of a tiny
model differently from fp32 and is then off by 3-4 in logits of magnitude 5.  So the HF routers are patched to take their expert INDICES from
runner.route_log (what the runner chose for the same rows); the weights stay HF's own fp32 probabilities gathered at those indices.  Then, with
the yardstick of test_gpu_qwen.py: our error <= 1.5 x the low-precision twin's under the same replayed routing + 0.02, arg-max equality on
decided rows.  Routing validity is checked separately against the fp32 model's own router logits: every expert the runner chose has a logit
>= the k-th largest - tau and every expert above the k-th + tau was chosen, tau = 2 x the largest router-logit difference between the
low-precision twin and fp32 in that run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import samd_hip
from samd_hip import SamdError
from samd_hip.llama import LlamaRunner
from test_gpu_lm_shapes import hf_low_precision_twin, tree_mask_4d, verify_against_hf

TINY = dict(hidden_size=512, intermediate_size=1024, moe_intermediate_size=256, num_hidden_layers=3, num_attention_heads=6, num_key_value_heads=2,
            head_dim=128, vocab_size=1024, max_position_embeddings=2048, rms_norm_eps=1e-6, num_experts=8, num_experts_per_tok=2)
A3B = dict(hidden_size=2048, intermediate_size=6144, moe_intermediate_size=768, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=4,
           vocab_size=151936, num_experts=128, num_experts_per_tok=8, norm_topk_prob=True)
WIDE = dict(hidden_size=4096, intermediate_size=14336, moe_intermediate_size=14336, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=8,
            vocab_size=32000, num_experts=8, num_experts_per_tok=2, norm_topk_prob=True)
# (prompt length, draft nodes): 70 = one full chunk + a part, 300 = five chunks; every row bucket 1 .. 64
PLAN = [(70, 1), (300, 8), (70, 16), (300, 32), (70, 48), (300, 64)]


def hf_moe(cfg_kw, seed, std=0.05):
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    cfg = Qwen3MoeConfig(**dict(TINY, **cfg_kw), tie_word_embeddings=False, rope_parameters=dict(rope_type="default", rope_theta=1e6))
    cfg._attn_implementation = "eager"
    torch.manual_seed(seed)
    with torch.device("cuda"):
        lm = Qwen3MoeForCausalLM(cfg)
    lm = lm.float().eval()
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g, device="cuda") * std)
            elif name.endswith(("q_norm.weight", "k_norm.weight")):
                mag = 0.5 + 1.5 * torch.rand(p.shape, generator=g, device="cuda")
                p.copy_(mag * torch.where(torch.rand(p.shape, generator=g, device="cuda") < 0.5, -1.0, 1.0))
            else:
                p.copy_(1 + 0.05 * torch.randn(p.shape, generator=g, device="cuda"))
    return lm


class Replay:
    """patches the routers of HF modules: indices from runner.route_log, in the order the runner met the rows (the prompt's 64-row chunks, then
    the draft); weights HF's own fp32 probabilities at those indices.  Keeps every model's router logits."""

    def __init__(self, runner):
        self.runner, self.ptr, self.logits = runner, {}, {}

    def reset(self):
        self.runner.route_log = []
        self.ptr, self.logits = {}, {}

    def take(self, key, li, T):
        entries = [e for e in self.runner.route_log if e[0] == li]
        p, rows, got = self.ptr.get((key, li), 0), [], 0
        while got < T:
            _, n, idx, _ = entries[p]
            rows.append(idx[:n])
            got, p = got + n, p + 1
        assert got == T, (li, got, T)
        self.ptr[(key, li)] = p
        return torch.cat(rows).long()

    def patch(self, lm, key):
        for li, lyr in enumerate(lm.model.layers):
            gate = getattr(lyr.mlp, "gate", None)
            if gate is None or not hasattr(lyr.mlp, "experts"):
                continue

            def forward(hidden_states, _gate=gate, _li=li):
                hs = hidden_states.reshape(-1, _gate.hidden_dim)
                logits = torch.nn.functional.linear(hs, _gate.weight)
                probs = torch.nn.functional.softmax(logits, dtype=torch.float, dim=-1)
                idx = self.take(key, _li, hs.shape[0])
                val = probs.gather(1, idx)
                if _gate.norm_topk_prob:
                    val = val / val.sum(dim=-1, keepdim=True)
                self.logits.setdefault((key, _li), []).append(logits.float())
                return logits, val.to(logits.dtype), idx
            gate.forward = forward


def compare(lm, lm_low, runner, replay, prompt_len, n, vocab, seed, label):
    from transformers import DynamicCache
    replay.reset()
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
    print(f"{label} L={prompt_len} n={n}: ours {e_pre:.4f} / {e_tree:.4f}, HF low precision (same routing) {hf_pre:.4f} / {hf_tree:.4f}")
    assert e_pre <= 1.5 * hf_pre + 0.02 and e_tree <= 1.5 * hf_tree + 0.02, (label, n, e_pre, hf_pre, e_tree, hf_tree)
    top2 = c["want"].topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * max(e_tree, hf_tree) + 1e-3
    assert bool((c["argmax"] == c["want"].argmax(-1))[decided].all()), label
    # routing validity against the fp32 model's own router logits
    k = runner.shape.top_k
    for li in [i for i, sp in enumerate(runner.shape.sparse) if sp]:
        ref, low = torch.cat(replay.logits[("fp32", li)]), torch.cat(replay.logits[("low", li)])
        chosen = torch.cat([e[2][:e[1]] for e in runner.route_log if e[0] == li]).long()
        assert chosen.shape[0] == ref.shape[0] == prompt_len + n
        tau = 2 * (ref - low).abs().max().item()
        srt = ref.sort(dim=-1, descending=True).values
        kth = srt[:, k - 1:k]
        gap = (srt[:, k - 1] - srt[:, k]).median().item() if k < ref.shape[1] else float("inf")
        picked = torch.zeros_like(ref, dtype=torch.bool).scatter_(1, chosen, True)
        print(f"    layer {li}: tau {tau:.4f}, median k-th gap {gap:.4f}, rows routed as fp32 {float((picked == (ref >= kth)).all(-1).float().mean()):.3f}")
        assert bool((ref.gather(1, chosen) >= kth - tau).all()), (label, li, "an expert below the k-th logit - tau was chosen")
        assert bool((picked | ~(ref > kth + tau)).all()), (label, li, "an expert above the k-th logit + tau was not chosen")


def build(cfg_kw, seed, dtype, std=0.05):
    lm = hf_moe(cfg_kw, seed, std)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype)
    lm_low = hf_low_precision_twin(lm, dtype)
    replay = Replay(runner)
    replay.patch(lm, "fp32"), replay.patch(lm_low, "low")
    return lm, lm_low, runner, replay


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("norm_topk", [True, False])
@pytest.mark.parametrize("stack", ["sparse", "mixed"])
def test_tiny_qwen3_moe_matches_hf_under_replayed_routing(dtype, norm_topk, stack):
    kw = dict(norm_topk_prob=norm_topk, **(dict(mlp_only_layers=[1]) if stack == "mixed" else {}))
    lm, lm_low, runner, replay = build(kw, seed=13 + norm_topk, dtype=dtype)
    assert runner.shape.sparse == ([True, False, True] if stack == "mixed" else [True] * 3)
    assert runner.row_major_released and runner.qkv_epilogue and not runner.norm_fold and runner.max_draft_rows() == 64
    rep = runner.memory_report()
    assert rep["packed_moe_gu"] == 2 * rep["packed_moe_down"] == sum(runner.shape.sparse) * 8 * 2 * 256 * 512 * 2
    assert all(l["experts_gu"].device.type == "meta" for l, sp in zip(runner.w["layers"], runner.shape.sparse) if sp)
    for prompt_len, n in PLAN:
        compare(lm, lm_low, runner, replay, prompt_len, n, TINY["vocab_size"], seed=prompt_len + n, label=f"{stack} norm={norm_topk} {dtype}")
    with pytest.raises(SamdError, match="row-major"):            # the 128-row bucket: the existing error
        runner.forward_rows(128, runner.pf_tokens, runner.pf_relpos, runner.pf_mask, torch.zeros(1, dtype=torch.int32, device="cuda"), runner.pf_n)


def test_many_experts_tiny(dtype=torch.bfloat16):
    lm, lm_low, runner, replay = build(dict(num_experts=128, num_experts_per_tok=8, norm_topk_prob=True), seed=5, dtype=dtype)
    for prompt_len, n in ((70, 16), (300, 64)):
        compare(lm, lm_low, runner, replay, prompt_len, n, TINY["vocab_size"], seed=n, label="E=128 k=8")


@pytest.mark.parametrize("name,cfg", [("qwen3-30b-a3b", A3B), ("wide-experts", WIDE)])
def test_real_geometry_two_layers_matches_hf(name, cfg):
    lm, lm_low, runner, replay = build(cfg, seed=3, dtype=torch.bfloat16, std=0.02)
    for prompt_len, n in ((300, 48), (70, 16), (70, 1)):
        compare(lm, lm_low, runner, replay, prompt_len, n, cfg["vocab_size"], seed=n, label=name)
    del runner, lm, lm_low, replay
    torch.cuda.empty_cache()


def test_random_init_takes_a_moe_config_and_rejections_hold_on_the_gpu():
    cfg = dict(TINY, model_type="qwen3_moe", decoder_sparse_step=2, norm_topk_prob=True)
    r = LlamaRunner.random_init(cfg, 256, torch.float16)
    assert r.shape.sparse == [False, True, False] and "moe_gu" in r.wp["layers"][1] and "moe_gu" not in r.wp["layers"][0]
    assert r.wp["layers"][0]["wgu"] is not None                  # the dense layers keep their fused gate|up form
    sess = samd_hip.Session(256)
    r.prefill(sess, torch.arange(3, 103, device="cuda")[None])
    assert r.route_log is None
    for kw in (dict(weight_format="fp8"), dict(weight_format="mxfp4"), dict(native_gemm=False)):
        with pytest.raises(SamdError, match="mixture-of-experts"):
            LlamaRunner.random_init(cfg, 256, torch.float16, **kw)
    r.draft_head = True
    with pytest.raises(SamdError, match="draft head"):
        r.warm(16)


@pytest.mark.parametrize("R,n", [(16, 11), (64, 64)])
def test_graph_replay_equals_the_eager_forward(R, n):
    lm = hf_moe(dict(norm_topk_prob=True, mlp_only_layers=[1]), seed=9)
    runner = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.bfloat16)
    rng = np.random.default_rng(4)
    sess = samd_hip.Session(512)
    runner.prefill(sess, torch.tensor([rng.integers(3, 1024, 90).tolist()], device="cuda"))
    dev = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()
    sess.set_draft(dev(rng.integers(3, 1024, n).tolist()), dev([-1] + [int(rng.integers(0, i)) for i in range(1, n)]), n, type_=1)
    runner.route_log = []
    eager = runner.verify(sess, R)["logits"][:n].clone()
    torch.cuda.synchronize()
    assert len(runner.route_log) == 2 and runner.route_log[0][1] == n
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        runner.verify(sess, R)
    assert len(runner.route_log) == 2, "route_log is ignored under capture"
    runner._buffers(R)["logits"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(runner._buffers(R)["logits"][:n], eager)


def _near_tie(runner, prefix, a, b, eps=5e-2):
    sess = samd_hip.Session(len(prefix) + 8)
    lg = runner.prefill(sess, torch.tensor([prefix], device="cuda")).float()
    return abs(lg[a].item() - lg[b].item()) < eps


def test_generate_speculative_equals_autoregressive():
    """the near-tie rule of test_gpu_qwen.py, with the logits of the SAME runner (HF in low precision routes differently)"""
    import samd_sam_only as SO
    lm = hf_moe(dict(vocab_size=512, norm_topk_prob=True, mlp_only_layers=[0]), seed=3, std=0.08).half()
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, 512, 70).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=64, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]
    probe = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=torch.float16)

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
