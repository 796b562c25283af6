"""Qwen2 / Qwen3 support without a GPU: shape and flag parsing from the configs, every rejection of what the runner does not run (on
CPU-built modules, before any device work), the ChatML template, and the float64 restatement of the q|k|v epilogue
(tests/qkv_epilogue_ref.py) against HF's own Qwen3RMSNorm and biased nn.Linear."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from samd_hip import SamdError
from samd_hip.llama import LlamaRunner, LlamaShape
import qkv_epilogue_ref as R

TINY = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=6, num_key_value_heads=2, head_dim=128,
            vocab_size=300, max_position_embeddings=512, rms_norm_eps=1e-6)


def qwen(kind, **kw):
    from transformers import Qwen2Config, Qwen2ForCausalLM, Qwen3Config, Qwen3ForCausalLM
    C, M = (Qwen2Config, Qwen2ForCausalLM) if kind == "qwen2" else (Qwen3Config, Qwen3ForCausalLM)
    cfg = C(**dict(TINY, **kw))
    return cfg, M(cfg)


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
def test_shape_and_flags_from_qwen_configs(kind):
    cfg, lm = qwen(kind, rope_parameters=dict(rope_type="default", rope_theta=1e6))
    s = LlamaShape(cfg)
    assert (s.hidden, s.heads, s.kv_heads, s.head_dim, s.layers) == (512, 6, 2, 128, 2)
    assert s.heads * s.head_dim == 768 != s.hidden                      # q width differs from hidden
    assert s.rope_theta == 1e6
    assert (s.qkv_bias, s.qk_norm) == ((True, False) if kind == "qwen2" else (False, True))
    assert LlamaRunner._hf_layer_extras(lm.model.layers) == (s.qkv_bias, s.qk_norm)


def test_llama_with_qkv_biases_only_is_accepted_and_plain_llama_is_unchanged():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(**dict(TINY, num_attention_heads=4))
    lm = LlamaForCausalLM(cfg)
    assert LlamaRunner._hf_layer_extras(lm.model.layers) == (False, False)
    s = LlamaShape(cfg)
    assert (s.qkv_bias, s.qk_norm, s.model_type) == (False, False, "llama")
    for lyr in lm.model.layers:
        for lin in (lyr.self_attn.q_proj, lyr.self_attn.k_proj, lyr.self_attn.v_proj):
            lin.bias = torch.nn.Parameter(torch.zeros(lin.out_features))
    assert LlamaRunner._hf_layer_extras(lm.model.layers) == (True, False)


@pytest.mark.parametrize("what", ["sliding", "layer_types"])
def test_sliding_window_is_rejected(what):
    kw = dict(use_sliding_window=True, sliding_window=64, max_window_layers=0) if what == "sliding" else \
        dict(layer_types=["full_attention", "sliding_attention"], sliding_window=64)
    cfg, lm = qwen("qwen2", **kw)
    with pytest.raises(SamdError, match="sliding"):
        LlamaShape(cfg)
    with pytest.raises(SamdError, match="sliding"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def test_o_proj_bias_is_rejected():
    cfg, lm = qwen("qwen3", attention_bias=True)
    with pytest.raises(SamdError, match="o_proj"):
        LlamaShape(cfg)
    with pytest.raises(SamdError, match="o_proj"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    cfg, lm = qwen("qwen2")
    lm.model.layers[1].self_attn.o_proj.bias = torch.nn.Parameter(torch.zeros(512))
    with pytest.raises(SamdError, match="o_proj"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def test_mlp_bias_is_rejected():
    from transformers import LlamaConfig, LlamaForCausalLM
    with pytest.raises(SamdError, match="MLP"):
        LlamaShape(LlamaConfig(**dict(TINY, num_attention_heads=4), mlp_bias=True))
    cfg, lm = qwen("qwen3")
    lm.model.layers[0].mlp.down_proj.bias = torch.nn.Parameter(torch.zeros(512))
    with pytest.raises(SamdError, match="MLP"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def test_unknown_attention_parameter_is_rejected_not_dropped():
    cfg, lm = qwen("qwen3")
    lm.model.layers[1].self_attn.register_parameter("sinks", torch.nn.Parameter(torch.zeros(6)))
    with pytest.raises(SamdError, match="sinks"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    cfg, lm = qwen("qwen2")
    lm.model.layers[0].self_attn.k_proj.bias = None                     # q and v biased, k not: not a form the runner reads
    with pytest.raises(SamdError, match="k_proj.bias"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def test_patch_dict_registers_qwen():
    from transformers import Qwen2ForCausalLM, Qwen3ForCausalLM, LlamaForCausalLM
    from samd_sam_only.model_patch import patch_dict
    assert {LlamaForCausalLM, Qwen2ForCausalLM, Qwen3ForCausalLM} <= set(patch_dict)


def test_chatml_template():
    from evaluation.templates import get_conversation_template
    conv = get_conversation_template("qwen")
    conv.system = "You are helpful."
    conv.append_message(conv.roles[0], "Hi")
    conv.append_message(conv.roles[1], None)
    assert conv.get_prompt() == "<|im_start|>system\nYou are helpful.<|im_end|>\n<|im_start|>user\nHi<|im_end|>\n<|im_start|>assistant\n"
    assert conv.stop_str == "<|im_end|>"
    assert get_conversation_template("Qwen/Qwen3-8B").name == "qwen"
    assert get_conversation_template("vicuna").name == "vicuna_v1.1"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_restatement_matches_hf_qwen3_rmsnorm(dtype):
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    g = torch.Generator().manual_seed(0)
    x = (torch.randint(-63, 64, (40, 128), generator=g).float() / 64).to(dtype)       # sums of squares exact in fp32
    x[3] = 0
    norm = Qwen3RMSNorm(128, eps=1e-6).to(dtype)
    with torch.no_grad():
        norm.weight.copy_((0.5 + 1.5 * torch.rand(128, generator=g)) * torch.where(torch.rand(128, generator=g) < 0.5, -1.0, 1.0))
        want = norm(x).float()
    got = R.head_norm(x.float(), norm.weight.detach(), 1e-6, dtype)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_restatement_matches_hf_biased_linear(dtype):
    """x = round_T(sum + bias): HF's nn.Linear in fp32 on values whose products and sums are exact, rounded once to T, equals the
    restatement over split-K partials of the same product; and a bias that is far from zero moves x by many ulps"""
    g = torch.Generator().manual_seed(1)
    a = torch.randint(-8, 9, (5, 256), generator=g).float() / 16
    w = torch.randint(-8, 9, (768, 256), generator=g).float() / 16
    b = torch.randint(-120, 121, (768,), generator=g).float() / 32          # exact in bf16 as well
    lin = torch.nn.Linear(256, 768, bias=True)
    with torch.no_grad():
        lin.weight.copy_(w), lin.bias.copy_(b)
        want = lin(a).to(dtype).float()
    parts = torch.stack([a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].T for k0 in range(0, 256, 64)])
    assert torch.equal(R.epilogue_x(None, parts, b.to(dtype), dtype), want)
    assert (R.epilogue_x(None, parts, None, dtype) != want).float().mean() > 0.9


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
def test_chat_cli_loader_keeps_the_qwen_class(tmp_path, kind):
    """the chat CLIs (evaluation/chat.py run_console) load a saved checkpoint as its own class: a Qwen checkpoint read into
    LlamaForCausalLM would lose its q|k|v biases / q-k norm weights before the runner could see them.  The loaded module reaches SamdModel's
    runner factory with its extra parameters intact."""
    import samd_sam_only as SO
    from evaluation.chat import load_lm
    cfg, lm = qwen(kind)
    lm.save_pretrained(tmp_path)
    got = load_lm(str(tmp_path), torch.float32, "cpu")
    assert type(got) is type(lm)
    assert LlamaRunner._hf_layer_extras(got.model.layers) == ((True, False) if kind == "qwen2" else (False, True))
    model = SO.SamdModel(SO.SamdConfig(max_predicts=8), got, None, 2, torch.float32, "cpu")
    assert model._runner_factory is not None


def test_eagle_heads_refuse_a_qwen_base_module():
    """EAGLE / EAGLE-2 heads are Llama-only: an HF Qwen module as the base model (whose runner does not exist yet) raises, a Llama one does not"""
    from transformers import LlamaConfig, LlamaForCausalLM
    from samd.tree_model.eagle2 import Eagle2, Eagle2Head
    head_cfg = dict(hidden_size=512, intermediate_size=512, num_attention_heads=4, num_key_value_heads=4, vocab_size=300, rms_norm_eps=1e-5, bias=True)
    for kind in ("qwen2", "qwen3"):
        _, lm = qwen(kind)
        with pytest.raises(SamdError, match="Llama base models only"):
            Eagle2(None, lm, torch.float32, "cpu", head=Eagle2Head(head_cfg, dtype=torch.float32, device="cpu"))
    llama = LlamaForCausalLM(LlamaConfig(**dict(TINY, num_attention_heads=4)))
    Eagle2(None, llama, torch.float32, "cpu", head=Eagle2Head(head_cfg, dtype=torch.float32, device="cpu"))


def test_fp8_scales_held_as_parameters_are_the_projections_own():
    """an FP8 checkpoint whose projections keep weight_scale / input_scale as nn.Parameters (not buffers) passes the layer guard, with its
    Qwen extras recognised; any other extra parameter still raises"""
    _, lm = qwen("qwen2")
    for lyr in lm.model.layers:
        for lin in (lyr.self_attn.q_proj, lyr.self_attn.k_proj, lyr.self_attn.v_proj, lyr.self_attn.o_proj, lyr.mlp.gate_proj, lyr.mlp.up_proj,
                    lyr.mlp.down_proj):
            lin.weight = torch.nn.Parameter(lin.weight.detach().to(torch.float8_e4m3fn), requires_grad=False)
            lin.weight_scale = torch.nn.Parameter(torch.ones(lin.out_features, 1), requires_grad=False)
            lin.input_scale = torch.nn.Parameter(torch.ones(()), requires_grad=False)
    assert LlamaRunner._hf_layer_extras(lm.model.layers) == (True, False)
    lm.model.layers[0].input_layernorm.weight_scale = torch.nn.Parameter(torch.ones(()))     # not a projection's: extra
    with pytest.raises(SamdError, match="input_layernorm.weight_scale"):
        LlamaRunner._hf_layer_extras(lm.model.layers)
