"""head_dim 64 without a GPU: LlamaShape takes a 64-wide Llama config and rejects other widths and the 64-wide forms that stay 128-only."""
import pytest

torch = pytest.importorskip("torch")

from samd_hip import SamdError
from samd_hip.llama import LlamaShape

LLAMA_1B = dict(model_type="llama", hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=32, num_key_value_heads=8,
                head_dim=64, vocab_size=128256, max_position_embeddings=131072, rms_norm_eps=1e-5, rope_theta=500000.0)


def test_a_64_wide_llama_is_accepted_and_other_widths_are_not():
    s = LlamaShape(LLAMA_1B)
    assert (s.head_dim, s.heads, s.kv_heads, s.qkv_bias, s.qk_norm, s.moe) == (64, 32, 8, False, False, False)
    assert LlamaShape(dict(LLAMA_1B, head_dim=None, num_key_value_heads=4)).head_dim == 64       # TinyLlama: hidden / heads
    with pytest.raises(SamdError, match="128.*64"):                                               # the message names both widths
        LlamaShape(dict(LLAMA_1B, head_dim=96))


@pytest.mark.parametrize("kind", ["qwen2", "qwen3", "qwen3_moe"])
def test_64_wide_qwen_forms_are_rejected(kind):
    cfg = dict(LLAMA_1B, model_type=kind, num_experts=8, num_experts_per_tok=2, moe_intermediate_size=256)
    assert LlamaShape(dict(cfg, head_dim=128)).head_dim == 128
    with pytest.raises(SamdError, match="head_dim 64"):
        LlamaShape(cfg)
