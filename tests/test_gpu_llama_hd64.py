"""LlamaRunner on a head_dim-64 Llama (8 query / 2 KV heads): prefill + tree verify against fp32 HuggingFace with the bounds of
tests/test_gpu_llama.py, that file's speculative == autoregressive test on this model, and an INT4 runner held to the INT4 tests' yardstick."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import test_gpu_llama
from samd_hip.llama import LlamaRunner
from test_gpu_int4_runner import to_int4_checkpoint
from test_gpu_lm_shapes import hf_llama, hf_low_precision_twin, verify_against_hf
from test_gpu_mxfp4_runner import parity

CFG = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, vocab_size=512,
           max_position_embeddings=512, head_dim=64, rms_norm_eps=1e-5)


@pytest.mark.parametrize("dtype,tol", [(torch.float16, test_gpu_llama.TOL), (torch.bfloat16, 0.15)])
@pytest.mark.parametrize("prompt_len,tied", [(75, True), (150, False)])    # the 64-row chunks; the one-pass prefill (SDPA for its attention)
def test_prefill_and_tree_verify_match_hf(prompt_len, tied, dtype, tol):
    lm = hf_llama(CFG, seed=1)
    if tied:
        lm.lm_head.weight = lm.model.embed_tokens.weight
    runner = LlamaRunner.from_hf(lm, max_cache_len=256, dtype=dtype)
    assert runner.shape.head_dim == 64 and not runner.norm_fold and not runner.v_transposed
    for n in (5, 17, 33):                                   # the 8-, 32- and 48-row buckets: prefill, then a bushy tree over the cache, both < tol
        verify_against_hf(lm, runner, prompt_len, n, 512, tol, seed=n)


def test_speculative_equals_autoregressive(monkeypatch):
    """test_gpu_llama's test (graphs on and off, the granular form) with the 64-wide model in place of its 128-wide one"""
    monkeypatch.setattr(test_gpu_llama, "tiny_llama", lambda kv_heads=2, seed=0, vocab=512: hf_llama(CFG, seed))
    test_gpu_llama.test_speculative_equals_autoregressive()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_int4_runner_hd64(dtype):
    """the INT4 runner and a model-dtype runner holding the dequantised weights, both against fp32 HF on those weights"""
    lm = hf_llama(dict(CFG, vocab_size=1024), seed=23, std=0.05)
    ck = to_int4_checkpoint(lm, dtype, "awq")               # lm now holds the dequantised weights (fp32)
    runners = dict(int4=LlamaRunner.from_hf(ck, max_cache_len=256, dtype=dtype), dense=LlamaRunner.from_hf(lm, max_cache_len=256, dtype=dtype))
    assert runners["int4"].weight_format == "int4g128" and runners["dense"]._fmt is None and runners["int4"].shape.head_dim == 64
    lm_low = hf_low_precision_twin(lm, dtype)
    shares = [parity(lm, lm_low, r, 70, n, 1024, seed=n, label=f"hd64 {name} {dtype}") for n in (16, 48) for name, r in runners.items()]
    assert max(shares) > 0, shares
