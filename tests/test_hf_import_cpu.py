"""samd_hip/hf_import.py without a GPU: classify puts each per-layer question to the module at most once, moves nothing, and says in a
Checkpoint what the import then does -- on the hand-built Qwen3-MoE modules of the mixture-of-experts CPU tests, one per expert form."""
import collections

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from samd_hip import hf_import as HF
from samd_hip import moe as MOE
from test_moe_cpu import qwen3_moe
from test_moe_fp8_cpu import to_fp8_moe_checkpoint
from test_moe_int4_cpu import to_int4_moe_checkpoint
from test_moe_int8_cpu import to_int8_moe_checkpoint
from test_moe_mxfp4_cpu import quantise_module

BF16 = torch.bfloat16
SPARSE = [True, False, True, True]                               # mlp_only_layers=[1]
PREDICATES = ("experts_are_int8", "experts_are_fp8", "experts_are_int4", "experts_are_4bit")
# name -> (the module made of a Qwen3-MoE module, dense format, expert format, dequantise, sparse)
FORMS = {
    "experts/model-dtype": (lambda lm: lm, None, None, None, SPARSE),
    "experts/int8g128": (lambda lm: to_int8_moe_checkpoint(lm, BF16, v2=True), None, "int8g128", None, SPARSE),
    "experts/fp8b128": (lambda lm: to_fp8_moe_checkpoint(lm, BF16), None, "fp8b128", "fp8b128", SPARSE),
    "experts/int4g128": (lambda lm: to_int4_moe_checkpoint(lm, BF16, "gptq_v2"), None, "int4g128", None, SPARSE),
    "experts/mxfp4": (lambda lm: quantise_module(lm, BF16), None, "mxfp4", None, SPARSE),
    "int4 attention beside int4 experts": (lambda lm: to_int4_moe_checkpoint(lm, BF16, "gptq_v2", attention=True), None, "int4g128", "int4g128", SPARSE),
    "fp8 attention beside fp8 experts": (lambda lm: to_fp8_moe_checkpoint(lm, BF16, "per_expert", attention=True), None, "fp8b128", "fp8b128", SPARSE),
    "dense/model-dtype": (lambda lm: lm, None, None, None, [False] * 4),
    "dense/int8g128": (lambda lm: to_int8_moe_checkpoint(lm, BF16, v2=True, attention=True), "int8g128", None, None, [False] * 4),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_classify_asks_each_layer_once_and_answers_in_data(form, monkeypatch):
    make, dense, experts, dequantise, sparse = FORMS[form]
    for env in ("SAMD_EXPERT_FORMAT", "SAMD_WEIGHT_FORMAT"):
        monkeypatch.delenv(env, raising=False)
    torch.manual_seed(7)
    ck = make(qwen3_moe(mlp_only_layers=[1] if any(sparse) else [0, 1, 2, 3])[1])
    index = {id(lyr): i for i, lyr in enumerate(ck.model.layers)}
    asked = collections.Counter()
    for name in PREDICATES:
        def counting(lyr, *a, _name=name, _real=getattr(HF, name)):
            asked[_name, index[id(lyr)]] += 1
            return _real(lyr, *a)
        monkeypatch.setattr(HF, name, counting)
    before = {n: (t.device, t.dtype, t.data_ptr()) for n, t in list(ck.named_parameters()) + list(ck.named_buffers())}
    got = HF.classify(ck, None, MOE.AUTO, BF16, True, False)
    # every per-expert scan at most once per layer, and the two that every import needs of every layer exactly once
    assert asked and max(asked.values()) == 1, asked
    assert all(asked["experts_are_fp8", i] == 1 and asked["experts_are_int4", i] == 1 for i in range(4)), asked
    assert isinstance(got, HF.Checkpoint) and got._fields == ("shape", "dtype", "sparse", "qkv_bias", "qk_norm", "dense", "experts", "dequantise",
                                                               "qcfg", "qcfg8")
    assert (got.dense.name if got.dense is not None else None) == dense
    assert got.experts is MOE.EXPERT[experts] and got.experts.name == experts
    assert got.dequantise == dequantise
    assert got.sparse == sparse == list(got.shape.sparse)
    assert got.dtype == BF16 and (got.qkv_bias, got.qk_norm) == (False, True)
    # nothing moved, nothing converted, nothing kept: the record holds no tensor, and the module's tensors are where and what they were
    assert not any(isinstance(v, torch.Tensor) for v in got)
    assert before == {n: (t.device, t.dtype, t.data_ptr()) for n, t in list(ck.named_parameters()) + list(ck.named_buffers())}
