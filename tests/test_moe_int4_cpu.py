"""INT4 (AWQ / GPTQ) experts of Qwen3-MoE without a GPU: the quantise / dequantise round trip of the fused expert tensors, every decision
about `expert_format` with three formats, from_hf on hand-built modules with per-expert AWQ / GPTQ modules (`mlp.experts.{e}.gate_proj.qweight`
...: the stacked canonical tensors against the ones quantised directly, every rejection by name, all before any device work), and static
checks of the compiled k_moe_i4_* kernels inside libsamd_hip.so."""
import copy
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from samd_hip import SamdError
from samd_hip import int4 as I4
from samd_hip import moe as MOE
from samd_hip.llama import LlamaRunner, LlamaShape
from test_codeobject_cpu import READELF, SO, gfx950_code_objects
from test_int4_weights_cpu import AWQ_CFG, GPTQ2_CFG, GPTQ_CFG, awq_module, gptq_module
from test_moe_cpu import OBJDUMP, qwen3_moe
from test_moe_mxfp4_cpu import experts, quantise_module

CONFIGS = {"awq": AWQ_CFG, "gptq": GPTQ_CFG, "gptq_v2": GPTQ2_CFG}
ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")


def qlinear(w, dtype, layout, **kw):
    """(an AWQ / GPTQ module of w [N, K] quantised per group of 128 in `dtype`, its canonical (q, z, s)).  The scales are stored as fp16, as a
    checkpoint stores them (exact for these magnitudes: asserted), so the import's one rounding to a bf16 runner gives them back."""
    q, z, s = I4.quantize_groups(w.detach().to(dtype), dtype)
    s16 = s.to(torch.float16)
    assert torch.equal(s16.to(dtype), s)
    q, z, s16 = q.cpu(), z.cpu(), s16.cpu()
    if layout == "awq":
        return awq_module(q, z, s16, **kw), (q, z, s.cpu())
    if layout == "gptq":
        assert int(z.min()) >= 1                             # (a v1 checkpoint stores z - 1; Gaussian groups of 128 straddle zero)
    return gptq_module(q, z, s16, v2=layout == "gptq_v2", **kw), (q, z, s.cpu())


class Expert(torch.nn.Module):
    """one expert of a 4-bit Qwen3-MoE checkpoint: three AWQ / GPTQ modules"""

    def __init__(self, gate, up, down):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = gate, up, down


def to_int4_moe_checkpoint(lm, dtype, layout="awq", attention=False, layers=None):
    """a 4-bit checkpoint of a Qwen3-MoE module: in every sparse layer (or `layers`) `mlp.experts` becomes a ModuleList of E Expert modules
    quantised from the fused tensors (gate = rows [:I] of gate_up_proj, up = rows [I:]); attention=True makes q / k / v / o (and a dense
    layer's MLP projections) AWQ / GPTQ modules too.  config.quantization_config is set.  `lm` is left as it is."""
    ck = copy.deepcopy(lm)
    for i, lyr in enumerate(ck.model.layers):
        ex = getattr(lyr.mlp, "experts", None)
        if ex is not None and (layers is None or i in layers):
            gu, dn = ex.gate_up_proj.detach(), ex.down_proj.detach()
            I = gu.shape[1] // 2
            lyr.mlp.experts = torch.nn.ModuleList(
                Expert(qlinear(gu[e, :I], dtype, layout)[0], qlinear(gu[e, I:], dtype, layout)[0], qlinear(dn[e], dtype, layout)[0])
                for e in range(gu.shape[0]))
        if attention:
            for p in ATTN:
                setattr(lyr.self_attn, p, qlinear(getattr(lyr.self_attn, p).weight, dtype, layout)[0])
            if ex is None:
                for p in MOE.INT4_EXPERT_PROJECTIONS:
                    setattr(lyr.mlp, p, qlinear(getattr(lyr.mlp, p).weight, dtype, layout)[0])
    ck.config.quantization_config = dict(CONFIGS[layout])
    return ck


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_quantise_dequantise_round_trip(dtype):
    """what the round trip guarantees: every dequantised weight is a value of the model dtype and a function of (q, z, s) alone, so a twin
    that holds dequantize(quantize(W)) holds exactly the weights a runner that quantised W multiplies by.  Quantising the DEQUANTISED weights
    a second time is NOT the identity for int4.py's min / max rule, unlike MXFP4's power-of-two scales: the second scale is
    rne((rne((15 - z) s) - rne(-z s)) / 15), which misses s by an ulp in 0.9 % (fp16) / 2.0 % (bf16) of Gaussian groups, and a group whose
    top code is 14 gets 14 s / 15.  The figures are printed; tests that need equal weights on both sides share one (q, z, s)."""
    E, I, H = 3, 256, 512
    gate_up, down = experts(E, I, H, 1)
    gu, dn = MOE.quantize_experts_int4(gate_up.to(dtype), down.to(dtype), dtype)
    assert [tuple(t.shape) for t in gu + dn] == [(E, 2 * I, H // 2), (E, 2 * I, H // 128), (E, 2 * I, H // 128),
                                                 (E, H, I // 2), (E, H, I // 128), (E, H, I // 128)]
    assert [t.dtype for t in gu + dn] == [torch.uint8, torch.uint8, dtype] * 2
    for e in range(E):                                           # per expert it is int4.quantize_groups, nothing else
        for have, want in zip(gu, I4.quantize_groups(gate_up[e].to(dtype), dtype)):
            assert torch.equal(have[e], want)
    w_gu, w_dn = MOE.dequantize_experts_int4(*gu), MOE.dequantize_experts_int4(*dn)
    assert w_gu.dtype == torch.float32 and tuple(w_gu.shape) == (E, 2 * I, H) and tuple(w_dn.shape) == (E, H, I)
    assert torch.equal(w_gu, w_gu.to(dtype).float()) and torch.equal(w_dn, w_dn.to(dtype).float())      # values of the model dtype
    assert torch.equal(MOE.dequantize_experts_int4(*gu, dtype=dtype).float(), w_gu)
    # dequantising again from the same (q, z, s) gives the same bits; a second quantisation moves a few groups by an ulp of their scale
    assert torch.equal(MOE.dequantize_experts_int4(*(t.clone() for t in gu)), w_gu)
    gu2, _ = MOE.quantize_experts_int4(w_gu.to(dtype), w_dn.to(dtype), dtype)
    w2 = MOE.dequantize_experts_int4(*gu2)
    print(f"{dtype}: a second quantisation changes {(w2 != w_gu).reshape(E, 2 * I, H // 128, 128).any(-1).float().mean().item():.4f} of the groups, "
          f"relative change {((w2 - w_gu).norm() / w_gu.norm()).item():.5f}")
    rel = ((w_gu - gate_up.to(dtype).float()).norm() / gate_up.norm()).item()       # int4.py: 10.1 % on Gaussian rows
    assert 0.05 < rel < 0.15, rel
    MOE.check_int4_experts(gu, dn, dtype)
    with pytest.raises(SamdError, match="do not belong together"):
        MOE.quantize_experts_int4(gate_up, down[:, :, :128], dtype)
    with pytest.raises(SamdError, match="do not belong together"):
        MOE.check_int4_experts(gu, tuple(t[:, :256] for t in dn), dtype)
    bad_z = gu[1].clone()
    bad_z[1, 5, 0] = 16
    with pytest.raises(SamdError, match=r"experts\.gate_up_proj: a zero point above 15"):
        MOE.check_int4_experts((gu[0], bad_z, gu[2]), dn, dtype)
    bad_s = dn[2].clone()
    bad_s[2, 7, 0] = 0
    with pytest.raises(SamdError, match=r"L3\.down_proj: INT4 group scales must be finite and > 0"):
        MOE.check_int4_experts(gu, (dn[0], dn[1], bad_s), dtype, "L3")
    with pytest.raises(SamdError, match="scales of dtype"):
        MOE.check_int4_experts((gu[0], gu[1], gu[2].float()), dn, dtype)
    with pytest.raises(SamdError, match=r"one per 128"):
        MOE.check_int4_experts((gu[0], gu[1][:, :, :1], gu[2]), dn, dtype)


def test_format_resolution_in_every_combination(monkeypatch):
    assert MOE.EXPERT_FORMATS == (None, "mxfp4")                 # the pinned pair; the third format lives in EXPERT_FORMATS_ALL
    assert MOE.EXPERT_FORMATS_ALL == (None, "mxfp4", "int4g128")
    R = MOE.resolve_expert_format
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    # three positional arguments and their results, as before
    assert R(MOE.AUTO, False, True) is None and R(None, False, True) is None and R("mxfp4", False, True) == "mxfp4"
    assert R(MOE.AUTO, True, True) == "mxfp4" and R("mxfp4", True, True) == "mxfp4"
    with pytest.raises(SamdError, match="expert_format=None"):
        R(None, True, True)
    # the new format, on load and from what the weights carry
    assert R("int4g128", False, True) == "int4g128"
    assert R(MOE.AUTO, False, True, carries_int4=True) == "int4g128" and R("int4g128", False, True, carries_int4=True) == "int4g128"
    for explicit in (None, "mxfp4"):
        with pytest.raises(SamdError, match="INT4 .* expert tensors"):
            R(explicit, False, True, carries_int4=True)
    with pytest.raises(SamdError, match="MXFP4.*int4g128"):
        R("int4g128", True, True)
    with pytest.raises(SamdError, match="a mix of MXFP4 and INT4"):
        R(MOE.AUTO, True, True, carries_int4=True)
    for bad in ("fp8", "int4", "int3"):
        with pytest.raises(SamdError, match="expert_format") as ei:
            R(bad, False, True)
        assert "'int4g128'" in str(ei.value) and "'mxfp4'" in str(ei.value) and "None" in str(ei.value)
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        R("int4g128", False, False)
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "int4g128")
    assert R(MOE.AUTO, False, True) == "int4g128" and R(None, False, True) is None and R(MOE.AUTO, True, True) == "mxfp4"
    # weight_format keeps its rejection, "int4g128" included
    for wf in ("fp8", "mxfp4", "int4g128"):
        with pytest.raises(SamdError, match="quantised experts are not supported"):
            MOE.reject_unsupported(wf)


def test_expert_format_int4g128_reaches_the_device_and_rejections_come_first(monkeypatch):
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    _, lm = qwen3_moe(mlp_only_layers=[0])
    with pytest.raises(SamdError, match="no MI355X"):            # quantise on load: accepted up to the point where the device is needed
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="int4g128")
    with pytest.raises(SamdError, match="native_gemm"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="int4g128", native_gemm=False)
    with pytest.raises(SamdError, match="mixture-of-experts"):   # weight_format keeps its meaning and its rejection
        LlamaRunner.from_hf(lm, 256, device="cpu", weight_format="int4g128")
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="int4g128", weight_format="int4g128")
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "int4g128")
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    # MXFP4 tensors against the INT4 format
    lm4 = quantise_module(qwen3_moe()[1])
    with pytest.raises(SamdError, match="MXFP4.*int4g128"):
        LlamaRunner.from_hf(lm4, 256, dtype=torch.bfloat16, device="cpu", expert_format="int4g128")


def test_expert_format_int4g128_on_a_dense_model_raises(monkeypatch):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    lm = Qwen3ForCausalLM(Qwen3Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                      head_dim=128, vocab_size=300))
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="int4g128")
    _, moe_dense = qwen3_moe(mlp_only_layers=[0, 1, 2, 3])
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        LlamaRunner.from_hf(moe_dense, 256, device="cpu", expert_format="int4g128")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("layout", ["awq", "gptq", "gptq_v2"])
def test_per_expert_modules_import_to_the_tensors_quantised_directly(layout, dtype):
    """the stacked (q, z, s) of a 4-bit checkpoint's expert modules are quantize_experts_int4's of the fused tensors it was made from, and the
    module passes every guard of from_hf up to the point where device work starts"""
    torch.manual_seed(3)
    cfg, lm = qwen3_moe(mlp_only_layers=[1])
    ck = to_int4_moe_checkpoint(lm, dtype, layout)
    assert LlamaRunner._hf_sparse_layers(ck.model.layers) == [True, False, True, True]
    assert LlamaRunner._hf_layer_extras(ck.model.layers) == (False, True)
    assert [LlamaRunner._hf_experts_are_int4(l, i) for i, l in enumerate(ck.model.layers)] == [True, False, True, True]
    assert not any(n.startswith("mlp.experts.") for n, _ in ck.model.layers[0].named_parameters())       # buffers, not parameters
    for i in (0, 2, 3):
        ex = lm.model.layers[i].mlp.experts
        gu, dn = MOE.quantize_experts_int4(ex.gate_up_proj.detach().to(dtype), ex.down_proj.detach().to(dtype), dtype)
        got = MOE.import_experts_int4(ck.model.layers[i].mlp.experts, f"layers.{i}.mlp.experts", dtype, "cpu", ck.config.quantization_config)
        assert sorted(got) == ["experts_down", "experts_down_s", "experts_down_z", "experts_gu", "experts_gu_s", "experts_gu_z"]
        for key, want in zip(("experts_gu", "experts_gu_z", "experts_gu_s", "experts_down", "experts_down_z", "experts_down_s"), gu + dn):
            assert got[key].dtype == want.dtype and torch.equal(got[key], want), (i, key)
        MOE.check_int4_experts(tuple(got[k] for k in ("experts_gu", "experts_gu_z", "experts_gu_s")),
                               tuple(got[k] for k in ("experts_down", "experts_down_z", "experts_down_s")), dtype)
    for kw in ({}, dict(expert_format="int4g128")):              # INT4 expert modules make the runner "int4g128" by themselves
        with pytest.raises(SamdError, match="no MI355X"):
            LlamaRunner.from_hf(ck, 256, dtype=dtype, device="cpu", **kw)
    for explicit in (None, "mxfp4"):
        with pytest.raises(SamdError, match="INT4 .* expert tensors"):
            LlamaRunner.from_hf(ck, 256, dtype=dtype, device="cpu", expert_format=explicit)
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(ck, 256, dtype=dtype, device="cpu", weight_format="int4g128")


def test_int4_attention_of_a_moe_module_is_accepted_and_an_int4_router_is_not():
    torch.manual_seed(4)
    cfg, lm = qwen3_moe(mlp_only_layers=[1])
    ck = to_int4_moe_checkpoint(lm, torch.bfloat16, "gptq_v2", attention=True)
    assert LlamaRunner._hf_layer_extras(ck.model.layers) == (False, True)
    with pytest.raises(SamdError, match="no MI355X"):            # attention and the dense layer's MLP are dequantised at import
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu", weight_format="int4g128")
    ck.model.layers[2].mlp.gate = qlinear(ck.model.layers[2].mlp.gate.weight.detach().repeat(16, 1), torch.bfloat16, "gptq_v2")[0]
    with pytest.raises(SamdError, match=r"layers\.2\.mlp\.gate: an INT4 router"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
    # INT4 attention beside model-dtype experts is no AWQ / GPTQ mixture-of-experts checkpoint: rejected as before
    ck = to_int4_moe_checkpoint(lm, torch.bfloat16, "awq", attention=True, layers=[])
    with pytest.raises(SamdError, match="quantised experts are not supported"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
    # a mix of INT4 and plain projections outside the experts still raises
    ck = to_int4_moe_checkpoint(lm, torch.bfloat16, "awq", attention=True)
    ck.model.layers[3].self_attn.o_proj = lm.model.layers[3].self_attn.o_proj
    with pytest.raises(SamdError, match="a mix of INT4 and other projections"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")


def test_rejections_reach_the_caller_by_module_name():
    torch.manual_seed(5)
    dtype = torch.float16
    cfg, lm = qwen3_moe()
    gu = lm.model.layers[0].mlp.experts.gate_up_proj.detach()

    def fresh(layout="gptq", **kw):
        return to_int4_moe_checkpoint(lm, dtype, layout, **kw)

    def load(ck, **kw):
        return LlamaRunner.from_hf(ck, 256, dtype=dtype, device="cpu", **kw)
    ck = fresh()                                                 # act-order: a g_idx other than k // g
    ck.model.layers[1].mlp.experts[5].up_proj.g_idx = ck.model.layers[1].mlp.experts[5].up_proj.g_idx.flip(0).contiguous()
    with pytest.raises(SamdError, match=r"layers\.1\.mlp\.experts\.5\.up_proj: act-order"):
        load(ck)
    ck = fresh()                                                 # desc_act in the config, no g_idx
    ck.config.quantization_config["desc_act"] = True
    del ck.model.layers[0].mlp.experts[0].gate_proj.g_idx
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts\.0\.gate_proj: act-order"):
        load(ck)
    for g in (32, 64):                                           # group sizes the kernel does not have
        ck = fresh("awq")
        m = ck.model.layers[2].mlp.experts[3].down_proj
        K, N = m.in_features, m.out_features
        m.scales = torch.ones((K // g, N), dtype=torch.float16)
        m.qzeros = torch.zeros((K // g, N // 8), dtype=torch.int32)
        ck.config.quantization_config["group_size"] = g
        with pytest.raises(SamdError, match=rf"mlp\.experts\.\d\.\w+: (group_size {g} is not supported|the tensors carry groups of)"):
            load(ck)
        ck.config.quantization_config = None
        with pytest.raises(SamdError, match=rf"layers\.2\.mlp\.experts\.3\.down_proj: group_size {g} is not supported"):
            load(ck)
    ck = fresh("awq")                                            # AWQ GEMV
    ck.config.quantization_config["version"] = "gemv"
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts\.0\.gate_proj: AWQ 'GEMV'"):
        load(ck)
    ck = fresh("gptq")                                           # a stored zero point of 15 under GPTQ v1
    ck.model.layers[3].mlp.experts[7].gate_proj.qzeros[0, 0] |= 15
    with pytest.raises(SamdError, match=r"layers\.3\.mlp\.experts\.7\.gate_proj: a stored zero point of 15"):
        load(ck)
    ck = fresh("gptq_v2")                                        # fp16 overflow of 15 * scale names bf16
    ck.model.layers[0].mlp.experts[2].down_proj.scales[0, 0] = 60000.0
    with pytest.raises(SamdError, match="bfloat16"):
        load(ck)
    # only some experts, or some of the three projections, INT4
    ck = fresh("awq")
    ck.model.layers[1].mlp.experts[4] = Expert(*(torch.nn.Linear(256, 256, bias=False) for _ in range(3)))
    with pytest.raises(SamdError, match=r"layers\.1\.mlp\.experts: a mix of INT4 and other expert projections .*layers\.1\.mlp\.experts\.4\.gate_proj"):
        load(ck)
    ck = fresh("awq")
    ck.model.layers[2].mlp.experts[6].down_proj = torch.nn.Linear(256, 256, bias=False)
    with pytest.raises(SamdError, match=r"layers\.2\.mlp\.experts\.6\.down_proj"):
        load(ck)
    ck = fresh("awq", layers=[0, 2])                             # INT4 experts in some sparse layers only
    with pytest.raises(SamdError, match="a mix of INT4 and other sparse layers"):
        load(ck)
    ck = fresh("awq")                                            # a bias on an expert projection
    ck.model.layers[0].mlp.experts[1].up_proj.bias = torch.nn.Parameter(torch.zeros(256), requires_grad=False)
    with pytest.raises(SamdError, match=r"mlp\.experts\.1\.up_proj\.bias"):
        load(ck)
    ck = fresh("awq")                                            # a shared expert
    ck.model.layers[1].mlp.shared_expert = torch.nn.Linear(256, 256, bias=False)
    with pytest.raises(SamdError, match="shared expert"):
        load(ck)
    ck = fresh("awq")                                            # fewer experts than the config says
    ck.model.layers[0].mlp.experts = torch.nn.ModuleList(list(ck.model.layers[0].mlp.experts)[:4])
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts: 4 expert modules, the config says num_experts = 8"):
        load(ck)
    assert gu.dtype == torch.float32                             # `lm` itself was never touched


def test_a_weights_dict_with_int4_experts_is_checked_before_device_work():
    cfg, lm = qwen3_moe(num_hidden_layers=1)
    s, dtype = LlamaShape(cfg), torch.bfloat16
    gate_up, down = experts(8, 256, 256, 2)
    gu, dn = MOE.quantize_experts_int4(gate_up, down, dtype)
    layer = dict(experts_gu=gu[0], experts_gu_z=gu[1], experts_gu_s=gu[2], experts_down=dn[0], experts_down_z=dn[1], experts_down_s=dn[2])
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner(s, dict(layers=[layer]), 256, dtype=dtype, device="cpu")
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner(s, dict(layers=[layer]), 256, dtype=dtype, device="cpu", expert_format="int4g128")
    for explicit in (None, "mxfp4"):
        with pytest.raises(SamdError, match="INT4 .* expert tensors"):
            LlamaRunner(s, dict(layers=[layer]), 256, dtype=dtype, device="cpu", expert_format=explicit)
    with pytest.raises(SamdError, match=r"layer 0 experts\.gate_up_proj: zero points"):
        LlamaRunner(s, dict(layers=[dict(layer, experts_gu_z=gu[1][:, :, :1])]), 256, dtype=dtype, device="cpu")
    with pytest.raises(SamdError, match=r"layer 0 experts\.down_proj: INT4 expert tensor without its zero points and scales"):
        LlamaRunner(s, dict(layers=[{k: v for k, v in layer.items() if k != "experts_down_s"}]), 256, dtype=dtype, device="cpu")
    with pytest.raises(SamdError, match="scales of dtype"):      # fp16 scales for a bf16 runner: as_scales rounds them, nothing else does
        LlamaRunner(s, dict(layers=[dict(layer, experts_gu_s=gu[2].to(torch.float16))]), 256, dtype=dtype, device="cpu")


# ------------------------------------------------------------------------------------------------ the compiled kernels
DEPTH = {1: 8, 2: 3, 3: 2, 4: 3}                                 # MoeW4Depth (csrc/gemm_kernels.hip), per row tile RT = rows / 16
WORKGROUPS_PER_CU = {1: 2, 2: 2, 3: 2, 4: 1}                     # what the depth table is chosen for
LIST_LDS = 1024                                                  # the list: 64 ints of static LDS, 1 KiB after the dynamic part's alignment


def _code_objects(tmp_path):
    blob = open(SO, "rb").read()
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        yield path


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_int4_expert_kernels_are_in_the_library_use_no_scratch_and_fit_their_lds(tmp_path):
    kernels = {}
    for path in _code_objects(tmp_path):
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:          # one kernel's entry: its keys are sorted, .agpr_count comes first
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            if "k_moe_i4_" not in name:
                continue
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"), vgprs=get("vgpr_count"),
                                 static_lds=get("group_segment_fixed_size"))
    want = {f"{kern}I{tt}Li{rt}E" for kern in ("21k_moe_i4_gate_up_silu", "13k_moe_i4_down") for tt in ("4GF16", "5GBF16") for rt in (1, 2, 3, 4)}
    assert len(kernels) == 16 and all(any(w in n for n in kernels) for w in want), sorted(kernels)     # 2 kernels x 2 dtypes x 4 row tiles
    bad = {n: v for n, v in kernels.items() if v["scratch"] or v["vgpr_spills"]}
    assert not bad, f"the INT4 expert kernels must not spill or use scratch: {bad}"
    for name, v in sorted(kernels.items()):
        rt = int(re.search(r"Li(\d)E", name).group(1))
        # the code object holds the static part only (the list).  The (DEPTH + 1) A buffers of R * 512 bytes are dynamic LDS, whose size is
        # the launch's argument and is NOT in the code object: DEPTH above restates MoeW4Depth, so this line checks the documented table
        # against the 160 KiB budget and cannot notice the kernel's table and the launch's size drifting apart (the GPU tests run every
        # row tile with streams longer than the ring, which a too-small dynamic size would not survive bit for bit)
        lds = (DEPTH[rt] + 1) * 16 * rt * 512 + v["static_lds"]
        print(name, v, "LDS", lds)
        assert v["static_lds"] == LIST_LDS, (name, v)
        assert WORKGROUPS_PER_CU[rt] * lds <= 160 * 1024, (name, lds)
        assert v["vgprs"] <= 512 // (2 * WORKGROUPS_PER_CU[rt]), (name, v)        # 8 waves per workgroup = 2 per SIMD: the registers of those workgroups
        assert (DEPTH[rt] - 1) * (3 + rt) <= 63                  # the counted wait's range (PC = 3 + XV, XV = RT)


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_no_register_copy_touches_an_in_flight_load_destination_of_the_int4_expert_gemms(tmp_path):
    """the check of test_int4_codeobject_cpu.py on k_moe_i4_*: an expert's stream is often shorter than the pipeline, so skipped prologue
    loads are the normal case; between the first hand-issued load and the first barrier behind it no v_mov reads or writes a destination"""
    found = 0
    for path in _code_objects(tmp_path):
        text = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
        for chunk in re.split(r"\n(?=[0-9a-f]+ <)", text):
            head = chunk.split("\n", 1)[0]
            if "k_moe_i4_" not in head:
                continue
            found += 1
            body = [l.split("//")[0].strip() for l in chunk.split("\n")[1:]]
            dests, load_at, group_loads = set(), [], 0
            for i, l in enumerate(body):
                m = re.match(r"global_load_dwordx([42]) v\[(\d+):(\d+)\], v\d+, s\[\d+:\d+\].* nt", l)  # (the hand-issued form: SGPR base, nt)
                if m:
                    dests |= set(range(int(m.group(2)), int(m.group(3)) + 1))
                    if m.group(1) == "4":
                        load_at.append(i)
                    else:
                        group_loads += 1
            assert len(load_at) >= 4 and group_loads >= 2, head
            assert any("global_load_lds_dwordx4" in l for l in body), f"{head}: the A tile is not filled by LDS-DMA"
            assert not any("atomic" in l for l in body), f"{head}: atomics"
            barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier") and i > load_at[0])
            bad = []
            for i in range(load_at[0], barrier):
                m = re.match(r"v_mov_b32_e32 v(\d+), (?:v(\d+))?", body[i])
                if m and (int(m.group(1)) in dests or (m.group(2) is not None and int(m.group(2)) in dests)):
                    bad.append(body[i])
            assert not bad, f"{head}: register copies of hand-issued load destinations: {bad[:8]}"
    assert found == 16, f"expected 16 INT4 expert GEMM instantiations (2 kernels x 2 dtypes x 4 row tiles), found {found}"
