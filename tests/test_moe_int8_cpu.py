"""INT8 (GPTQ) experts of Qwen3-MoE without a GPU: the quantise / dequantise round trip of the fused expert tensors, every decision about
`expert_format` with the fifth format, the raw-dict keys, from_hf on hand-built modules with per-expert 8-bit GPTQ modules
(`mlp.experts.{e}.gate_proj.qweight` ...: the stacked canonical tensors against the ones quantised directly, every rejection by name, all
before any device work), and static checks of the compiled k_moe_i8_* / k_moew_i8_* kernels inside libsamd_hip.so."""
import copy
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from samd_hip import SamdError
from samd_hip import int8 as I8
from samd_hip import moe as MOE
from samd_hip.llama import LlamaRunner, LlamaShape
from test_codeobject_cpu import READELF, SO, gfx950_code_objects
from test_int8_weights_cpu import GPTQ8_CFG, GPTQ8V2_CFG, gptq8_module
from test_moe_cpu import OBJDUMP, qwen3_moe
from test_moe_int4_cpu import Expert, to_int4_moe_checkpoint
from test_moe_mxfp4_cpu import experts, quantise_module

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
GKEYS, DKEYS = ("experts_gu", "experts_gu_z8", "experts_gu_s8"), ("experts_down", "experts_down_z8", "experts_down_s8")


def qlinear8(w, dtype, v2=False, g=128, **kw):
    """(an 8-bit GPTQ module of w [N, K] quantised per group of 128 in `dtype`, its canonical (q, z, s)).  The scales are stored as fp16, as a
    checkpoint stores them (exact for these magnitudes: asserted), so the import's one rounding to a bf16 runner gives them back.  g = 256:
    the module stores one (z, s) per 256 -- the pair of every second canonical group, which the import repeats."""
    q, z, s = I8.quantize_groups(w.detach().to(dtype), dtype)
    if g != 128:
        rep = g // 128
        z, s = z[:, ::rep].repeat_interleave(rep, dim=1).contiguous(), s[:, ::rep].repeat_interleave(rep, dim=1).contiguous()
    s16 = s.to(torch.float16)
    assert torch.equal(s16.to(dtype), s)
    q, z, s16 = q.cpu(), z.cpu(), s16.cpu()
    if not v2:
        assert int(z.min()) >= 1 and int(z.max()) <= 255         # (a v1 checkpoint stores z - 1; Gaussian groups of 128 straddle zero)
    rep = g // 128
    return gptq8_module(q, z[:, ::rep].contiguous(), s16[:, ::rep].contiguous(), g=g, v2=v2, **kw), (q, z, s.cpu())


def to_int8_moe_checkpoint(lm, dtype, v2=False, attention=False, layers=None, g=128):
    """a GPTQ-Int8 checkpoint of a Qwen3-MoE module: in every sparse layer (or `layers`) `mlp.experts` becomes a ModuleList of E Expert modules
    quantised from the fused tensors (gate = rows [:I] of gate_up_proj, up = rows [I:]); attention=True makes q / k / v / o (and a dense
    layer's MLP projections) 8-bit GPTQ modules too.  config.quantization_config is set.  `lm` is left as it is."""
    ck = copy.deepcopy(lm)
    ql = lambda w: qlinear8(w, dtype, v2, g)[0]
    for i, lyr in enumerate(ck.model.layers):
        ex = getattr(lyr.mlp, "experts", None)
        if ex is not None and (layers is None or i in layers):
            gu, dn = ex.gate_up_proj.detach(), ex.down_proj.detach()
            I = gu.shape[1] // 2
            lyr.mlp.experts = torch.nn.ModuleList(Expert(ql(gu[e, :I]), ql(gu[e, I:]), ql(dn[e])) for e in range(gu.shape[0]))
        if attention:
            for p in ATTN:
                setattr(lyr.self_attn, p, ql(getattr(lyr.self_attn, p).weight))
            if ex is None:
                for p in MOE.INT4_EXPERT_PROJECTIONS:
                    setattr(lyr.mlp, p, ql(getattr(lyr.mlp, p).weight))
    ck.config.quantization_config = dict(GPTQ8V2_CFG if v2 else GPTQ8_CFG, group_size=g)
    return ck


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_quantise_dequantise_check_round_trip(dtype):
    E, I, H = 3, 256, 512
    gate_up, down = experts(E, I, H, 1)
    gu, dn = MOE.quantize_experts_int8(gate_up.to(dtype), down.to(dtype), dtype)
    assert [tuple(t.shape) for t in gu + dn] == [(E, 2 * I, H), (E, 2 * I, H // 128), (E, 2 * I, H // 128), (E, H, I), (E, H, I // 128), (E, H, I // 128)]
    assert [t.dtype for t in gu + dn] == [torch.uint8, torch.uint8, dtype] * 2
    for e in range(E):                                           # per expert it is int8.quantize_groups, nothing else
        for have, want in zip(gu, I8.quantize_groups(gate_up[e].to(dtype), dtype)):
            assert torch.equal(have[e], want)
        for have, want in zip(dn, I8.quantize_groups(down[e].to(dtype), dtype)):
            assert torch.equal(have[e], want)
    w_gu, w_dn = MOE.dequantize_experts_int8(*gu), MOE.dequantize_experts_int8(*dn)
    assert w_gu.dtype == torch.float32 and tuple(w_gu.shape) == (E, 2 * I, H) and tuple(w_dn.shape) == (E, H, I)
    assert torch.equal(w_gu, w_gu.to(dtype).float()) and torch.equal(w_dn, w_dn.to(dtype).float())      # values of the model dtype
    assert torch.equal(MOE.dequantize_experts_int8(*gu, dtype=dtype).float(), w_gu)
    assert torch.equal(w_gu[1], I8.dequantize_groups(gu[0][1], gu[1][1], gu[2][1]))
    rel = ((w_gu - gate_up.to(dtype).float()).norm() / gate_up.norm()).item()       # int8.py: 0.6 % on Gaussian rows
    assert 0.003 < rel < 0.01, rel
    MOE.check_int8_experts(gu, dn, dtype)
    with pytest.raises(SamdError, match="do not belong together"):
        MOE.quantize_experts_int8(gate_up, down[:, :, :128], dtype)
    with pytest.raises(SamdError, match="do not belong together"):
        MOE.check_int8_experts(gu, tuple(t[:, :256] for t in dn), dtype)
    with pytest.raises(SamdError, match=r"experts\.gate_up_proj: INT8 codes and zero points are uint8"):
        MOE.check_int8_experts((gu[0].to(torch.int32), gu[1], gu[2]), dn, dtype)
    bad_s = dn[2].clone()
    bad_s[2, 7, 0] = 0
    with pytest.raises(SamdError, match=r"L3\.down_proj: INT8 group scales must be finite and > 0"):
        MOE.check_int8_experts(gu, (dn[0], dn[1], bad_s), dtype, "L3")
    with pytest.raises(SamdError, match="scales of dtype"):
        MOE.check_int8_experts((gu[0], gu[1], gu[2].float()), dn, dtype)
    with pytest.raises(SamdError, match=r"one per 128"):
        MOE.check_int8_experts((gu[0], gu[1][:, :, :1], gu[2]), dn, dtype)
    with pytest.raises(SamdError, match=r"down_proj: INT8 expert tensor without its zero points and scales"):
        MOE.check_int8_experts(gu, (dn[0], None, dn[2]), dtype)
    with pytest.raises(SamdError, match="N % 128 == 0 and K % 256 == 0"):
        MOE.check_int8_experts(tuple(t[:, :64] for t in gu), dn, dtype)
    # INT4 halves of the same shapes are not INT8 tensors: the codes are one per byte
    with pytest.raises(SamdError, match="one per 128"):
        MOE.check_int8_experts((gu[0][:, :, :H // 2], gu[1], gu[2]), dn, dtype)
    assert I8.packed_bytes(2 * I, H) * 32 == 2 * I * H * 33


def test_pack_refuses_before_the_device_and_buffers_of_other_formats_are_told_apart():
    """pack_experts_int8 checks first (no device needed to be refused); the launch guards work on marks and byte counts alone"""
    E, I, H = 8, 256, 256
    gate_up, down = experts(E, I, H, 2)
    gu, dn = MOE.quantize_experts_int8(gate_up, down, torch.float16)
    with pytest.raises(SamdError, match="scales of dtype"):
        MOE.pack_experts_int8(gu, dn, torch.bfloat16)
    b = MOE.MoeBuffers.__new__(MOE.MoeBuffers)
    b.rows_pad, b.hidden, b.moe_inter, b.n_experts, b.top_k, b.dt = 16, H, I, E, 2, 0
    want_gu, want_dn = E * I8.packed_bytes(2 * I, H), E * I8.packed_bytes(H, I)
    assert (want_gu, want_dn) == (E * 2 * I * H * 33 // 32, E * H * I * 33 // 32)
    pgu, pdn = torch.zeros(want_gu, dtype=torch.uint8), torch.zeros(want_dn, dtype=torch.uint8)
    h = d_n = torch.zeros(1)
    for bufs in (b, ):
        with pytest.raises(SamdError, match="pack_experts_int8 did not return"):         # right size, no mark: fails closed
            MOE.MoeBuffers.experts(bufs, h, pgu, pdn, d_n, "int8g128")
        with pytest.raises(SamdError, match="pack_experts_int8 did not return"):
            MOE._check_expert_buffers(bufs, pgu, pdn, "int8g128")
    pgu.expert_format = pdn.expert_format = "int8g128"
    MOE._check_expert_buffers(b, pgu, pdn, "int8g128")
    with pytest.raises(SamdError, match="pack_experts_int8 did not return"):             # a view loses the mark
        MOE._check_expert_buffers(b, pgu[:], pdn, "int8g128")
    with pytest.raises(SamdError, match=r"int8g128 gate\|up expert buffer"):             # swapped buffers: the byte counts differ
        MOE._check_expert_buffers(b, pdn, pgu, "int8g128")
    for other in (None, "mxfp4", "int4g128", "fp8b128"):                                 # an INT8 buffer under another format's launch
        with pytest.raises(SamdError, match="an INT8 expert buffer"):
            MOE.MoeBuffers.experts(b, h, pgu, pdn, d_n, other)
        with pytest.raises(SamdError, match="an INT8 expert buffer"):
            MOE._check_expert_buffers(b, pgu, pdn, other)
    i4 = torch.zeros(E * 2 * I * H * 17 // 32, dtype=torch.uint8)                        # another format's buffer under the INT8 launch
    i4.expert_format = "int4g128"
    with pytest.raises(SamdError, match="int8g128 gate"):
        MOE.MoeBuffers.experts(b, h, i4, i4, d_n, "int8g128")
    with pytest.raises(SamdError, match="expert_format 'int8'"):
        MOE.MoeBuffers.experts(b, h, pgu, pdn, d_n, "int8")


def test_format_resolution_with_the_fifth_format(monkeypatch):
    # the pinned constants keep their values; the wider ones sit beside them
    assert MOE.EXPERT_FORMATS == (None, "mxfp4") and MOE.EXPERT_FORMATS_ALL == (None, "mxfp4", "int4g128")
    assert MOE.EXPERT_FORMATS_KNOWN == (None, "mxfp4", "int4g128", "fp8b128")
    assert MOE.EXPERT_FORMATS_SERVED == MOE.EXPERT_FORMATS_KNOWN + ("int8g128",)
    assert MOE.WIDE_FORMAT_CODES == {None: 0, "mxfp4": 1, "int4g128": 2, "fp8b128": 3}
    assert MOE.WIDE_FORMAT_CODES_SERVED == dict(MOE.WIDE_FORMAT_CODES, int8g128=5) and set(MOE.WIDE_FORMAT_CODES_SERVED) == set(MOE.EXPERT_FORMATS_SERVED)
    R = MOE.resolve_expert_format
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    assert R("int8g128", False, True) == "int8g128"                                      # on load
    assert R(MOE.AUTO, False, True, carries_int8=True) == "int8g128" and R("int8g128", False, True, carries_int8=True) == "int8g128"
    for explicit in (None, "mxfp4", "int4g128", "fp8b128"):                              # an explicit mismatch
        with pytest.raises(SamdError, match="INT8 .* expert tensors"):
            R(explicit, False, True, carries_int8=True)
    for kw in (dict(carries_4bit=True), dict(carries_int4=True), dict(carries_fp8=True)):      # a mix
        with pytest.raises(SamdError, match="a mix of INT8 and other"):
            R(MOE.AUTO, kw.pop("carries_4bit", False), True, carries_int8=True, **kw)
    for kw in (dict(carries_int4=True), dict(carries_fp8=True)):                         # the format against other tensors
        with pytest.raises(SamdError, match="int8g128"):
            R("int8g128", False, True, **kw)
    with pytest.raises(SamdError, match="int8g128"):
        R("int8g128", True, True)
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        R("int8g128", False, False)
    with pytest.raises(SamdError, match="expert_format") as ei:
        R("int8", False, True)
    assert "'int8g128'" in str(ei.value) and "'int4g128'" in str(ei.value)
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "int8g128")
    assert R(MOE.AUTO, False, True) == "int8g128" and R(None, False, True) is None and R(MOE.AUTO, True, True) == "mxfp4"
    assert R(MOE.AUTO, False, True, carries_int4=True) == "int4g128"                     # what the weights carry wins over the environment
    for wf in ("fp8", "mxfp4", "int4g128", "int8g128"):                                  # weight_format keeps its rejection and its message
        with pytest.raises(SamdError, match=f"not available with weight_format '{wf}': quantised experts are not supported"):
            MOE.reject_unsupported(wf)


def test_expert_format_int8g128_reaches_the_device_and_rejections_come_first(monkeypatch):
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    _, lm = qwen3_moe(mlp_only_layers=[0])
    with pytest.raises(SamdError, match="no MI355X"):            # quantise on load: accepted up to the point where the device is needed
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="int8g128")
    with pytest.raises(SamdError, match="native_gemm"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="int8g128", native_gemm=False)
    for kw in (dict(weight_format="int8g128"), dict(expert_format="int8g128", weight_format="int8g128")):
        with pytest.raises(SamdError, match="mixture-of-experts"):       # weight_format keeps its meaning and its rejection
            LlamaRunner.from_hf(lm, 256, device="cpu", **kw)
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "int8g128")
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    lm4 = quantise_module(qwen3_moe()[1])                         # MXFP4 tensors against the INT8 format
    with pytest.raises(SamdError, match="int8g128"):
        LlamaRunner.from_hf(lm4, 256, dtype=torch.bfloat16, device="cpu", expert_format="int8g128")
    _, dense = qwen3_moe(mlp_only_layers=[0, 1, 2, 3])
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        LlamaRunner.from_hf(dense, 256, device="cpu", expert_format="int8g128")


def test_a_weights_dict_with_int8_experts_is_checked_before_device_work():
    cfg, lm = qwen3_moe(num_hidden_layers=1)
    s, dtype = LlamaShape(cfg), torch.bfloat16
    gate_up, down = experts(8, 256, 256, 2)
    gu, dn = MOE.quantize_experts_int8(gate_up, down, dtype)
    layer = dict(zip(GKEYS + DKEYS, gu + dn))
    assert layer["experts_gu"].dtype == torch.uint8 and tuple(layer["experts_gu"].shape) == (8, 512, 256)
    assert tuple(layer["experts_gu_z8"].shape) == tuple(layer["experts_gu_s8"].shape) == (8, 512, 2) and layer["experts_gu_s8"].dtype == dtype
    for kw in ({}, dict(expert_format="int8g128")):              # the _z8 / _s8 keys make the runner "int8g128" by themselves
        with pytest.raises(SamdError, match="no MI355X"):
            LlamaRunner(s, dict(layers=[layer]), 256, dtype=dtype, device="cpu", **kw)
    for explicit in (None, "mxfp4", "int4g128", "fp8b128"):
        with pytest.raises(SamdError, match="INT8 .* expert tensors"):
            LlamaRunner(s, dict(layers=[layer]), 256, dtype=dtype, device="cpu", expert_format=explicit)
    with pytest.raises(SamdError, match=r"layer 0 experts\.gate_up_proj: zero points"):
        LlamaRunner(s, dict(layers=[dict(layer, experts_gu_z8=gu[1][:, :, :1])]), 256, dtype=dtype, device="cpu")
    with pytest.raises(SamdError, match=r"layer 0 experts\.down_proj: INT8 expert tensor without its zero points and scales"):
        LlamaRunner(s, dict(layers=[{k: v for k, v in layer.items() if k != "experts_down_s8"}]), 256, dtype=dtype, device="cpu")
    with pytest.raises(SamdError, match="scales of dtype"):      # fp16 scales for a bf16 runner: as_scales rounds them, nothing else does
        LlamaRunner(s, dict(layers=[dict(layer, experts_gu_s8=gu[2].to(torch.float16))]), 256, dtype=dtype, device="cpu")
    # the INT4 keys beside 8-bit tensors are INT4's: the names cannot be mistaken for one another
    i4ish = {k.replace("_z8", "_z").replace("_s8", "_s"): v for k, v in layer.items()}
    with pytest.raises(SamdError, match="of another format; expert_format='int8g128'"):
        LlamaRunner(s, dict(layers=[i4ish]), 256, dtype=dtype, device="cpu", expert_format="int8g128")
    with pytest.raises(SamdError, match=r"for \[8, 512, 512\] experts"):             # with no argument they are read as INT4 (two codes per byte) and fail its checks
        LlamaRunner(s, dict(layers=[i4ish]), 256, dtype=dtype, device="cpu")
    with pytest.raises(SamdError, match="a mix of INT8 and other"):
        LlamaRunner(s, dict(layers=[dict(layer, experts_gu_z=gu[1])]), 256, dtype=dtype, device="cpu")
    two = LlamaShape(qwen3_moe(num_hidden_layers=2)[0])
    with pytest.raises(SamdError, match="a mix of INT8 and other sparse layers"):
        LlamaRunner(two, dict(layers=[layer, dict(experts_gu=gate_up.to(dtype), experts_down=down.to(dtype))]), 256, dtype=dtype, device="cpu")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("layout", ["gptq", "gptq_v2"])
def test_per_expert_modules_import_to_the_tensors_quantised_directly(layout, dtype):
    """the stacked (q, z, s) of a GPTQ-Int8 checkpoint's expert modules are quantize_experts_int8's of the fused tensors it was made from
    (the bf16 runner's scales: the checkpoint's fp16 ones rounded once), and the module passes every guard of from_hf up to the device"""
    torch.manual_seed(3)
    cfg, lm = qwen3_moe(mlp_only_layers=[1])
    ck = to_int8_moe_checkpoint(lm, dtype, v2=layout == "gptq_v2")
    assert LlamaRunner._hf_sparse_layers(ck.model.layers) == [True, False, True, True]
    assert LlamaRunner._hf_layer_extras(ck.model.layers) == (False, True)
    qcfg = ck.config.quantization_config
    assert [LlamaRunner._hf_experts_are_int8(l, qcfg) for l in ck.model.layers] == [True, False, True, True]
    for i in (0, 2, 3):
        ex = lm.model.layers[i].mlp.experts
        gu, dn = MOE.quantize_experts_int8(ex.gate_up_proj.detach().to(dtype), ex.down_proj.detach().to(dtype), dtype)
        got = MOE.import_experts_int8(ck.model.layers[i].mlp.experts, f"layers.{i}.mlp.experts", dtype, "cpu", qcfg)
        assert sorted(got) == sorted(GKEYS + DKEYS)
        for key, want in zip(GKEYS + DKEYS, gu + dn):
            assert got[key].dtype == want.dtype and torch.equal(got[key], want), (i, key)
        MOE.check_int8_experts(tuple(got[k] for k in GKEYS), tuple(got[k] for k in DKEYS), dtype)
    for kw in ({}, dict(expert_format="int8g128")):              # 8-bit expert modules make the runner "int8g128" by themselves
        with pytest.raises(SamdError, match="no MI355X"):
            LlamaRunner.from_hf(ck, 256, dtype=dtype, device="cpu", **kw)
    for explicit in (None, "mxfp4", "int4g128", "fp8b128"):
        with pytest.raises(SamdError, match="INT8 .* expert tensors"):
            LlamaRunner.from_hf(ck, 256, dtype=dtype, device="cpu", expert_format=explicit)
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(ck, 256, dtype=dtype, device="cpu", weight_format="int8g128")


def test_a_group_size_of_256_is_expanded_and_bf16_scales_are_rounded_once():
    torch.manual_seed(6)
    cfg, lm = qwen3_moe()
    ck = to_int8_moe_checkpoint(lm, torch.float16, v2=True, g=256)
    m = ck.model.layers[1].mlp.experts[3].down_proj
    assert tuple(m.scales.shape) == (1, 256) and tuple(m.qzeros.shape) == (1, 64)       # K = 256: one group of 256
    m = ck.model.layers[1].mlp.experts[3].gate_proj
    got = MOE.import_experts_int8(ck.model.layers[1].mlp.experts, "layers.1.mlp.experts", torch.float16, "cpu", ck.config.quantization_config)
    q, z, s = I8.linear_int8(m, "p", config=ck.config.quantization_config)
    assert tuple(s.shape) == (256, 2) and torch.equal(s[:, 0], s[:, 1]) and torch.equal(z[:, 0], z[:, 1])
    assert torch.equal(got["experts_gu"][3, :256], q) and torch.equal(got["experts_gu_z8"][3, :256], z) and torch.equal(got["experts_gu_s8"][3, :256], s)
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.float16, device="cpu")
    # a bf16 runner: every fp16 scale of the checkpoint rounded ONCE to bf16, scales that are not bf16 values included
    for e in range(8):
        sc = ck.model.layers[0].mlp.experts[e].up_proj.scales
        sc.copy_((sc.float() * (1 + 2.0 ** -10)).to(torch.float16))
    fp16_s = torch.stack([torch.cat([ck.model.layers[0].mlp.experts[e].gate_proj.scales.t(), ck.model.layers[0].mlp.experts[e].up_proj.scales.t()])
                          for e in range(8)])
    got = MOE.import_experts_int8(ck.model.layers[0].mlp.experts, "layers.0.mlp.experts", torch.bfloat16, "cpu", ck.config.quantization_config)
    assert got["experts_gu_s8"].dtype == torch.bfloat16 and torch.equal(got["experts_gu_s8"], fp16_s.repeat_interleave(2, dim=2).to(torch.bfloat16))
    assert not torch.equal(got["experts_gu_s8"].float(), fp16_s.repeat_interleave(2, dim=2).float())     # the rounding did something


def test_int8_attention_of_a_moe_module_is_accepted_and_an_int8_router_is_not():
    torch.manual_seed(4)
    cfg, lm = qwen3_moe(mlp_only_layers=[1])
    ck = to_int8_moe_checkpoint(lm, torch.bfloat16, v2=True, attention=True)
    assert LlamaRunner._hf_layer_extras(ck.model.layers) == (False, True)
    with pytest.raises(SamdError, match="no MI355X"):            # attention and the dense layer's MLP are dequantised at import
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu", weight_format="int8g128")
    ck.model.layers[2].mlp.gate = qlinear8(ck.model.layers[2].mlp.gate.weight.detach().repeat(16, 1), torch.bfloat16, v2=True)[0]
    with pytest.raises(SamdError, match=r"layers\.2\.mlp\.gate: an 8-bit router"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
    # 8-bit attention beside model-dtype experts is no GPTQ-Int8 mixture-of-experts checkpoint: rejected as before, by module name
    ck = to_int8_moe_checkpoint(lm, torch.bfloat16, v2=True, attention=True, layers=[])
    with pytest.raises(SamdError, match=r"layers\.0\.self_attn\.q_proj: an 8-bit GPTQ module in a mixture-of-experts model"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
    # a mix of 8-bit and plain projections outside the experts still raises
    ck = to_int8_moe_checkpoint(lm, torch.bfloat16, v2=True, attention=True)
    ck.model.layers[3].self_attn.o_proj = lm.model.layers[3].self_attn.o_proj
    with pytest.raises(SamdError, match="a mix of INT8 and other projections"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")


def test_rejections_reach_the_caller_by_module_name():
    torch.manual_seed(5)
    dtype = torch.float16
    cfg, lm = qwen3_moe()
    gu = lm.model.layers[0].mlp.experts.gate_up_proj.detach()

    def fresh(v2=False, **kw):
        return to_int8_moe_checkpoint(lm, dtype, v2, **kw)

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
        ck = fresh()
        m = ck.model.layers[2].mlp.experts[3].down_proj
        K, N = m.in_features, m.out_features
        m.scales = torch.ones((K // g, N), dtype=torch.float16)
        m.qzeros = torch.zeros((K // g, N // 4), dtype=torch.int32)
        ck.config.quantization_config["group_size"] = g
        with pytest.raises(SamdError, match=rf"mlp\.experts\.\d\.\w+: (group_size {g} is not supported|the tensors carry groups of)"):
            load(ck)
        ck.config.quantization_config = dict(bits=8)
        with pytest.raises(SamdError, match=rf"layers\.2\.mlp\.experts\.3\.down_proj: group_size {g} is not supported"):
            load(ck)
    ck = fresh()                                                 # AWQ
    ck.config.quantization_config["quant_method"] = "awq"
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts\.0\.gate_proj: quant_method 'awq'"):
        load(ck)
    ck = fresh()                                                 # a stored zero point of 255 under GPTQ v1
    ck.model.layers[3].mlp.experts[7].gate_proj.qzeros[0, 0] |= 255
    with pytest.raises(SamdError, match=r"layers\.3\.mlp\.experts\.7\.gate_proj: a stored zero point of 255"):
        load(ck)
    ck = fresh(v2=True)                                          # fp16 overflow of 255 * scale names bf16
    ck.model.layers[0].mlp.experts[2].down_proj.scales[0, 0] = 60000.0
    with pytest.raises(SamdError, match="bfloat16"):
        load(ck)
    # only some experts, or some of the three projections, 8-bit: the opening of the blanket rejection, by module name
    ck = fresh()
    ck.model.layers[1].mlp.experts[4] = Expert(*(torch.nn.Linear(256, 256, bias=False) for _ in range(3)))
    with pytest.raises(SamdError, match=r"layers\.1\.mlp\.experts\.0\.gate_proj: an 8-bit GPTQ module in a mixture-of-experts model"):
        load(ck)
    ck4 = to_int4_moe_checkpoint(lm, dtype, "gptq")               # an INT4 checkpoint with one expert projection 8-bit
    w = lm.model.layers[2].mlp.experts.down_proj.detach()[0]
    ck4.model.layers[2].mlp.experts[0].down_proj = qlinear8(w, dtype)[0]
    ck4.config.quantization_config = None
    with pytest.raises(SamdError, match=r"layers\.2\.mlp\.experts\.0\.down_proj: an 8-bit GPTQ module in a mixture-of-experts model"):
        load(ck4)
    ck = fresh()                                                 # one projection of one expert 4-bit among 8-bit ones
    ck.config.quantization_config = None                         # (each module's width by its qweight's shape)
    ck.model.layers[2].mlp.experts[6].down_proj = to_int4_moe_checkpoint(lm, dtype, "gptq").model.layers[2].mlp.experts[6].down_proj
    with pytest.raises(SamdError, match=r"layers\.2\.mlp\.experts\.0\.gate_proj: an 8-bit GPTQ module in a mixture-of-experts model"):
        load(ck)
    ck = fresh(layers=[0, 2])                                    # 8-bit experts in some sparse layers only
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts\.0\.gate_proj: an 8-bit GPTQ module in a mixture-of-experts model"):
        load(ck)
    ck = fresh()                                                 # a bias on an expert projection
    ck.model.layers[0].mlp.experts[1].up_proj.bias = torch.nn.Parameter(torch.zeros(256), requires_grad=False)
    with pytest.raises(SamdError, match=r"mlp\.experts\.1\.up_proj\.bias"):
        load(ck)
    ck = fresh()                                                 # a shared expert
    ck.model.layers[1].mlp.shared_expert = torch.nn.Linear(256, 256, bias=False)
    with pytest.raises(SamdError, match="shared expert"):
        load(ck)
    ck = fresh()                                                 # fewer experts than the config says
    ck.model.layers[0].mlp.experts = torch.nn.ModuleList(list(ck.model.layers[0].mlp.experts)[:4])
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts: 4 expert modules, the config says num_experts = 8"):
        load(ck)
    assert gu.dtype == torch.float32                             # `lm` itself was never touched


# ------------------------------------------------------------------------------------------------ the compiled kernels
DEPTH = {1: 4, 2: 3, 3: 2, 4: 1}                                 # MoeI8Depth (csrc/gemm_kernels.hip), per row tile RT = rows / 16
WORKGROUPS_PER_CU = {1: 2, 2: 2, 3: 2, 4: 2}                     # what the depth table is chosen for: two at every row tile
LIST_LDS = 1024                                                  # the list: 64 ints of static LDS, 1 KiB after the dynamic part's alignment
DECODE = ("21k_moe_i8_gate_up_silu", "13k_moe_i8_down")
WIDE = {"12k_moew_i8_gu": "21k_moe_i8_gate_up_silu", "12k_moew_i8_dn": "13k_moe_i8_down"}


def _code_objects(tmp_path):
    blob = open(SO, "rb").read()
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        yield path


def _is_ours(name):
    return "k_moe_i8_" in name or "k_moew_i8_" in name


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_int8_expert_kernels_are_in_the_library_use_no_scratch_and_fit_their_lds(tmp_path):
    kernels = {}
    for path in _code_objects(tmp_path):
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:          # one kernel's entry: its keys are sorted, .agpr_count comes first
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            if not _is_ours(name):
                continue
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"), vgprs=get("vgpr_count"),
                                 static_lds=get("group_segment_fixed_size"))
    decode = {n: v for n, v in kernels.items() if "k_moe_i8_" in n}
    wide = {n: v for n, v in kernels.items() if "k_moew_i8_" in n}
    want = {f"{kern}I{tt}Li{rt}E" for kern in DECODE for tt in ("4GF16", "5GBF16") for rt in (1, 2, 3, 4)}
    assert len(decode) == 16 and all(any(w in n for n in decode) for w in want), sorted(decode)        # 8 + 8: 2 kernels x 2 dtypes x 4 row tiles
    assert len(wide) == 4 and all(any(f"{k}I{tt}E" in n for n in wide) for k in WIDE for tt in ("4GF16", "5GBF16")), sorted(wide)
    assert not any("k_wmoe" in n for n in kernels)               # (names that the older counting tests do not count)
    bad = {n: v for n, v in kernels.items() if v["scratch"] or v["vgpr_spills"]}
    assert not bad, f"the INT8 expert kernels must not spill or use scratch: {bad}"
    for name, v in sorted(decode.items()):
        rt = int(re.search(r"Li(\d)E", name).group(1))
        # the static part only is in the code object; DEPTH restates MoeI8Depth, so this checks the documented table against the budgets
        lds = (DEPTH[rt] + 1) * 16 * rt * 512 + v["static_lds"]
        print(name, v, "LDS", lds)
        assert v["static_lds"] == LIST_LDS, (name, v)
        assert WORKGROUPS_PER_CU[rt] * lds <= 160 * 1024, (name, lds)
        assert v["vgprs"] <= 512 // (2 * WORKGROUPS_PER_CU[rt]), (name, v)        # 8 waves per workgroup = 2 per SIMD: the registers of those workgroups
        assert (DEPTH[rt] - 1) * (5 + rt) <= 63                  # the counted wait's range (PC = 5 + XV, XV = RT)
    for new, old in WIDE.items():                                # the wide twins: the static LDS and the registers of the 64-row decode kernel
        for tt in ("4GF16", "5GBF16"):
            a = [v for n, v in wide.items() if f"{new}I{tt}E" in n]
            b = [v for n, v in decode.items() if f"{old}I{tt}Li4E" in n]
            assert len(a) == len(b) == 1, (new, old, tt)
            assert a[0]["static_lds"] == b[0]["static_lds"] and a[0]["vgprs"] <= b[0]["vgprs"] + 2, (new, a, b)


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_no_register_copy_touches_an_in_flight_load_destination_of_the_int8_expert_gemms(tmp_path):
    """the check of test_moe_int4_cpu.py on k_moe_i8_* / k_moew_i8_*: an expert's stream is often shorter than the pipeline, so skipped
    prologue loads are the normal case; between the first hand-issued load and the first barrier behind it no v_mov reads or writes a
    destination.  Four code loads and one group-data load per chunk in flight."""
    found = 0
    for path in _code_objects(tmp_path):
        text = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
        for chunk in re.split(r"\n(?=[0-9a-f]+ <)", text):
            head = chunk.split("\n", 1)[0]
            if not _is_ours(head):
                continue
            found += 1
            rt = int(re.search(r"Li(\d)E", head).group(1)) if "k_moe_i8_" in head else 4
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
            assert len(load_at) >= 4 * DEPTH[rt] and group_loads >= DEPTH[rt], (head, len(load_at), group_loads)
            assert len(dests) == 18 * DEPTH[rt], (head, len(dests))          # 16 code registers + 2 of group data per chunk in flight, no more
            assert any("global_load_lds_dwordx4" in l for l in body), f"{head}: the A tile is not filled by LDS-DMA"
            assert not any("atomic" in l for l in body), f"{head}: atomics"
            barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier") and i > load_at[0])
            bad = []
            for i in range(load_at[0], barrier):
                m = re.match(r"v_mov_b32_e32 v(\d+), (?:v(\d+))?", body[i])
                if m and (int(m.group(1)) in dests or (m.group(2) is not None and int(m.group(2)) in dests)):
                    bad.append(body[i])
            assert not bad, f"{head}: register copies of hand-issued load destinations: {bad[:8]}"
    assert found == 20, f"expected 20 INT8 expert GEMM instantiations (2 kernels x 2 dtypes x 4 row tiles + 4 wide), found {found}"
