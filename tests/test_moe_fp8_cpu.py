"""Block-scaled FP8 experts of Qwen3-MoE (expert_format "fp8b128") without a GPU: the per-block quantiser of samd_hip/fp8.py against a
numpy restatement of e4m3fn round-to-nearest-even, the importer over transformers' own FP8Experts / FP8Linear modules (fused and per-expert
forms give identical raw tensors), every rejection by message, every decision about `expert_format` with four formats, from_hf on
hand-built modules up to the point where device work starts, a Python restatement of the packed buffer's scale table, and static checks of
the compiled k_moe8_* kernels inside libsamd_hip.so."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from samd_hip import SamdError
from samd_hip import fp8 as F8
from samd_hip import moe as MOE
from samd_hip.llama import LlamaRunner
from test_codeobject_cpu import READELF, SO, gfx950_code_objects
from test_fp8_weights_cpu import e4m3_rne, q_values
from test_moe_cpu import qwen3_moe
from test_moe_mxfp4_cpu import experts, quantise_module

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
PROJ = ("gate_proj", "up_proj", "down_proj")
QCFG = dict(quant_method="fp8", activation_scheme="dynamic", weight_block_size=[128, 128])


def fp8_linear(w, **kw):
    """transformers' FP8Linear holding quantize_blocks(w)"""
    from transformers.integrations.finegrained_fp8 import FP8Linear
    q, s = F8.quantize_blocks(w.detach())
    lin = FP8Linear(w.shape[1], w.shape[0], **dict(dict(block_size=(128, 128)), **kw)).to(w.device)
    lin.weight.data, lin.weight_scale_inv.data = q, s
    return lin


class Expert(torch.nn.Module):
    """one expert in the on-disk naming: mlp.experts.{e}.gate_proj.weight + weight_scale_inv ..."""

    def __init__(self, gate, up, down):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = gate, up, down


def to_fp8_moe_checkpoint(lm, dtype, form="fused", attention=False, layers=None):
    """a block-scaled FP8 checkpoint of a Qwen3-MoE module: in every sparse layer (or `layers`) `mlp.experts` becomes transformers'
    FP8Experts (form "fused") or a ModuleList of E Expert modules of FP8Linears (form "per_expert"), quantised per 128 x 128 block from
    the fused tensors rounded to `dtype` (gate = rows [:I] of gate_up_proj, up = rows [I:]); attention=True makes q / k / v / o (and a dense
    layer's MLP projections) FP8Linears too.  config.quantization_config is set.  `lm` is left as it is."""
    from transformers.integrations.finegrained_fp8 import FP8Experts
    ck = copy.deepcopy(lm)
    for i, lyr in enumerate(ck.model.layers):
        ex = getattr(lyr.mlp, "experts", None)
        if ex is not None and (layers is None or i in layers):
            gu, dn = ex.gate_up_proj.detach().to(dtype), ex.down_proj.detach().to(dtype)
            I = gu.shape[1] // 2
            if form == "fused":
                fe = FP8Experts(ck.config, block_size=(128, 128)).to(gu.device)
                (qg, sg), (qd, sd) = MOE.quantize_experts_fp8(gu, dn)
                fe.gate_up_proj.data, fe.gate_up_proj_scale_inv.data, fe.down_proj.data, fe.down_proj_scale_inv.data = qg, sg, qd, sd
                lyr.mlp.experts = fe
            else:
                lyr.mlp.experts = torch.nn.ModuleList(Expert(fp8_linear(gu[e, :I]), fp8_linear(gu[e, I:]), fp8_linear(dn[e])) for e in range(gu.shape[0]))
        if attention:
            for p in ATTN:
                setattr(lyr.self_attn, p, fp8_linear(getattr(lyr.self_attn, p).weight.to(dtype)))
            if ex is None:
                for p in PROJ:
                    setattr(lyr.mlp, p, fp8_linear(getattr(lyr.mlp, p).weight.to(dtype)))
    ck.config.quantization_config = dict(QCFG)
    return ck


# ------------------------------------------------------------------------------------------------ the quantiser
def test_block_quantiser_against_the_numpy_restatement():
    g = torch.Generator().manual_seed(0)
    W = torch.randn((256, 384), generator=g)
    W = (W.view(2, 128, 3, 128) * torch.tensor([[1e-3, 0.02, 1.0], [30.0, 5e3, 0.5]])[:, None, :, None]).reshape(256, 384)
    W[130, 140] = -9e5                                           # a block whose absmax is negative
    q, s = F8.quantize_blocks(W)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and tuple(s.shape) == (2, 3) and tuple(q.shape) == (256, 384)
    absmax = W.view(2, 128, 3, 128).abs().amax(dim=(1, 3))
    assert torch.equal(s, absmax / 448.0)
    se = s.repeat_interleave(128, 0).repeat_interleave(128, 1)
    qv = q_values(q)
    assert np.abs(qv).max() == 448.0 and qv[130, 140] == -448.0
    assert np.array_equal(qv, e4m3_rne((W / se).numpy()))        # per element: exactly the RNE of W / s (computed in fp32, as the quantiser does)
    assert torch.equal(q.view(torch.uint8), (W / se).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    deq = F8.dequantize_blocks(q, s)
    assert deq.dtype == torch.float32 and torch.equal(deq, q.float() * se)
    assert torch.equal(F8.dequantize_blocks(q.view(torch.uint8), s), deq)                  # (the bytes are taken as well)
    # a zero block gets scale 1 and zero codes; leading dimensions are batch dimensions
    Z = torch.randn((2, 128, 256), generator=g)
    Z[1, :, 128:] = 0
    qz, sz = F8.quantize_blocks(Z)
    assert tuple(sz.shape) == (2, 1, 2) and sz[1, 0, 1].item() == 1.0 and not q_values(qz)[1, :, 128:].any()
    for e in range(2):
        qe, se_ = F8.quantize_blocks(Z[e])
        assert torch.equal(qe.view(torch.uint8), qz[e].view(torch.uint8)) and torch.equal(se_, sz[e])
    with pytest.raises(SamdError, match="128"):
        F8.quantize_blocks(torch.zeros(128, 192))


def test_dequantise_of_quantise_errs_by_at_most_half_a_step_of_the_blocks_absmax():
    """the step of e4m3 at its largest binade (256 .. 448) is 32, so half a step of a block's absmax = 448 s is 16 s = absmax / 28; every
    smaller value has a smaller step.  (2^-20 relative slop for the fp32 division and product.)"""
    g = torch.Generator().manual_seed(2)
    W = torch.randn((3, 256, 512), generator=g) * 0.02
    W[1, :128, 128:256] *= 1e4
    q, s = F8.quantize_blocks(W)
    err = (F8.dequantize_blocks(q, s) - W).abs().view(3, 2, 128, 4, 128).amax(dim=(2, 4))
    absmax = W.view(3, 2, 128, 4, 128).abs().amax(dim=(2, 4))
    assert bool((err <= absmax / 28 * (1 + 2.0 ** -20)).all()), (err / absmax).max().item()
    assert bool((err >= absmax / 28 * 0.5).any()), "the bound is tight somewhere in 49152 draws per block"


def test_packed_bytes_and_the_scale_table_restated():
    """the buffer: E * N * K code bytes, then at a multiple of 256 one fp32 scale per (64 packed rows, 128 k).  Packed 64-row block 2 t of a
    gate|up expert holds gate rows 64 t .. (scale row-block t / 2), block 2 t + 1 the up rows I + 64 t .. (row-block (I + 64 t) / 128); for
    down both halves of tile t repeat row-block t."""
    assert F8.packed_block_bytes(1536, 2048) == 1536 * 2048 + 24 * 16 * 4 and F8.packed_block_bytes(128, 256) == 128 * 256 + 2 * 2 * 4
    assert F8.block_scale_offset(128, 256) == 32768 and F8.block_scale_offset(3, 100) == 512 and F8.block_scale_offset(0, 256) == 0
    for E, I, H in ((2, 256, 512), (3, 768, 256)):
        assert F8.block_scale_offset(E * 2 * I, H) == E * 2 * I * H and E * F8.packed_block_bytes(2 * I, H) == E * 2 * I * H + E * (2 * I // 64) * (H // 128) * 4
        g = torch.Generator().manual_seed(E)
        s_gu = torch.rand((E, 2 * I // 128, H // 128), generator=g) + 0.1
        s_dn = torch.rand((E, H // 128, I // 128), generator=g) + 0.1
        order = MOE.gate_up_tile_order(I)
        t_gu, t_dn = MOE.fp8_scale_table(s_gu, order), MOE.fp8_scale_table(s_dn)
        assert tuple(t_gu.shape) == (E * 2 * I // 64, H // 128) and tuple(t_dn.shape) == (E * H // 64, I // 128) and t_gu.dtype == torch.float32
        for e in range(E):
            for t in range(2 * I // 128):
                row = (e * (2 * I // 128) + t) * 2
                assert torch.equal(t_gu[row], s_gu[e, t // 2]), (e, t, "gate half")
                assert torch.equal(t_gu[row + 1], s_gu[e, (I + 64 * t) // 128]), (e, t, "up half")
                # ... which are the blocks of the rows the tile's waves hold: packed rows 128 t + 16 w .. of source rows order[...]
                for w in range(8):
                    src = order[128 * t + 16 * w:128 * t + 16 * w + 16]
                    assert bool((src // 128 == (t // 2 if w < 4 else (I + 64 * t) // 128)).all())
            for t in range(H // 128):
                row = (e * (H // 128) + t) * 2
                assert torch.equal(t_dn[row], s_dn[e, t]) and torch.equal(t_dn[row + 1], s_dn[e, t])


# ------------------------------------------------------------------------------------------------ the importer
def test_linear_importer_and_every_rejection_by_name():
    from transformers.integrations.finegrained_fp8 import FP8Linear
    g = torch.Generator().manual_seed(4)
    w = torch.randn((256, 384), generator=g) * 0.05
    lin = fp8_linear(w)
    assert isinstance(lin, FP8Linear) and tuple(lin.weight_scale_inv.shape) == (2, 3)
    q, s = F8.linear_fp8_block(lin, "L0.q_proj", QCFG)
    want = F8.quantize_blocks(w)
    assert torch.equal(q.view(torch.uint8), want[0].view(torch.uint8)) and torch.equal(s, want[1])
    assert F8.linear_fp8_block(torch.nn.Linear(128, 128), "plain") is None
    assert torch.equal(F8.linear_fp8_dequantized(lin, "L0.q_proj"), F8.dequantize_blocks(*want))
    with pytest.raises(SamdError, match="block-scaled FP8"):     # the dense importer keeps rejecting the format
        F8.linear_fp8(lin, "L0.q_proj")

    def bad(match, cfg=None, **edit):
        m = copy.deepcopy(lin)
        for k, v in edit.items():
            if isinstance(v, torch.Tensor):
                setattr(m, k, torch.nn.Parameter(v, requires_grad=False))
            else:
                setattr(m, k, v)
        with pytest.raises(SamdError, match=match):
            F8.linear_fp8_block(m, "L3.o_proj", cfg)
    for other in ("float8_e4m3fnuz", "float8_e5m2"):
        bad(rf"L3\.o_proj: weights in {other}", weight=lin.weight.detach().view(getattr(torch, other)))
    bad(r"L3\.o_proj: weight_scale_inv of dtype torch\.float16", weight_scale_inv=lin.weight_scale_inv.detach().half())
    if hasattr(torch, "float8_e8m0fnu"):                         # a ue8m0 scale_fmt checkpoint
        bad(r"L3\.o_proj: weight_scale_inv of dtype torch\.float8_e8m0fnu.*ue8m0", weight_scale_inv=torch.zeros((2, 3), dtype=torch.uint8).view(torch.float8_e8m0fnu))
    bad(r"L3\.o_proj: scale_fmt 'ue8m0'", cfg=dict(QCFG, scale_fmt="ue8m0"))
    bad(r"L3\.o_proj: weight_scale_inv of shape \(2, 2\).*\[2, 3\]", weight_scale_inv=lin.weight_scale_inv.detach()[:, :2].contiguous())
    bad(r"L3\.o_proj: weight_scale_inv of shape \(256,\)", weight_scale_inv=torch.ones(256))
    for v in (float("inf"), float("nan"), 0.0, -1.0):
        sc = lin.weight_scale_inv.detach().clone()
        sc[1, 2] = v
        bad(r"L3\.o_proj: weight_scale_inv must be finite and positive", weight_scale_inv=sc)
    bad(r"L3\.o_proj: activation_scheme 'static'", activation_scheme="static")
    bad(r"L3\.o_proj: activation_scheme 'static'", cfg=dict(QCFG, activation_scheme="static"))
    bad(r"L3\.o_proj: block_size \[64, 128\]", block_size=(64, 128))
    bad(r"L3\.o_proj: weight_block_size \[128, 64\]", cfg=dict(QCFG, weight_block_size=[128, 64]))
    m = copy.deepcopy(lin)
    m.weight_scale_inv = None
    with pytest.raises(SamdError, match=r"L3\.o_proj: float8_e4m3fn weight without a weight_scale_inv"):
        F8.linear_fp8_block(m, "L3.o_proj")
    # a weight with a partial block
    part = torch.nn.Linear(192, 128, bias=False)
    part.weight = torch.nn.Parameter(torch.zeros((128, 192), dtype=torch.float8_e4m3fn), requires_grad=False)
    part.weight_scale_inv = torch.nn.Parameter(torch.ones(1, 2), requires_grad=False)
    with pytest.raises(SamdError, match="partial blocks"):
        F8.linear_fp8_block(part, "L3.o_proj")
    # an object with attributes counts as a config too
    class Cfg:
        weight_block_size, activation_scheme = (128, 128), "static"
    with pytest.raises(SamdError, match="activation_scheme 'static'"):
        F8.linear_fp8_block(lin, "L3.o_proj", Cfg())


def test_fused_and_per_expert_modules_import_to_the_same_raw_tensors():
    """transformers' own FP8Experts (constructed on the CPU with its four tensors) and per-expert FP8Linear modules, quantised from the same
    values: identical experts_gu / experts_gu_sinv / experts_down / experts_down_sinv, equal to quantize_experts_fp8 of the fused tensors"""
    from transformers.integrations.finegrained_fp8 import FP8Experts
    torch.manual_seed(3)
    cfg, lm = qwen3_moe(mlp_only_layers=[1])
    dtype = torch.bfloat16
    fused, per = to_fp8_moe_checkpoint(lm, dtype, "fused"), to_fp8_moe_checkpoint(lm, dtype, "per_expert")
    E, I, H = cfg.num_experts, cfg.moe_intermediate_size, cfg.hidden_size
    ex = fused.model.layers[0].mlp.experts
    assert isinstance(ex, FP8Experts) and ex.gate_up_proj.dtype == torch.float8_e4m3fn
    assert [tuple(t.shape) for t in (ex.gate_up_proj, ex.gate_up_proj_scale_inv, ex.down_proj, ex.down_proj_scale_inv)] == \
        [(E, 2 * I, H), (E, 2 * I // 128, H // 128), (E, H, I), (E, H // 128, I // 128)]
    assert per.model.layers[0].mlp.experts[0].gate_proj.weight_scale_inv.dtype == torch.float32
    for ck in (fused, per):
        assert LlamaRunner._hf_sparse_layers(ck.model.layers) == [True, False, True, True]
        assert LlamaRunner._hf_layer_extras(ck.model.layers) == (False, True)
        assert [LlamaRunner._hf_experts_are_fp8(l, i) for i, l in enumerate(ck.model.layers)] == [True, False, True, True]
    for i in (0, 2, 3):
        src = lm.model.layers[i].mlp.experts
        gu, dn = MOE.quantize_experts_fp8(src.gate_up_proj.detach().to(dtype), src.down_proj.detach().to(dtype))
        a = MOE.import_experts_fp8(fused.model.layers[i].mlp.experts, f"layers.{i}.mlp.experts", "cpu", QCFG)
        b = MOE.import_experts_fp8(per.model.layers[i].mlp.experts, f"layers.{i}.mlp.experts", "cpu", QCFG)
        assert sorted(a) == sorted(b) == ["experts_down", "experts_down_sinv", "experts_gu", "experts_gu_sinv"]
        for key, want in (("experts_gu", gu[0]), ("experts_gu_sinv", gu[1]), ("experts_down", dn[0]), ("experts_down_sinv", dn[1])):
            assert a[key].dtype == b[key].dtype == want.dtype and a[key].is_contiguous() and b[key].is_contiguous()
            view = (lambda t: t.view(torch.uint8)) if want.dtype == torch.float8_e4m3fn else (lambda t: t)
            assert torch.equal(view(a[key]), view(want)) and torch.equal(view(b[key]), view(want)), (i, key)
        MOE.check_fp8_experts((a["experts_gu"], a["experts_gu_sinv"]), (a["experts_down"], a["experts_down_sinv"]))
        MOE.check_fp8_experts((a["experts_gu"].view(torch.uint8), a["experts_gu_sinv"]), (a["experts_down"], a["experts_down_sinv"]))   # the bytes
        assert torch.equal(MOE.dequantize_experts_fp8(a["experts_gu"], a["experts_gu_sinv"]), F8.dequantize_blocks(*gu))


def test_expert_importer_rejections_by_name():
    torch.manual_seed(5)
    cfg, lm = qwen3_moe()
    fused, per = to_fp8_moe_checkpoint(lm, torch.float16, "fused", layers=[0]), to_fp8_moe_checkpoint(lm, torch.float16, "per_expert", layers=[0])
    ex = fused.model.layers[0].mlp.experts
    imp = lambda e, c=None: MOE.import_experts_fp8(e, "layers.0.mlp.experts", "cpu", c)

    def fused_bad(match, cfg_=None, **edit):
        m = copy.deepcopy(ex)
        for k, v in edit.items():
            setattr(m, k, torch.nn.Parameter(v, requires_grad=False) if isinstance(v, torch.Tensor) else v)
        with pytest.raises(SamdError, match=match):
            imp(m, cfg_)
    fused_bad(r"layers\.0\.mlp\.experts\.gate_up_proj: weights in float8_e5m2", gate_up_proj=ex.gate_up_proj.detach().view(torch.float8_e5m2))
    fused_bad(r"layers\.0\.mlp\.experts\.down_proj: weight_scale_inv of dtype torch\.bfloat16", down_proj_scale_inv=ex.down_proj_scale_inv.detach().bfloat16())
    fused_bad(r"layers\.0\.mlp\.experts\.gate_up_proj: weight_scale_inv of shape", gate_up_proj_scale_inv=ex.gate_up_proj_scale_inv.detach()[:, :1].contiguous())
    sc = ex.down_proj_scale_inv.detach().clone()
    sc[3, 0, 1] = float("nan")
    fused_bad(r"layers\.0\.mlp\.experts\.down_proj: weight_scale_inv must be finite and positive", down_proj_scale_inv=sc)
    fused_bad(r"layers\.0\.mlp\.experts: activation_scheme 'static'", activation_scheme="static")
    fused_bad(r"layers\.0\.mlp\.experts: block_size \[128, 256\]", block_size=(128, 256))
    fused_bad(r"layers\.0\.mlp\.experts: weight_block_size \[64, 64\]", cfg_=dict(QCFG, weight_block_size=[64, 64]))
    fused_bad(r"layers\.0\.mlp\.experts: scale_fmt 'ue8m0'", cfg_=dict(QCFG, scale_fmt="ue8m0"))
    m = copy.deepcopy(per.model.layers[0].mlp.experts)
    m[5].up_proj.weight_scale_inv.data[0, 1] = 0.0
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts\.5\.up_proj: weight_scale_inv must be finite and positive"):
        imp(m, QCFG)
    m = copy.deepcopy(per.model.layers[0].mlp.experts)
    m[2].down_proj.activation_scheme = "static"
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts\.2\.down_proj: activation_scheme 'static'"):
        imp(m, QCFG)
    # check_fp8_experts: shapes that do not belong together, a missing scale, a K the kernels do not serve
    gu, dn = MOE.quantize_experts_fp8(*experts(2, 256, 512, 1))
    MOE.check_fp8_experts(gu, dn)
    with pytest.raises(SamdError, match="do not belong together"):
        MOE.check_fp8_experts(gu, (dn[0][:, :256].contiguous(), dn[1][:, :2].contiguous()))
    with pytest.raises(SamdError, match=r"L7\.down_proj: FP8 expert tensor without its block scales"):
        MOE.check_fp8_experts(gu, (dn[0], None), "L7")
    g3, d3 = MOE.quantize_experts_fp8(*experts(2, 384, 256, 1))
    with pytest.raises(SamdError, match=r"K % 256 == 0"):
        MOE.check_fp8_experts(g3, d3)
    with pytest.raises(SamdError, match="do not belong together"):
        MOE.quantize_experts_fp8(*(lambda a, b: (a, b[:, :, :128]))(*experts(2, 256, 512, 1)))


# ------------------------------------------------------------------------------------------------ the format
def test_format_resolution_with_four_formats(monkeypatch):
    assert MOE.EXPERT_FORMATS == (None, "mxfp4")                 # the pinned constants stay; the wider one is what is validated against
    assert MOE.EXPERT_FORMATS_ALL == (None, "mxfp4", "int4g128")
    assert MOE.EXPERT_FORMATS_KNOWN == (None, "mxfp4", "int4g128", "fp8b128")
    R = MOE.resolve_expert_format
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    assert R("fp8b128", False, True) == "fp8b128"                # on load
    assert R(MOE.AUTO, False, True, carries_fp8=True) == "fp8b128" and R("fp8b128", False, True, carries_fp8=True) == "fp8b128"
    for explicit in (None, "mxfp4", "int4g128"):
        with pytest.raises(SamdError, match="block-scaled FP8 expert tensors.*'fp8b128'"):
            R(explicit, False, True, carries_fp8=True)
    with pytest.raises(SamdError, match="4-bit expert tensors.*fp8b128"):
        R("fp8b128", True, True)
    with pytest.raises(SamdError, match="4-bit expert tensors.*fp8b128"):
        R("fp8b128", False, True, carries_int4=True)
    with pytest.raises(SamdError, match="a mix of block-scaled FP8 and 4-bit"):
        R(MOE.AUTO, True, True, carries_fp8=True)
    with pytest.raises(SamdError, match="a mix of block-scaled FP8 and 4-bit"):
        R(MOE.AUTO, False, True, carries_int4=True, carries_fp8=True)
    with pytest.raises(SamdError, match="expected one of") as ei:        # the dense format's spelling stays an unknown expert format, with a hint
        R("fp8", False, True)
    assert all(x in str(ei.value) for x in ("'fp8'", "None", "'mxfp4'", "'int4g128'", "'fp8b128'"))
    for bad in ("fp8b64", "fp8_block", "e4m3"):
        with pytest.raises(SamdError, match="expected one of"):
            R(bad, False, True)
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        R("fp8b128", False, False)
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "fp8b128")
    assert R(MOE.AUTO, False, True) == "fp8b128" and R(None, False, True) is None
    assert R(MOE.AUTO, True, True) == "mxfp4" and R(MOE.AUTO, False, True, carries_int4=True) == "int4g128"      # what the weights carry wins over the env
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "mxfp4")
    assert R(MOE.AUTO, False, True, carries_fp8=True) == "fp8b128"
    for wf in ("fp8", "mxfp4", "int4g128"):                      # weight_format keeps its rejection for mixture-of-experts models
        with pytest.raises(SamdError, match="quantised experts are not supported"):
            MOE.reject_unsupported(wf)


def test_from_hf_argument_errors_come_before_device_work(monkeypatch):
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    torch.manual_seed(7)
    _, lm = qwen3_moe(mlp_only_layers=[0])
    with pytest.raises(SamdError, match="no MI355X"):            # quantise on load: accepted up to the point where the device is needed
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="fp8b128")
    with pytest.raises(SamdError, match="native_gemm"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="fp8b128", native_gemm=False)
    for wf in ("fp8", "int4g128"):                               # weight_format keeps its meaning and its rejection
        with pytest.raises(SamdError, match="mixture-of-experts"):
            LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="fp8b128", weight_format=wf)
    with pytest.raises(SamdError, match="expected one of") as ei:
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="fp8")
    assert "'fp8b128'" in str(ei.value)
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "fp8b128")
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    monkeypatch.delenv("SAMD_EXPERT_FORMAT")
    with pytest.raises(SamdError, match="4-bit expert tensors.*fp8b128"):       # MXFP4 tensors against the FP8 format
        LlamaRunner.from_hf(quantise_module(qwen3_moe()[1]), 256, dtype=torch.bfloat16, device="cpu", expert_format="fp8b128")
    from transformers import Qwen3Config, Qwen3ForCausalLM
    dense = Qwen3ForCausalLM(Qwen3Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                         head_dim=128, vocab_size=300))
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        LlamaRunner.from_hf(dense, 256, device="cpu", expert_format="fp8b128")


@pytest.mark.parametrize("form", ["fused", "per_expert"])
@pytest.mark.parametrize("attention", [False, True])
def test_a_module_shaped_like_the_official_checkpoint_passes_every_guard(monkeypatch, form, attention):
    """FP8 experts (and FP8 attention / dense-MLP projections beside them) are detected before checkpoint_is_fp8 would reject the block
    scales: from_hf, with no extra arguments, gets as far as the device"""
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    torch.manual_seed(8)
    _, lm = qwen3_moe(mlp_only_layers=[1])
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, form, attention=attention)
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu")
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu", expert_format="fp8b128")
    for explicit in (None, "mxfp4", "int4g128"):
        with pytest.raises(SamdError, match="block-scaled FP8 expert tensors"):
            LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu", expert_format=explicit)
    with pytest.raises(SamdError, match="native_gemm"):
        LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu", native_gemm=False)


def test_module_level_rejections(monkeypatch):
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    torch.manual_seed(9)
    _, lm = qwen3_moe()
    H = lambda ck, **kw: LlamaRunner.from_hf(ck, 256, dtype=torch.bfloat16, device="cpu", **kw)
    # a mix of formats across sparse layers
    with pytest.raises(SamdError, match=r"a mix of block-scaled FP8 and other sparse layers \(2 of 4.*layers \[1, 3\]"):
        H(to_fp8_moe_checkpoint(lm, torch.bfloat16, "fused", layers=[0, 2]))
    # some experts only / one fused tensor only
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, "per_expert")
    ck.model.layers[1].mlp.experts[3].up_proj = torch.nn.Linear(256, 256, bias=False)
    with pytest.raises(SamdError, match=r"layers\.1\.mlp\.experts: a mix of FP8 and other expert tensors.*experts\.3\.up_proj"):
        H(ck)
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, "fused")
    ck.model.layers[2].mlp.experts.down_proj = torch.nn.Parameter(torch.zeros(8, 256, 256), requires_grad=False)
    with pytest.raises(SamdError, match=r"layers\.2\.mlp\.experts: a mix of FP8 and other expert tensors.*down_proj"):
        H(ck)
    # an FP8 router
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, "fused")
    gate = ck.model.layers[0].mlp.gate
    gate.weight = torch.nn.Parameter(gate.weight.detach().to(torch.float8_e4m3fn), requires_grad=False)
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.gate: an FP8 router is not supported"):
        H(ck)
    # rejections of the importer reach from_hf by name: a static checkpoint, another block size, a bad attention scale
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, "fused")
    ck.config.quantization_config["activation_scheme"] = "static"
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts: activation_scheme 'static'"):
        H(ck)
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, "fused", attention=True)
    ck.config.quantization_config["weight_block_size"] = [64, 64]
    with pytest.raises(SamdError, match=r"layers\.0\.self_attn\.q_proj: weight_block_size \[64, 64\]"):
        H(ck)
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, "per_expert", attention=True)
    ck.model.layers[1].self_attn.o_proj.weight_scale_inv.data[0, 0] = -1.0
    with pytest.raises(SamdError, match=r"layers\.1\.self_attn\.o_proj: weight_scale_inv must be finite and positive"):
        H(ck)
    # the number of experts
    ck = to_fp8_moe_checkpoint(lm, torch.bfloat16, "per_expert")
    ck.model.layers[3].mlp.experts = torch.nn.ModuleList(list(ck.model.layers[3].mlp.experts)[:7])
    with pytest.raises(SamdError, match=r"layers\.3\.mlp\.experts: 7 experts, the config says num_experts = 8"):
        H(ck)
    # FP8 projections beside non-FP8 experts stay rejected as before (the dense importer meets the block scales)
    plain = copy.deepcopy(lm)
    for lyr in plain.model.layers:
        for p in ATTN:
            setattr(lyr.self_attn, p, fp8_linear(getattr(lyr.self_attn, p).weight))
    with pytest.raises(SamdError, match="block-scaled FP8 .* is not supported"):
        H(plain)


# ------------------------------------------------------------------------------------------------ the compiled kernels
@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_no_instantiation_of_the_fp8_expert_kernels_uses_scratch(tmp_path):
    """k_moe8_* issue their weight loads by hand and wait with counted vmcnt: a spilled destination would be stored to scratch before its data
    has landed.  16 instantiations (gate|up and down x 2 dtypes x 4 row tiles), none with a private segment; the 16-row tile, two workgroups
    per CU, inside 128 VGPRs."""
    blob = open(SO, "rb").read()
    kernels = {}
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split(".name:")[1:]:
            name = block.split()[0]
            if "k_moe8_" not in name or name.endswith(".kd"):
                continue
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"), vgprs=get("vgpr_count"))
    for name, v in sorted(kernels.items()):
        print(name, v)
    assert len(kernels) == 16, sorted(kernels)
    bad = {n: v for n, v in kernels.items() if v["scratch"] or v["vgpr_spills"]}
    assert not bad, f"kernels with hand-issued loads must not spill: {bad}"
    assert all(v["vgprs"] <= 128 for n, v in kernels.items() if "Li1E" in n), "the 16-row tile runs two workgroups per CU"
