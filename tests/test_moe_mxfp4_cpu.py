"""MXFP4 experts of Qwen3-MoE without a GPU: the quantise / dequantise round trip of the fused expert tensors, the gate|up row order the packed
4-bit form uses, every decision from_hf makes about `expert_format` (on CPU-built modules, before any device work), and static checks of the
compiled k_moe4_* kernels inside libsamd_hip.so."""
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from samd_hip import SamdError
from samd_hip import moe as MOE
from samd_hip import mxfp4 as MX
from samd_hip.llama import LlamaRunner
from test_codeobject_cpu import READELF, SO, gfx950_code_objects
from test_moe_cpu import OBJDUMP, qwen3_moe


def experts(E, I, H, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((E, 2 * I, H), generator=g) * scale, torch.randn((E, H, I), generator=g) * scale


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_quantise_dequantise_round_trip_is_idempotent(dtype):
    E, I, H = 3, 64, 96
    gate_up, down = experts(E, I, H, 1)
    quad = MOE.quantize_experts(gate_up.to(dtype), down.to(dtype), dtype)
    q_gu, e8_gu, q_down, e8_down = quad
    assert [tuple(t.shape) for t in quad] == [(E, 2 * I, H // 2), (E, 2 * I, H // 32), (E, H, I // 2), (E, H, I // 32)]
    assert all(t.dtype == torch.uint8 for t in quad)
    # randn * 0.05 stays inside the fp16 exponent range: the GPU fixtures (the same distribution) are admissible in both dtypes
    lo, hi = MX.EXPONENT_RANGE[torch.float16]
    for e8 in (e8_gu, e8_down):
        ex = e8.to(torch.int32) - 127
        assert lo <= int(ex.min()) and int(ex.max()) <= hi, (int(ex.min()), int(ex.max()))
    w_gu, w_down = MOE.dequantize_experts(q_gu, e8_gu), MOE.dequantize_experts(q_down, e8_down)
    assert w_gu.dtype == torch.float32 and tuple(w_gu.shape) == (E, 2 * I, H) and tuple(w_down.shape) == (E, H, I)
    # every dequantised weight is a value of the model dtype
    assert torch.equal(w_gu, w_gu.to(dtype).float()) and torch.equal(w_down, w_down.to(dtype).float())
    assert torch.equal(MOE.dequantize_experts(q_gu, e8_gu, dtype).float(), w_gu)
    # quantising the dequantised weights gives the same weights again
    again = MOE.quantize_experts(w_gu.to(dtype), w_down.to(dtype), dtype)
    assert torch.equal(MOE.dequantize_experts(again[0], again[1]), w_gu) and torch.equal(MOE.dequantize_experts(again[2], again[3]), w_down)
    # and about 11.5 % relative RMS error against the originals (mxfp4.py), nothing grosser
    rel = ((w_gu - gate_up.to(dtype).float()).norm() / gate_up.norm()).item()
    assert 0.05 < rel < 0.16, rel
    with pytest.raises(SamdError, match="do not belong together"):
        MOE.quantize_experts(gate_up, down[:, :, :32], dtype)


@pytest.mark.parametrize("I", [128, 192, 768])
def test_gate_up_tile_order_is_the_documented_interleave(I):
    """k_moe_pack: packed row 128 t + q is gate row 64 t + q for q < 64 and up row 64 t + q - 64 (of the up half) otherwise"""
    order = MOE.gate_up_tile_order(I).tolist()
    want = []
    for t in range(2 * I // 128):
        want += [64 * t + q for q in range(64)] + [I + 64 * t + q for q in range(64)]
    assert order == want and sorted(order) == list(range(2 * I))
    # on a small [E, 2 I, H]: tile t of the permuted tensor = 64 gate rows | the 64 up rows they multiply
    E, H = 2, 32
    gu = torch.arange(E * 2 * I * H, dtype=torch.float32).reshape(E, 2 * I, H)
    p = gu[:, MOE.gate_up_tile_order(I)]
    for t in range(2 * I // 128):
        assert torch.equal(p[:, 128 * t:128 * t + 64], gu[:, 64 * t:64 * t + 64])
        assert torch.equal(p[:, 128 * t + 64:128 * t + 128], gu[:, I + 64 * t:I + 64 * t + 64])


def test_expert_format_reaches_the_device_and_rejections_come_first(monkeypatch):
    assert MOE.EXPERT_FORMATS == (None, "mxfp4")
    _, lm = qwen3_moe(mlp_only_layers=[0])
    with pytest.raises(SamdError, match="no MI355X"):            # accepted up to the point where the device is needed
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="mxfp4")
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format=None)
    with pytest.raises(SamdError) as ei:                         # an unknown value: the message lists the accepted ones
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="fp8")
    assert "'fp8'" in str(ei.value) and "'mxfp4'" in str(ei.value) and "None" in str(ei.value)
    with pytest.raises(SamdError, match="native_gemm"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="mxfp4", native_gemm=False)
    with pytest.raises(SamdError, match="draft head"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="mxfp4", draft_head=True)
    with pytest.raises(SamdError, match="mxfp4"):                # weight_format keeps its meaning and its rejection
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="mxfp4", weight_format="mxfp4")
    # the environment serves callers that cannot pass the argument; an explicit argument wins
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "int3")
    with pytest.raises(SamdError, match="int3"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format=None)
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "mxfp4")
    assert MOE.resolve_expert_format(MOE.AUTO, False, True) == "mxfp4" and MOE.resolve_expert_format(None, False, True) is None
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    monkeypatch.delenv("SAMD_EXPERT_FORMAT")
    assert MOE.resolve_expert_format(MOE.AUTO, False, True) is None and MOE.resolve_expert_format(MOE.AUTO, True, True) == "mxfp4"


def test_expert_format_on_a_dense_model_raises(monkeypatch):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    lm = Qwen3ForCausalLM(Qwen3Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                      head_dim=128, vocab_size=300))
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu", expert_format="mxfp4")
    _, moe_dense = qwen3_moe(mlp_only_layers=[0, 1, 2, 3])      # a Qwen3-MoE config whose every layer is dense
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        LlamaRunner.from_hf(moe_dense, 256, device="cpu", expert_format="mxfp4")
    monkeypatch.setenv("SAMD_EXPERT_FORMAT", "mxfp4")
    with pytest.raises(SamdError, match="without mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def quantise_module(lm, dtype=torch.bfloat16, layers=None, scales_as="parameter"):
    """replace the expert tensors of the sparse layers (all, or `layers`) by their 4-bit form + block scales, in this project's convention"""
    for i, lyr in enumerate(lm.model.layers):
        ex = getattr(lyr.mlp, "experts", None)
        if ex is None or (layers is not None and i not in layers):
            continue
        q_gu, e8_gu, q_down, e8_down = MOE.quantize_experts(ex.gate_up_proj.detach(), ex.down_proj.detach(), dtype)
        ex.gate_up_proj = torch.nn.Parameter(q_gu, requires_grad=False)
        ex.down_proj = torch.nn.Parameter(q_down, requires_grad=False)
        for name, t in (("gate_up_proj_scale", e8_gu), ("down_proj_scale", e8_down)):
            if scales_as == "parameter":
                ex.register_parameter(name, torch.nn.Parameter(t, requires_grad=False))
            else:
                ex.register_buffer(name, t)
    return lm


@pytest.mark.parametrize("scales_as", ["parameter", "buffer"])
def test_a_module_with_4bit_experts_passes_the_guards(scales_as):
    cfg, lm = qwen3_moe(mlp_only_layers=[1])
    quantise_module(lm, scales_as=scales_as)
    assert LlamaRunner._hf_layer_extras(lm.model.layers) == (False, True)
    assert LlamaRunner._hf_sparse_layers(lm.model.layers) == [True, False, True, True]
    for kw in ({}, dict(expert_format="mxfp4")):                 # 4-bit experts make the runner "mxfp4" by themselves
        with pytest.raises(SamdError, match="no MI355X"):
            LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu", **kw)
    with pytest.raises(SamdError, match="expert_format=None"):   # explicit None against 4-bit tensors: nothing dequantises them
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu", expert_format=None)
    if MX._F4 is not None and MX._E8 is not None:                # the same bytes under torch's own 4-bit / e8m0 dtypes
        for lyr in lm.model.layers:
            ex = getattr(lyr.mlp, "experts", None)
            if ex is not None:
                ex.gate_up_proj = torch.nn.Parameter(ex.gate_up_proj.data.view(MX._F4), requires_grad=False)
                ex.down_proj = torch.nn.Parameter(ex.down_proj.data.view(MX._F4), requires_grad=False)
                for name in ("gate_up_proj_scale", "down_proj_scale"):
                    t = getattr(ex, name).data.view(MX._E8)
                    setattr(ex, name, torch.nn.Parameter(t, requires_grad=False) if scales_as == "parameter" else t)
        assert LlamaRunner._hf_layer_extras(lm.model.layers) == (False, True)
        with pytest.raises(SamdError, match="no MI355X"):
            LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")


def test_block_scales_beside_plain_experts_are_extra_parameters():
    cfg, lm = qwen3_moe()
    ex = lm.model.layers[1].mlp.experts
    ex.register_parameter("gate_up_proj_scale", torch.nn.Parameter(torch.zeros((8, 512, 8), dtype=torch.uint8), requires_grad=False))
    with pytest.raises(SamdError, match="gate_up_proj_scale"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def test_ill_formed_4bit_experts_raise_by_name():
    def fresh():
        return quantise_module(qwen3_moe()[1])
    lm = fresh()                                                 # a scale tensor of another block size
    ex = lm.model.layers[2].mlp.experts
    ex.down_proj_scale = torch.nn.Parameter(ex.down_proj_scale[:, :, :4].contiguous(), requires_grad=False)
    with pytest.raises(SamdError, match=r"layers\.2\.mlp\.experts\.down_proj_scale of shape"):
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")
    lm = fresh()                                                 # the NaN code
    lm.model.layers[3].mlp.experts.gate_up_proj_scale.data[5, 17, 2] = 255
    with pytest.raises(SamdError, match=r"layers\.3\.mlp\.experts\.gate_up_proj_scale: a block scale is NaN"):
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")
    lm = fresh()                                                 # no scales at all
    del lm.model.layers[0].mlp.experts.down_proj_scale
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.experts\.down_proj: 4-bit expert tensor without its block scales"):
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")
    lm = fresh()                                                 # scales of a float dtype
    ex = lm.model.layers[1].mlp.experts
    ex.gate_up_proj_scale = torch.nn.Parameter(ex.gate_up_proj_scale.float(), requires_grad=False)
    with pytest.raises(SamdError, match=r"gate_up_proj_scale of dtype"):
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")
    lm = quantise_module(qwen3_moe()[1], layers=[0, 2])          # a mix of 4-bit and plain sparse layers
    with pytest.raises(SamdError, match="a mix of 4-bit and model-dtype sparse layers"):
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")
    lm = fresh()                                                 # one tensor of a layer only
    ex = lm.model.layers[1].mlp.experts
    ex.down_proj = torch.nn.Parameter(torch.zeros((8, 256, 256)), requires_grad=False)
    with pytest.raises(SamdError, match=r"layers\.1\.mlp\.experts: gate_up_proj is"):
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")


def test_fp16_exponents_out_of_range_raise_and_name_bf16():
    lm = quantise_module(qwen3_moe()[1])
    lm.model.layers[1].mlp.experts.gate_up_proj_scale.data[0, 0, 0] = 127 + 14         # 6 * 2^14 overflows fp16
    with pytest.raises(SamdError, match="bfloat16") as ei:
        LlamaRunner.from_hf(lm, 256, dtype=torch.float16, device="cpu")
    assert "layers.1.mlp.experts.gate_up_proj_scale" in str(ei.value) and "[-23, 13]" in str(ei.value)
    with pytest.raises(SamdError, match="no MI355X"):            # the same module is admissible in bf16
        LlamaRunner.from_hf(lm, 256, dtype=torch.bfloat16, device="cpu")
    lm.model.layers[1].mlp.experts.gate_up_proj_scale.data[0, 0, 0] = 127 - 24
    with pytest.raises(SamdError, match="bfloat16"):
        LlamaRunner.from_hf(lm, 256, dtype=torch.float16, device="cpu")


def test_a_weights_dict_with_4bit_experts_is_checked_before_device_work():
    from samd_hip.llama import LlamaShape
    cfg, lm = qwen3_moe(num_hidden_layers=1)
    s = LlamaShape(cfg)
    gate_up, down = experts(8, 256, 256, 2)
    q_gu, e8_gu, q_down, e8_down = MOE.quantize_experts(gate_up, down, torch.bfloat16)
    layer = dict(experts_gu=q_gu, experts_gu_scale=e8_gu, experts_down=q_down, experts_down_scale=e8_down)
    with pytest.raises(SamdError, match="no MI355X"):
        LlamaRunner(s, dict(layers=[layer]), 256, dtype=torch.bfloat16, device="cpu")
    with pytest.raises(SamdError, match="expert_format=None"):
        LlamaRunner(s, dict(layers=[layer]), 256, dtype=torch.bfloat16, device="cpu", expert_format=None)
    with pytest.raises(SamdError, match="layer 0 experts.gate_up_proj_scale of shape"):
        LlamaRunner(s, dict(layers=[dict(layer, experts_gu_scale=e8_gu[:, :, :4])]), 256, dtype=torch.bfloat16, device="cpu")
    with pytest.raises(SamdError, match="without its block scales"):
        LlamaRunner(s, dict(layers=[{k: v for k, v in layer.items() if k != "experts_down_scale"}]), 256, dtype=torch.bfloat16, device="cpu")


# ------------------------------------------------------------------------------------------------ the compiled kernels
def _code_objects(tmp_path):
    blob = open(SO, "rb").read()
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        yield path


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_4bit_expert_kernels_are_in_the_library_and_use_no_scratch(tmp_path):
    kernels = {}
    for path in _code_objects(tmp_path):
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split(".name:")[1:]:
            name = block.split()[0]
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"))
    count = lambda frag: len([n for n in kernels if frag in n])
    assert (count("k_moe4_gate_up_silu"), count("k_moe4_down")) == (8, 8), sorted(n for n in kernels if "k_moe4_" in n)   # 2 dtypes x 4 row tiles
    bad = {n: v for n, v in kernels.items() if "k_moe4_" in n and (v["scratch"] or v["vgpr_spills"])}
    assert not bad, f"the 4-bit expert kernels must not spill or use scratch: {bad}"
    # the names the existing counts go by are untouched
    assert (count("k_moe_gate_up_silu"), count("k_moe_down"), count("k_moe_route"), count("k_moe_combine"), count("k_moe_lists"), count("k_moe_pack"),
            count("k_gemm_skinny_f4")) == (8, 8, 2, 2, 1, 1, 8)


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_no_register_copy_touches_an_in_flight_load_destination_of_the_4bit_expert_gemms(tmp_path):
    """the check of test_mxfp4_codeobject_cpu.py on k_moe4_*: an expert's stream is often shorter than the pipeline (1 or 3 chunks against a
    depth of up to 8), so skipped prologue loads are the normal case; the destinations are in-out operands of one value each, and between the
    first hand-issued load and the first barrier behind it no v_mov reads or writes one"""
    found = 0
    for path in _code_objects(tmp_path):
        text = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
        for chunk in re.split(r"\n(?=[0-9a-f]+ <)", text):
            head = chunk.split("\n", 1)[0]
            if "k_moe4_gate_up_silu" not in head and "k_moe4_down" not in head:
                continue
            found += 1
            body = [l.split("//")[0].strip() for l in chunk.split("\n")[1:]]
            dests, load_at, scale_loads = set(), [], 0
            for i, l in enumerate(body):
                m = re.match(r"global_load_dwordx4 v\[(\d+):(\d+)\], v\d+, s\[\d+:\d+\].* nt", l)      # (the hand-issued form: SGPR base, nt)
                if m:
                    dests |= set(range(int(m.group(1)), int(m.group(2)) + 1))
                    load_at.append(i)
                m = re.match(r"global_load_ushort v(\d+), v\d+, s\[\d+:\d+\].* nt", l)
                if m:
                    dests.add(int(m.group(1)))
                    scale_loads += 1
            assert len(load_at) >= 4 and scale_loads >= 2, head
            assert any("global_load_lds_dwordx4" in l for l in body), f"{head}: the A tile is not filled by LDS-DMA"
            assert any(re.match(r"v_cvt_scalef32_pk_(f16|bf16)_fp4", l) for l in body), f"{head}: no scaled fp4 conversion"
            barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier") and i > load_at[0])
            bad = []
            for i in range(load_at[0], barrier):
                m = re.match(r"v_mov_b32_e32 v(\d+), (?:v(\d+))?", body[i])
                if m and (int(m.group(1)) in dests or (m.group(2) is not None and int(m.group(2)) in dests)):
                    bad.append(body[i])
            assert not bad, f"{head}: register copies of hand-issued load destinations: {bad[:8]}"
    assert found == 16, f"expected 16 4-bit expert GEMM instantiations (2 kernels x 2 dtypes x 4 row tiles), found {found}"
