"""Dense block-scaled FP8 (weight_format "fp8b128": e4m3fn codes + one fp32 scale per 128 x 128 block), without a GPU: the fusing helper,
the format resolution table, the importer's rejections through from_hf on a tiny module of transformers' own FP8Linears, a numpy restatement
of the numeric contract, and what the hand-issued loads of k_gemm_skinny_f8b need from its code object."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from samd_hip import SamdError
from samd_hip import fp8 as F8
from samd_hip import llama as LL
from samd_hip.llama import LlamaRunner
from test_codeobject_cpu import READELF, SO, gfx950_code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "k_gemm_skinny_f8b"
ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP = ("gate_proj", "up_proj", "down_proj")
QCFG = dict(quant_method="fp8", activation_scheme="dynamic", weight_block_size=[128, 128])


# ------------------------------------------------------------------------------------------------ helpers of the format
def test_fusing_before_or_after_quantising_gives_the_same_bytes():
    g = torch.Generator().manual_seed(3)
    parts = [torch.randn((n, 512), generator=g) * s for n, s in ((256, 0.02), (128, 0.5), (128, 3.0))]
    q_all, s_all = F8.quantize_blocks(torch.cat(parts, 0).to(torch.float16))
    q_cat, s_cat = F8.fuse_fp8_blocks([F8.quantize_blocks(p.to(torch.float16)) for p in parts], "cpu")
    assert q_cat.dtype == torch.float8_e4m3fn and s_cat.dtype == torch.float32 and tuple(s_cat.shape) == (4, 4)
    assert torch.equal(q_all.view(torch.uint8), q_cat.view(torch.uint8)) and torch.equal(s_all, s_cat)
    assert F8.block_scaled_bytes(512, 512) == 512 * 512 + 4 * 4 * 4 == q_cat.numel() + 4 * s_cat.numel()


def test_fusing_rejects_parts_whose_blocks_would_straddle_by_name():
    q, s = F8.quantize_blocks(torch.ones(256, 256))
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.up_proj: a \[192, 256\]"):
        F8.fuse_fp8_blocks([(q, s), (q[:192], s)], "cpu", ["layers.0.mlp.gate_proj", "layers.0.mlp.up_proj"])
    with pytest.raises(SamdError, match="part 1"):
        F8.fuse_fp8_blocks([(q, s), (q, s[:1])], "cpu")


def _weights(kind, layers=2):
    """a raw weights dict as LlamaRunner takes it, projections only: "plain", "row" (per-row FP8) or "block" (block-scaled FP8)"""
    out = []
    for _ in range(layers):
        l = {}
        for k in F8.PROJECTIONS:
            w = torch.zeros(256, 256, dtype=torch.float16)
            if kind == "plain":
                l[k] = w
            elif kind == "row":
                l[k], l[k + "_scale"] = F8.quantize_rows(w)
            else:
                l[k], l[k + "_sinv"] = F8.quantize_blocks(w)
        out.append(l)
    return dict(layers=out)


def test_format_resolution_table(monkeypatch):
    W, h = LL._weight_format, torch.float16
    # explicit values on plain weights
    for fmt in ("fp8", "fp8b128", "mxfp4", "int4g128"):
        assert W(fmt, _weights("plain"), h) == fmt
    assert W(None, _weights("plain"), h) is None and W("fp16", _weights("plain"), h) is None and W(h, _weights("plain"), h) is None
    # what the tensors carry: the _sinv keys tell block-scaled from per-row
    assert W(None, _weights("block"), h) == "fp8b128" and W("fp8b128", _weights("block"), h) == "fp8b128"
    assert W(None, _weights("row"), h) == "fp8" and W("fp8", _weights("row"), h) == "fp8"
    # every conflict
    for other in ("fp8", "mxfp4", "int4g128", "fp16", h):
        with pytest.raises(SamdError, match=r"the weights carry block-scaled FP8 projections; .*pass None or 'fp8b128'"):
            W(other, _weights("block"), h)
    with pytest.raises(SamdError, match=r"the weights carry float8_e4m3fn projections; .*pass None or 'fp8'\)"):
        W("fp8b128", _weights("row"), h)
    with pytest.raises(SamdError, match="expected None, 'fp8', 'mxfp4', 'int4g128', 'fp8b128' or the model dtype"):
        W("fp8b64", _weights("plain"), h)
    with pytest.raises(SamdError, match="spelled 'int4g128'"):
        W("int4", _weights("plain"), h)
    # the environment reaches callers that cannot pass a format; an explicit value wins
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "fp8b128")
    assert LL._env_weight_format(None) == "fp8b128" and LL._env_weight_format("fp8") == "fp8"
    monkeypatch.delenv("SAMD_WEIGHT_FORMAT")
    assert LL._env_weight_format(None) is None


# ------------------------------------------------------------------------------------------------ from_hf on a tiny module of FP8Linears
def fp8_linear(w, **kw):
    """transformers' FP8Linear holding quantize_blocks(w) (partial blocks: the scale keeps the module's own ceil shape, untouched)"""
    from transformers.integrations.finegrained_fp8 import FP8Linear
    lin = FP8Linear(w.shape[1], w.shape[0], **dict(dict(block_size=(128, 128)), **kw)).to(w.device)
    if w.shape[0] % 128 == 0 and w.shape[1] % 128 == 0:
        lin.weight.data, lin.weight_scale_inv.data = F8.quantize_blocks(w.detach())
    else:
        lin.weight.data = w.detach().to(torch.float8_e4m3fn)
        lin.weight_scale_inv.data = torch.ones(tuple(lin.weight_scale_inv.shape), dtype=torch.float32)
    return lin


def tiny_dense(inter=1024, qwen3=False):
    if qwen3:
        from transformers import Qwen3Config as Cfg, Qwen3ForCausalLM as LM
    else:
        from transformers import LlamaConfig as Cfg, LlamaForCausalLM as LM
    torch.manual_seed(inter)
    return LM(Cfg(hidden_size=512, intermediate_size=inter, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                  vocab_size=300, tie_word_embeddings=False))


def to_block_checkpoint(lm, dtype=torch.float16):
    ck = copy.deepcopy(lm)
    for lyr in ck.model.layers:
        for p in ATTN:
            setattr(lyr.self_attn, p, fp8_linear(getattr(lyr.self_attn, p).weight.to(dtype)))
        for p in MLP:
            setattr(lyr.mlp, p, fp8_linear(getattr(lyr.mlp, p).weight.to(dtype)))
    ck.config.quantization_config = dict(QCFG)
    return ck


@pytest.fixture(scope="module")
def dense():
    return tiny_dense()


def H(ck, **kw):
    return LlamaRunner.from_hf(ck, 256, dtype=torch.float16, device="cpu", **kw)


@pytest.mark.parametrize("qwen3", [False, True])
def test_a_dense_block_scaled_module_passes_every_guard(monkeypatch, qwen3):
    """all seven projections per layer block-scaled: decided before checkpoint_is_fp8 (which rejects block scales); from_hf gets as far as the
    device with no argument, with the format's own name and with the environment's; any other format raises"""
    monkeypatch.delenv("SAMD_WEIGHT_FORMAT", raising=False)
    ck = to_block_checkpoint(tiny_dense(qwen3=qwen3))
    linears = [(f"layers.{i}.{p}", getattr(lyr.self_attn if p in ATTN else lyr.mlp, p)) for i, lyr in enumerate(ck.model.layers) for p in ATTN + MLP]
    assert F8.checkpoint_is_fp8_block(linears, QCFG) is True
    with pytest.raises(SamdError, match="block-scaled FP8"):                 # the per-row importer keeps rejecting such a Linear
        F8.checkpoint_is_fp8(linears)
    for kw in ({}, dict(weight_format="fp8b128")):
        with pytest.raises(SamdError, match="no MI355X"):
            H(ck, **kw)
    for other in ("fp8", "mxfp4", "int4g128", "fp16"):
        with pytest.raises(SamdError, match="block-scaled FP8 projections.*pass None or 'fp8b128'"):
            H(ck, weight_format=other)
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "fp8b128")
    with pytest.raises(SamdError, match="no MI355X"):
        H(ck)
    with pytest.raises(SamdError, match="no MI355X"):                        # quantise on load from a plain module
        H(tiny_dense(qwen3=qwen3))


def test_plain_and_per_row_modules_are_not_block_scaled(dense):
    lins = [(f"layers.{i}.{p}", getattr(lyr.self_attn, p)) for i, lyr in enumerate(dense.model.layers) for p in ATTN]
    assert F8.checkpoint_is_fp8_block(lins) is False


def test_importer_rejections_reach_from_hf_by_name(monkeypatch, dense):
    monkeypatch.delenv("SAMD_WEIGHT_FORMAT", raising=False)
    # ue8m0 scales (by the config's word, and by a scale that is not fp32), fp16 scales
    ck = to_block_checkpoint(dense)
    ck.config.quantization_config["scale_fmt"] = "ue8m0"
    with pytest.raises(SamdError, match=r"layers\.0\.self_attn\.q_proj: scale_fmt 'ue8m0'"):
        H(ck)
    for bad in (torch.uint8, torch.float16):
        ck = to_block_checkpoint(dense)
        lin = ck.model.layers[1].mlp.up_proj
        lin.weight_scale_inv = torch.nn.Parameter(lin.weight_scale_inv.detach().to(bad), requires_grad=False)
        with pytest.raises(SamdError, match=rf"layers\.1\.mlp\.up_proj: weight_scale_inv of dtype {bad}"):
            H(ck)
    # a wrong scale shape
    ck = to_block_checkpoint(dense)
    lin = ck.model.layers[0].self_attn.o_proj
    lin.weight_scale_inv = torch.nn.Parameter(torch.ones(4, 2), requires_grad=False)
    with pytest.raises(SamdError, match=r"layers\.0\.self_attn\.o_proj: weight_scale_inv of shape \(4, 2\)"):
        H(ck)
    ck = to_block_checkpoint(dense)
    ck.model.layers[1].mlp.down_proj.weight_scale_inv.data[1, 2] = float("inf")
    with pytest.raises(SamdError, match=r"layers\.1\.mlp\.down_proj: weight_scale_inv must be finite and positive"):
        H(ck)
    # [64, 64] blocks: the config's, and a module's own
    ck = to_block_checkpoint(dense)
    ck.config.quantization_config["weight_block_size"] = [64, 64]
    with pytest.raises(SamdError, match=r"layers\.0\.self_attn\.q_proj: weight_block_size \[64, 64\]"):
        H(ck)
    ck = to_block_checkpoint(dense)
    ck.model.layers[0].self_attn.k_proj.block_size = (64, 64)
    with pytest.raises(SamdError, match=r"layers\.0\.self_attn\.k_proj: block_size \[64, 64\]"):
        H(ck)
    # static activation scheme
    ck = to_block_checkpoint(dense)
    ck.config.quantization_config["activation_scheme"] = "static"
    with pytest.raises(SamdError, match=r"layers\.0\.self_attn\.q_proj: activation_scheme 'static'"):
        H(ck)
    # another FP8 encoding
    ck = to_block_checkpoint(dense)
    lin = ck.model.layers[0].mlp.gate_proj
    lin.weight = torch.nn.Parameter(lin.weight.detach().float().to(torch.float8_e5m2), requires_grad=False)
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.gate_proj: weights in float8_e5m2"):
        H(ck)


def test_mixes_are_rejected_with_examples(monkeypatch, dense):
    monkeypatch.delenv("SAMD_WEIGHT_FORMAT", raising=False)
    # block-scaled beside a plain projection
    ck = to_block_checkpoint(dense)
    ck.model.layers[1].mlp.up_proj = torch.nn.Linear(512, 1024, bias=False)
    with pytest.raises(SamdError, match=r"a mix of block-scaled FP8 and other projections \(13 of 14.*layers\.1\.mlp\.up_proj are not FP8"):
        H(ck)
    # block-scaled beside per-row FP8
    ck = to_block_checkpoint(dense)
    for p in ("q_proj", "v_proj"):
        w = dense.model.layers[0].self_attn.__getattr__(p).weight.detach()
        lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False)
        q, s = F8.quantize_rows(w)
        lin.weight = torch.nn.Parameter(q, requires_grad=False)
        lin.register_buffer("weight_scale", s)
        setattr(ck.model.layers[0].self_attn, p, lin)
    with pytest.raises(SamdError, match=r"a mix of block-scaled FP8.*\(12 of 14.*layers\.0\.self_attn\.q_proj, layers\.0\.self_attn\.v_proj carry a per-row"):
        H(ck)
    # attention block-scaled, MLP plain (half a checkpoint)
    ck = copy.deepcopy(dense)
    for lyr in ck.model.layers:
        for p in ATTN:
            setattr(lyr.self_attn, p, fp8_linear(getattr(lyr.self_attn, p).weight))
    with pytest.raises(SamdError, match=r"a mix of block-scaled FP8.*\(8 of 14.*layers\.0\.mlp\.gate_proj"):
        H(ck)


def test_shapes_the_kernel_cannot_run_are_rejected_by_projection(monkeypatch):
    monkeypatch.delenv("SAMD_WEIGHT_FORMAT", raising=False)
    # an intermediate size that is no multiple of 128: gate|up blocks would straddle (the module's own scale has a partial block)
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.gate_proj: weight_scale_inv of shape \(9, 4\).*partial blocks"):
        H(to_block_checkpoint(tiny_dense(inter=1088)))
    # a multiple of 128 that is no multiple of 256: the down projection's K
    with pytest.raises(SamdError, match=r"layers\.0\.mlp\.down_proj: a block-scaled FP8 projection of shape \(512, 384\).*K % 256 == 0"):
        H(to_block_checkpoint(tiny_dense(inter=384)))


def test_an_fp8_lm_head_stays_rejected(dense):
    ck = to_block_checkpoint(dense)
    ck.lm_head = fp8_linear(torch.randn(384, 512))
    with pytest.raises(SamdError, match="FP8 embedding / lm_head"):
        H(ck)


def test_the_new_format_stays_rejected_for_mixture_of_experts_models(monkeypatch):
    from samd_hip import moe as MOE
    from test_moe_cpu import qwen3_moe
    monkeypatch.delenv("SAMD_EXPERT_FORMAT", raising=False)
    with pytest.raises(SamdError, match="mixture-of-experts"):
        MOE.reject_unsupported("fp8b128")
    torch.manual_seed(7)
    _, lm = qwen3_moe(mlp_only_layers=[0])
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu", weight_format="fp8b128")
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "fp8b128")
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


# ------------------------------------------------------------------------------------------------ the numeric contract, restated
def contract_np(A, q, s):
    """out = sum_b s_b * (sum_{k in block b} A q): the block sum in fp32, ONE fp32 FMA per block (a float64 product and sum of fp32 values,
    rounded once: the product of two fp32 values is exact in float64), blocks in ascending order"""
    A, q, s = A.astype(np.float32), q.astype(np.float32), s.astype(np.float32)
    M, K = A.shape
    N = q.shape[0]
    acc = np.zeros((M, N), np.float32)
    for b in range(K // 128):
        blk = np.zeros((M, N), np.float32)
        for k in range(128 * b, 128 * b + 128):                              # fp32 accumulation, one product at a time
            blk = (blk + A[:, k:k + 1] * q[None, :, k]).astype(np.float32)
        sb = np.repeat(s[:, b], 128)[None, :]
        acc = (blk.astype(np.float64) * sb.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_contract_matches_the_dequantised_product_within_fp32_rounding(dtype):
    """against float64 A @ dequantize_blocks(q, s).T.  Bound, per output: every product is exact in fp32 (an 11- or 8-bit A times a 4-bit code),
    a block sum of 128 terms errs by at most 127 u * sum|a q| (u = 2^-24), each of the K / 128 FMAs adds one rounding of a partial result
    bounded by sum|a w|, and the reference itself rounds every weight once (fl32(float(q) * s)): (127 + K / 128 + 1) u * sum|a||w| in all,
    first order; 1.01 x that for the higher-order terms."""
    g = torch.Generator().manual_seed(11)
    N, K, M = 256, 768, 8
    W = torch.randn((N, K), generator=g) * torch.exp2(torch.randint(-6, 3, (N // 128, K // 128), generator=g).float()).repeat_interleave(128, 0).repeat_interleave(128, 1)
    q, s = F8.quantize_blocks(W)
    A = torch.randn((M, K), generator=g).to(dtype)
    Wd = F8.dequantize_blocks(q, s)
    want = A.double() @ Wd.double().t()
    got = contract_np(A.float().numpy(), q.float().numpy(), s.numpy())
    bound = 1.01 * (127 + K // 128 + 1) * 2.0 ** -24 * (A.double().abs() @ Wd.double().abs().t()).numpy()
    err = np.abs(got.astype(np.float64) - want.numpy())
    assert (err <= bound).all(), (err / bound).max()
    # the scales matter: the next k block's scale misses by far more than the bound
    wrong = contract_np(A.float().numpy(), q.float().numpy(), np.roll(s.numpy(), 1, axis=1))
    assert (np.abs(wrong.astype(np.float64) - want.numpy()) > bound).mean() > 0.9


# ------------------------------------------------------------------------------------------------ the compiled kernels
def _disassembled_kernels(tmp_path):
    blob = open(SO, "rb").read()
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        text = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
        for chunk in re.split(r"\n(?=[0-9a-f]+ <)", text):
            head = chunk.split("\n", 1)[0]
            if KERNEL in head:
                yield head, [l.split("//")[0].strip() for l in chunk.split("\n")[1:]]


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_hand_issued_loads_are_the_only_vector_loads_and_no_copy_touches_them(tmp_path):
    """k_gemm_skinny_f8b waits with counted vmcnt (PC = 4 + XV memory operations per thread and chunk), so in every instantiation
      * the only vector loads from memory are the 16-byte nt weight loads and the 16-byte LDS-DMA A loads -- the block scales arrive as scalar
        8-byte loads, which count on lgkmcnt;
      * no register copy touches a hand-issued load's destination in the prologue (first load to the first phase's barrier), where a short
        split's skipped loads would be merged with loaded values by copies."""
    found = 0
    for head, body in _disassembled_kernels(tmp_path):
        found += 1
        dests, load_at, lds_dma, scalar2, other = set(), [], 0, 0, []
        for i, l in enumerate(body):
            m = re.match(r"global_load_dwordx4 v\[(\d+):(\d+)\], v\d+, s\[\d+:\d+\](?: offset:\d+)? nt$", l)
            if m:
                dests |= set(range(int(m.group(1)), int(m.group(2)) + 1))
                load_at.append(i)
            elif re.match(r"global_load_lds_dwordx4 ", l):
                lds_dma += 1
            elif re.match(r"(global|flat|buffer|scratch)_(load|atomic)", l) or re.match(r"(tbuffer_load|image_)", l):
                other.append(l)
            elif re.match(r"s_load_dwordx2 ", l):
                scalar2 += 1
        assert not other, f"{head}: vector loads beside the weight and A streams break the counted waits: {other[:6]}"
        assert len(load_at) >= 12 and lds_dma >= 3 and len(dests) in (48, 64), (head, len(load_at), lds_dma, len(dests))
        assert scalar2 >= 3, f"{head}: the block scales are wave-uniform 8-byte scalar loads (found {scalar2} besides none expected elsewhere)"
        barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier") and i > load_at[0])
        bad = []
        for i in range(load_at[0], barrier):
            m = re.match(r"v_mov_b32_e32 v(\d+), (?:v(\d+))?", body[i])
            if m and (int(m.group(1)) in dests or (m.group(2) is not None and int(m.group(2)) in dests)):
                bad.append(body[i])
        assert not bad, f"{head}: register copies of hand-issued load destinations: {bad[:8]}"
    assert found == 8, f"expected the 8 instantiations of {KERNEL} (2 dtypes x 4 row tiles), found {found}"


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_no_instantiation_spills_and_two_workgroups_fit_where_the_lds_allows(tmp_path):
    """a spilled load destination would be stored to scratch before its data has landed: no private segment, no VGPR spills.  The 16- and
    32-row tiles (40 / 64 KiB of LDS) keep two workgroups per CU: 4 waves per SIMD, at most 128 VGPRs"""
    blob = open(SO, "rb").read()
    kernels = {}
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split(".name:")[1:]:
            name = block.split()[0]
            if KERNEL not in name or name.endswith(".kd"):
                continue
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"), vgprs=get("vgpr_count"),
                                 sgpr_spills=get("sgpr_spill_count"))
    for name, v in sorted(kernels.items()):
        print(name, v)
    assert len(kernels) == 8, f"expected the 8 instantiations of {KERNEL}, found {sorted(kernels)}"
    bad = {n: v for n, v in kernels.items() if v["scratch"] or v["vgpr_spills"] or v["sgpr_spills"]}
    assert not bad, f"kernels with hand-issued loads must not spill: {bad}"
    for n, v in kernels.items():
        if "Li1E" in n or "Li2E" in n:
            assert v["vgprs"] <= 128, (n, v)
        else:
            assert v["vgprs"] <= 256, (n, v)
