"""Everything that reads a HuggingFace module: what LlamaRunner.from_hf is handed, decided once and written down as data.

classify(lm, ...) asks the module every question the import needs -- per decoder layer (Layer: is it sparse, which quantised form do its
experts have) and per model (which format do the seven projections arrive in) -- makes every refusal that needs no device, and returns a
Checkpoint.  load(lm, ckpt, ...) is the import loop; it reads the Checkpoint and no module type.  LlamaRunner.from_hf's docstring is the
contract of both.

A new checkpoint format adds here: a per-layer predicate (experts_are_*) with its Layer property if its experts have
a module form of their own, a place in classify's precedence, and its record in formats.DENSE_FORMATS / moe.EXPERT, which load() imports
through.  classify is the one place where formats are still told apart by name: it is precedence logic, written out."""
import os
from functools import cached_property
from typing import NamedTuple, Optional

import torch

from . import SamdError
from . import fp8 as F8
from . import mxfp4 as MX
from . import int4 as I4
from . import int8 as I8
from . import moe as MOE
from .formats import DENSE, DenseFormat, is_f4_tensor, tiles

# the seven projections of a decoder layer (a sparse layer's MLP has no gate / up / down projections of its own)
PARTS = (("self_attn", "q_proj"), ("self_attn", "k_proj"), ("self_attn", "v_proj"), ("self_attn", "o_proj"), ("mlp", "gate_proj"),
         ("mlp", "up_proj"), ("mlp", "down_proj"))
# the parameters of a decoder layer that load() reads (named_parameters; FP8 checkpoints' weight_scale tensors are buffers)
LAYER_PARAMS = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight", "input_layernorm.weight", "post_attention_layernorm.weight")
QKV_BIAS = ("self_attn.q_proj.bias", "self_attn.k_proj.bias", "self_attn.v_proj.bias")
QK_NORM = ("self_attn.q_norm.weight", "self_attn.k_norm.weight")


def _expert_modules(lyr):
    """a layer's `mlp.experts` when it is indexable per expert (a ModuleList of modules with gate_proj / up_proj / down_proj), else None"""
    ex = getattr(getattr(lyr, "mlp", None), "experts", None)
    if ex is None or hasattr(ex, "gate_up_proj") or not hasattr(ex, "__len__") or not hasattr(ex, "__getitem__"):
        return None
    return ex


def experts_are_4bit(lyr, i):
    """does sparse layer i carry pre-quantised experts?  Both fused tensors 4-bit: True; neither: False; one of them raises by name"""
    ex = lyr.mlp.experts
    gu, dn = is_f4_tensor(ex.gate_up_proj), is_f4_tensor(ex.down_proj)
    if gu != dn:
        raise SamdError(f"layers.{i}.mlp.experts: gate_up_proj is {ex.gate_up_proj.dtype} and down_proj {ex.down_proj.dtype}; "
                        "4-bit experts need both tensors 4-bit")
    return gu


def experts_are_fp8(lyr, i):
    """does layer i hold FP8 experts -- the fused form (transformers' FP8Experts: float8 gate_up_proj and down_proj) or an indexable
    `mlp.experts` of modules whose gate_proj / up_proj / down_proj weights are all float8?  All: True; none (or no experts): False; some
    only: raises by name"""
    ex = getattr(getattr(lyr, "mlp", None), "experts", None)
    if ex is None:
        return False
    if hasattr(ex, "gate_up_proj"):
        kinds = [(f"layers.{i}.mlp.experts.{p}", F8.is_fp8_dtype(getattr(ex, p).dtype)) for p in ("gate_up_proj", "down_proj")
                 if getattr(ex, p, None) is not None]
    elif _expert_modules(lyr) is not None:
        kinds = [(f"layers.{i}.mlp.experts.{e}.{p}", F8.is_fp8_dtype(getattr(ex[e], p).weight.dtype))
                 for e in range(len(ex)) for p in MOE.INT4_EXPERT_PROJECTIONS if getattr(getattr(ex[e], p, None), "weight", None) is not None]
    else:
        return False
    n8 = sum(k for _, k in kinds)
    if 0 < n8 < len(kinds):
        plain = [n for n, k in kinds if not k][:3]
        raise SamdError(f"layers.{i}.mlp.experts: a mix of FP8 and other expert tensors ({n8} of {len(kinds)} are FP8; e.g. "
                        f"{', '.join(plain)} are not): FP8 experts need every expert tensor float8_e4m3fn")
    return n8 > 0


def experts_are_int8(lyr, config=None):
    """does the layer hold per-expert 8-bit GPTQ modules -- an indexable `mlp.experts` of modules whose gate_proj, up_proj and down_proj
    are ALL 8-bit (int8.is_int8_module)?  Anything less is False: classify then refuses whatever 8-bit module it finds, by name"""
    ex = _expert_modules(lyr)
    if ex is None or len(ex) == 0:
        return False
    return all(I8.is_int8_module(getattr(ex[e], p, None), config) for e in range(len(ex)) for p in MOE.INT4_EXPERT_PROJECTIONS)


def experts_are_int4(lyr, i):
    """does layer i hold per-expert INT4 (AWQ / GPTQ) modules -- an indexable `mlp.experts` of modules with gate_proj / up_proj / down_proj
    that are all INT4 (int4.is_int4_module)?  All: True; none (or the fused form, or no experts): False; some experts or some of the
    three projections only: raises by name"""
    ex = _expert_modules(lyr)
    if ex is None:
        return False
    kinds = [(f"layers.{i}.mlp.experts.{e}.{p}", I4.is_int4_module(getattr(ex[e], p, None)))
             for e in range(len(ex)) for p in MOE.INT4_EXPERT_PROJECTIONS]
    n4 = sum(k for _, k in kinds)
    if 0 < n4 < len(kinds):
        plain = [n for n, k in kinds if not k][:3]
        raise SamdError(f"layers.{i}.mlp.experts: a mix of INT4 and other expert projections ({n4} of {len(kinds)} are INT4; e.g. "
                        f"{', '.join(plain)} are not): INT4 experts need gate_proj, up_proj and down_proj of every expert INT4")
    return n4 > 0


class Layer:
    """one decoder layer and what its MLP holds.  Each question is put to the module when it is first asked and at most once -- the answer is
    kept, and a question that raises ends the import -- so the order in which classify asks is the order of its refusals, and the per-expert
    scans (every expert x 3 projections) do not repeat.  `int4` is also true of 8-bit GPTQ modules (they carry qweight / qzeros / scales
    too): whether a stack's experts are 8-bit is decided over all its layers, first."""

    def __init__(self, module, index, qcfg=None):
        self.module, self.index, self.qcfg = module, index, qcfg

    @cached_property
    def sparse(self):
        """does its MLP hold experts (an HF Qwen3MoeSparseMoeBlock)?"""
        return any(n.startswith("mlp.experts.") for n, _ in self.module.named_parameters()) or self.int4

    int8 = cached_property(lambda self: experts_are_int8(self.module, self.qcfg))
    fp8 = cached_property(lambda self: experts_are_fp8(self.module, self.index))
    int4 = cached_property(lambda self: experts_are_int4(self.module, self.index))
    mxfp4 = cached_property(lambda self: experts_are_4bit(self.module, self.index))


def sparse_layers(layers):
    """per decoder layer: does its MLP hold experts?"""
    return [Layer(lyr, i).sparse for i, lyr in enumerate(layers)]


def layer_extras(layers, facts=None):
    """(qkv_bias, qk_norm) of an HF decoder stack (Llama, Qwen2, Qwen3).  Every layer's named parameters must be exactly the set the runner
    consumes: the Llama ones, plus q|k|v biases, plus q / k norm weights, the same in every layer (an FP8 projection's weight_scale /
    input_scale count as its own, whether buffers or parameters).  Anything else -- an o_proj or MLP bias, a parameter the runner would
    not read -- raises instead of being dropped.  A Qwen3-MoE layer whose MLP is a sparse block holds, instead of the three MLP projections,
    the router `mlp.gate.weight` and the fused expert tensors `mlp.experts.gate_up_proj` / `mlp.experts.down_proj` (dense and sparse layers
    may alternate); a shared expert or any other MLP parameter raises by name.  facts: classify's Layer records of the same layers."""
    if len(layers) == 0:
        raise SamdError("the model has no decoder layers")
    facts = facts or [Layer(lyr, i) for i, lyr in enumerate(layers)]
    def names_of(lyr, i):
        # an FP8 projection's scales may be parameters as well as buffers (fbgemm / compressed-tensors layers): the runner reads
        # weight_scale through samd_hip/fp8.py (input scales are not used: weight-only FP8), so they are not extra parameters
        # (the same holds for an MXFP4 projection -- a float4_e2m1fn_x2 or uint8 weight -- and its e8m0 weight_scale)
        skip = {f"{n[:-len('.weight')]}.{sc}" for n, p in lyr.named_parameters()
                if n.endswith(".weight") and (F8.is_fp8_dtype(p.dtype) or is_f4_tensor(p))
                for sc in ("weight_scale", "input_scale", "weight_scale_inv")}
        # the block scales of 4-bit expert tensors (samd_hip/moe.py), which the runner reads; beside plain experts they are extra
        params = dict(lyr.named_parameters())
        # an AWQ / GPTQ projection holds qweight / qzeros / scales (/ g_idx) and maybe a bias, as buffers or parameters, in place of a
        # `weight`: it counts as that weight, and its bias counts as a bias
        for n, mod in lyr.named_modules():
            if n and I4.is_int4_module(mod):
                for own in list(params):
                    if own.startswith(n + "."):
                        del params[own]
                params[n + ".weight"] = None
                if getattr(mod, "bias", None) is not None:
                    params[n + ".bias"] = None
        if any(is_f4_tensor(params.get(n)) for n in MOE.SPARSE_MLP_PARAMS[1:]):
            skip |= set(MOE.EXPERT_SCALE_PARAMS)
        # FP8 experts (samd_hip/moe.py): the fused form's two scale tensors are read.  The per-expert forms -- FP8
        # (mlp.experts.{e}.gate_proj.weight + weight_scale_inv, skipped above) and INT4 (their tensors are buffers) -- count as the two
        # fused expert tensors; a bias of one of them stays in the set and raises by name below
        if facts[i].fp8:
            skip |= set(MOE.FP8_EXPERT_SCALE_PARAMS)
        for per_expert in (facts[i].fp8 and not hasattr(lyr.mlp.experts, "gate_up_proj"), facts[i].int4):
            if per_expert:
                for e in range(len(lyr.mlp.experts)):
                    for pn in MOE.INT4_EXPERT_PROJECTIONS:
                        params.pop(f"mlp.experts.{e}.{pn}.weight", None)
                params.update({n: None for n in MOE.SPARSE_MLP_PARAMS[1:]})
        return set(params) - skip
    names0 = names_of(layers[0], 0)
    qkv_bias = any(n in names0 for n in QKV_BIAS)
    qk_norm = any(n in names0 for n in QK_NORM)
    want = set(LAYER_PARAMS) | (set(QKV_BIAS) if qkv_bias else set()) | (set(QK_NORM) if qk_norm else set())
    want_sparse = (want - set(MOE.DENSE_MLP_PARAMS)) | set(MOE.SPARSE_MLP_PARAMS)
    for i, lyr in enumerate(layers):
        names = names_of(lyr, i)
        if names == want:
            continue
        if any(n.startswith("mlp.experts.") or n == "mlp.gate.weight" for n in names):      # a sparse (Qwen3-MoE) layer
            if names == want_sparse:
                continue
            if any("shared_expert" in n for n in names):
                raise SamdError(f"layer {i}: a shared expert is not supported (parameters {sorted(n for n in names if 'shared_expert' in n)})")
            raise SamdError(f"layer {i}: sparse MLP parameters the runner does not consume {sorted(names - want_sparse)}, or lacks "
                            f"{sorted(want_sparse - names)} (it reads mlp.gate.weight and the fused mlp.experts.gate_up_proj / down_proj)")
        extra, missing = sorted(names - want), sorted(want - names)
        if "self_attn.o_proj.bias" in extra:
            raise SamdError(f"layer {i}: o_proj bias is not supported (q|k|v biases are)")
        if any(n.startswith("mlp.") and n.endswith(".bias") for n in extra):
            raise SamdError(f"layer {i}: MLP projection biases are not supported")
        raise SamdError(f"layer {i}: parameters the runner does not consume {extra}, or lacks {missing} "
                        f"(it reads the Llama layer, q|k|v biases (Qwen2) and q / k norm weights (Qwen3))")
    return qkv_bias, qk_norm


class Checkpoint(NamedTuple):
    """what classify decided about a module: all load() reads"""
    shape: object                    # the LlamaShape
    dtype: torch.dtype               # the model dtype the runner computes in
    sparse: list                     # per decoder layer: is its MLP a sparse block?
    qkv_bias: bool
    qk_norm: bool
    dense: Optional[DenseFormat]     # the format the seven projections are imported in, as they are; None: plain weights
    experts: MOE.ExpertFormat        # the format the sparse layers' experts are imported in, as they are (name None: HF's fused model-dtype tensors)
    dequantise: Optional[str]        # the format whose attention / dense-MLP projections, beside experts of that format, are dequantised once at import
    qcfg: object                     # config.quantization_config as the INT4 / INT8 importers read it
    qcfg8: object                    # ... and as the FP8 importers do


def _refuse_stray_int8(layers, int8, qcfg):
    """8-bit GPTQ modules in a module with sparse layers are taken when EVERY sparse layer's experts are 8-bit GPTQ modules throughout
    (`int8`: expert_format "int8g128"); then the attention and dense-MLP projections may be 8-bit too (dequantised once at import).
    Anywhere else in such a module -- some experts or projections of a layer only, a router, 8-bit projections beside other experts -- an
    8-bit module raises by name"""
    served = {f"{a}.{b}" for a, b in PARTS} if int8 else set()
    for l in sorted(layers, key=lambda l: l.sparse and l.int8):      # (a layer whose experts are 8-bit only in part is named first)
        for n, mod in l.module.named_modules():
            if n and I8.is_int8_module(mod, qcfg) and n not in served and not (int8 and l.sparse and n.startswith("mlp.experts.")):
                if int8 and n == "mlp.gate":
                    raise SamdError(f"layers.{l.index}.{n}: an 8-bit router is not supported: the router stays a plain `weight` in the model dtype")
                if int8:
                    raise SamdError(f"layers.{l.index}.{n}: an 8-bit GPTQ module in a mixture-of-experts model with INT8 experts: only the "
                                    "experts, the attention projections and a dense layer's MLP projections may be 8-bit")
                raise SamdError(f"layers.{l.index}.{n}: an 8-bit GPTQ module in a mixture-of-experts model whose sparse layers' experts are not "
                                "all 8-bit GPTQ modules throughout: 8-bit modules are taken there only beside such experts (expert_format "
                                "'int8g128'); weight_format 'int8g128' covers dense models only, and nothing is dequantised silently")


def classify(lm, weight_format=None, expert_format=MOE.AUTO, dtype=None, native_gemm=True, draft_head=False):
    """the Checkpoint of a transformers causal LM, or the SamdError of the first thing about it the runner does not take.  No device work,
    nothing allocated beyond the per-layer records; the order of the checks is the order in which two applicable refusals are raised."""
    from .llama import LlamaShape                                # (llama imports this module)
    m = lm.model
    qcfg = I4.quant_config(getattr(lm, "config", None))
    qcfg8 = getattr(getattr(lm, "config", None), "quantization_config", None)
    layers = [Layer(lyr, i, qcfg) for i, lyr in enumerate(m.layers)]
    linears = [(f"layers.{l.index}.{a}.{b}", getattr(getattr(l.module, a), b)) for l in layers for a, b in PARTS if hasattr(getattr(l.module, a), b)]
    # 8-bit GPTQ modules are decided first: they carry qweight / qzeros / scales too, so the INT4 tests are true for them
    sparse = [l.sparse for l in layers]
    int8 = any(sparse) and [l.sparse and l.int8 for l in layers] == sparse
    if any(sparse):
        _refuse_stray_int8(layers, int8, qcfg)
    dense_i8 = I8.checkpoint_is_int8(linears, qcfg)              # all seven projections of every layer, or a SamdError for a mix
    dense_i4 = (not dense_i8) and I4.checkpoint_is_int4(linears)     # AWQ / GPTQ modules (qweight / qzeros / scales, no `weight`)
    # a module with block-scaled FP8 EXPERTS (the official Qwen3-MoE FP8 checkpoints) is not a weight_format "fp8" one: its FP8 attention
    # and dense-MLP projections are dequantised once at import.  Decided before checkpoint_is_fp8, which rejects block scales
    fp8_experts = any([l.fp8 for l in layers])
    # a module WITHOUT sparse layers whose projections are all block-scaled FP8 (the dense Qwen3-*-FP8 checkpoints) is imported as it is,
    # codes and scales untouched, and the runner is "fp8b128" by itself; modules with sparse layers are left to the branches above
    dense_f8b = not (dense_i4 or dense_i8 or fp8_experts or any(sparse)) and F8.checkpoint_is_fp8_block(linears, qcfg8)
    if dense_f8b:
        if weight_format not in (None, "fp8b128"):
            raise SamdError(f"the module carries block-scaled FP8 projections; weight_format {weight_format!r} would need them dequantised "
                            "(pass None or 'fp8b128')")
        for name, lin in linears:                                # shapes the kernel cannot run, by projection, before any device work
            if not tiles(*lin.weight.shape):
                raise SamdError(f"{name}: a block-scaled FP8 projection of shape {tuple(lin.weight.shape)}; the kernel needs N % 128 == 0 and K % 256 == 0")
    dense_f8 = not (dense_i4 or dense_i8 or fp8_experts or dense_f8b) and F8.checkpoint_is_fp8(linears)
    dense_f4 = not (dense_i4 or dense_i8) and MX.checkpoint_is_mxfp4(linears)
    if F8.is_fp8_dtype(lm.lm_head.weight.dtype) or F8.is_fp8_dtype(m.embed_tokens.weight.dtype):
        raise SamdError("FP8 embedding / lm_head weights are not supported: they stay in the model dtype")
    if is_f4_tensor(lm.lm_head.weight) or is_f4_tensor(m.embed_tokens.weight):
        raise SamdError("4-bit embedding / lm_head weights are not supported: they stay in the model dtype")
    dtype = dtype or next(p.dtype for p in lm.parameters() if p.dtype.is_floating_point and p.dtype.itemsize >= 2)
    qkv_bias, qk_norm = layer_extras(m.layers, layers)
    shape = LlamaShape(lm.config, qkv_bias=qkv_bias, qk_norm=qk_norm)
    holders = [l for l in layers if l.sparse]
    i4 = [not int8 and l.int4 for l in holders]
    # INT4 / INT8 / FP8 EXPERTS whose attention / dense-MLP projections are quantised likewise (an AWQ / GPTQ / FP8 mixture-of-experts
    # checkpoint): those are dequantised once at import, so the runner is not a weight_format one.  Quantised projections beside
    # model-dtype experts or experts of another format stay rejected: as the dense format they are, by reject_unsupported below
    dequantise = "int4g128" if dense_i4 and any(i4) else "int8g128" if dense_i8 and int8 else "fp8b128" if fp8_experts else None
    # the one dense format the module's projections are imported in, as they are (at most one detector holds)
    dense = None if dequantise in ("int4g128", "int8g128") else DENSE.get(
        "int4g128" if dense_i4 else "int8g128" if dense_i8 else "mxfp4" if dense_f4 else "fp8b128" if dense_f8b else "fp8" if dense_f8 else None)
    moe = any(sparse) or shape.moe
    if moe:
        if sparse != list(shape.sparse):
            raise SamdError(f"the module's sparse MLP layers {[i for i, x in enumerate(sparse) if x]} are not the ones its config implies "
                            f"{[i for i, x in enumerate(shape.sparse) if x]} (model_type '{shape.model_type}')")
        MOE.reject_unsupported(dense.name if dense is not None else weight_format, native_gemm, draft_head)
    # quantised experts: decided and checked on the module's own tensors (the runner resolves the format again from the weights it is given)
    f8 = [l.fp8 for l in holders]
    f4 = [not a and not int8 and not b and l.mxfp4 for l, a, b in zip(holders, i4, f8)]
    MOE.resolve_expert_format(expert_format, any(f4), moe, carries_int4=any(i4), carries_fp8=any(f8), carries_int8=int8)
    experts = MOE.EXPERT["fp8b128" if any(f8) else "int4g128" if any(i4) else "int8g128" if int8 else "mxfp4" if any(f4) else None]
    lacking = lambda carried: [l.index for l, c in zip(holders, carried) if not c]
    if any(f8):
        if not all(f8):
            raise MOE.EXPERT["fp8b128"].mix_refusal(f8, lacking(f8))
        for l in holders:
            ex = l.module.mlp.experts
            n_ex = ex.gate_up_proj.shape[0] if hasattr(ex, "gate_up_proj") else len(ex)
            if n_ex != shape.n_experts:
                raise SamdError(f"layers.{l.index}.mlp.experts: {n_ex} experts, the config says num_experts = {shape.n_experts}")
            gate = getattr(l.module.mlp, "gate", None)
            if gate is None or getattr(gate, "weight", None) is None or F8.is_fp8_dtype(gate.weight.dtype):
                raise SamdError(f"layers.{l.index}.mlp.gate: an FP8 router is not supported: the router stays a plain `weight` in the model dtype")
    if any(i4) and not all(i4):
        raise MOE.EXPERT["int4g128"].mix_refusal(i4, lacking(i4))
    for l in holders:
        if (any(i4) or int8) and len(l.module.mlp.experts) != shape.n_experts:
            raise SamdError(f"layers.{l.index}.mlp.experts: {len(l.module.mlp.experts)} expert modules, the config says num_experts = {shape.n_experts}")
        if I4.is_int4_module(getattr(l.module.mlp, "gate", None)):
            raise SamdError(f"layers.{l.index}.mlp.gate: an INT4 router is not supported: the router stays a plain `weight` in the model dtype")
    if any(f4):
        if not all(f4):
            raise MOE.EXPERT["mxfp4"].mix_refusal(f4, lacking(f4))
        for l in holders:
            ex = l.module.mlp.experts
            MOE.check_quantised_experts(ex.gate_up_proj.detach(), getattr(ex, "gate_up_proj_scale", None), ex.down_proj.detach(),
                                        getattr(ex, "down_proj_scale", None), dtype, f"layers.{l.index}.mlp.experts")
    return Checkpoint(shape, dtype, sparse, qkv_bias, qk_norm, dense, experts, dequantise, qcfg, qcfg8)


def _dequantise_groups(Q, linear):
    """INT4 / INT8: rne_dtype((q - z) * s), one rounding"""
    def dequantise(mod, name, dtype, ckpt):
        q, z, sc = linear(mod, name, config=ckpt.qcfg)
        return Q.dequantize_groups(q, z, Q.as_scales(sc, dtype, name)).to(dtype)
    return dequantise


def _dequantise_fp8(mod, name, dtype, ckpt):
    """rne_dtype(fl32(float(q) * s)), one rounding; a plain projection beside FP8 ones is taken as it is"""
    w = F8.linear_fp8_dequantized(mod, name, ckpt.qcfg8)
    return mod.weight if w is None else w.to(dtype)


# Checkpoint.dequantise -> (module, name, dtype, ckpt) -> the projection's weight, exactly what a quantised launch would multiply by
DEQUANTISE = {None: lambda mod, name, dtype, ckpt: mod.weight, "int4g128": _dequantise_groups(I4, I4.linear_int4),
              "int8g128": _dequantise_groups(I8, I8.linear_int8), "fp8b128": _dequantise_fp8}


def load(lm, ckpt, device, share=None):
    """the raw weights dict LlamaRunner's constructor takes, on `device`, of a module classify has answered for.  share: from_hf's
    share_weights."""
    dev, dtype, m = torch.device(device), ckpt.dtype, lm.model
    dense, lin_w = ckpt.dense, DEQUANTISE[ckpt.dequantise]

    def get(t):
        return t.detach().to(device=dev, dtype=dtype).contiguous()
    # The runner reads q|k|v and gate|up as ONE matrix each.  When the HF module already lives on this device in this dtype, its
    # separate projection weights are re-pointed at row slices of the concatenated matrices (same values, the module keeps working),
    # so the model exists once row-major (+ once packed) instead of the HF copy + the concatenated copy + the packed copy.
    # Opt-in (share_weights=True / SAMD_SHARE_HF_WEIGHTS=1): by default the caller's module is left untouched.
    share = (os.environ.get("SAMD_SHARE_HF_WEIGHTS", "0") == "1") if share is None else bool(share)
    shared = 0

    def fuse(linears, names):
        """one matrix of a group of projections (q|k|v, o, gate|up, down), in the model dtype"""
        nonlocal shared
        ws = [lin_w(l, n, dtype, ckpt) for l, n in zip(linears, names)]
        if len(ws) == 1:
            return get(ws[0])
        if any(w is not getattr(l, "weight", None) for w, l in zip(ws, linears)):      # dequantised: there is no HF `weight` to re-point
            return get(torch.cat([w.to(dtype) for w in ws], dim=0))
        cat = get(torch.cat(ws, dim=0))
        if share and all(w.device == cat.device and w.dtype == cat.dtype for w in ws):
            r = 0
            for l in linears:
                n = l.weight.shape[0]
                l.weight.data = cat[r:r + n]
                r += n
            shared += 1
        return cat
    layers = []
    for li, lyr in enumerate(m.layers):
        a, f = lyr.self_attn, lyr.mlp
        groups, lw = [("wqkv", a, "self_attn", ("q_proj", "k_proj", "v_proj")), ("wo", a, "self_attn", ("o_proj",))], {}
        if not ckpt.sparse[li]:
            groups += [("wgu", f, "mlp", ("gate_proj", "up_proj")), ("wdown", f, "mlp", ("down_proj",))]
        for k, own, part, names in groups:
            mods = [getattr(own, x) for x in names]
            if dense is not None:                                # the checkpoint's own codes and side data; the runner checks and packs them
                lw.update({k + sfx: t for sfx, t in zip(dense.raw_keys, dense.import_hf(mods, names, li, part, dev, dtype, ckpt.qcfg, ckpt.qcfg8))})
            else:
                lw[k] = fuse(mods, [f"layers.{li}.{part}.{x}" for x in names])
        if ckpt.sparse[li]:                                      # router + the experts as the module holds them (moe.EXPERT: import_hf)
            lw.update(router=get(f.gate.weight), **ckpt.experts.import_hf(f.experts, f"layers.{li}.mlp.experts", dtype, dev, ckpt.qcfg, ckpt.qcfg8))
        lw.update(ln1=get(lyr.input_layernorm.weight), ln2=get(lyr.post_attention_layernorm.weight))
        if ckpt.qkv_bias:                                        # Qwen2 q|k|v bias, Qwen3 q / k norm (samd_rope_kv_write_epi)
            lw["bqkv"] = get(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]))
        if ckpt.qk_norm:
            lw["q_norm"], lw["k_norm"] = get(a.q_norm.weight), get(a.k_norm.weight)
        layers.append(lw)
    weights = dict(embed=get(m.embed_tokens.weight), layers=layers, norm=get(m.norm.weight), lm_head=get(lm.lm_head.weight))
    if shared:
        import logging
        logging.getLogger("samd_hip").info("LlamaRunner.from_hf: %d fused projection groups now back the HF module's q/k/v and gate/up "
                                           "weights (share_weights); its parameters are views of the runner's matrices", shared)
    return weights
