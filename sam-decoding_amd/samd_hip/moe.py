"""Mixture-of-experts MLP blocks (Qwen3-MoE) on the streaming kernels: which layers are sparse, the shapes the kernels serve, the expert
weights in their packed form and the three launches of a sparse layer (include/samd_hip.h: samd_moe_route, samd_moe_gate_up_silu,
samd_moe_down_combine).

A sparse layer holds `mlp.gate.weight` [E, H] (the router), `mlp.experts.gate_up_proj` [E, 2 I, H] and `mlp.experts.down_proj` [E, H, I] (this
transformers' fused form).  The experts are packed once at load -- per expert the 128-column tile layout of the dense streaming GEMM, gate
and up interleaved in groups of 64 so that a tile holds matching columns, experts end to end -- and no row-major copy is kept.

expert_format "mxfp4" (EXPERT_FORMATS) keeps the EXPERTS, and nothing else, as MXFP4 (samd_hip/mxfp4.py: e2m1 elements, one e8m0 scale per 32
along k): q [E, N, K/2] + e8 [E, N, K/32] per fused tensor, packed by samd_gemm_pack_f4 as one matrix of E * N rows and streamed by
samd_moe_gate_up_silu_f4 / samd_moe_down_combine_f4.  Router, attention, dense MLP layers, embedding and lm_head stay in the model dtype.
transformers has no quantised form of its fused Qwen3-MoE expert module, so the pre-quantised convention is this project's own: a sparse
layer's `mlp.experts.gate_up_proj` [E, 2 I, H/2] and `mlp.experts.down_proj` [E, H, I/2] as uint8 or float4_e2m1fn_x2 (low nibble = the even
element), with `mlp.experts.gate_up_proj_scale` [E, 2 I, H/32] and `mlp.experts.down_proj_scale` [E, H, I/32] as uint8 or float8_e8m0fnu,
parameters or buffers; in a raw weights dict: experts_gu, experts_gu_scale, experts_down, experts_down_scale.

expert_format "int4g128" keeps the EXPERTS as AWQ / GPTQ INT4 (samd_hip/int4.py: 4-bit codes, one zero point and one scale in the model dtype
per 128 along k, W = rne_dtype((q - z) * s)): (q [E, N, K/2], z [E, N, K/128], s [E, N, K/128]) per fused tensor, packed by samd_gemm_pack_i4
as one matrix of E * N rows (the buffer is dtype-specific) and streamed by samd_moe_gate_up_silu_i4 / samd_moe_down_combine_i4.  A 4-bit
Qwen3-MoE checkpoint holds an indexable `mlp.experts` of E modules with AWQ / GPTQ gate_proj / up_proj / down_proj (`mlp.experts.{e}.
gate_proj.qweight` ...), which LlamaRunner.from_hf imports through int4.linear_int4; in a raw weights dict: experts_gu uint8 [E, 2 I, H/2],
experts_gu_z uint8 [E, 2 I, H/128], experts_gu_s model dtype [E, 2 I, H/128], and experts_down / _z / _s likewise with [E, H, I/...] -- the
_z / _s keys are what tells INT4 from MXFP4 (_scale).  EXPERT_FORMATS stays the pair of the first two formats (callers pin it);
EXPERT_FORMATS_ALL is the first three (pinned likewise); EXPERT_FORMATS_KNOWN is what an expert_format is validated against.

expert_format "fp8b128" keeps the EXPERTS as block-scaled FP8 (samd_hip/fp8.py: OCP e4m3fn codes, one fp32 scale per 128 x 128 block,
W = float(q) * s, never formed: one fp32 FMA per accumulator and 128-k block): (q [E, N, K] float8_e4m3fn, s [E, N/128, K/128] fp32) per fused
tensor -- exactly transformers' FP8Experts (`mlp.experts.gate_up_proj` + `gate_up_proj_scale_inv`, `down_proj` + `down_proj_scale_inv`), the
form the official Qwen3-MoE FP8 checkpoints load into; per-expert modules (`mlp.experts.{e}.gate_proj.weight` + `weight_scale_inv`, the
on-disk naming) are taken as well.  In a raw weights dict: experts_gu (float8_e4m3fn or its bytes), experts_gu_sinv, experts_down,
experts_down_sinv -- the _sinv keys are what tells this format from the others.  Packed by pack_experts_fp8 (codes: samd_gemm_pack_f8 over
E * N rows; then the fp32 scale table [E * N / 64][K / 128]) and streamed by samd_moe_gate_up_silu_f8 / samd_moe_down_combine_f8.  The
buffer does not depend on the model dtype.

expert_format "int8g128" keeps the EXPERTS as GPTQ INT8 (samd_hip/int8.py: 8-bit codes, one per byte, one 8-bit zero point and one scale in
the model dtype per 128 along k, W = rne_dtype((q - z) * s)): (q [E, N, K], z [E, N, K/128], s [E, N, K/128]) per fused tensor, packed by
samd_gemm_pack_i8 as one matrix of E * N rows (E * N * K * 33 / 32 bytes; the buffer is dtype-specific) and streamed by
samd_moe_gate_up_silu_i8 / samd_moe_down_combine_i8.  An 8-bit GPTQ Qwen3-MoE checkpoint holds an indexable `mlp.experts` of E modules with
8-bit GPTQ gate_proj / up_proj / down_proj, which LlamaRunner.from_hf imports through int8.linear_int8; in a raw weights dict: experts_gu
uint8 [E, 2 I, H], experts_gu_z8 uint8 [E, 2 I, H/128], experts_gu_s8 model dtype [E, 2 I, H/128], and experts_down / _z8 / _s8 likewise
with [E, H, I...] -- the _z8 / _s8 keys (the dense INT8 projections' suffixes) are what tells INT8 from INT4 (_z / _s), MXFP4 (_scale) and
FP8 (_sinv).  The pinned tuples above stay as they are; EXPERT_FORMATS_SERVED is EXPERT_FORMATS_KNOWN plus "int8g128" and is what an
expert_format is validated against (WIDE_FORMAT_CODES_SERVED likewise for the wide calls' codes).

MoeBuffers serves one row bucket of at most 64 rows (decode, verify, the chunked prefill).  MoeWideBuffers serves 1 .. 4096 rows in one
route, one lists, one gate|up and one down + combine (include/samd_hip.h: samd_moe_wide_*): an expert's list may be longer than a 64-row
tile and is served in several through a tile table, every row with the bits MoeBuffers gives it, over the same packed expert buffers in
every format.  LlamaRunner._prefill_moe runs a prompt of 128 tokens or more through it, SAMD_MOE_PREFILL_ROWS (prefill_rows) rows at a
time; wide_lists_reference restates the lists and the tile table in plain Python."""
import os

import torch

from typing import Callable, NamedTuple, Optional

from . import SamdError, _ptr, check, current_stream, lib, torch_dtype_code
from . import fp8 as F8
from . import int4 as I4
from . import int8 as I8
from . import mxfp4 as MX
from .formats import QUANT_FORMATS, is_f4_tensor

MAX_EXPERTS = 256
MAX_TOPK = 8
# the parameters of a sparse layer's MLP that the runner reads (named_parameters of an HF Qwen3MoeDecoderLayer)
SPARSE_MLP_PARAMS = ("mlp.gate.weight", "mlp.experts.gate_up_proj", "mlp.experts.down_proj")
DENSE_MLP_PARAMS = ("mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")
# the block scales of pre-quantised (4-bit) expert tensors: consumed only beside 4-bit expert tensors
EXPERT_SCALE_PARAMS = ("mlp.experts.gate_up_proj_scale", "mlp.experts.down_proj_scale")
# what the experts of the sparse layers may be held in: None = the model dtype
EXPERT_FORMATS = (None, "mxfp4")
EXPERT_FORMATS_ALL = EXPERT_FORMATS + ("int4g128",)
EXPERT_FORMATS_KNOWN = EXPERT_FORMATS_ALL + ("fp8b128",)
# the three tuples above are pinned by their callers; this one is what an expert_format is validated against
EXPERT_FORMATS_SERVED = EXPERT_FORMATS_KNOWN + ("int8g128",)
# the scale tensors of transformers' FP8Experts: consumed only beside float8_e4m3fn expert tensors
FP8_EXPERT_SCALE_PARAMS = ("mlp.experts.gate_up_proj_scale_inv", "mlp.experts.down_proj_scale_inv")
# the projections of one expert module of an INT4 (AWQ / GPTQ) checkpoint: mlp.experts.{e}.gate_proj / up_proj / down_proj
INT4_EXPERT_PROJECTIONS = ("gate_proj", "up_proj", "down_proj")


class _Auto:
    """the default of `expert_format`: the environment's SAMD_EXPERT_FORMAT, else what the weights carry.  A sentinel, so that an explicit
    expert_format=None (experts in the model dtype, an error against 4-bit expert tensors) can be told from no argument"""

    def __repr__(self):
        return "AUTO"


AUTO = _Auto()


def sparse_layer_map(n_layers, n_experts, mlp_only_layers, decoder_sparse_step):
    """which decoder layers hold a sparse MLP block, as Qwen3MoeDecoderLayer.__init__ decides it"""
    only = set(int(i) for i in (mlp_only_layers or ()))
    step = int(decoder_sparse_step or 1)
    return [i not in only and n_experts > 0 and (i + 1) % step == 0 for i in range(n_layers)]


def check_shape(hidden, moe_inter, n_experts, top_k):
    """the shapes the expert kernels serve; anything else raises at load"""
    if hidden % 256 != 0 or moe_inter < 256 or moe_inter % 256 != 0:
        raise SamdError(f"mixture-of-experts layers need hidden_size % 256 == 0 and moe_intermediate_size % 256 == 0 (got {hidden}, {moe_inter})")
    if not 1 <= n_experts <= MAX_EXPERTS:
        raise SamdError(f"mixture-of-experts layers serve 1..{MAX_EXPERTS} experts (num_experts = {n_experts})")
    if not 1 <= top_k <= min(MAX_TOPK, n_experts):
        raise SamdError(f"mixture-of-experts layers serve 1..{MAX_TOPK} experts per token, at most num_experts (num_experts_per_tok = {top_k})")


def reject_unsupported(weight_format=None, native_gemm=True, draft_head=False):
    """what a runner with sparse layers does not offer; raises before any device work"""
    if weight_format in QUANT_FORMATS:
        raise SamdError(f"mixture-of-experts models are not available with weight_format '{weight_format}': quantised experts are not supported")
    if not native_gemm:
        raise SamdError("mixture-of-experts layers exist only in the streaming kernels' packed form: native_gemm=False is not available")
    if draft_head:
        raise SamdError("mixture-of-experts layers are not supported on an EAGLE draft head")


def _format_error(expert_format):
    hint = " ('fp8' is weight_format's spelling of per-row FP8; block-scaled FP8 experts are 'fp8b128')" if expert_format == "fp8" else ""
    return SamdError(f"expert_format {expert_format!r}: expected one of {', '.join(repr(f) for f in EXPERT_FORMATS_SERVED)}{hint}")


def resolve_expert_format(expert_format, carries_4bit, has_sparse, carries_int4=False, carries_fp8=False, carries_int8=False):
    """None, "mxfp4", "int4g128", "fp8b128" or "int8g128" from the argument (AUTO: env SAMD_EXPERT_FORMAT, for callers that cannot pass one)
    and from what the weights carry: MXFP4 expert tensors (carries_4bit) make the runner "mxfp4" by themselves, INT4 ones (carries_int4)
    "int4g128", block-scaled FP8 ones (carries_fp8) "fp8b128", 8-bit GPTQ ones (carries_int8) "int8g128"; any other explicit format against
    them raises.  Raises before any device work."""
    explicit = expert_format is not AUTO
    if not explicit:
        expert_format = os.environ.get("SAMD_EXPERT_FORMAT") or None
    if expert_format not in EXPERT_FORMATS_SERVED:
        raise _format_error(expert_format)
    if expert_format is not None and not has_sparse:
        raise SamdError(f"expert_format '{expert_format}' on a model without mixture-of-experts (sparse) layers: it covers the experts only; "
                        "weight_format covers the dense projections")
    if carries_int8:
        if carries_4bit or carries_int4 or carries_fp8:
            raise SamdError("a mix of INT8 and other quantised expert tensors: the runner takes the experts of all sparse layers in one format")
        if explicit and expert_format != "int8g128":
            raise SamdError(f"the sparse layers carry INT8 (GPTQ) expert tensors; expert_format={expert_format!r} would need them "
                            "dequantised or re-quantised (leave it out or pass 'int8g128')")
        return "int8g128"
    if explicit and expert_format == "int8g128" and (carries_4bit or carries_int4 or carries_fp8):
        raise SamdError("the sparse layers carry quantised expert tensors of another format; expert_format='int8g128' would need them "
                        "re-quantised (leave it out)")
    if carries_4bit and carries_int4:
        raise SamdError("a mix of MXFP4 and INT4 expert tensors: the runner takes the experts of all sparse layers in one format")
    if carries_fp8 and (carries_4bit or carries_int4):
        raise SamdError("a mix of block-scaled FP8 and 4-bit expert tensors: the runner takes the experts of all sparse layers in one format")
    if carries_fp8:
        if explicit and expert_format != "fp8b128":
            raise SamdError(f"the sparse layers carry block-scaled FP8 expert tensors; expert_format={expert_format!r} would need them "
                            "dequantised or re-quantised (leave it out or pass 'fp8b128')")
        return "fp8b128"
    if explicit and expert_format == "fp8b128" and (carries_int4 or carries_4bit):
        raise SamdError("the sparse layers carry 4-bit expert tensors; expert_format='fp8b128' would need them re-quantised (leave it out)")
    if carries_int4:
        if explicit and expert_format != "int4g128":
            raise SamdError(f"the sparse layers carry INT4 (AWQ / GPTQ) expert tensors; expert_format={expert_format!r} would need them "
                            "dequantised (leave it out or pass 'int4g128')")
        return "int4g128"
    if carries_4bit:
        if explicit and expert_format == "int4g128":
            raise SamdError("the sparse layers carry 4-bit (MXFP4) expert tensors; expert_format='int4g128' would need them re-quantised "
                            "(leave it out or pass 'mxfp4')")
        if explicit and expert_format is None:
            raise SamdError("the sparse layers carry 4-bit (MXFP4) expert tensors; expert_format=None would need them dequantised "
                            "(leave it out or pass 'mxfp4')")
        return "mxfp4"
    return expert_format


is_4bit = is_f4_tensor


def gate_up_tile_order(moe_inter, device=None):
    """source row of every packed gate|up row: packed row 128 t + r is gate row 64 t + r for r < 64 and up row I + 64 t + r - 64 otherwise,
    so that a 128-column tile holds 64 gate columns and the 64 up columns they meet (k_moe_pack's interleave)"""
    p = torch.arange(2 * moe_inter, device=device)
    t, r = p // 128, p % 128
    return torch.where(r < 64, 64 * t + r, moe_inter + 64 * t + r - 64)


def check_quantised_experts(q_gu, e8_gu, q_down, e8_down, dtype, name="experts"):
    """the shapes, dtypes and block-scale codes of 4-bit expert tensors; raises SamdError by tensor name.  Plain torch, any device."""
    for what, q, e8 in ((f"{name}.gate_up_proj", q_gu, e8_gu), (f"{name}.down_proj", q_down, e8_down)):
        if e8 is None:
            raise SamdError(f"{what}: 4-bit expert tensor without its block scales ({what}_scale)")
        if not is_4bit(q) or q.dim() != 3:
            raise SamdError(f"{what}: expected uint8 / float4_e2m1fn_x2 [E, N, K/2], got {q.dtype} {tuple(q.shape)}")
        if not (e8.dtype == torch.uint8 or (MX._E8 is not None and e8.dtype == MX._E8)):
            raise SamdError(f"{what}_scale of dtype {e8.dtype}; MXFP4 block scales are e8m0 (float8_e8m0fnu or uint8)")
        E, N, Kh = q.shape
        if (2 * Kh) % MX.BLOCK != 0 or tuple(e8.shape) != (E, N, 2 * Kh // MX.BLOCK):
            raise SamdError(f"{what}_scale of shape {tuple(e8.shape)} for [{E}, {N}, {2 * Kh}] experts; MXFP4 has one scale per 32 elements "
                            f"along K: [{E}, {N}, {2 * Kh // MX.BLOCK}]")
        MX.check_exponents(e8, dtype, f"{what}_scale")
    E, N2, Hh = q_gu.shape
    if tuple(q_down.shape) != (E, 2 * Hh, N2 // 4):
        raise SamdError(f"{name}: 4-bit expert tensors of shapes {tuple(q_gu.shape)} and {tuple(q_down.shape)} do not belong together "
                        f"(gate_up_proj [E, 2 I, H/2], down_proj [E, H, I/2])")


def quantize_experts(gate_up, down, dtype, name="experts"):
    """(q_gu [E, 2 I, H/2], e8_gu [E, 2 I, H/32], q_down [E, H, I/2], e8_down [E, H, I/32]), all uint8, of HF's fused expert tensors
    [E, 2 I, H] / [E, H, I]: mxfp4.quantize_blocks on every row (round to nearest, no calibration: for benches and tests), the exponents
    clamped to and checked against the range in which fp4 * 2^e is exact in `dtype`."""
    E, N2, H = gate_up.shape
    if tuple(down.shape) != (E, H, N2 // 2):
        raise SamdError(f"{name}: expert tensors of shapes {tuple(gate_up.shape)} and {tuple(down.shape)} do not belong together")
    out = []
    for what, t in (("gate_up_proj", gate_up), ("down_proj", down)):
        _, N, K = t.shape
        q = torch.empty((E, N, K // 2), dtype=torch.uint8, device=t.device)
        e8 = torch.empty((E, N, K // MX.BLOCK), dtype=torch.uint8, device=t.device)
        for e in range(E):                                       # (expert by expert: the fp32 temporaries stay small)
            q[e], e8[e] = MX.quantize_blocks(t[e], dtype)
        MX.check_exponents(e8, dtype, f"{name}.{what}")
        out += [q, e8]
    return tuple(out)


def dequantize_experts(q, e8, dtype=None):
    """fp4(q) * 2^(e8 - 127), [E, N, K] in fp32 (or `dtype`, exact over mxfp4.EXPONENT_RANGE): the weights the 4-bit expert kernels multiply by"""
    qb, eb = MX._bytes(q), MX._bytes(e8)
    E, N, Kh = qb.shape
    w = MX.dequantize_blocks(qb.reshape(E * N, Kh), eb.reshape(E * N, -1)).reshape(E, N, 2 * Kh)
    return w if dtype is None else w.to(dtype)


def pack_experts_mxfp4(q_gu, e8_gu, q_down, e8_down):
    """(packed gate|up, packed down): uint8 buffers of E * N * K / 2 + E * N * K / 32 bytes each in samd_gemm_pack_f4's layout, the experts
    end to end as one matrix of E * N rows (tile e * N / 128 + t is expert e's tile t).  The gate|up rows are permuted first
    (gate_up_tile_order; MX blocks run along k, so whole blocks move).  Tensors already on the GPU."""
    E, N2, Hh = q_gu.shape
    I, H = N2 // 2, 2 * Hh
    if tuple(q_down.shape) != (E, H, I // 2) or tuple(e8_gu.shape) != (E, N2, H // MX.BLOCK) or tuple(e8_down.shape) != (E, H, I // MX.BLOCK):
        raise SamdError(f"4-bit expert tensors of shapes {tuple(q_gu.shape)}, {tuple(e8_gu.shape)}, {tuple(q_down.shape)}, {tuple(e8_down.shape)} "
                        "do not belong together")
    order = gate_up_tile_order(I, q_gu.device)
    out = []
    for q, e8, N, K in ((MX._bytes(q_gu)[:, order], MX._bytes(e8_gu)[:, order], N2, H), (MX._bytes(q_down), MX._bytes(e8_down), H, I)):
        q, e8 = q.contiguous(), e8.contiguous()
        buf = torch.empty(E * MX.packed_bytes(N, K), dtype=torch.uint8, device=q.device)
        check(lib().samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(buf), E * N, K, current_stream()))
        out.append(buf)
    return tuple(out)


def quantize_experts_int4(gate_up, down, dtype, name="experts"):
    """((q, z, s) of gate|up, (q, z, s) of down) of HF's fused expert tensors [E, 2 I, H] / [E, H, I]: int4.quantize_groups on every expert
    (asymmetric min / max per group of 128 along K, round to nearest, no calibration: for benches and tests).  q uint8 [E, N, K/2], z uint8
    [E, N, K/128], s `dtype` [E, N, K/128]."""
    E, N2, H = gate_up.shape
    if tuple(down.shape) != (E, H, N2 // 2):
        raise SamdError(f"{name}: expert tensors of shapes {tuple(gate_up.shape)} and {tuple(down.shape)} do not belong together")
    out = []
    for t in (gate_up, down):
        _, N, K = t.shape
        if K % I4.GROUP != 0:
            raise SamdError(f"{name}: INT4 needs K % 128 == 0, got [{E}, {N}, {K}] experts")
        q = torch.empty((E, N, K // 2), dtype=torch.uint8, device=t.device)
        z = torch.empty((E, N, K // I4.GROUP), dtype=torch.uint8, device=t.device)
        s = torch.empty((E, N, K // I4.GROUP), dtype=dtype, device=t.device)
        for e in range(E):                                       # (expert by expert: the fp32 temporaries stay small)
            q[e], z[e], s[e] = I4.quantize_groups(t[e], dtype)
        out.append((q, z, s))
    return tuple(out)


def dequantize_experts_int4(q, z, s, dtype=None):
    """rne_{s.dtype}((q - z) * s), [E, N, K] in fp32 (or `dtype`): the weights the INT4 expert kernels of a runner in s.dtype multiply by"""
    E, N, Kh = q.shape
    w = I4.dequantize_groups(q.reshape(E * N, Kh), z.reshape(E * N, -1), s.reshape(E * N, -1)).reshape(E, N, 2 * Kh)
    return w if dtype is None else w.to(dtype)


def check_int4_experts(gu, down, dtype, name="experts"):
    """the shapes, dtypes, zero points and scales of INT4 expert tensors (gu, down: (q, z, s) each) for a runner in `dtype`; raises SamdError
    by tensor name.  Plain torch, any device."""
    for what, (q, z, s) in ((f"{name}.gate_up_proj", gu), (f"{name}.down_proj", down)):
        if z is None or s is None:
            raise SamdError(f"{what}: INT4 expert tensor without its zero points and scales")
        if q.dtype != torch.uint8 or z.dtype != torch.uint8 or q.dim() != 3:
            raise SamdError(f"{what}: INT4 codes and zero points are uint8 tensors (q [E, N, K/2], z [E, N, K/128]), got {q.dtype} "
                            f"{tuple(q.shape)} and {z.dtype} {tuple(z.shape)}")
        E, N, Kh = q.shape
        if N % 128 != 0 or (2 * Kh) % 256 != 0:
            raise SamdError(f"{what} of shape ({E}, {N}, {2 * Kh}): the INT4 expert kernels need N % 128 == 0 and K % 256 == 0")
        want = (E, N, 2 * Kh // I4.GROUP)
        if tuple(z.shape) != want or tuple(s.shape) != want:
            raise SamdError(f"{what}: zero points {tuple(z.shape)} / scales {tuple(s.shape)} for [{E}, {N}, {2 * Kh}] experts; one per 128 "
                            f"along K is {want}")
        if s.dtype != dtype:
            raise SamdError(f"{what}: scales of dtype {s.dtype} for a {dtype} runner (int4.as_scales rounds a checkpoint's fp16 scales once)")
        if bool((z > 15).any()):
            raise SamdError(f"{what}: a zero point above 15")
        I4.check_scales(s, dtype, what)
    E, N2, Hh = gu[0].shape
    if tuple(down[0].shape) != (E, 2 * Hh, N2 // 4):
        raise SamdError(f"{name}: INT4 expert tensors of shapes {tuple(gu[0].shape)} and {tuple(down[0].shape)} do not belong together "
                        f"(gate_up_proj [E, 2 I, H/2], down_proj [E, H, I/2])")


def pack_experts_int4(gu, down, dtype):
    """(packed gate|up, packed down) of (q, z, s) triples: uint8 buffers of E * int4.packed_bytes(N, K) bytes each in samd_gemm_pack_i4's
    layout, the experts end to end as one matrix of E * N rows (tile e * N / 128 + t is expert e's tile t).  The gate|up rows are permuted
    first (gate_up_tile_order; groups run along k, so whole rows move with their zero points and scales).  The buffers are specific to
    `dtype` (scales and pre-biased zero points are stored in it).  Tensors already on the GPU.  The two returned tensors carry the mark
    MoeBuffers.experts(..., expert_format="int4g128") asks for; pass them on as they are."""
    check_int4_experts(gu, down, dtype)
    E, N2, Hh = gu[0].shape
    I, H = N2 // 2, 2 * Hh
    order = gate_up_tile_order(I, gu[0].device)
    dt_code = torch_dtype_code(dtype)
    out = []
    for (q, z, s), N, K in ((tuple(t[:, order] for t in gu), N2, H), (down, H, I)):
        q, z, s = q.contiguous(), z.contiguous(), s.contiguous()
        buf = torch.empty(E * I4.packed_bytes(N, K), dtype=torch.uint8, device=q.device)
        check(lib().samd_gemm_pack_i4(_ptr(q), _ptr(z), _ptr(s), _ptr(buf), E * N, K, dt_code, current_stream()))
        # as many bytes as the MXFP4 form: MoeBuffers.experts takes only tensors that carry this mark as INT4 ones.  A copy, a view or a
        # slice does not carry it and is refused -- the guard fails closed; hand over the tensors this function returned
        buf.expert_format = "int4g128"
        out.append(buf)
    return tuple(out)


def import_experts_int4(experts, name, dtype, device, config=None):
    """the raw-weights-dict entries (experts_gu / _z / _s, experts_down / _z / _s) of an indexable of E expert modules whose gate_proj /
    up_proj / down_proj are AWQ / GPTQ modules: each imported by int4.linear_int4 (`config`: the model's quantization_config; its rejections
    reach the caller by module name), gate|up fused per expert, the experts stacked on `device`, the scales rounded once to `dtype`."""
    gu, dn = [], []
    for e in range(len(experts)):
        g, u, d = (I4.linear_int4(getattr(experts[e], p), f"{name}.{e}.{p}", config=config) for p in INT4_EXPERT_PROJECTIONS)
        gu.append(I4.fuse_int4([g, u], device, dtype))
        dn.append(I4.fuse_int4([d], device, dtype))
    out = {}
    for key, parts in (("experts_gu", gu), ("experts_down", dn)):
        for sfx, j in (("", 0), ("_z", 1), ("_s", 2)):
            out[key + sfx] = torch.stack([p[j] for p in parts]).contiguous()
    return out


def quantize_experts_int8(gate_up, down, dtype, name="experts"):
    """((q, z, s) of gate|up, (q, z, s) of down) of HF's fused expert tensors [E, 2 I, H] / [E, H, I]: int8.quantize_groups on every expert
    (asymmetric min / max per group of 128 along K, round to nearest, no calibration: for benches and tests).  q uint8 [E, N, K], z uint8
    [E, N, K/128], s `dtype` [E, N, K/128]."""
    E, N2, H = gate_up.shape
    if tuple(down.shape) != (E, H, N2 // 2):
        raise SamdError(f"{name}: expert tensors of shapes {tuple(gate_up.shape)} and {tuple(down.shape)} do not belong together")
    out = []
    for t in (gate_up, down):
        _, N, K = t.shape
        if K % I8.GROUP != 0:
            raise SamdError(f"{name}: INT8 needs K % 128 == 0, got [{E}, {N}, {K}] experts")
        q = torch.empty((E, N, K), dtype=torch.uint8, device=t.device)
        z = torch.empty((E, N, K // I8.GROUP), dtype=torch.uint8, device=t.device)
        s = torch.empty((E, N, K // I8.GROUP), dtype=dtype, device=t.device)
        for e in range(E):                                       # (expert by expert: the fp32 temporaries stay small)
            q[e], z[e], s[e] = I8.quantize_groups(t[e], dtype)
        out.append((q, z, s))
    return tuple(out)


def dequantize_experts_int8(q, z, s, dtype=None):
    """rne_{s.dtype}((q - z) * s), [E, N, K] in fp32 (or `dtype`): the weights the INT8 expert kernels of a runner in s.dtype multiply by"""
    E, N, K = q.shape
    w = I8.dequantize_groups(q.reshape(E * N, K), z.reshape(E * N, -1), s.reshape(E * N, -1)).reshape(E, N, K)
    return w if dtype is None else w.to(dtype)


def check_int8_experts(gu, down, dtype, name="experts"):
    """the shapes, dtypes and scales of INT8 expert tensors (gu, down: (q, z, s) each) for a runner in `dtype`; raises SamdError by tensor
    name.  Plain torch, any device."""
    for what, (q, z, s) in ((f"{name}.gate_up_proj", gu), (f"{name}.down_proj", down)):
        if z is None or s is None:
            raise SamdError(f"{what}: INT8 expert tensor without its zero points and scales")
        if q.dtype != torch.uint8 or z.dtype != torch.uint8 or q.dim() != 3:
            raise SamdError(f"{what}: INT8 codes and zero points are uint8 tensors (q [E, N, K], z [E, N, K/128]), got {q.dtype} "
                            f"{tuple(q.shape)} and {z.dtype} {tuple(z.shape)}")
        E, N, K = q.shape
        if N % 128 != 0 or K % 256 != 0:
            raise SamdError(f"{what} of shape ({E}, {N}, {K}): the INT8 expert kernels need N % 128 == 0 and K % 256 == 0")
        want = (E, N, K // I8.GROUP)
        if tuple(z.shape) != want or tuple(s.shape) != want:
            raise SamdError(f"{what}: zero points {tuple(z.shape)} / scales {tuple(s.shape)} for [{E}, {N}, {K}] experts; one per 128 "
                            f"along K is {want}")
        if s.dtype != dtype:
            raise SamdError(f"{what}: scales of dtype {s.dtype} for a {dtype} runner (int8.as_scales rounds a checkpoint's fp16 scales once)")
        I8.check_scales(s, dtype, what)
    E, N2, H = gu[0].shape
    if tuple(down[0].shape) != (E, H, N2 // 2):
        raise SamdError(f"{name}: INT8 expert tensors of shapes {tuple(gu[0].shape)} and {tuple(down[0].shape)} do not belong together "
                        f"(gate_up_proj [E, 2 I, H], down_proj [E, H, I])")


def pack_experts_int8(gu, down, dtype):
    """(packed gate|up, packed down) of (q, z, s) triples: uint8 buffers of E * int8.packed_bytes(N, K) = E * N * K * 33 / 32 bytes each in
    samd_gemm_pack_i8's layout, the experts end to end as one matrix of E * N rows (tile e * N / 128 + t is expert e's tile t).  The gate|up
    rows are permuted first (gate_up_tile_order; groups run along k, so whole rows move with their zero points and scales).  The buffers
    are specific to `dtype` (scales and pre-biased zero points are stored in it).  Tensors already on the GPU.  The two returned tensors
    carry the mark MoeBuffers.experts(..., expert_format="int8g128") asks for; pass them on as they are."""
    check_int8_experts(gu, down, dtype)
    E, N2, H = gu[0].shape
    I = N2 // 2
    order = gate_up_tile_order(I, gu[0].device)
    dt_code = torch_dtype_code(dtype)
    out = []
    for (q, z, s), N, K in ((tuple(t[:, order] for t in gu), N2, H), (down, H, I)):
        q, z, s = q.contiguous(), z.contiguous(), s.contiguous()
        buf = torch.empty(E * I8.packed_bytes(N, K), dtype=torch.uint8, device=q.device)
        check(lib().samd_gemm_pack_i8(_ptr(q), _ptr(z), _ptr(s), _ptr(buf), E * N, K, dt_code, current_stream()))
        # the byte count does not name the dtype the buffer was packed for, nor tells a packed buffer from raw bytes of that length: the
        # launches take only tensors that carry this mark.  A copy, a view or a slice does not carry it and is refused -- the guard fails
        # closed; hand over the tensors this function returned
        buf.expert_format = "int8g128"
        out.append(buf)
    return tuple(out)


def import_experts_int8(experts, name, dtype, device, config=None):
    """the raw-weights-dict entries (experts_gu / _z8 / _s8, experts_down / _z8 / _s8) of an indexable of E expert modules whose gate_proj /
    up_proj / down_proj are 8-bit GPTQ modules: each imported by int8.linear_int8 (`config`: the model's quantization_config; its rejections
    reach the caller by module name), gate|up fused per expert, the experts stacked on `device`, the scales rounded once to `dtype`."""
    gu, dn = [], []
    for e in range(len(experts)):
        parts = []
        for p in INT4_EXPERT_PROJECTIONS:
            r = I8.linear_int8(getattr(experts[e], p, None), f"{name}.{e}.{p}", config=config)
            if r is None:
                raise SamdError(f"{name}.{e}.{p}: not an 8-bit GPTQ module beside 8-bit experts: the experts of a layer come in one format")
            parts.append(r)
        g, u, d = parts
        gu.append(I8.fuse_int8([g, u], device, dtype))
        dn.append(I8.fuse_int8([d], device, dtype))
    out = {}
    for key, parts in (("experts_gu", gu), ("experts_down", dn)):
        for sfx, j in (("", 0), ("_z8", 1), ("_s8", 2)):
            out[key + sfx] = torch.stack([p[j] for p in parts]).contiguous()
    return out


def _f8_view(t):
    return t.view(torch.float8_e4m3fn) if t.dtype == torch.uint8 else t


def quantize_experts_fp8(gate_up, down, name="experts"):
    """((q, s) of gate|up, (q, s) of down) of HF's fused expert tensors [E, 2 I, H] / [E, H, I]: fp8.quantize_blocks on every expert
    (symmetric absmax / 448 per 128 x 128 block, round to nearest even, no calibration: for benches and tests).  q float8_e4m3fn [E, N, K],
    s fp32 [E, N/128, K/128]."""
    E, N2, H = gate_up.shape
    if tuple(down.shape) != (E, H, N2 // 2):
        raise SamdError(f"{name}: expert tensors of shapes {tuple(gate_up.shape)} and {tuple(down.shape)} do not belong together")
    out = []
    for t in (gate_up, down):
        _, N, K = t.shape
        if N % F8.BLOCK != 0 or K % F8.BLOCK != 0:
            raise SamdError(f"{name}: block-scaled FP8 needs N % 128 == 0 and K % 128 == 0, got [{E}, {N}, {K}] experts")
        q = torch.empty((E, N, K), dtype=torch.float8_e4m3fn, device=t.device)
        s = torch.empty((E, N // F8.BLOCK, K // F8.BLOCK), dtype=torch.float32, device=t.device)
        for e in range(E):                                       # (expert by expert: the fp32 temporaries stay small)
            q[e], s[e] = F8.quantize_blocks(t[e])
        out.append((q, s))
    return tuple(out)


def dequantize_experts_fp8(q, s, dtype=None):
    """fl32(float(q) * s), [E, N, K] in fp32 (or rounded once to `dtype`): the weights the FP8 expert kernels multiply by"""
    w = F8.dequantize_blocks(_f8_view(q), s)
    return w if dtype is None else w.to(dtype)


def check_fp8_experts(gu, down, name="experts"):
    """the shapes, dtypes and scales of block-scaled FP8 expert tensors (gu, down: (q, s) each; q float8_e4m3fn or its bytes); raises
    SamdError by tensor name.  Plain torch, any device."""
    for what, (q, s) in ((f"{name}.gate_up_proj", gu), (f"{name}.down_proj", down)):
        if s is None:
            raise SamdError(f"{what}: FP8 expert tensor without its block scales ({what}_scale_inv)")
        if q.dim() != 3:
            raise SamdError(f"{what}: expected float8_e4m3fn [E, N, K], got {q.dtype} {tuple(q.shape)}")
        F8.check_block_scales(_f8_view(q), s, what)
        E, N, K = q.shape
        if N % 128 != 0 or K % 256 != 0:
            raise SamdError(f"{what} of shape ({E}, {N}, {K}): the FP8 expert kernels need N % 128 == 0 and K % 256 == 0")
    E, N2, H = gu[0].shape
    if tuple(down[0].shape) != (E, H, N2 // 2):
        raise SamdError(f"{name}: FP8 expert tensors of shapes {tuple(gu[0].shape)} and {tuple(down[0].shape)} do not belong together "
                        f"(gate_up_proj [E, 2 I, H], down_proj [E, H, I])")


def fp8_scale_table(s, order=None):
    """the packed buffer's scale table [E * N / 64, K / 128] fp32 of block scales s [E, N / 128, K / 128]: one row per 64 PACKED rows.
    Packed row block j of an expert starts at source row order[64 j] (gate|up: gate_up_tile_order, so block 2 t is gate row 64 t -- scale
    row-block t / 2 -- and block 2 t + 1 is up row I + 64 t -- row-block (I + 64 t) / 128; down: the identity, both halves of a tile
    repeat one scale row).  64 divides 128 and the gate / up halves start at multiples of 64, so a 64-row packed block never straddles
    two scale blocks."""
    E, NB, KB = s.shape
    first = torch.arange(0, NB * F8.BLOCK, 64, device=s.device)
    src = first if order is None else order[first]
    return s.float()[:, src // F8.BLOCK, :].reshape(E * NB * 2, KB).contiguous()


def pack_experts_fp8(gu, down):
    """(packed gate|up, packed down) of (q, s) pairs: uint8 buffers of E * fp8.packed_block_bytes(N, K) bytes each -- the codes in
    samd_gemm_pack_f8's layout, the experts end to end as one matrix of E * N rows (tile e * N / 128 + t is expert e's tile t), the gate|up
    rows permuted first (gate_up_tile_order); then, at fp8.block_scale_offset(E * N, K), the fp32 table of fp8_scale_table.  Tensors
    already on the GPU; the buffers serve both model dtypes."""
    check_fp8_experts(gu, down)
    E, N2, H = gu[0].shape
    I = N2 // 2
    order = gate_up_tile_order(I, gu[0].device)
    out = []
    for (q, s), N, K, perm in ((gu, N2, H, order), (down, H, I, None)):
        qb = q.view(torch.uint8) if q.dtype != torch.uint8 else q
        qb = (qb if perm is None else qb[:, perm]).contiguous()
        off = F8.block_scale_offset(E * N, K)
        buf = torch.empty(E * F8.packed_block_bytes(N, K), dtype=torch.uint8, device=q.device)
        assert off == E * N * K and buf.numel() == off + E * (N // 64) * (K // F8.BLOCK) * 4
        check(lib().samd_gemm_pack_f8(_ptr(qb), _ptr(buf), E * N, K, current_stream()))
        buf[off:].view(torch.float32).copy_(fp8_scale_table(s, perm).reshape(-1))
        out.append(buf)
    return tuple(out)


def is_fp8_experts_module(experts):
    """the fused form: a module with float8 gate_up_proj / down_proj tensors (transformers' FP8Experts)"""
    gu, dn = getattr(experts, "gate_up_proj", None), getattr(experts, "down_proj", None)
    return gu is not None and dn is not None and (F8.is_fp8_dtype(gu.dtype) or F8.is_fp8_dtype(dn.dtype))


def import_experts_fp8(experts, name, device, config=None):
    """the raw-weights-dict entries (experts_gu / experts_gu_sinv / experts_down / experts_down_sinv) of a sparse layer's block-scaled FP8
    experts, on `device`: either the fused form (transformers' FP8Experts: gate_up_proj [E, 2 I, H] + gate_up_proj_scale_inv [E, 2 I/128,
    H/128], down_proj [E, H, I] + down_proj_scale_inv) or an indexable of E modules whose gate_proj / up_proj / down_proj carry `weight` +
    `weight_scale_inv` (the on-disk naming), each imported by fp8.linear_fp8_block, gate|up fused per expert and the experts stacked.
    `config`: the model's quantization_config.  Rejections reach the caller by tensor name."""
    mv = lambda t: t.detach().view(torch.uint8).to(device).view(torch.float8_e4m3fn).contiguous()
    if hasattr(experts, "gate_up_proj"):
        F8.check_block_config(config, name)
        bs = getattr(experts, "block_size", None)
        if bs is not None and tuple(int(x) for x in bs) != (F8.BLOCK, F8.BLOCK):
            raise SamdError(f"{name}: block_size {list(bs)} is not supported; block-scaled FP8 takes [128, 128]")
        if getattr(experts, "activation_scheme", None) == "static":
            raise SamdError(f"{name}: activation_scheme 'static' is not supported; the runner is weight-only and takes 'dynamic' checkpoints")
        out = {}
        for key, pn in (("experts_gu", "gate_up_proj"), ("experts_down", "down_proj")):
            q, s = getattr(experts, pn), getattr(experts, pn + "_scale_inv", None)
            F8.check_block_scales(q.detach(), None if s is None else s.detach(), f"{name}.{pn}")
            out[key], out[key + "_sinv"] = mv(q), s.detach().to(device).contiguous()
        return out
    gu, dn = [], []
    for e in range(len(experts)):
        parts = []
        for p in INT4_EXPERT_PROJECTIONS:
            r = F8.linear_fp8_block(getattr(experts[e], p), f"{name}.{e}.{p}", config)
            if r is None:
                raise SamdError(f"{name}.{e}.{p}: not an FP8 weight beside FP8 experts: the experts of a layer come in one format")
            parts.append(r)
        g, u, d = parts
        gu.append((torch.cat([mv(g[0]).view(torch.uint8), mv(u[0]).view(torch.uint8)], dim=0), torch.cat([g[1].to(device), u[1].to(device)], dim=0)))
        dn.append((mv(d[0]).view(torch.uint8), d[1].to(device)))
    out = {}
    for key, parts in (("experts_gu", gu), ("experts_down", dn)):
        out[key] = torch.stack([p[0] for p in parts]).view(torch.float8_e4m3fn).contiguous()
        out[key + "_sinv"] = torch.stack([p[1] for p in parts]).contiguous()
    return out


def pack_experts(gate_up, down):
    """(packed gate|up, packed down) of HF's fused expert tensors [E, 2 I, H] / [E, H, I], already on the GPU in the model dtype"""
    E, N2, H = gate_up.shape
    if tuple(down.shape) != (E, H, N2 // 2):
        raise SamdError(f"expert tensors of shapes {tuple(gate_up.shape)} and {tuple(down.shape)} do not belong together")
    gate_up, down = gate_up.contiguous(), down.contiguous()
    pgu, pd = torch.empty_like(gate_up), torch.empty_like(down)
    check(lib().samd_moe_pack_experts(_ptr(gate_up), _ptr(pgu), E, N2, H, 1, current_stream()))
    check(lib().samd_moe_pack_experts(_ptr(down), _ptr(pd), E, H, N2 // 2, 0, current_stream()))
    return pgu, pd


class MoeBuffers:
    """device buffers of the three launches for one row bucket: topk_idx / topk_w [RP, k], act [RP * k, I], the workspace (routing lists +
    down products) and out [RP, hidden]"""

    def __init__(self, rows_pad, hidden, moe_inter, n_experts, top_k, dtype, dt_code, device):
        self.rows_pad, self.hidden, self.moe_inter, self.n_experts, self.top_k, self.dt = rows_pad, hidden, moe_inter, n_experts, top_k, dt_code
        self.topk_idx = torch.full((rows_pad, top_k), -1, dtype=torch.int32, device=device)
        self.topk_w = torch.zeros((rows_pad, top_k), dtype=dtype, device=device)
        self.act = torch.zeros((rows_pad * top_k, moe_inter), dtype=dtype, device=device)
        self.ws = torch.zeros(lib().samd_moe_workspace(rows_pad, hidden, n_experts, top_k, dt_code), dtype=torch.uint8, device=device)
        self.out = torch.zeros((rows_pad, hidden), dtype=dtype, device=device)

    def route(self, h, router, d_n, norm_topk):
        check(lib().samd_moe_route(_ptr(h), _ptr(router), _ptr(d_n), self.rows_pad, self.hidden, self.n_experts, self.top_k, int(bool(norm_topk)),
                                   _ptr(self.topk_idx), _ptr(self.topk_w), _ptr(self.ws), self.dt, current_stream()))

    def lists(self, d_n):
        """the routing lists from self.topk_idx as it stands (routing decided elsewhere)"""
        check(lib().samd_moe_lists(_ptr(self.topk_idx), _ptr(d_n), self.rows_pad, self.n_experts, self.top_k, _ptr(self.ws), current_stream()))

    def experts(self, h, wgu_packed, wdown_packed, d_n, expert_format=None):
        """the two expert launches over the buffers that expert_format's packer returned (EXPERT: pack; the INT4 and INT8 ones are packed
        for this runner's dtype)"""
        if expert_format not in EXPERT_FORMATS_SERVED:
            raise _format_error(expert_format)
        _check_expert_buffers(self, wgu_packed, wdown_packed, expert_format)      # (the guards come before any device work)
        L, st, sfx = lib(), current_stream(), EXPERT[expert_format].launch_suffix
        check(getattr(L, "samd_moe_gate_up_silu" + sfx)(_ptr(h), _ptr(wgu_packed), _ptr(self.ws), self.rows_pad, self.hidden, self.moe_inter,
                                                        self.n_experts, self.top_k, _ptr(self.act), self.dt, st))
        check(getattr(L, "samd_moe_down_combine" + sfx)(_ptr(self.act), _ptr(wdown_packed), _ptr(self.topk_idx), _ptr(self.topk_w), _ptr(d_n),
                                                        _ptr(self.ws), self.rows_pad, self.hidden, self.moe_inter, self.n_experts, self.top_k,
                                                        _ptr(self.out), self.dt, st))
        return self.out

    def routing_state(self):
        """(n_active, active experts, counts, lists) read back from the workspace: for tests and profiling"""
        active, count, lst, stride, words = (lib().samd_moe_workspace_layout(f) for f in range(5))
        w = self.ws[:4 * words].view(torch.int32).cpu()
        n = int(w[0])
        return (n, w[active:active + n].tolist(), w[count:count + n].tolist(),
                [w[lst + stride * a:lst + stride * a + int(w[count + a])].tolist() for a in range(n)])


# ---- the wide form: a sparse layer's MLP over all rows of a prompt (or of a super-chunk of it) in one route, one lists, one gate|up and one
# down + combine (include/samd_hip.h: samd_moe_wide_*).  Every row gets the bits MoeBuffers gives it.
WIDE_MAX_ROWS = 4096
WIDE_TILE = 64
PREFILL_ROWS_ENV = "SAMD_MOE_PREFILL_ROWS"
# the C ABI's expert_format codes
WIDE_FORMAT_CODES = {None: 0, "mxfp4": 1, "int4g128": 2, "fp8b128": 3}
# (pinned, as EXPERT_FORMATS_KNOWN is; the calls take the codes of this one.  "int8g128" is 5: callers also pin 4 as a code the library
# refuses as unknown, so 4 stays unassigned)
WIDE_FORMAT_CODES_SERVED = dict(WIDE_FORMAT_CODES, int8g128=5)


def prefill_rows(value=None):
    """rows of a super-chunk of the one-pass prefill: `value`, else env SAMD_MOE_PREFILL_ROWS, else 4096.  A multiple of 64 in
    [128, 4096]; anything else raises."""
    raw = os.environ.get(PREFILL_ROWS_ENV) if value is None else value
    if raw is None or raw == "":
        return WIDE_MAX_ROWS
    try:
        n = int(raw)
    except (TypeError, ValueError):
        raise SamdError(f"{PREFILL_ROWS_ENV}={raw!r}: expected an integer") from None
    if n % WIDE_TILE != 0 or not 2 * WIDE_TILE <= n <= WIDE_MAX_ROWS:
        raise SamdError(f"{PREFILL_ROWS_ENV}={n}: expected a multiple of {WIDE_TILE} in [{2 * WIDE_TILE}, {WIDE_MAX_ROWS}]")
    return n


def wide_rows_pad(rows):
    return (rows + WIDE_TILE - 1) // WIDE_TILE * WIDE_TILE


def wide_tile_bound(rows, n_experts, top_k):
    """tile slots of a wide expert launch: sum_e ceil(c_e / 64) <= active experts + total / 64, every active expert having at most one
    partly filled tile"""
    total = wide_rows_pad(rows) * top_k
    return min(n_experts, total) + total // WIDE_TILE


def wide_lists_reference(topk_idx, n, n_experts):
    """what samd_moe_wide_lists writes, in plain Python from topk_idx (rows x top_k nested lists or a tensor): dict(active, counts, offsets,
    entries, tiles) -- the active experts ascending, per active expert its entry count and its first entry's place, the entries
    p = row * top_k + slot expert by expert and ascending within one, the tile records (expert, first entry, entries <= 64).  Ignored:
    rows >= n, indices outside [0, n_experts), an expert (any value, in fact) that an earlier slot of the row already holds."""
    rows = topk_idx.tolist() if hasattr(topk_idx, "tolist") else [list(r) for r in topk_idx]
    per = {}
    for r, row in enumerate(rows):
        if r >= n:
            break
        for j, e in enumerate(row):
            if 0 <= e < n_experts and e not in row[:j]:
                per.setdefault(e, []).append(r * len(row) + j)
    active = sorted(per)
    counts = [len(per[e]) for e in active]
    offsets = [sum(counts[:a]) for a in range(len(active))]
    entries = [p for e in active for p in per[e]]
    tiles = [(e, off + t, min(WIDE_TILE, c - t)) for e, c, off in zip(active, counts, offsets) for t in range(0, c, WIDE_TILE)]
    return dict(active=active, counts=counts, offsets=offsets, entries=entries, tiles=tiles)


class MoeWideBuffers:
    """device buffers of the wide calls for up to `rows` rows (padded to 64): topk_idx / topk_w [RP, k], act [RP * k, I], the workspace
    (lists + tile table + down products) and out [RP, hidden].  `rows` is fixed; *d_n says how many of them count in a call."""

    def __init__(self, rows, hidden, moe_inter, n_experts, top_k, dtype, dt_code, device):
        nbytes = lib().samd_moe_wide_workspace(rows, hidden, moe_inter, n_experts, top_k, dt_code)
        check(0 if nbytes >= 0 else nbytes)
        self.rows, self.rows_pad = rows, wide_rows_pad(rows)
        self.hidden, self.moe_inter, self.n_experts, self.top_k, self.dt = hidden, moe_inter, n_experts, top_k, dt_code
        RP = self.rows_pad
        self.topk_idx = torch.full((RP, top_k), -1, dtype=torch.int32, device=device)
        self.topk_w = torch.zeros((RP, top_k), dtype=dtype, device=device)
        self.act = torch.zeros((RP * top_k, moe_inter), dtype=dtype, device=device)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.out = torch.zeros((RP, hidden), dtype=dtype, device=device)

    def _rows(self, rows):
        """a call may serve fewer rows than the buffers hold (smaller grids; every offset only shrinks)"""
        if rows is None:
            return self.rows
        if not 1 <= rows <= self.rows:
            raise SamdError(f"{rows} rows over wide expert buffers of {self.rows}")
        return rows

    def route(self, h, router, d_n, norm_topk, rows=None):
        """topk_idx / topk_w of h [RP, hidden]; the lists are a call of their own"""
        check(lib().samd_moe_wide_route(_ptr(h), _ptr(router), _ptr(d_n), self._rows(rows), self.hidden, self.n_experts, self.top_k, int(bool(norm_topk)),
                                        _ptr(self.topk_idx), _ptr(self.topk_w), self.dt, current_stream()))

    def lists(self, d_n, rows=None):
        check(lib().samd_moe_wide_lists(_ptr(self.topk_idx), _ptr(d_n), self._rows(rows), self.n_experts, self.top_k, _ptr(self.ws), current_stream()))

    def experts(self, h, wgu_packed, wdown_packed, d_n, expert_format=None, rows=None):
        """the two expert launches over the buffers MoeBuffers.experts takes for `expert_format`; returns out [RP, hidden]"""
        if expert_format not in EXPERT_FORMATS_SERVED:
            raise _format_error(expert_format)
        _check_expert_buffers(self, wgu_packed, wdown_packed, expert_format)
        L, st, code, rows = lib(), current_stream(), EXPERT[expert_format].wide_code, self._rows(rows)
        check(L.samd_moe_wide_gate_up_silu(_ptr(h), _ptr(wgu_packed), _ptr(self.ws), rows, self.hidden, self.moe_inter, self.n_experts, self.top_k,
                                           code, _ptr(self.act), self.dt, st))
        check(L.samd_moe_wide_down_combine(_ptr(self.act), _ptr(wdown_packed), _ptr(self.topk_idx), _ptr(self.topk_w), _ptr(d_n), _ptr(self.ws), rows,
                                           self.hidden, self.moe_inter, self.n_experts, self.top_k, code, _ptr(self.out), self.dt, st))
        return self.out

    def routing_state(self):
        """the workspace's routing part read back in wide_lists_reference's form, plus n_tiles / n_active: for tests and profiling"""
        lay = [lib().samd_moe_wide_workspace_layout(f, self.rows, self.top_k) for f in range(8)]
        active, count, offset, tile, tile_ints, entry, words = lay[:7]
        w = self.ws[:4 * words].view(torch.int32).cpu()
        n_tiles, n_active = int(w[0]), int(w[1])
        counts = w[count:count + n_active].tolist()
        return dict(n_tiles=n_tiles, n_active=n_active, active=w[active:active + n_active].tolist(), counts=counts,
                    offsets=w[offset:offset + n_active].tolist(), entries=w[entry:entry + sum(counts)].tolist(),
                    tiles=[tuple(w[tile + tile_ints * t:tile + tile_ints * (t + 1)].tolist()) for t in range(n_tiles)])

    def routing_bytes(self):
        """the routing part of the workspace as it stands (a copy)"""
        return self.ws[:4 * lib().samd_moe_wide_workspace_layout(6, self.rows, self.top_k)].clone()


def _check_expert_buffers(b, wgu_packed, wdown_packed, expert_format):
    """the byte counts and marks the expert launches (MoeBuffers.experts and the wide calls) ask of packed expert buffers"""
    fmt = EXPERT[expert_format]
    for other in EXPERT.values():                                # a buffer whose packer's mark says it may pass as nothing else
        if other.mark_exclusive and other is not fmt and other.name in (getattr(wgu_packed, "expert_format", None), getattr(wdown_packed, "expert_format", None)):
            raise SamdError(f"an {other.label} expert buffer ({other.packer}) under expert_format {expert_format!r}: pass expert_format='{other.name}'")
    if fmt.packed_bytes is None:
        if wgu_packed.dtype == torch.uint8 or wdown_packed.dtype == torch.uint8:
            raise SamdError("uint8 expert buffers are MXFP4 ones: pass expert_format='mxfp4'")
        return
    for what, t, want in (("gate|up", wgu_packed, b.n_experts * fmt.packed_bytes(2 * b.moe_inter, b.hidden)),
                          ("down", wdown_packed, b.n_experts * fmt.packed_bytes(b.hidden, b.moe_inter))):
        if t.dtype != torch.uint8 or t.numel() != want:
            raise SamdError(f"{fmt.name} {what} expert buffer of {t.numel()} {t.dtype} elements is no {fmt.label} expert buffer of this shape: "
                            f"{fmt.packer} gives {want} bytes")
        if fmt.mark_why is not None and getattr(t, "expert_format", None) != fmt.name:
            raise SamdError(f"expert_format '{fmt.name}' over a buffer that {fmt.packer} did not return ({fmt.mark_why}; a copy or a view of "
                            f"an {fmt.label} buffer loses the packer's mark)")


# ---- the expert formats, one record each: everything LlamaRunner and the launches above need to know about a format.  A new format is one
# more record, beside its check_* / quantize_experts_* / pack_experts_* / import_experts_* functions above.
class ExpertFormat(NamedTuple):
    name: Optional[str]      # the expert_format; None: the model dtype
    doc: str                 # which module forms from_hf takes as this format (the module docstring has the numeric contract)
    label: str               # "<label> experts", "an <label> expert buffer"
    mix_label: str           # "a mix of <mix_label> sparse layers"
    raw_keys: tuple          # the suffixes of the raw weights dict's entries of gate|up ("experts_gu" + ...) and down: codes, then side data
    carried: Callable        # (sparse layer dict) -> does it carry this format's expert tensors?
    carries_kw: str          # resolve_expert_format's keyword for "the weights carry this format"
    check: Callable          # (gu, down, dtype, name): check_*_experts over the two key tuples' tensors
    quantize: Optional[Callable]    # (gate_up, down, dtype, name) -> (gu, down) tuples: quantize_experts_*; None: nothing to quantise
    pack: Callable           # (gu, down, dtype) -> (packed gate|up, packed down): pack_experts_*
    packer: str              # ... its name, for messages
    import_hf: Callable      # (HF experts module, name, dtype, device, qcfg, qcfg8) -> the raw-dict entries: import_experts_*
    packed_bytes: Optional[Callable]    # (N, K) -> bytes of one expert's packed matrix; None: the model dtype's N * K elements
    launch_suffix: str       # samd_moe_gate_up_silu<suffix> / samd_moe_down_combine<suffix>
    meta_dtype: Callable = lambda t: t.dtype      # (tensor) -> the dtype its released meta shape keeps
    codes_per_byte: int = 1  # a raw code tensor's K is the matrix's K over this
    raw_view: Callable = lambda t: t      # how a carried tensor is read (MXFP4: float4 / e8m0 dtypes as their bytes)
    mark_why: Optional[str] = None        # not None: the launches take only buffers that carry the packer's mark, and this is why
    mark_exclusive: bool = False          # a buffer with this format's mark is refused under every other expert_format
    recount_keys: tuple = ()              # raw entries weight_bytes counts a second time (their packed form is twice as wide)

    @property
    def wide_code(self):
        """the wide calls' expert_format code"""
        return WIDE_FORMAT_CODES_SERVED[self.name]

    @property
    def gu_keys(self):
        return tuple("experts_gu" + s for s in self.raw_keys)

    @property
    def down_keys(self):
        return tuple("experts_down" + s for s in self.raw_keys)

    def mix_refusal(self, carried, lacking=None):
        """the refusal of sparse layers of which only some carry this format (carried: one answer per sparse layer); lacking: the decoder
        layers that do not, where the caller knows them by index"""
        eg = "" if lacking is None else f"; e.g. layers {lacking[:3]} do not"
        return SamdError(f"a mix of {self.mix_label} sparse layers ({sum(carried)} of {len(carried)} carry {self.label} experts{eg}): "
                         "the runner takes the experts of all sparse layers in one format")

    def check_layers(self, layers, carried, dtype):
        """every sparse layer of a raw weights dict carries this format (or none does), with tensors the kernels take"""
        if not all(carried):
            raise self.mix_refusal(carried)
        for i, l in enumerate(layers):
            if "experts_gu" in l:
                self.check(*(tuple(l[k] if j == 0 else l.get(k) for j, k in enumerate(ks)) for ks in (self.gu_keys, self.down_keys)), dtype,
                           f"layer {i} experts")


def _has_any(keys):
    return lambda l: any(k in l for k in keys)


def _import_experts_plain(ex, name, dtype, dev, qcfg, qcfg8):
    """HF's fused expert tensors [E, 2 I, H] / [E, H, I] in the model dtype"""
    return {k: t.detach().to(device=dev, dtype=dtype).contiguous() for k, t in (("experts_gu", ex.gate_up_proj), ("experts_down", ex.down_proj))}


def _import_experts_mxfp4(ex, name, dtype, dev, qcfg, qcfg8):
    """the 4-bit expert tensors and their block scales, as they are"""
    raw = lambda t: MX._bytes(t.detach()).to(dev).contiguous()
    return dict(experts_gu=raw(ex.gate_up_proj), experts_gu_scale=raw(ex.gate_up_proj_scale),
                experts_down=raw(ex.down_proj), experts_down_scale=raw(ex.down_proj_scale))


def _quantize_experts_mxfp4(gate_up, down, dtype, name):
    quad = quantize_experts(gate_up, down, dtype, name)
    return quad[:2], quad[2:]


_PLAIN = ExpertFormat(
    name=None, label="model-dtype",
    doc="HF's fused expert tensors mlp.experts.gate_up_proj [E, 2 I, H] / down_proj [E, H, I], in the model dtype",
    mix_label="", raw_keys=("",), carried=lambda l: False, carries_kw="", check=None, quantize=None,
    pack=lambda gu, down, dtype: pack_experts(gu[0], down[0]), packer="pack_experts", import_hf=_import_experts_plain,
    packed_bytes=None, launch_suffix="")
_INT8 = ExpertFormat(
    name="int8g128", label="INT8",
    doc="every sparse layer holds an indexable `mlp.experts` of E modules whose gate_proj / up_proj / down_proj are ALL 8-bit GPTQ modules "
        "(the `Qwen3-30B-A3B-GPTQ-Int8` kind): each is imported through int8.linear_int8 with the config's quantization_config (so "
        "act-order, group sizes 32 / 64, AWQ or a stored 255 under 'gptq' raise by module name), gate|up fused per expert, the experts "
        "stacked, the scales rounded once for a bf16 runner", mix_label="INT8 and other", raw_keys=("", "_z8", "_s8"),
    carried=_has_any(("experts_gu_z8", "experts_gu_s8", "experts_down_z8", "experts_down_s8")), carries_kw="carries_int8",
    check=check_int8_experts, quantize=quantize_experts_int8, pack=pack_experts_int8, packer="pack_experts_int8",
    import_hf=lambda ex, name, dtype, dev, qcfg, qcfg8: import_experts_int8(ex, name, dtype, dev, qcfg),
    packed_bytes=I8.packed_bytes, launch_suffix="_i8",
    mark_why="the byte count alone does not tell a packed INT8 buffer from other bytes", mark_exclusive=True,
    recount_keys=("experts_gu_z8", "experts_down_z8"))       # the packed bytes are N K 33 / 32: a zero point is a 16-bit word there
_INT4 = ExpertFormat(
    name="int4g128", label="INT4",
    doc="every sparse layer holds an indexable `mlp.experts` of E modules whose gate_proj / up_proj / down_proj are AWQ / GPTQ modules "
        "(`mlp.experts.{e}.gate_proj.qweight` ...): each is imported through int4.linear_int4 with the config's quantization_config (so "
        "act-order, group sizes 32 / 64, GEMV or a v1 zero point of 15 raise by module name), gate|up fused per expert, the experts "
        "stacked, the scales rounded once for a bf16 runner", mix_label="INT4 and other", raw_keys=("", "_z", "_s"),
    carried=_has_any(("experts_gu_z", "experts_gu_s", "experts_down_z", "experts_down_s")), carries_kw="carries_int4",
    check=check_int4_experts, quantize=quantize_experts_int4, pack=pack_experts_int4, packer="pack_experts_int4",
    import_hf=lambda ex, name, dtype, dev, qcfg, qcfg8: import_experts_int4(ex, name, dtype, dev, qcfg),
    packed_bytes=I4.packed_bytes, launch_suffix="_i4",
    codes_per_byte=2, mark_why="an MXFP4 buffer of this shape has the same byte count and other contents")
_FP8 = ExpertFormat(
    name="fp8b128", label="FP8",
    doc="every sparse layer holds transformers' fused FP8Experts (`mlp.experts.gate_up_proj` + `gate_up_proj_scale_inv`, `down_proj` + "
        "`down_proj_scale_inv`; Qwen3-30B-A3B-FP8: weight_block_size [128, 128]) or per-expert modules (`mlp.experts.{e}.gate_proj.weight` "
        "+ `weight_scale_inv`): codes and scales are imported as they are (samd_hip/fp8.py has the rejections, by tensor name)",
    mix_label="block-scaled FP8 and other", raw_keys=("", "_sinv"),
    carried=lambda l: "experts_gu_sinv" in l or "experts_down_sinv" in l or F8.is_fp8_dtype(l["experts_gu"].dtype) or F8.is_fp8_dtype(l["experts_down"].dtype),
    carries_kw="carries_fp8", check=lambda gu, down, dtype, name: check_fp8_experts(gu, down, name),
    quantize=lambda gate_up, down, dtype, name: quantize_experts_fp8(gate_up, down, name),
    pack=lambda gu, down, dtype: pack_experts_fp8(gu, down), packer="pack_experts_fp8",      # (the buffer serves both model dtypes)
    import_hf=lambda ex, name, dtype, dev, qcfg, qcfg8: import_experts_fp8(ex, name, dev, qcfg8),
    packed_bytes=F8.packed_block_bytes, launch_suffix="_f8", meta_dtype=lambda t: torch.float8_e4m3fn if t.dtype == torch.uint8 else t.dtype)
_MXFP4 = ExpertFormat(
    name="mxfp4", label="MXFP4",
    doc="every sparse layer's fused expert tensors are 4-bit, with their block scales (this project's own convention, the module "
        "docstring): imported as they are", mix_label="4-bit and model-dtype", raw_keys=("", "_scale"),
    # 4-bit tensors that no other format's keys claim
    carried=lambda l: not any(f.carried(l) for f in (_INT8, _INT4, _FP8)) and (is_4bit(l["experts_gu"]) or is_4bit(l["experts_down"])),
    carries_kw="carries_4bit", check=lambda gu, down, dtype, name: check_quantised_experts(*gu, *down, dtype, name),
    quantize=_quantize_experts_mxfp4, pack=lambda gu, down, dtype: pack_experts_mxfp4(*gu, *down), packer="pack_experts_mxfp4",
    import_hf=_import_experts_mxfp4, packed_bytes=MX.packed_bytes, launch_suffix="_f4", meta_dtype=lambda t: torch.uint8, codes_per_byte=2,
    raw_view=MX._bytes)
EXPERT = {f.name: f for f in (_PLAIN, _MXFP4, _INT4, _FP8, _INT8)}


def experts_carried(layers):
    """{expert format: per sparse layer of a raw weights dict, does it carry that format's expert tensors?}"""
    sparse = [l for l in layers if "experts_gu" in l]
    return {f.name: [f.carried(l) for l in sparse] for f in EXPERT.values() if f.name is not None}


def resolve_carried(expert_format, carried, has_sparse):
    """resolve_expert_format over experts_carried's answer"""
    return resolve_expert_format(expert_format, has_sparse=has_sparse, **{EXPERT[n].carries_kw: any(c) for n, c in carried.items()})
