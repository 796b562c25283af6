"""The quantised weight formats of the four dense projections (weight_format), one record each: everything LlamaRunner needs to know about
a format -- how a raw weights dict shows it, how a projection is packed, which entry points stream and unpack it, how its bytes are
reported and how a checkpoint's modules are imported.  A new format is one more record here; the runner itself
names no format.  The expert formats (expert_format) have their table beside the functions it names: moe.EXPERT.

Every format keeps embedding and lm_head in the model dtype, has no row-major copy and no fused or norm-fold forms: its projections exist
only packed and are streamed by its own samd_gemm_skinny_* at every bucket up to 64 rows; the model-dtype matrix is dropped as soon as it
is packed (only its shape stays, as a meta tensor)."""
from typing import Callable, NamedTuple, Optional

import torch

from . import SamdError, _ptr, check, current_stream, lib
from . import fp8 as F8
from . import int4 as I4
from . import int8 as I8
from . import mxfp4 as MX

PROJECTIONS = ("wqkv", "wo", "wgu", "wdown")


def is_f4_tensor(t):
    """is this tensor 4-bit codes -- packed bytes or float4_e2m1fn_x2?  (None is not.)  moe.is_4bit is the same test"""
    return t is not None and (t.dtype == torch.uint8 or MX.is_fp4_dtype(t.dtype))


def tiles(N, K):
    """does an [N, K] matrix fit the streaming kernels' tiles?"""
    return N % 128 == 0 and K % 256 == 0


def _nbytes(t):
    return t.numel() * t.element_size()


class DenseFormat(NamedTuple):
    name: str                # the weight_format
    suffix: str              # a layer's packed projection k is runner.wp["layers"][i][k + suffix]
    label: str               # "the weights carry <label> projections"
    short: str               # "<short> projections exist only in the streaming kernel's packed form"
    doc: str                 # the format's contract, in words
    carried: Callable        # (layer dict, k) -> does raw projection k arrive in this format?
    pack: Callable           # (layer dict, k, device, dtype, dtype code) -> the packed operand; releases the raw entries
    raw_keys: tuple          # the suffixes of a pre-quantised projection's raw-dict entries, in import_hf's order
    import_hf: Callable      # (modules, their names, layer index, "self_attn" | "mlp", device, dtype, qcfg, qcfg8) -> the raw_keys' tensors
    gemm: str                # samd_gemm_skinny_*
    unpack: str              # samd_gemm_unpack_*
    packer: str              # samd_gemm_pack_*
    scales_key: str          # memory_report's key for the scales / group data
    codes_per_scale: Optional[int] = None    # one buffer: this many KiB of codes, then 1 KiB of side data; None: (codes, scales) tensors
    precheck: Optional[Callable] = None      # (shape, weights): shapes the kernel cannot run, refused before any device work

    def tensors(self, op):
        """the device tensors of a packed operand: the entry points take one pointer each, in this order"""
        return op if self.codes_per_scale is None else (op,)

    def pointers(self, op):
        return tuple(_ptr(t) for t in self.tensors(op))

    def report_bytes(self, op):
        """(bytes of codes, bytes of scales / group data) of a packed operand"""
        if self.codes_per_scale is None:
            return _nbytes(op[0]), _nbytes(op[1])
        return _nbytes(op) * self.codes_per_scale // (self.codes_per_scale + 1), _nbytes(op) // (self.codes_per_scale + 1)

    def streamed_bytes(self, op):
        """what a decode step streams of a packed operand: all of it"""
        return sum(_nbytes(t) for t in self.tensors(op))

    def carried_by(self, weights):
        return any(self.carried(l, k) for l in weights["layers"] for k in PROJECTIONS)


def _need_tiles(N, K, what, kernel):
    if not tiles(N, K):
        raise SamdError(f"{what}: the {kernel} kernel needs N % 128 == 0 and K % 256 == 0")


def pack_f8(l, k, device, dtype, dt):
    """(packed e4m3fn bytes, fp32 column scales) of projection k: quantised on load (symmetric per row) unless the checkpoint brought its
    own (q, scale)"""
    t = l[k]
    N, K = t.shape
    _need_tiles(N, K, f"FP8 projection {k} of shape {tuple(t.shape)}", "FP8")
    if t.dtype == torch.float8_e4m3fn:
        q, scale = t.to(device).contiguous(), l.pop(k + "_scale").to(device=device, dtype=torch.float32).contiguous()
    else:
        q, scale = F8.quantize_rows(t)
    l[k] = torch.empty(t.shape, dtype=torch.float8_e4m3fn, device="meta")
    del t
    out = torch.empty_like(q)
    check(lib().samd_gemm_pack_f8(_ptr(q), _ptr(out), N, K, current_stream()))
    return out, scale


def pack_f8b(l, k, device, dtype, dt):
    """(packed e4m3fn bytes, fp32 [N/128][K/128] block scales) of projection k: quantised on load (symmetric per 128 x 128 block,
    uncalibrated) unless the checkpoint brought its own (q, s), which are taken as they are -- the codes packed by samd_gemm_pack_f8, the
    table untouched"""
    t = l[k]
    N, K = t.shape
    if t.dtype == torch.float8_e4m3fn:
        q, sinv = t.to(device).contiguous(), l.pop(k + "_sinv").to(device=device).contiguous()
        F8.check_block_scales(q, sinv, f"block-scaled FP8 projection {k}")
    else:
        q, sinv = F8.quantize_blocks(t)
    l[k] = torch.empty(t.shape, dtype=torch.float8_e4m3fn, device="meta")
    del t
    out = torch.empty_like(q)
    check(lib().samd_gemm_pack_f8(_ptr(q), _ptr(out), N, K, current_stream()))
    return out, sinv


def precheck_f8b(shape, weights):
    if shape.inter % 128 != 0:
        raise SamdError(f"block-scaled FP8 projection wgu: intermediate_size {shape.inter} is not a multiple of 128, so a 128 x 128 block "
                        "would straddle gate and up")
    for li, l in enumerate(weights["layers"]):
        for k in PROJECTIONS:
            N, K = l[k].shape
            if not tiles(N, K):
                raise SamdError(f"block-scaled FP8 projection {k} of layer {li}, shape ({N}, {K}): the kernel needs N % 128 == 0 and K % 256 == 0")


def pack_f4(l, k, device, dtype, dt):
    """projection k in samd_gemm_pack_f4's form (e2m1 elements with their e8m0 block scales inline): quantised on load per block of 32
    unless the checkpoint brought its own (q, e8), whose exponents must lie in the model dtype's exact range"""
    t = l[k]
    N, K = (t.shape[0], 2 * t.shape[1]) if is_f4_tensor(t) else t.shape
    _need_tiles(N, K, f"MXFP4 projection {k} of shape ({N}, {K})", "MXFP4")
    if is_f4_tensor(t):
        q, e8 = MX.fuse_mxfp4([(t, l.pop(k + "_e8"))], device)
        if tuple(e8.shape) != (N, K // 32):
            raise SamdError(f"MXFP4 projection {k}: block scales of shape {tuple(e8.shape)} for a ({N}, {K}) matrix")
        MX.check_exponents(e8, dtype, f"MXFP4 projection {k}")
    else:
        q, e8 = MX.quantize_blocks(t, dtype)
    l[k] = torch.empty((N, K), dtype=torch.uint8, device="meta")
    del t
    out = torch.empty(MX.packed_bytes(N, K), dtype=torch.uint8, device=device)
    check(lib().samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(out), N, K, current_stream()))
    return out


def _pack_groups(Q, fuse, raw_z, raw_s, short, codes_per_byte, packer):
    """pack_i4 / pack_i8: projection k in samd_gemm_pack_i4 / _i8's form (codes with their group scales and zero points inline):
    quantised on load per group of 128 (uncalibrated) unless the checkpoint brought its own (q, z, s), whose scales are taken in the
    model dtype (a bf16 runner rounds fp16 scales once) and checked"""
    def pack(l, k, device, dtype, dt):
        t = l[k]
        if k + raw_z in l:
            q, z, sc = fuse([(t, l.pop(k + raw_z), l.pop(k + raw_s))], device, dtype)
        else:
            _need_tiles(t.shape[0], t.shape[1], f"{short} projection {k} of shape {tuple(t.shape)}", short)
            q, z, sc = Q.quantize_groups(t, dtype)
        Q.check_groups(q, z, sc, dtype, k)
        N, K = q.shape[0], codes_per_byte * q.shape[1]
        l[k] = torch.empty((N, K), dtype=torch.uint8, device="meta")
        del t
        out = torch.empty(Q.packed_bytes(N, K), dtype=torch.uint8, device=device)
        check(getattr(lib(), packer)(_ptr(q), _ptr(z), _ptr(sc), _ptr(out), N, K, dt, current_stream()))
        return out
    return pack


pack_i4 = _pack_groups(I4, I4.fuse_int4, "_z", "_s", "INT4", 2, "samd_gemm_pack_i4")
pack_i8 = _pack_groups(I8, I8.fuse_int8, "_z8", "_s8", "INT8", 1, "samd_gemm_pack_i8")


def _import_f8b(mods, names, li, part, dev, dtype, qcfg, qcfg8):
    full = [f"layers.{li}.{part}.{x}" for x in names]
    return F8.fuse_fp8_blocks([F8.linear_fp8_block(m, n, qcfg8) for m, n in zip(mods, full)], dev, full)


DENSE_FORMATS = (
    DenseFormat(
        name="fp8", suffix="_f8", label="float8_e4m3fn", short="FP8",
        doc="OCP e4m3fn with one fp32 scale per output column (samd_hip/fp8.py).  float8_e4m3fn projections (an FP8 checkpoint, beside "
            "k + '_scale') make the runner FP8 by themselves.  from_hf: a module whose projections hold float8_e4m3fn weights with a "
            "`weight_scale` (per tensor, [N] or [N, 1]) is imported as it is (fp8.linear_fp8).",
        carried=lambda l, k: k in l and l[k].dtype == torch.float8_e4m3fn and k + "_sinv" not in l,
        pack=pack_f8, raw_keys=("", "_scale"),
        import_hf=lambda mods, names, li, part, dev, dtype, qcfg, qcfg8: F8.fuse_fp8([F8.linear_fp8(x) for x in mods], dev),
        gemm="samd_gemm_skinny_f8", unpack="samd_gemm_unpack_f8", packer="samd_gemm_pack_f8", scales_key="fp8_scales"),
    DenseFormat(
        name="fp8b128", suffix="_f8b", label="block-scaled FP8", short="FP8",
        doc="OCP e4m3fn with one fp32 scale per 128 x 128 block (the weight / weight_scale_inv of transformers' fine-grained FP8 "
            "checkpoints; samd_hip/fp8.py has the contract), streamed from (samd_gemm_pack_f8's packed codes, the checkpoint's own scale "
            "table).  float8_e4m3fn projections beside k + '_sinv' make the runner fp8b128: the _sinv keys tell them from per-row fp8.  "
            "from_hf: a module WITHOUT sparse layers whose seven projections per layer are all `weight` float8_e4m3fn + `weight_scale_inv` "
            "fp32 with weight_block_size [128, 128] (the dense Qwen3-*-FP8 checkpoints) is imported through fp8.linear_fp8_block.",
        carried=lambda l, k: k + "_sinv" in l,
        pack=pack_f8b, raw_keys=("", "_sinv"), import_hf=_import_f8b,
        gemm="samd_gemm_skinny_f8b", unpack="samd_gemm_unpack_f8b", packer="samd_gemm_pack_f8", scales_key="fp8_block_scales",
        precheck=precheck_f8b),
    DenseFormat(
        name="mxfp4", suffix="_f4", label="MXFP4", short="MXFP4",
        doc="e2m1 elements with one e8m0 scale per 32 along K (samd_hip/mxfp4.py).  Packed e2m1 bytes (uint8 / float4_e2m1fn_x2 [N, K/2] "
            "beside k + '_e8') make the runner MXFP4 by themselves.  from_hf: a module whose projections hold float4_e2m1fn_x2 or uint8 "
            "weights [N, K/2] with an e8m0 `weight_scale` [N, K/32] is imported as it is (mxfp4.linear_mxfp4).",
        carried=lambda l, k: k in l and is_f4_tensor(l[k]) and k + "_z" not in l and k + "_z8" not in l,
        pack=pack_f4, raw_keys=("", "_e8"),
        import_hf=lambda mods, names, li, part, dev, dtype, qcfg, qcfg8: MX.fuse_mxfp4([MX.linear_mxfp4(x) for x in mods], dev),
        gemm="samd_gemm_skinny_f4", unpack="samd_gemm_unpack_f4", packer="samd_gemm_pack_f4", scales_key="mxfp4_scales", codes_per_scale=16),
    DenseFormat(
        name="int4g128", suffix="_i4", label="INT4 (AWQ / GPTQ)", short="INT4",
        doc="AWQ / GPTQ 4-bit codes with one scale (model dtype) and one zero point per 128 along K (samd_hip/int4.py).  uint8 [N, K/2] "
            "beside k + '_z' and k + '_s' make the runner INT4 by themselves.  The plain word 'int4' stays an unknown format: the name "
            "carries the group size.  from_hf: a module whose projections are AWQ ('GEMM') or GPTQ modules -- int32 `qweight` / `qzeros` "
            "and a floating `scales` -- is imported by the layout its config.quantization_config names (int4.linear_int4: group sizes, "
            "zero-point conventions and what raises); a bf16 runner rounds the checkpoint's fp16 scales once to bf16.",
        carried=lambda l, k: k + "_z" in l,
        pack=pack_i4, raw_keys=("", "_z", "_s"),
        import_hf=lambda mods, names, li, part, dev, dtype, qcfg, qcfg8: I4.fuse_int4(
            [I4.linear_int4(m, f"layers.{li}.{x}", config=qcfg) for m, x in zip(mods, names)], dev, dtype),
        gemm="samd_gemm_skinny_i4", unpack="samd_gemm_unpack_i4", packer="samd_gemm_pack_i4", scales_key="int4_group_data", codes_per_scale=16),
    DenseFormat(
        name="int8g128", suffix="_i8", label="INT8 (GPTQ)", short="INT8",
        doc="GPTQ 8-bit codes with one scale (model dtype) and one zero point per 128 along K (samd_hip/int8.py).  uint8 [N, K] beside "
            "k + '_z8' and k + '_s8' make the runner INT8 by themselves.  from_hf: a module whose seven projections per layer are all 8-bit "
            "GPTQ modules (the `...-GPTQ-Int8` releases: bits 8 by config.quantization_config, by the module's own `bits`, or by qweight's "
            "shape [K/4, N]) is imported through int8.linear_int8 (group sizes, zero-point conventions and what raises); a mix of 8-bit "
            "and 4-bit or plain projections raises, and so does a module with sparse layers that carries 8-bit modules anywhere but as "
            "moe.EXPERT's int8g128 describes.",
        carried=lambda l, k: k + "_z8" in l,
        pack=pack_i8, raw_keys=("", "_z8", "_s8"),
        import_hf=lambda mods, names, li, part, dev, dtype, qcfg, qcfg8: I8.fuse_int8(
            [I8.linear_int8(m, f"layers.{li}.{x}", config=qcfg) for m, x in zip(mods, names)], dev, dtype),
        gemm="samd_gemm_skinny_i8", unpack="samd_gemm_unpack_i8", packer="samd_gemm_pack_i8", scales_key="int8_group_data", codes_per_scale=32),
)
DENSE = {f.name: f for f in DENSE_FORMATS}
QUANT_FORMATS = tuple(DENSE)
