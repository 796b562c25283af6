"""INT8 weight-only decoding (GPTQ 8-bit checkpoints): the numeric contract of the runner's group-scaled 8-bit projections (DESIGN.md,
"INT8 weights (GPTQ)").  The runner's name for the format is weight_format="int8g128": 8.25 bits per weight.  int4.py's sibling, layer by layer.

Canonical form of one projection [N, K], `dtype` the runner's dtype (fp16 or bf16), group = 128 elements along K:
    q  uint8 [N, K]: one code per byte, 0..255;
    z  uint8 [N, K/128]: zero points 0..255;
    s  dtype [N, K/128]: scales, finite and > 0;
    W[n][k] = rne_dtype((q[n][k] - z[n][k/128]) * s[n][k/128]).
(q - z) is an exact integer in [-255, 255] and its product with a 16-bit float has at most 9 + 11 significant bits, so it is exact in fp32:
the weight the MFMA sees carries exactly ONE rounding, to the model dtype (fp16: with subnormals, what v_pk_mul_f16 delivers).  This is how
the public GPTQ loaders dequantise.  255 * max(s) must stay finite in the dtype (check_scales).  A checkpoint's scales are fp16: an fp16
runner takes them as they are, a bf16 runner rounds each scale ONCE to bf16 at import (as_scales) -- its weights are then the contract's W
for the rounded scales, not the fp16 ones.

The kernel's group size is 128 and only 128: the importer expands a checkpoint whose group_size is a multiple of 128 that divides K, or -1
(one group per row), by repeating z and s; group sizes 32 and 64, act-order (a g_idx other than k // g), bit widths other than 8 and AWQ
modules raise.  4-bit modules are int4.py's.

quantize_groups is the uncalibrated path (asymmetric min / max per group, round to nearest): for benches, random-init models and tests.  On
Gaussian rows it costs 0.6 % relative RMS weight error (tests/test_int8_weights_cpu.py measures it: 0.00592 in fp16, 0.00617 in bf16, whose
rounding of the weight itself shows at this step size; int4.py's 0.1006 times 15 / 255 is 0.0059).  Everything here is plain torch and runs
on any device."""
import torch

from . import SamdError
from .int4 import _cfg, quant_config, is_int4_module       # noqa: F401  (the config reader and the qweight / qzeros / scales test are shared)

GROUP = 128
PROJECTIONS = ("wqkv", "wo", "wgu", "wdown")
DTYPES = (torch.float16, torch.bfloat16)
QMAX = 255


def _check_dtype(dtype):
    if dtype not in DTYPES:
        raise SamdError(f"INT8 projections run in fp16 or bf16, not {dtype}")


def check_scales(s, dtype, name="projection"):
    """raise SamdError unless every scale is finite and > 0 and 255 * max(s) is finite in `dtype`"""
    _check_dtype(dtype)
    sf = s.float()
    if not bool(torch.isfinite(sf).all()) or bool((sf <= 0).any()):
        raise SamdError(f"{name}: INT8 group scales must be finite and > 0")
    top = 255.0 * float(sf.max()) if sf.numel() else 0.0
    if top > torch.finfo(dtype).max:
        way_out = "; bfloat16 holds the products: run the model with dtype=torch.bfloat16" if dtype == torch.float16 else ""
        raise SamdError(f"{name}: 255 * max(scale) = {top:.6g} overflows {dtype} (largest finite value {torch.finfo(dtype).max:.6g}){way_out}")


def as_scales(s, dtype, name="projection"):
    """a checkpoint's scales in the runner's dtype: fp16 as they are; for a bf16 runner each scale rounded once to bf16.  Checked."""
    _check_dtype(dtype)
    if not s.dtype.is_floating_point:
        raise SamdError(f"{name}: scales of dtype {s.dtype}")
    sf = s.float()
    if not bool(torch.isfinite(sf).all()) or bool((sf <= 0).any()):
        raise SamdError(f"{name}: INT8 group scales must be finite and > 0")
    if dtype == torch.float16 and sf.numel() and float(sf.max()) > torch.finfo(dtype).max:
        raise SamdError(f"{name}: a scale of {float(sf.max()):.6g} overflows {dtype}; bfloat16 holds it: run the model with dtype=torch.bfloat16")
    out = s.to(dtype)
    check_scales(out, dtype, name)
    return out.contiguous()


def quantize_groups(W, dtype):
    """W [N, K] (any float dtype, any device, K % 128 == 0) -> (q uint8 [N, K], z uint8 [N, K/128], s dtype [N, K/128]).  Per group of 128
    along K: lo = min(min, 0), hi = max(max, 0) (zero is always representable); s = max((hi - lo) / 255, smallest normal of dtype) rounded to
    dtype; z = clamp(round(-lo / s), 0, 255) and q = clamp(round(W / s) + z, 0, 255), both with the ROUNDED s; an all-zero group gives
    s = 1, z = 0, q = 0.  Uncalibrated (see the module docstring for the measured error)."""
    _check_dtype(dtype)
    N, K = W.shape
    if K % GROUP != 0:
        raise SamdError(f"INT8 needs K % 128 == 0, got a [{N}, {K}] matrix")
    Wb = W.float().reshape(N, K // GROUP, GROUP)
    lo = Wb.amin(dim=2).clamp_max(0.0)
    hi = Wb.amax(dim=2).clamp_min(0.0)
    s = ((hi - lo) / float(QMAX)).clamp_min(torch.finfo(dtype).tiny)
    s = torch.where(hi == lo, torch.ones_like(s), s).to(dtype)
    check_scales(s, dtype, "quantize_groups")
    sf = s.float()
    z = torch.round(-lo / sf).clamp_(0, QMAX)
    q = (torch.round(Wb / sf[:, :, None]) + z[:, :, None]).clamp_(0, QMAX).reshape(N, K).to(torch.uint8)
    return q.contiguous(), z.to(torch.uint8).contiguous(), s.contiguous()


def dequantize_groups(q, z, s):
    """rne_{s.dtype}((q - z) * s) in fp32, [N, K]: the weights an INT8 runner in s.dtype multiplies by (group = 128 along K)"""
    N, K = q.shape
    d = (q.to(torch.int32).reshape(N, K // GROUP, GROUP) - z.to(torch.int32)[:, :, None]).float()
    return (d * s.float()[:, :, None]).to(s.dtype).float().reshape(N, K)        # the fp32 product is exact; .to() is the one rounding


def check_groups(q, z, s, dtype, name="projection"):
    """shapes, dtypes and value ranges of one canonical projection for a runner in `dtype`"""
    _check_dtype(dtype)
    if q.dtype != torch.uint8 or z.dtype != torch.uint8 or q.dim() != 2:
        raise SamdError(f"{name}: INT8 codes and zero points are uint8 tensors (q [N, K], z [N, K/128])")
    N, K = q.shape
    if N % 128 != 0 or K % 256 != 0:
        raise SamdError(f"INT8 projection {name} of shape ({N}, {K}): the INT8 kernel needs N % 128 == 0 and K % 256 == 0")
    if tuple(z.shape) != (N, K // GROUP) or tuple(s.shape) != (N, K // GROUP):
        raise SamdError(f"{name}: zero points {tuple(z.shape)} / scales {tuple(s.shape)} for a ({N}, {K}) matrix; one per 128 along K is "
                        f"({N}, {K // GROUP})")
    if s.dtype != dtype:
        raise SamdError(f"{name}: scales of dtype {s.dtype} for a {dtype} runner (as_scales rounds a checkpoint's fp16 scales once)")
    check_scales(s, dtype, name)


# ---------------------------------------------------------------------------------------------------------------------
# checkpoint importer
def _bits(mod, config=None):
    """the bit width of a quantised projection module: quantization_config.bits, else the module's own `bits`, else what qweight's shape says
    against (in_features, out_features) -- [K/4, N] is 8-bit, [K/8, N] (GPTQ) or [K, N/8] (AWQ) 4-bit; None when nothing decides"""
    bits = _cfg(config, "bits", None)
    if bits is None:
        bits = getattr(mod, "bits", getattr(mod, "w_bit", None))
    if bits is not None:
        return int(bits)
    K, N = int(mod.in_features), int(mod.out_features)
    shape = tuple(mod.qweight.shape)
    if shape == (K // 4, N):
        return 8
    if shape in ((K // 8, N), (K, N // 8)):
        return 4
    return None


def is_int8_module(mod, config=None):
    """a projection module counts as INT8 when it is a quantised module (int32 qweight and qzeros, a floating scales, in_features /
    out_features: int4.is_int4_module's test, which does not look at the width) whose bit width (_bits) is 8"""
    return is_int4_module(mod) and _bits(mod, config) == 8


def _bytes(t):
    """int32 [R, C] -> uint8 [R, C, 4]: byte p = bits 8p .. 8p+7"""
    shifts = torch.arange(0, 32, 8, dtype=torch.int32, device=t.device)
    return ((t.unsqueeze(-1) >> shifts) & 255).to(torch.uint8)


def linear_int8(mod, name="projection", zero_offset=None, config=None):
    """(q uint8 [N, K], z uint8 [N, K/128], s [N, K/128] in the checkpoint's scale dtype) of a GPTQ 8-bit projection module, or None for a
    module that is not a quantised one (int4.is_int4_module).  `config` is the model's quantization_config (dict or object: quant_method
    "gptq", bits, group_size, checkpoint_format, desc_act); without one GPTQ v1 is assumed.  zero_offset: what is added to the stored zero
    point (default: 1 for checkpoint_format "gptq", 0 for "gptq_v2").
      GPTQ: qweight [K/4, N], byte p of [r][n] = q[n][4 r + p]; qzeros [K/g, N/4], byte p of [G][j] = column 4 j + p; scales [K/g, N];
            optional g_idx [K], which must be k // g.
    Raises SamdError for bits != 8, quant_method "awq", group sizes that are no multiple of 128 dividing K (32, 64), act-order, a stored
    zero point of 255 under GPTQ v1 (public loaders disagree on whether it means 256 or wraps to 0), ill-shaped tensors."""
    if not is_int4_module(mod):
        return None
    K, N = int(mod.in_features), int(mod.out_features)
    qw, qz, sc = mod.qweight.detach(), mod.qzeros.detach(), mod.scales.detach()
    bits = _bits(mod, config)
    if bits is None:
        raise SamdError(f"{name}: qweight of shape {tuple(qw.shape)} is not GPTQ 8-bit [{K // 4}, {N}] and nothing names a bit width")
    if bits != 8:
        raise SamdError(f"{name}: {bits}-bit quantisation; the INT8 importer takes 8-bit GPTQ checkpoints only"
                        + (" (4-bit AWQ / GPTQ modules are int4.linear_int4's)" if bits == 4 else ""))
    method = _cfg(config, "quant_method", None)
    method = str(getattr(method, "value", method)).lower() if method is not None else "gptq"
    if method != "gptq":
        raise SamdError(f"{name}: quant_method {method!r}; the INT8 importer takes 'gptq' only")
    if N % 4 != 0 or K % 4 != 0 or tuple(qw.shape) != (K // 4, N):
        raise SamdError(f"{name}: qweight of shape {tuple(qw.shape)}; 8-bit GPTQ stores [{K // 4}, {N}] for a ({N}, {K}) projection")
    if sc.dim() != 2 or sc.shape[1] != N or sc.shape[0] < 1 or K % sc.shape[0] != 0:
        raise SamdError(f"{name}: scales of shape {tuple(sc.shape)} for a ({N}, {K}) projection; expected [K / group_size, {N}]")
    n_groups = sc.shape[0]
    g = K // n_groups
    cfg_g = _cfg(config, "group_size", None)
    if cfg_g is not None and int(cfg_g) not in (g, -1 if g == K else g):
        raise SamdError(f"{name}: the tensors carry groups of {g}, the quantization_config says group_size {int(cfg_g)}")
    if g % GROUP != 0:
        raise SamdError(f"{name}: group_size {g} is not supported: the kernel's group is 128, and the importer expands multiples of 128 "
                        "that divide K and -1 (per channel) only")
    if tuple(qz.shape) != (n_groups, N // 4):
        raise SamdError(f"{name}: qzeros of shape {tuple(qz.shape)}; expected [{n_groups}, {N // 4}]")
    if getattr(mod, "bias", None) is not None and name.rsplit(".", 1)[-1] in ("o_proj", "gate_proj", "up_proj", "down_proj"):
        raise SamdError(f"{name}: a bias on an o / gate / up / down projection is not supported")
    g_idx = getattr(mod, "g_idx", None)
    if _cfg(config, "desc_act", False) and g_idx is None:
        raise SamdError(f"{name}: act-order (desc_act) GPTQ checkpoints are not supported")
    if torch.is_tensor(g_idx):
        gi = g_idx.detach()
        want = torch.arange(K, device=gi.device) // g
        if gi.numel() != K or not torch.equal(gi.reshape(-1).to(want.dtype), want):
            raise SamdError(f"{name}: act-order (a g_idx other than k // group_size) GPTQ checkpoints are not supported")
    fmt = str(_cfg(config, "checkpoint_format", "gptq") or "gptq").lower()
    if fmt not in ("gptq", "gptq_v2"):
        raise SamdError(f"{name}: GPTQ checkpoint_format {fmt!r}; the importer takes 'gptq' and 'gptq_v2'")
    offset = (1 if fmt == "gptq" else 0) if zero_offset is None else int(zero_offset)
    codes = _bytes(qw).permute(1, 0, 2).reshape(N, K)
    zeros = _bytes(qz).reshape(n_groups, N).t().to(torch.int32) + offset
    if bool((zeros > QMAX).any()):
        raise SamdError(f"{name}: a stored zero point of 255 with the GPTQ v1 offset of +1 ('gptq' checkpoint_format): public loaders disagree "
                        "on whether it means 256 or wraps to 0; re-save the checkpoint as 'gptq_v2'")
    rep = g // GROUP
    z = zeros.to(torch.uint8).repeat_interleave(rep, dim=1).contiguous()
    s = sc.t().repeat_interleave(rep, dim=1).contiguous()
    return codes.contiguous(), z, s


def fuse_int8(parts, device, dtype=None):
    """row-concatenate the (q, z, s) of q|k|v or gate|up on `device` (dtype: the runner's, to which the scales are rounded once: as_scales).
    Groups run along K, so fusing before or after quantising is the same."""
    q = torch.cat([p[0].to(device) for p in parts], dim=0).contiguous()
    z = torch.cat([p[1].to(device) for p in parts], dim=0).contiguous()
    s = torch.cat([p[2].to(device) for p in parts], dim=0).contiguous()
    return q, z, (as_scales(s, dtype) if dtype is not None else s)


def checkpoint_is_int8(linears, config=None):
    """True when every projection module carries 8-bit GPTQ weights, False when none does; a mix (with 4-bit or plain projections) raises
    SamdError"""
    kinds = [(name, is_int8_module(lin, config)) for name, lin in linears]
    n8 = sum(k for _, k in kinds)
    if 0 < n8 < len(kinds):
        other = [n for n, k in kinds if not k][:3]
        raise SamdError(f"a mix of INT8 and other projections ({n8} of {len(kinds)} are INT8; e.g. {', '.join(other)} are not); "
                        "the runner takes all projections in one format")
    return n8 > 0


def packed_bytes(N, K):
    """bytes of samd_gemm_pack_i8's output: the codes and, inline behind every 32 KiB of them, their 1 KiB of group data"""
    return N * K + N * K // 32
