"""INT4 weight-only decoding (AWQ / GPTQ checkpoints): the numeric contract of the runner's group-scaled 4-bit projections (DESIGN.md,
"INT4 weights (AWQ / GPTQ)").  The runner's name for the format is weight_format="int4g128".

Canonical form of one projection [N, K], `dtype` the runner's dtype (fp16 or bf16), group = 128 elements along K:
    q  uint8 [N, K/2]: low nibble = element 2i, high nibble = element 2i+1 (as mxfp4.py); codes 0..15;
    z  uint8 [N, K/128]: zero points 0..15;
    s  dtype [N, K/128]: scales, finite and > 0;
    W[n][k] = rne_dtype((q[n][k] - z[n][k/128]) * s[n][k/128]).
(q - z) is an exact integer in [-15, 15] and its product with a 16-bit float is exact in fp32, so the weight the MFMA sees carries exactly
ONE rounding, to the model dtype (fp16: with subnormals, what v_pk_mul_f16 delivers).  15 * max(s) must stay finite in the dtype
(check_scales).  A checkpoint's scales are fp16: an fp16 runner takes them as they are, a bf16 runner rounds each scale ONCE to bf16 at import
(as_scales) -- its weights are then the contract's W for the rounded scales, not the fp16 ones.

The kernel's group size is 128 and only 128: the importers expand a checkpoint whose group_size is a multiple of 128 that divides K, or -1
(one group per row), by repeating z and s; group sizes 32 and 64, act-order (a g_idx other than k // g), bit widths other than 4 and
AWQ's "GEMV" layout raise.

quantize_groups is the uncalibrated path (asymmetric min / max per group, round to nearest): for benches, random-init models and tests.  On
Gaussian rows it costs 10.1 % relative RMS weight error (tests/test_int4_weights_cpu.py measures it: 0.1006 in fp16 and in bf16);
quality-sensitive users import a checkpoint that was calibrated elsewhere.  Everything here is plain torch and runs on any device."""
import torch

from . import SamdError

GROUP = 128
PROJECTIONS = ("wqkv", "wo", "wgu", "wdown")
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)           # nibble p of an AWQ "GEMM" int32 is column 8 j + AWQ_ORDER[p]
DTYPES = (torch.float16, torch.bfloat16)


def _check_dtype(dtype):
    if dtype not in DTYPES:
        raise SamdError(f"INT4 projections run in fp16 or bf16, not {dtype}")


def check_scales(s, dtype, name="projection"):
    """raise SamdError unless every scale is finite and > 0 and 15 * max(s) is finite in `dtype`"""
    _check_dtype(dtype)
    sf = s.float()
    if not bool(torch.isfinite(sf).all()) or bool((sf <= 0).any()):
        raise SamdError(f"{name}: INT4 group scales must be finite and > 0")
    top = 15.0 * float(sf.max()) if sf.numel() else 0.0
    if top > torch.finfo(dtype).max:
        way_out = "; bfloat16 holds the products: run the model with dtype=torch.bfloat16" if dtype == torch.float16 else ""
        raise SamdError(f"{name}: 15 * max(scale) = {top:.6g} overflows {dtype} (largest finite value {torch.finfo(dtype).max:.6g}){way_out}")


def as_scales(s, dtype, name="projection"):
    """a checkpoint's scales in the runner's dtype: fp16 as they are; for a bf16 runner each scale rounded once to bf16.  Checked."""
    _check_dtype(dtype)
    if not s.dtype.is_floating_point:
        raise SamdError(f"{name}: scales of dtype {s.dtype}")
    sf = s.float()
    if not bool(torch.isfinite(sf).all()) or bool((sf <= 0).any()):
        raise SamdError(f"{name}: INT4 group scales must be finite and > 0")
    if dtype == torch.float16 and sf.numel() and float(sf.max()) > torch.finfo(dtype).max:
        raise SamdError(f"{name}: a scale of {float(sf.max()):.6g} overflows {dtype}; bfloat16 holds it: run the model with dtype=torch.bfloat16")
    out = s.to(dtype)
    check_scales(out, dtype, name)
    return out.contiguous()


def pack_nibbles(codes):
    """codes uint8 [N, K] (0..15) -> q uint8 [N, K/2], low nibble = even k"""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack_nibbles(q):
    """q uint8 [N, K/2] -> codes uint8 [N, K]"""
    return torch.stack([q & 15, q >> 4], dim=2).reshape(q.shape[0], 2 * q.shape[1])


def quantize_groups(W, dtype):
    """W [N, K] (any float dtype, any device, K % 128 == 0) -> (q uint8 [N, K/2], z uint8 [N, K/128], s dtype [N, K/128]).  Per group of 128
    along K: lo = min(min, 0), hi = max(max, 0) (zero is always representable); s = max((hi - lo) / 15, smallest normal of dtype) rounded to
    dtype; z = clamp(round(-lo / s), 0, 15) and q = clamp(round(W / s) + z, 0, 15), both with the ROUNDED s; an all-zero group gives
    s = 1, z = 0, q = 0.  Uncalibrated (see the module docstring for the measured error)."""
    _check_dtype(dtype)
    N, K = W.shape
    if K % GROUP != 0:
        raise SamdError(f"INT4 needs K % 128 == 0, got a [{N}, {K}] matrix")
    Wb = W.float().reshape(N, K // GROUP, GROUP)
    lo = Wb.amin(dim=2).clamp_max(0.0)
    hi = Wb.amax(dim=2).clamp_min(0.0)
    s = ((hi - lo) / 15.0).clamp_min(torch.finfo(dtype).tiny)
    s = torch.where(hi == lo, torch.ones_like(s), s).to(dtype)
    check_scales(s, dtype, "quantize_groups")
    sf = s.float()
    z = torch.round(-lo / sf).clamp_(0, 15)
    codes = (torch.round(Wb / sf[:, :, None]) + z[:, :, None]).clamp_(0, 15).reshape(N, K).to(torch.uint8)
    return pack_nibbles(codes), z.to(torch.uint8).contiguous(), s.contiguous()


def dequantize_groups(q, z, s):
    """rne_{s.dtype}((q - z) * s) in fp32, [N, K]: the weights an INT4 runner in s.dtype multiplies by (group = 128 along K)"""
    N, K = q.shape[0], 2 * q.shape[1]
    d = (unpack_nibbles(q).to(torch.int32).reshape(N, K // GROUP, GROUP) - z.to(torch.int32)[:, :, None]).float()
    return (d * s.float()[:, :, None]).to(s.dtype).float().reshape(N, K)        # the fp32 product is exact; .to() is the one rounding


def check_groups(q, z, s, dtype, name="projection"):
    """shapes, dtypes and value ranges of one canonical projection for a runner in `dtype`"""
    _check_dtype(dtype)
    if q.dtype != torch.uint8 or z.dtype != torch.uint8 or q.dim() != 2:
        raise SamdError(f"{name}: INT4 codes and zero points are uint8 tensors (q [N, K/2], z [N, K/128])")
    N, K = q.shape[0], 2 * q.shape[1]
    if N % 128 != 0 or K % 256 != 0:
        raise SamdError(f"INT4 projection {name} of shape ({N}, {K}): the INT4 kernel needs N % 128 == 0 and K % 256 == 0")
    if tuple(z.shape) != (N, K // GROUP) or tuple(s.shape) != (N, K // GROUP):
        raise SamdError(f"{name}: zero points {tuple(z.shape)} / scales {tuple(s.shape)} for a ({N}, {K}) matrix; one per 128 along K is "
                        f"({N}, {K // GROUP})")
    if s.dtype != dtype:
        raise SamdError(f"{name}: scales of dtype {s.dtype} for a {dtype} runner (as_scales rounds a checkpoint's fp16 scales once)")
    if bool((z > 15).any()):
        raise SamdError(f"{name}: a zero point above 15")
    check_scales(s, dtype, name)


# ---------------------------------------------------------------------------------------------------------------------
# checkpoint importers
def _cfg(cfg, key, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def quant_config(lm_config):
    """the `quantization_config` (dict or object) of a model config, or None"""
    return _cfg(lm_config, "quantization_config", None)


def is_int4_module(mod):
    """a projection module counts as INT4 when it carries int32 qweight and qzeros, a floating scales, and in_features / out_features"""
    qw, qz, sc = getattr(mod, "qweight", None), getattr(mod, "qzeros", None), getattr(mod, "scales", None)
    return (torch.is_tensor(qw) and torch.is_tensor(qz) and torch.is_tensor(sc) and qw.dtype == torch.int32 and qz.dtype == torch.int32
            and sc.dtype.is_floating_point and hasattr(mod, "in_features") and hasattr(mod, "out_features"))


def _nibbles(t):
    """int32 [R, C] -> uint8 [R, C, 8]: nibble p = bits 4p .. 4p+3"""
    shifts = torch.arange(0, 32, 4, dtype=torch.int32, device=t.device)
    return ((t.unsqueeze(-1) >> shifts) & 15).to(torch.uint8)


def _unpack_awq_cols(t):
    """AWQ int32 [R, N/8] -> uint8 [R, N]: nibble p of [r][j] is column 8 j + AWQ_ORDER[p]"""
    nib = _nibbles(t)
    out = torch.empty_like(nib)
    out[:, :, list(AWQ_ORDER)] = nib
    return out.reshape(t.shape[0], 8 * t.shape[1])


def linear_int4(mod, name="projection", zero_offset=None, config=None):
    """(q uint8 [N, K/2], z uint8 [N, K/128], s [N, K/128] in the checkpoint's scale dtype) of an AWQ or GPTQ projection module, or None for
    a module that is not INT4 (is_int4_module).  `config` is the model's quantization_config (dict or object: quant_method "awq" / "gptq",
    bits, group_size, version, checkpoint_format, desc_act); without one the layout is decided by qweight.shape against
    (in_features, out_features) and GPTQ v1 is assumed.  zero_offset: what is added to the stored zero point (default: 1 for GPTQ
    checkpoint_format "gptq", 0 for "gptq_v2" and AWQ).
      AWQ "GEMM": qweight [K, N/8], nibble p of [k][j] = q[8 j + AWQ_ORDER[p]][k]; qzeros [K/g, N/8] likewise; scales [K/g, N].
      GPTQ:       qweight [K/8, N], nibble p of [r][n] = q[n][8 r + p]; qzeros [K/g, N/8], nibble p of [G][j] = column 8 j + p;
                  scales [K/g, N]; optional g_idx [K], which must be k // g.
    Raises SamdError for AWQ "GEMV", bits != 4, group sizes that are no multiple of 128 dividing K (32, 64), act-order, a stored zero
    point of 15 under GPTQ v1 (public loaders disagree on whether it means 16 or wraps to 0), ill-shaped tensors."""
    if not is_int4_module(mod):
        return None
    K, N = int(mod.in_features), int(mod.out_features)
    qw, qz, sc = mod.qweight.detach(), mod.qzeros.detach(), mod.scales.detach()
    bits = _cfg(config, "bits", None)
    if bits is None:
        bits = getattr(mod, "bits", getattr(mod, "w_bit", 4))
    if int(bits) != 4:
        raise SamdError(f"{name}: {int(bits)}-bit quantisation; the runner takes 4-bit AWQ / GPTQ checkpoints only")
    method = _cfg(config, "quant_method", None)
    method = str(getattr(method, "value", method)).lower() if method is not None else None
    if method not in (None, "awq", "gptq"):
        raise SamdError(f"{name}: quant_method {method!r}; the INT4 importer takes 'awq' and 'gptq'")
    version = str(_cfg(config, "version", "") or "").lower()
    version = version.split(".")[-1]                               # (an enum's str: "AWQLinearVersion.GEMM")
    gemv_shapes = sc.dim() == 2 and sc.shape[0] == N and sc.shape[1] != N
    if version == "gemv" or (method in (None, "awq") and gemv_shapes):
        raise SamdError(f"{name}: AWQ 'GEMV' layout (qweight {tuple(qw.shape)}, scales {tuple(sc.shape)}) is not supported; the importer "
                        "takes AWQ 'GEMM'")
    if method is None:
        if tuple(qw.shape) == (K, N // 8):
            method = "awq"
        elif tuple(qw.shape) == (K // 8, N):
            method = "gptq"
        else:
            raise SamdError(f"{name}: qweight of shape {tuple(qw.shape)} is neither AWQ GEMM [{K}, {N // 8}] nor GPTQ [{K // 8}, {N}]")
    if method == "awq" and version not in ("", "gemm"):
        raise SamdError(f"{name}: AWQ version {version!r} is not supported; the importer takes AWQ 'GEMM'")
    want_qw = (K, N // 8) if method == "awq" else (K // 8, N)
    if N % 8 != 0 or K % 8 != 0 or tuple(qw.shape) != want_qw:
        raise SamdError(f"{name}: qweight of shape {tuple(qw.shape)}; {method.upper()} stores [{want_qw[0]}, {want_qw[1]}] for a ({N}, {K}) projection")
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
    if tuple(qz.shape) != (n_groups, N // 8):
        raise SamdError(f"{name}: qzeros of shape {tuple(qz.shape)}; expected [{n_groups}, {N // 8}]")
    if method == "awq":
        codes = _unpack_awq_cols(qw).t()                           # [N, K]
        zeros = _unpack_awq_cols(qz).t()                           # [N, K/g]
        offset = 0 if zero_offset is None else int(zero_offset)
    else:
        g_idx = getattr(mod, "g_idx", None)
        if _cfg(config, "desc_act", False) and g_idx is None:
            raise SamdError(f"{name}: act-order (desc_act) GPTQ checkpoints are not supported")
        if torch.is_tensor(g_idx):
            gi = g_idx.detach()
            want = torch.arange(K, device=gi.device) // g
            if gi.numel() != K or not torch.equal(gi.reshape(-1).to(want.dtype), want):
                raise SamdError(f"{name}: act-order (a g_idx other than k // group_size) GPTQ checkpoints are not supported")
        codes = _nibbles(qw).permute(1, 0, 2).reshape(N, K)
        zeros = _nibbles(qz).reshape(n_groups, N).t()
        fmt = str(_cfg(config, "checkpoint_format", "gptq") or "gptq").lower()
        if fmt not in ("gptq", "gptq_v2"):
            raise SamdError(f"{name}: GPTQ checkpoint_format {fmt!r}; the importer takes 'gptq' and 'gptq_v2'")
        offset = (1 if fmt == "gptq" else 0) if zero_offset is None else int(zero_offset)
    zeros = zeros.to(torch.int32) + offset
    if bool((zeros > 15).any()):
        raise SamdError(f"{name}: a stored zero point of 15 with the GPTQ v1 offset of +1 ('gptq' checkpoint_format): public loaders disagree "
                        "on whether it means 16 or wraps to 0; re-save the checkpoint as 'gptq_v2'")
    rep = g // GROUP
    z = zeros.to(torch.uint8).repeat_interleave(rep, dim=1).contiguous()
    s = sc.t().repeat_interleave(rep, dim=1).contiguous()
    return pack_nibbles(codes.contiguous()), z, s


def fuse_int4(parts, device, dtype=None):
    """row-concatenate the (q, z, s) of q|k|v or gate|up on `device` (dtype: the runner's, to which the scales are rounded once: as_scales).
    Groups run along K, so fusing before or after quantising is the same."""
    q = torch.cat([p[0].to(device) for p in parts], dim=0).contiguous()
    z = torch.cat([p[1].to(device) for p in parts], dim=0).contiguous()
    s = torch.cat([p[2].to(device) for p in parts], dim=0).contiguous()
    return q, z, (as_scales(s, dtype) if dtype is not None else s)


def checkpoint_is_int4(linears):
    """True when every projection module carries INT4 weights, False when none does; a mix raises SamdError"""
    kinds = [(name, is_int4_module(lin)) for name, lin in linears]
    n4 = sum(k for _, k in kinds)
    if 0 < n4 < len(kinds):
        plain = [n for n, k in kinds if not k][:3]
        raise SamdError(f"a mix of INT4 and other projections ({n4} of {len(kinds)} are INT4; e.g. {', '.join(plain)} are not); "
                        "the runner takes all projections in one format")
    return n4 > 0


def packed_bytes(N, K):
    """bytes of samd_gemm_pack_i4's output: the codes and, inline behind every 16 KiB of them, their 1 KiB of group data"""
    return N * K // 2 + N * K // 32
