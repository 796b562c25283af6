"""FP8 weight-only decoding: the numeric contract of the runner's e4m3fn projections ("FP8 weights").

Weights are OCP float8_e4m3fn (gfx950's FP8; not the e4m3fnuz of MI300), one fp32 scale per output row of the HF weight, i.e. per output
column of the projection: W[n][k] ~ float(q[n][k]) * scale[n].  Quantising on load is symmetric per row:
    scale = absmax / 448 (fp32; a zero row gets 1),  q = clamp(W / scale, +-448).to(float8_e4m3fn)  (round to nearest even).
Checkpoints that already carry FP8 projections (an nn.Linear whose weight is float8_e4m3fn and that has a `weight_scale`: per tensor, [N] or
[N, 1]) are imported as they are.  Everything here is plain torch and runs on any device."""
import torch

from . import SamdError

E4M3_MAX = 448.0
PROJECTIONS = ("wqkv", "wo", "wgu", "wdown")


def quantize_rows(W):
    """W [N, K] (any float dtype, any device) -> (q float8_e4m3fn [N, K], scale fp32 [N]), symmetric per row"""
    Wf = W.float()
    absmax = Wf.abs().amax(dim=1)
    scale = absmax / E4M3_MAX
    scale = torch.where(absmax > 0, scale, torch.ones_like(scale))
    q = (Wf / scale[:, None]).clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q, scale.contiguous()


def dequantize_rows(q, scale):
    """float(q) * scale in fp32: the weights an FP8 runner multiplies by"""
    return q.float() * scale.float()[:, None]


_OTHER_FP8 = {getattr(torch, n): n for n in ("float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz") if hasattr(torch, n)}


def is_fp8_dtype(dtype):
    return dtype == torch.float8_e4m3fn or dtype in _OTHER_FP8


def linear_fp8(lin, name="projection"):
    """(q [N, K] float8_e4m3fn, scale fp32 [N]) of an FP8 checkpoint's nn.Linear, or None when its weight is not an FP8 dtype.
    Raises SamdError for what the runner cannot run: another FP8 encoding, block scales, a missing or ill-shaped weight_scale."""
    w = lin.weight
    if w.dtype in _OTHER_FP8:
        raise SamdError(f"{name}: weights in {_OTHER_FP8[w.dtype]} are not supported; the runner takes OCP float8_e4m3fn (gfx950's FP8)")
    if w.dtype != torch.float8_e4m3fn:
        return None
    if getattr(lin, "weight_scale_inv", None) is not None:
        raise SamdError(f"{name}: block-scaled FP8 (weight_scale_inv of shape {tuple(lin.weight_scale_inv.shape)}) is not supported; "
                        "the runner takes one scale per tensor or per output row")
    s = getattr(lin, "weight_scale", None)
    if s is None:
        raise SamdError(f"{name}: float8_e4m3fn weight without a weight_scale")
    N = w.shape[0]
    shp = tuple(s.shape)
    if s.numel() == 1 and len(shp) <= 2:
        scale = s.detach().float().reshape(1).expand(N)
    elif shp in ((N,), (N, 1)):
        scale = s.detach().float().reshape(N)
    else:
        raise SamdError(f"{name}: weight_scale of shape {shp} for a [{N}, {w.shape[1]}] weight; only per-tensor, [N] and [N, 1] scales are "
                        "supported (block scales are not)")
    if not bool(torch.isfinite(scale).all()) or not bool((scale > 0).all()):
        raise SamdError(f"{name}: weight_scale must be finite and positive")
    return w.detach(), scale.contiguous()


def fuse_fp8(parts, device):
    """row-concatenate the (q, scale) of q|k|v or gate|up on `device` (the bytes are moved as uint8)"""
    q = torch.cat([p[0].to(device).view(torch.uint8) for p in parts], dim=0).view(torch.float8_e4m3fn).contiguous()
    scale = torch.cat([p[1].to(device) for p in parts], dim=0).contiguous()
    return q, scale


def checkpoint_is_fp8(linears):
    """True when every projection Linear carries FP8 weights, False when none does; a mix raises SamdError"""
    kinds = [(name, linear_fp8(lin, name) is not None) for name, lin in linears]
    n8 = sum(k for _, k in kinds)
    if 0 < n8 < len(kinds):
        plain = [n for n, k in kinds if not k][:3]
        raise SamdError(f"a mix of FP8 and non-FP8 projections ({n8} of {len(kinds)} are FP8; e.g. {', '.join(plain)} are not); "
                        "the runner takes all projections in one format")
    return n8 > 0

