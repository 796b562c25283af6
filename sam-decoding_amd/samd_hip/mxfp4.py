"""MXFP4 weight-only decoding: the numeric contract of the runner's 4-bit projections ("MXFP4 weights").

OCP Microscaling FP4: e2m1 elements, one e8m0 scale per block of 32 elements along K, 4.25 bits per weight; no per-row or per-tensor scale.
    q  uint8 [N, K/2]: low nibble = element 2i, high nibble = element 2i+1 (torch's float4_e2m1fn_x2 byte); a nibble has its sign in bit 3
       and indexes the magnitude into {0, .5, 1, 1.5, 2, 3, 4, 6};
    e8 uint8 [N, K/32]: the block scale is 2^(e8 - 127) (torch's float8_e8m0fnu byte; 255 is NaN);
    W[n][k] = fp4(q[n][k]) * 2^(e8[n][k/32] - 127).
The kernel widens a weight to the model dtype WITH its block scale, so "widening adds no error" holds only where fp4 * 2^e is exact in that
dtype: EXPONENT_RANGE.  quantize_blocks clamps to it; a checkpoint exponent outside it is an error (check_exponents).
Quantising on load (round to nearest, no calibration) costs about 11.5 % relative RMS weight error: it is for benches, random-init models and
tests.  Quality-sensitive users import a checkpoint that was calibrated elsewhere.  Everything here is plain torch and runs on any device."""
import torch

from . import SamdError

BLOCK = 32
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1_MAX = 6.0
PROJECTIONS = ("wqkv", "wo", "wgu", "wdown")
# block-scale exponents e (scale 2^e) for which every fp4 * 2^e is exact in the dtype.  fp16: 0.5 * 2^-23 is the smallest subnormal and
# 6 * 2^13 the largest product below 65504; v_cvt_scalef32_pk_f16_fp4 delivers the subnormals exactly (tests/test_gpu_mxfp4_gemm.py decides
# this bound on the GPU).  bf16: 0.5 * 2^-125 is its smallest normal.
FP16_EMIN = -23
EXPONENT_RANGE = {torch.float16: (FP16_EMIN, 13), torch.bfloat16: (-125, 125)}

_F4 = getattr(torch, "float4_e2m1fn_x2", None)
_E8 = getattr(torch, "float8_e8m0fnu", None)


def is_fp4_dtype(dtype):
    return _F4 is not None and dtype == _F4


def exponent_range(dtype=None):
    """(lowest, highest) block-scale exponent of a runner in `dtype`; None: the widest range the kernel takes (bf16's)"""
    if dtype is None:
        return EXPONENT_RANGE[torch.bfloat16]
    if dtype not in EXPONENT_RANGE:
        raise SamdError(f"MXFP4 projections run in fp16 or bf16, not {dtype}")
    return EXPONENT_RANGE[dtype]


def _bytes(t):
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def _exp2(e):
    """2^e in fp32 for an int32 tensor e in [-127, 127], built from its bits: exact on every device (a library pow / ldexp need not be)"""
    bits = torch.where(e > -127, (e + 127) << 23, torch.full_like(e, 0x00400000))     # 2^-127 is the fp32 subnormal 0x00400000
    return bits.to(torch.int32).view(torch.float32)


def quantize_blocks(W, dtype=None):
    """W [N, K] (any float dtype, any device, K % 32 == 0) -> (q uint8 [N, K/2], e8 uint8 [N, K/32]).  Per block of 32 along K:
    e = floor(log2(absmax)) - 2 clamped to exponent_range(dtype) (a block whose elements all come out 0 gets e = 0), elements
    clamp(W / 2^e, +-6) rounded to the nearest grid point, ties to the even code; a negative value that rounds to 0 becomes +0."""
    N, K = W.shape
    if K % BLOCK != 0:
        raise SamdError(f"MXFP4 needs K % 32 == 0, got a [{N}, {K}] matrix")
    lo, hi = exponent_range(dtype)
    Wb = W.float().reshape(N, K // BLOCK, BLOCK)
    absmax = Wb.abs().amax(dim=2)
    _, ex = torch.frexp(absmax)                                  # absmax = m * 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    e = (ex.to(torch.int32) - 3).clamp_(lo, hi)
    a = (Wb * _exp2(-e)[:, :, None]).clamp_(-E2M1_MAX, E2M1_MAX)           # (a power-of-two multiply: exact)
    mag = a.abs()
    code = torch.zeros_like(mag, dtype=torch.int32)
    # the midpoint above an even code stays (>), the one above an odd code goes up (>=): ties to the even code
    for mid, up_on_tie in ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)):
        code += (mag >= mid) if up_on_tie else (mag > mid)
    code = code | (((a < 0) & (code != 0)).to(torch.int32) << 3)
    e = torch.where((code & 7).amax(dim=2) == 0, torch.zeros_like(e), e)
    code = code.reshape(N, K).to(torch.uint8)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    return q, (e + 127).to(torch.uint8).contiguous()


def dequantize_blocks(q, e8):
    """fp4(q) * 2^(e8 - 127) in fp32, [N, K]: the weights an MXFP4 runner multiplies by"""
    qb, eb = _bytes(q), _bytes(e8)
    N, Kh = qb.shape
    grid = torch.tensor(GRID + tuple(-g for g in GRID), dtype=torch.float32, device=qb.device)
    vals = torch.stack([grid[(qb & 15).long()], grid[(qb >> 4).long()]], dim=2).reshape(N, 2 * Kh)
    return (vals.reshape(N, -1, BLOCK) * _exp2(eb.to(torch.int32) - 127)[:, :, None]).reshape(N, 2 * Kh)


def check_exponents(e8, dtype, name="projection"):
    """raise SamdError unless every e8m0 code is a number (not 255) whose exponent lies in exponent_range(dtype)"""
    eb = _bytes(e8)
    if bool((eb == 255).any()):
        raise SamdError(f"{name}: a block scale is NaN (e8m0 code 255)")
    lo, hi = exponent_range(dtype)
    ex = eb.to(torch.int32) - 127
    if bool(((ex < lo) | (ex > hi)).any()):
        way_out = "; bfloat16 holds every product exactly for exponents -125 .. 125: run the model with dtype=torch.bfloat16" \
            if dtype == torch.float16 else ""
        raise SamdError(f"{name}: block-scale exponents {int(ex.min())} .. {int(ex.max())} leave [{lo}, {hi}], the range in which "
                        f"fp4 * 2^e is exact in {dtype}{way_out}")


def linear_mxfp4(lin, name="projection"):
    """(q uint8 [N, K/2], e8 uint8 [N, K/32]) of an MXFP4 checkpoint's nn.Linear: float4_e2m1fn_x2 or uint8 weights [N, K/2] with a
    `weight_scale` [N, K/32] of dtype float8_e8m0fnu or uint8.  None for every other Linear.  Raises SamdError for what the runner cannot
    run: K % 32 != 0, another block size, a second-level scale (NVFP4), a missing or ill-typed weight_scale, a NaN scale."""
    w = lin.weight
    if not (is_fp4_dtype(w.dtype) or w.dtype == torch.uint8):
        return None
    for second in ("weight_scale_2", "weight_global_scale"):
        if getattr(lin, second, None) is not None:
            raise SamdError(f"{name}: a second-level scale ({second}) makes this NVFP4, not MXFP4; the runner takes e8m0 block scales alone")
    s = getattr(lin, "weight_scale", None)
    if s is None:
        raise SamdError(f"{name}: {w.dtype} weight without a weight_scale")
    if w.dim() != 2:
        raise SamdError(f"{name}: packed 4-bit weight of shape {tuple(w.shape)}; expected [N, K/2]")
    N, K = w.shape[0], 2 * w.shape[1]
    if K % BLOCK != 0:
        raise SamdError(f"{name}: K = {K} is not a multiple of the MX block of 32")
    if not (s.dtype == torch.uint8 or (_E8 is not None and s.dtype == _E8)):
        raise SamdError(f"{name}: weight_scale of dtype {s.dtype}; MXFP4 block scales are e8m0 (float8_e8m0fnu or uint8)")
    if tuple(s.shape) != (N, K // BLOCK):
        raise SamdError(f"{name}: weight_scale of shape {tuple(s.shape)} for a [{N}, {K}] weight; MXFP4 has one scale per 32 elements along K, "
                        f"[{N}, {K // BLOCK}] (other block sizes are not supported)")
    e8 = _bytes(s.detach())
    if bool((e8 == 255).any()):
        raise SamdError(f"{name}: a block scale is NaN (e8m0 code 255)")
    return _bytes(w.detach()), e8


def fuse_mxfp4(parts, device):
    """row-concatenate the (q, e8) of q|k|v or gate|up on `device`.  Blocks run along K, so fusing before or after quantising is the same."""
    q = torch.cat([_bytes(p[0]).to(device) for p in parts], dim=0).contiguous()
    e8 = torch.cat([_bytes(p[1]).to(device) for p in parts], dim=0).contiguous()
    return q, e8


def checkpoint_is_mxfp4(linears):
    """True when every projection Linear carries MXFP4 weights, False when none does; a mix raises SamdError"""
    kinds = [(name, linear_mxfp4(lin, name) is not None) for name, lin in linears]
    n4 = sum(k for _, k in kinds)
    if 0 < n4 < len(kinds):
        plain = [n for n, k in kinds if not k][:3]
        raise SamdError(f"a mix of MXFP4 and other projections ({n4} of {len(kinds)} are MXFP4; e.g. {', '.join(plain)} are not); "
                        "the runner takes all projections in one format")
    return n4 > 0


def packed_bytes(N, K):
    """bytes of samd_gemm_pack_f4's output: the elements and, inline behind every 16 KiB of them, their 1 KiB of scales"""
    return N * K // 2 + N * K // BLOCK
