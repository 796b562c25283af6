"""FP8 weight-only decoding: the numeric contract of the runner's e4m3fn projections ("FP8 weights").

Weights are OCP float8_e4m3fn (gfx950's FP8; not the e4m3fnuz of MI300), one fp32 scale per output row of the HF weight, i.e. per output
column of the projection: W[n][k] ~ float(q[n][k]) * scale[n].  Quantising on load is symmetric per row:
    scale = absmax / 448 (fp32; a zero row gets 1),  q = clamp(W / scale, +-448).to(float8_e4m3fn)  (round to nearest even).
Checkpoints that already carry FP8 projections (an nn.Linear whose weight is float8_e4m3fn and that has a `weight_scale`: per tensor, [N] or
[N, 1]) are imported as they are.  Everything here is plain torch and runs on any device.

BLOCK-SCALED FP8 (the official Qwen3-MoE FP8 checkpoints: `weight` float8_e4m3fn with `weight_scale_inv` fp32, one scale per 128 x 128 block,
quantization_config.weight_block_size = [128, 128]; the dense Qwen3-*-FP8 checkpoints and everything else transformers' fine-grained FP8
quantiser writes) is the format of mixture-of-experts experts (expert_format "fp8b128", samd_hip/moe.py) and of the dense runner's
weight_format "fp8b128" (samd_gemm_skinny_f8b: the same contract, the checkpoint's own scale table); linear_fp8 keeps rejecting it for the
per-row weight_format "fp8".  Its numeric contract:
    W[n][k] = float(q[n][k]) * s[n / 128][k / 128],  q OCP e4m3fn, s fp32, finite and positive.
The kernels never form W.  Per output element they compute out = sum_b s_b * (sum_{k in block b} A[m][k] * q[n][k]): the inner sum is
an fp32 MFMA accumulation over the block's 128 k with q widened exactly (v_cvt_scalef32_pk_{f16,bf16}_fp8 at scale 1: every e4m3fn value is
exact in fp16 and in bf16), the outer step ONE fp32 FMA per accumulator and block, acc = fma(acc_blk, s_b, acc), in ascending block order.
That is the weight side of HF's own block-FP8 matmul; it cannot overflow fp16.  The epilogues' roundings (HF's: gate, up, their product, the
down product, the combine) are unchanged.  Activations stay in the model dtype: weight-only; a checkpoint's "dynamic" activation
quantisation is not reproduced.  Projections that are dequantised at import (the attention of a module with FP8 experts) become
rne_dtype(fl32(float(q) * s)): dequantize_blocks, then one rounding.  Quantising on load is symmetric per block: s = absmax / 448 (a zero
block gets 1), q = clamp(W / s, +-448) rounded to nearest even."""
import torch

from . import SamdError

E4M3_MAX = 448.0
PROJECTIONS = ("wqkv", "wo", "wgu", "wdown")
BLOCK = 128                            # block-scaled FP8: one fp32 scale per BLOCK x BLOCK weights


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



def quantize_blocks(W):
    """W [..., N, K] (any float dtype, any device; N, K multiples of 128) -> (q float8_e4m3fn [..., N, K], s fp32 [..., N/128, K/128]),
    symmetric per 128 x 128 block: s = absmax / 448, a zero block gets 1"""
    *lead, N, K = W.shape
    if N % BLOCK != 0 or K % BLOCK != 0:
        raise SamdError(f"block-scaled FP8 needs N % 128 == 0 and K % 128 == 0, got a weight of shape {tuple(W.shape)}")
    Wb = W.float().reshape(*lead, N // BLOCK, BLOCK, K // BLOCK, BLOCK)
    absmax = Wb.abs().amax(dim=(-3, -1))
    s = absmax / E4M3_MAX
    s = torch.where(absmax > 0, s, torch.ones_like(s))
    q = (Wb / s[..., :, None, :, None]).clamp_(-E4M3_MAX, E4M3_MAX).reshape(*lead, N, K).to(torch.float8_e4m3fn)
    return q, s.contiguous()


def dequantize_blocks(q, s):
    """fl32(float(q) * s) in fp32, q [..., N, K] float8_e4m3fn (or its bytes), s [..., N/128, K/128]: the weights a block-scaled FP8 launch
    multiplies by"""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    *lead, N, K = q.shape
    qb = q.float().reshape(*lead, N // BLOCK, BLOCK, K // BLOCK, BLOCK)
    return (qb * s.float()[..., :, None, :, None]).reshape(*lead, N, K)


def block_scale_offset(rows, K):
    """byte offset of the scale table inside a packed block-scaled buffer of `rows` x K codes: after the codes, at a multiple of 256"""
    return (rows * K + 255) // 256 * 256


def packed_block_bytes(N, K):
    """bytes of one [N, K] block-scaled FP8 matrix in the expert kernels' packed form: N * K codes (samd_gemm_pack_f8's layout) and one fp32
    scale per (64 packed rows, 128 k).  N % 128 == 0 and K % 256 == 0 make N * K a multiple of 256, so E matrices end to end take E times this"""
    return N * K + (N // 64) * (K // BLOCK) * 4


def _cfg_get(config, key):
    if config is None:
        return None
    return config.get(key) if isinstance(config, dict) else getattr(config, key, None)


def check_block_config(config, name="quantization_config"):
    """what a checkpoint's quantization_config (a dict or an object; None passes) may say for the block importer: weight_block_size [128, 128],
    activation_scheme "dynamic" (ignored: weight-only), fp32 scales"""
    bs = _cfg_get(config, "weight_block_size")
    if bs is not None and tuple(int(x) for x in bs) != (BLOCK, BLOCK):
        raise SamdError(f"{name}: weight_block_size {list(bs)} is not supported; block-scaled FP8 takes [128, 128]")
    if _cfg_get(config, "activation_scheme") == "static":
        raise SamdError(f"{name}: activation_scheme 'static' is not supported; the runner is weight-only and takes 'dynamic' checkpoints")
    fmt = _cfg_get(config, "scale_fmt")
    if fmt not in (None, "float"):
        raise SamdError(f"{name}: scale_fmt {fmt!r} is not supported; block scales are fp32")


def check_block_scales(q, s, name="weight"):
    """q [..., N, K] float8_e4m3fn with s fp32 [..., N/128, K/128], finite and positive; raises SamdError by `name`"""
    if q.dtype in _OTHER_FP8:
        raise SamdError(f"{name}: weights in {_OTHER_FP8[q.dtype]} are not supported; the runner takes OCP float8_e4m3fn (gfx950's FP8)")
    if q.dtype != torch.float8_e4m3fn:
        raise SamdError(f"{name}: expected a float8_e4m3fn weight, got {q.dtype}")
    if s is None:
        raise SamdError(f"{name}: float8_e4m3fn weight without a weight_scale_inv")
    if s.dtype != torch.float32:
        raise SamdError(f"{name}: weight_scale_inv of dtype {s.dtype} is not supported (ue8m0 scale_fmt?); block scales are fp32")
    *lead, N, K = q.shape
    want = (*lead, N // BLOCK, K // BLOCK)
    if N % BLOCK != 0 or K % BLOCK != 0 or tuple(s.shape) != want:
        raise SamdError(f"{name}: weight_scale_inv of shape {tuple(s.shape)} for a {list(q.shape)} weight; one scale per 128 x 128 block is "
                        f"{list(want)} (partial blocks are not supported)")
    if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()):
        raise SamdError(f"{name}: weight_scale_inv must be finite and positive")


def linear_fp8_block(lin, name="projection", config=None):
    """(q [N, K] float8_e4m3fn, s fp32 [N/128, K/128]) of a block-scaled FP8 checkpoint's Linear (`weight` + `weight_scale_inv`), or None
    when its weight is not an FP8 dtype.  `config`: the model's quantization_config.  Raises SamdError by `name` for another FP8 encoding,
    a scale that is not fp32, a scale of another shape, non-finite or non-positive scales, activation_scheme "static" and block sizes
    other than [128, 128] (the module's own attributes count as well as the config's)."""
    w = lin.weight
    if not is_fp8_dtype(w.dtype):
        return None
    check_block_config(config, name)
    bs = getattr(lin, "block_size", None)
    if bs is not None and tuple(int(x) for x in bs) != (BLOCK, BLOCK):
        raise SamdError(f"{name}: block_size {list(bs)} is not supported; block-scaled FP8 takes [128, 128]")
    if getattr(lin, "activation_scheme", None) == "static":
        raise SamdError(f"{name}: activation_scheme 'static' is not supported; the runner is weight-only and takes 'dynamic' checkpoints")
    s = getattr(lin, "weight_scale_inv", None)
    check_block_scales(w, None if s is None else s.detach(), name)
    return w.detach(), s.detach().contiguous()


def linear_fp8_dequantized(lin, name="projection", config=None):
    """fl32(float(q) * s) [N, K] in fp32 of an FP8 Linear, block-scaled (weight_scale_inv) or per row / per tensor (weight_scale); None when
    its weight is not an FP8 dtype"""
    if not is_fp8_dtype(lin.weight.dtype):
        return None
    if getattr(lin, "weight_scale_inv", None) is not None:
        return dequantize_blocks(*linear_fp8_block(lin, name, config))
    return dequantize_rows(*linear_fp8(lin, name))


def block_scaled_bytes(N, K):
    """bytes of one [N, K] block-scaled FP8 projection as the dense runner holds it (weight_format "fp8b128"): N * K codes in
    samd_gemm_pack_f8's layout and the checkpoint's own table, one fp32 scale per 128 x 128 block"""
    return N * K + (N // BLOCK) * (K // BLOCK) * 4


def fuse_fp8_blocks(parts, device, names=None):
    """row-concatenate the (q [N_i, K], s [N_i/128, K/128]) of q|k|v or gate|up on `device` (the bytes are moved as uint8).  The block rows of
    the parts line up in the fused table because every part has N_i % 128 == 0; a part that has not raises SamdError by its name"""
    names = names or [f"part {i}" for i in range(len(parts))]
    K = parts[0][0].shape[1]
    for (q, s), name in zip(parts, names):
        N = q.shape[0]
        if N % BLOCK != 0 or q.shape[1] != K or K % BLOCK != 0 or tuple(s.shape) != (N // BLOCK, K // BLOCK):
            raise SamdError(f"{name}: a [{N}, {q.shape[1]}] block-scaled FP8 part with scales {list(s.shape)} cannot be fused: every part needs "
                            f"N % 128 == 0 (a 128 x 128 block would straddle two parts), the same K % 128 == 0 and one scale per block")
    q = torch.cat([p[0].to(device).view(torch.uint8) for p in parts], dim=0).view(torch.float8_e4m3fn).contiguous()
    s = torch.cat([p[1].to(device=device, dtype=torch.float32) for p in parts], dim=0).contiguous()
    return q, s


def checkpoint_is_fp8_block(linears, config=None):
    """True when every projection Linear is block-scaled FP8 (an FP8 `weight` beside a `weight_scale_inv`; each is then checked by
    linear_fp8_block with the module's quantization_config, whose rejections apply by name), False when none is; a mix -- block-scaled
    beside per-row / per-tensor FP8, plain or other formats -- raises SamdError naming examples"""
    def kind(lin):
        w = getattr(lin, "weight", None)
        if w is None or not is_fp8_dtype(w.dtype):
            return "other"
        return "block" if getattr(lin, "weight_scale_inv", None) is not None else "row"
    kinds = [(name, kind(lin)) for name, lin in linears]
    nb = sum(k == "block" for _, k in kinds)
    if nb == 0:
        return False
    if nb < len(kinds):
        rows = [n for n, k in kinds if k == "row"][:3]
        other = [n for n, k in kinds if k == "other"][:3]
        what = "; ".join(x for x in (f"e.g. {', '.join(rows)} carry a per-row / per-tensor weight_scale" if rows else "",
                                     f"e.g. {', '.join(other)} are not FP8" if other else "") if x)
        raise SamdError(f"a mix of block-scaled FP8 and other projections ({nb} of {len(kinds)} are block-scaled FP8; {what}); "
                        "the runner takes all projections in one format")
    for name, lin in linears:
        linear_fp8_block(lin, name, config)
    return True
