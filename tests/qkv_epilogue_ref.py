"""Restatement of the q|k|v epilogue of samd_rope_kv_write_epi (include/samd_hip.h samd_qkv_epilogue_t) in float64 / float32 torch on the
CPU (no product import): the value of every rounding the kernels make, in their order.

  x = round_T(sum of the fp32 partials + float(bias))   or   round_T(float(qkv) + float(bias))   (no bias: the product as it is)
  q / k heads with the norms: y = round_T(x * rsqrt(sum(x^2) / 128 + eps)), z = round_T(float(w) * float(y))   (HF Qwen3RMSNorm)
  RoPE (rotate_half): o1 = round_T(x1 c - x2 s), o2 = round_T(x2 c + x1 s), each product and sum an fp32 rounding (no FMA)

`inv_ulps` shifts the fp32 value of rsqrt by that many units in the last place: the device's rsqrtf is within one of the correctly
rounded value, so a test accepts a head whose output equals the restatement at one of the shifts -1, 0, +1."""
import torch

F32 = torch.float32


def epilogue_x(qkv, parts, bias, dtype):
    """x [rows, cols] as float32 values of dtype: qkv (dtype) when parts is None, else parts [n_part, rows, cols] float32 summed in order"""
    if parts is None:
        x = qkv.to(F32)
        if bias is not None:
            x = (x + bias.to(F32)).to(dtype).to(F32)
        return x
    acc = torch.zeros(parts.shape[1:], dtype=F32)
    for p in parts:
        acc = acc + p
    if bias is not None:
        acc = acc + bias.to(F32)
    return acc.to(dtype).to(F32)


def head_norm(x, w, eps, dtype, inv_ulps=0):
    """HF Qwen3RMSNorm over the last dim (128) of x (float32 values of dtype), as the kernel rounds it"""
    ss = (x.double() ** 2).sum(-1, keepdim=True).to(F32)                # exact for the planted values the tests use
    var = (ss / 128.0).to(F32) + torch.tensor(eps, dtype=F32)
    inv = (1.0 / var.double().sqrt()).to(F32)
    if inv_ulps:
        inv = torch.nextafter(inv, torch.full_like(inv, float("inf") if inv_ulps > 0 else 0.0))
    y = (x * inv).to(dtype).to(F32)
    return (w.to(F32) * y).to(dtype).to(F32)


def rope(x, cos, sin, dtype):
    """x [rows, heads, 128] float32, cos / sin [rows, 64] float32 -> rotated, rounded to dtype (float32 values)"""
    x1, x2 = x[..., :64], x[..., 64:]
    c, s = cos[:, None, :], sin[:, None, :]
    o1 = (x1 * c) - (x2 * s)
    o2 = (x2 * c) + (x1 * s)
    return torch.cat([o1, o2], -1).to(dtype).to(F32)


def restate(qkv, parts, bias, q_norm, k_norm, eps, cos, sin, H, Hkv, dtype, inv_ulps=0):
    """(q_rot [rows, H, 128], k_rot [rows, Hkv, 128], v [rows, Hkv, 128]) as float32 values of dtype"""
    x = epilogue_x(qkv, parts, bias, dtype)
    rows = x.shape[0]
    x = x.view(rows, H + 2 * Hkv, 128)
    q, k, v = x[:, :H], x[:, H:H + Hkv], x[:, H + Hkv:]
    if q_norm is not None:
        q, k = head_norm(q, q_norm, eps, dtype, inv_ulps), head_norm(k, k_norm, eps, dtype, inv_ulps)
    return rope(q, cos, sin, dtype), rope(k, cos, sin, dtype), v.clone()
