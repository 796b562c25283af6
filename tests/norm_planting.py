"""Planted RMSNorm / residual-stream inputs and their float64 references (numpy + torch only; no product import).

randn rows all have mean(x^2) ~ 1: a row that takes another row's 1 / rms, a dropped 16-column tile of the sum of squares, a lost eps or
a missing intermediate rounding moves the output by less than a max-error bar relative to the whole tensor.  Here every row is PLANTED:

  spread    N(0, 1) scaled to an RMS of 10^U(-2, -1) (even rows) or 10^U(1, 2) (odd rows): row r and its partner r ^ 1 differ by >= 100x
            in scale, or the partner is one of the rows below, whose 1 / rms is >= 9x away as well
  tile      >= 95 % of the row's energy in ONE 16-column window (a tile of the [hidden / 16][16] sums of squares, or for k_rmsnorm any
            window starting at a multiple of 8 columns), scaled like a spread row
  tiny      mean(x^2) = eps / 8: 1 / rms is decided by eps (dropping it, or adding it outside the square root, multiplies it by ~3)
  massive   N(0, 1) with two channels at +2000 and -2000 (Llama-2's BOS-token outliers); always at an odd row
  zero      all zeros: out = 0 for any finite 1 / rms
Norm weights are drawn from +-[0.5, 4] with random signs, so that a weight applied to the wrong channels shows.

References round to the model dtype T where HF does: LlamaRMSNorm h = (x * rsqrt(mean(x^2) + eps)).to(T), out = (w * h).to(T);
LlamaDecoderLayer residual = (x + proj.to(T)).to(T); LlamaMLP silu(gate.to(T)).to(T) * up.to(T), rounded.  `faulted` recomputes a
reference with one named fault, and `self_check_max` / `self_check_fraction` assert that the bar of the test would see it: every
max-error fault misses the bar by >= 50x (and every targeted row by >= 2x), every rounding fault changes >= 10x the capped fraction
of elements."""
import math

import numpy as np
import torch

F64 = torch.float64
TILE = 16
ROUND_TILES = 32                       # tiles per round of norm_issue (NT / 16 with NT = 512 threads)
TOL = {torch.float16: 4e-3, torch.bfloat16: 3e-2}    # the fold kernels' tolerance, per (row, head) / per row
FLOOR = 0.25                           # |want_row|_inf below this is held to tol * FLOOR
ULP_BAR = 2                            # RMSNorm outputs: every element within 2 ulp_T of the reference
FRAC_CAP = 0.01                        # ... and at most 1 % of the elements different from it
MISS, ROW_MISS, FRAC_MISS = 50.0, 2.0, 10.0
ACT_MISS = 20.0                        # silu(gate) * up rows are heavy-tailed (a product of two normals): a bar relative to the row's largest
                                       # element sees a fault that moves every element by ~its typical size only 30-45x over; also the
                                       # margin of faults that must travel through several residual layers
KINDS = ("spread", "tile", "tiny", "massive", "zero")
PATTERN = ("spread", "massive", "tile", "tile", "tiny", "spread", "zero", "tile")     # kind of row r: PATTERN[r % 8]
MAX_FAULTS = ("other_row", "drop_tile", "no_eps", "eps_outside", "w_shift8")
TARGETS = {"other_row": ("spread",), "drop_tile": ("tile",), "no_eps": ("tiny",), "eps_outside": ("tiny",),
           "w_shift8": ("spread", "tile", "tiny")}          # (a massive row is decided by two weights: a shift may keep their size)
ROUNDING_FAULTS = ("no_h_round", "divisor")          # for the residual adds: "no_proj_round"
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}


def rounded(x, dtype):
    """float64 tensor of the values `x` takes in `dtype`"""
    return torch.as_tensor(x).to(dtype).to(F64)


def ulp(v, dtype):
    """spacing of `dtype` at |v| (float64): 2^(floor(log2|v|) - mantissa bits), subnormal spacing below the smallest normal"""
    a = torch.as_tensor(v, dtype=F64).abs()
    _, e = torch.frexp(a)                                   # a = m 2^e, m in [0.5, 1)  ->  floor(log2 a) = e - 1
    e = torch.clamp(torch.where(a > 0, e - 1, EMIN[dtype]), min=EMIN[dtype])        # (frexp(0) has exponent 0)
    return torch.ldexp(torch.ones_like(a), e - MANT[dtype])


def partner(rows):
    """the row whose 1 / rms the `other_row` fault hands to row r: r ^ 1 (itself for a last odd-one-out row)"""
    p = torch.arange(rows) ^ 1
    return torch.where(p < rows, p, torch.arange(rows))


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def rms_scale(x, eps, fault=None, hot=None):
    """float64 1 / rms per row of x [rows, hidden]; hot[r] = first column of row r's planted window (or -1)"""
    hidden = x.shape[-1]
    sq = x * x
    if fault == "drop_tile":
        sq = sq.clone()
        for r, c in enumerate(hot):
            if c >= 0:
                sq[r, c:c + TILE] = 0
    m = sq.sum(-1) / (hidden - TILE if fault == "divisor" else hidden)
    if fault == "no_eps":
        rs = 1.0 / torch.sqrt(m)
    elif fault == "eps_outside":
        rs = 1.0 / (torch.sqrt(m) + eps)
    else:
        rs = 1.0 / torch.sqrt(m + eps)
    if fault == "other_row":
        rs = rs[partner(len(rs)).to(rs.device)]
    return rs


def rmsnorm(x, w, eps, dtype, fault=None, hot=None):
    """LlamaRMSNorm of the rounded rows x with the rounded weight w, in float64 with HF's two roundings"""
    rs = rms_scale(x, eps, fault, hot)
    if fault == "w_shift8":
        w = torch.roll(w, 8)
    t = x * rs[:, None]
    h = t if fault == "no_h_round" else rounded(t, dtype)
    return rounded(w * h, dtype)


def add_delta(x, delta, dtype):
    """residual add from a T tensor"""
    return rounded(x + delta, dtype)


def add_partials(x, parts, dtype, fault=None):
    """residual add from fp32 split-K partials [n][rows, hidden]: their sum is rounded to T before the add"""
    s = parts.sum(0)
    return rounded(x + (s if fault == "no_proj_round" else rounded(s, dtype)), dtype)


def tile_ssq(y):
    """[rows, hidden / 16] float64 sums of squares per 16-column tile"""
    rows, hidden = y.shape
    return (y * y).view(rows, hidden // TILE, TILE).sum(-1)


def ssq_layout(y, rows_total=16, fill=float("nan")):
    """the kernels' [hidden / 16][16] fp32 layout (tile-major, row m at [t][m]) of y's rows; rows >= len(y) get `fill`"""
    t = tile_ssq(y)
    out = torch.full((t.shape[1], rows_total), fill, dtype=torch.float32, device=y.device)
    out[:, :t.shape[0]] = t.t().float()
    return out


def ssq_rows(layout, rows):
    """inverse of ssq_layout: [rows, hidden / 16] float64"""
    return layout[:, :rows].t().to(F64)


def cs_residual(x, A, W, dtype, fault=None):
    """k_gemm_cs_residual: y = (x + (A W^T).to(T)).to(T); also the unrounded projection"""
    p = A @ W.t()
    return rounded(x + (p if fault == "no_proj_round" else rounded(p, dtype)), dtype), p


def accumulation_slack(A, W, K):
    """|fp32 sum - exact| <= d 2^-24 sum_k |a_k w_k| with d = K / 128 + 64 >= the summation depth of the MFMA stream (K / 256 chunk adds per
    wave, 8 wave shares, <= 32 products inside one MFMA), the standard bound for a depth-d summation"""
    return (K / 128 + 64) * 2.0 ** -24 * (A.abs() @ W.abs().t())


def cs_residual_bar(y_want, p, slack, dtype):
    """per element: 1 ulp_T(y) for the final rounding, 1 ulp_T(p) for a flipped rounding of the projection, plus the accumulation slack"""
    return ulp(y_want, dtype) + ulp(p.abs() + slack, dtype) + slack


def rope(y, cs):
    """rotate_half RoPE of y [rows, heads, 128] with caller-supplied cos | sin rows cs [rows, 128] (float64)"""
    c, s = cs[:, None, :64], cs[:, None, 64:]
    return torch.cat((y[..., :64] * c - y[..., 64:] * s, y[..., 64:] * c + y[..., :64] * s), dim=-1)


def qkv_norm(x, w_norm, eps, W, cs, H, Hkv, dtype, fault=None, hot=None):
    """norm-fold q|k|v: a = RMSNorm(x), y = (a W^T).to(T), q / k rotated and rounded, v = y; -> q [rows, H, 128], k, v [rows, Hkv, 128]"""
    a = rmsnorm(x, w_norm, eps, dtype, fault, hot)
    y = rounded(a @ W.t(), dtype).view(x.shape[0], H + 2 * Hkv, 128)
    r = rounded(rope(y[:, :H + Hkv], cs), dtype)
    return r[:, :H], r[:, H:], y[:, H + Hkv:]


def pairs_silu_norm(x, w_norm, eps, Wg, Wu, dtype, fault=None, hot=None):
    """norm-fold gate|up: a = RMSNorm(x), silu(gate.to(T)).to(T) * up.to(T), rounded"""
    a = rmsnorm(x, w_norm, eps, dtype, fault, hot)
    g, u = rounded(a @ Wg.t(), dtype), rounded(a @ Wu.t(), dtype)
    return rounded(rounded(g / (1.0 + torch.exp(-g)), dtype) * u, dtype)


def sum_partials_bias(parts, bias, dtype):
    """the EAGLE head's fc epilogue: (sum of fp32 partials + bias), rounded once"""
    s = parts.sum(0)
    return rounded(s if bias is None else s + bias, dtype)


def grid_values(rng, shape, step=2.0 ** -14, bound=4.0):
    """float64 multiples of `step` below `bound` in magnitude: up to 12 of them (and a bias on a 2^-7 grid) add up EXACTLY in fp32
    (< 2^24 steps), so a sum of partials has one correct value and the only rounding is the one to T"""
    return torch.from_numpy(np.round(rng.uniform(-bound, bound, shape) / step) * step)


# ---- planting -----------------------------------------------------------------------------------------------------------------------------
class Plan:
    """per row: kind[r], hot[r] (first column of the planted window, -1 if none); eps and the seam windows it covers"""

    def __init__(self, kinds, hot, eps):
        self.kind, self.hot, self.eps = list(kinds), list(hot), eps

    def rows(self, kinds):
        return [r for r, k in enumerate(self.kind) if k in kinds]


def seam_tiles(tiles):
    """tiles of the [hidden / 16][16] sums of squares where norm_issue / norm_finish go wrong: 0, the last, both sides of every round of
    ROUND_TILES tiles (32 k - 1 is the p = 31 share norm_finish adds last)"""
    c = [0, tiles - 1]
    for k in range(1, (tiles + ROUND_TILES - 1) // ROUND_TILES):
        c += [ROUND_TILES * k - 1, ROUND_TILES * k]
    return sorted(set(t for t in c if 0 <= t < tiles))


def vector_windows(hidden, threads):
    """k_rmsnorm: 16-column windows that straddle two threads' 8-element vectors (start 8 mod 16), the first and the last columns, and
    (hidden > 8 x threads) the seam between a thread's first and second vector"""
    c = [0, 8, hidden - TILE, hidden // 2 - 8]
    if hidden > 8 * threads:
        c += [8 * threads - 8, 8 * threads]
    return sorted(set(x for x in c if 0 <= x <= hidden - TILE))


def plant(rng, rows, hidden, dtype, eps, windows=(), kinds=None):
    """planted rows x (float64, rounded to T) and their Plan; tile rows take the windows (first columns) in order, cyclically"""
    kinds = list(kinds) if kinds is not None else [PATTERN[r % 8] for r in range(rows)]
    windows = list(windows) or [0, hidden - TILE]
    x = torch.zeros((rows, hidden), dtype=F64)
    hot = [-1] * rows
    nt = 0
    for r, kind in enumerate(kinds):
        band = 10.0 ** (rng.uniform(-2, -1) if r % 2 == 0 else rng.uniform(1, 2))
        v = torch.from_numpy(rng.standard_normal(hidden))
        if kind == "spread":
            x[r] = v / v.pow(2).mean().sqrt() * band
        elif kind == "tile":
            c = windows[nt % len(windows)]
            nt += 1
            hot[r] = c
            amp = math.sqrt(19.0 * (hidden - TILE) / TILE)         # 16 amp^2 = 19 (hidden - 16): 95 % of the energy in the window
            v[c:c + TILE] *= amp
            x[r] = v / v.pow(2).mean().sqrt() * band
        elif kind == "tiny":
            x[r] = v / v.pow(2).mean().sqrt() * math.sqrt(eps / 8)
        elif kind == "massive":
            assert r % 2 == 1, "a massive row's partner must be a low-band row"
            i, j = rng.choice(hidden, 2, replace=False)
            v[i], v[j] = 2000.0, -2000.0
            x[r] = v
        elif kind != "zero":
            raise ValueError(kind)
    return rounded(x, dtype), Plan(kinds, hot, eps)


def norm_weight(rng, hidden, dtype):
    """+-[0.5, 4], random signs, rounded"""
    s = np.where(rng.random(hidden) < 0.5, -1.0, 1.0)
    return rounded(torch.from_numpy(s * rng.uniform(0.5, 4.0, hidden)), dtype)


# ---- bars and self checks -----------------------------------------------------------------------------------------------------------------
def ulp_bar(want, dtype):
    return ULP_BAR * ulp(want, dtype)


def row_bar(want, dtype):
    """tol * max(|want_row|_inf, FLOOR) over the last dimension (per (row, head) for [rows, heads, 128], per row for [rows, N])"""
    return TOL[dtype] * want.abs().amax(-1, keepdim=True).clamp(min=FLOOR)


def row_miss(wrong, want, bar):
    """per row: max over its elements of |wrong - want| / bar (NaN or inf -> inf)"""
    e = torch.nan_to_num((wrong - want).abs() / bar, nan=float("inf"), posinf=float("inf"))
    return e.reshape(e.shape[0], -1).amax(-1)


def fold_miss(wrong, want, dtype):
    """the fold kernels' bars, per (row, head) / per row of the last dimension, as multiples (<= 1 passes), worst per row:
    |err|_inf <= tol max(|want|_inf, FLOOR)  and  |err|_2 <= tol max(|want|_2, FLOOR sqrt(n)).  The second sees a fault that moves every
    element of a heavy-tailed row (silu(gate) * up) by a fraction of its typical size, not of its largest element"""
    n = want.shape[-1]
    d = torch.nan_to_num(wrong - want, nan=float("inf"), posinf=float("inf"), neginf=float("inf")).abs()
    inf = d.amax(-1) / (TOL[dtype] * want.abs().amax(-1).clamp(min=FLOOR))
    l2 = d.pow(2).sum(-1).sqrt() / (TOL[dtype] * want.pow(2).sum(-1).sqrt().clamp(min=FLOOR * math.sqrt(n)))
    m = torch.maximum(inf, l2)
    return m.reshape(m.shape[0], -1).amax(-1)


def mismatch(got, want):
    """fraction of elements that differ from the reference (NaN counts)"""
    return float((~(got == want)).double().mean())


def self_check_max(plan, want, wrongs, bar, label="", factor=MISS):
    """every max-error fault: its targeted rows miss the bar by >= MISS at the worst and >= ROW_MISS each; faults with no targeted row in
    this plan are skipped (a single row has no partner).  `bar`: an element-wise bar, or a function (wrong, want) -> per-row misses.
    -> the faults checked"""
    done = []
    for fault, wrong in wrongs.items():
        tgt = [r for r in plan.rows(TARGETS[fault]) if fault != "other_row" or int(partner(len(plan.kind))[r]) != r]
        if not tgt:
            continue
        m = (bar(wrong, want) if callable(bar) else row_miss(wrong, want, bar)).cpu()[tgt]
        assert float(m.max()) >= factor and float(m.min()) >= ROW_MISS, \
            f"{label}: fault {fault} would miss the bar by only {float(m.max()):.1f}x (rows {tgt}, per row {[round(float(v), 1) for v in m]})"
        done.append(fault)
    return done


def self_check_fraction(want, wrongs, cap=FRAC_CAP, label=""):
    """every rounding fault changes >= FRAC_MISS x cap of the elements"""
    for fault, wrong in wrongs.items():
        f = mismatch(wrong, want)
        assert f >= FRAC_MISS * cap, f"{label}: rounding fault {fault} changes only {f:.4f} of the elements (cap {cap})"


def rmsnorm_faults(x, w, eps, dtype, plan):
    """the RMSNorm references with each fault -> ({max-error fault: out}, {rounding fault: out})"""
    mx = {f: rmsnorm(x, w, eps, dtype, f, plan.hot) for f in MAX_FAULTS}
    rd = {f: rmsnorm(x, w, eps, dtype, f, plan.hot) for f in ROUNDING_FAULTS}
    return mx, rd
