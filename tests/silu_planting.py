"""Inputs that hold the SiLU epilogues (k_silu_mul, k_gemm_skinny<EPI 1>, k_gemm_pairs_silu with and without NORM, moe_side_store<GU>) by
equality over the WHOLE gate range of the model dtype T, their float64 reference and named faults (numpy + torch only; no product import).

The contract is HF's act_fn(gate) * up with gate, up, silu(gate) and the product each rounded once to T:

    g_T = round_T(exact gate sum)    u_T = round_T(exact up sum)    s_T = round_T(silu_ref(g_T))    out = round_T(s_T * u_T)

  silu_ref     g / (1 + exp(-g)) in float64 where -g <= log(FLT_MAX) = 88.7228...; -0 for finite g below that (fp32 exp(-g) overflows and
               g / inf = -0, as in HF's fp32 evaluation; bf16 could hold the float64 value); +inf -> +inf, -inf -> NaN, NaN -> NaN.
  gates        every bit pattern of T (`sweep`); the GEMM sites take the finite ones (`finite_runs`), the direct entry point all 2^16.
  margin       an fp32 evaluation of the expression does not land on the float64 value, so a gate is NEAR-TIE when silu_ref(g) lies within
               MARGIN_ULPS = 32 fp32 ulps of the midpoint of the two adjacent T values around it; an fp32 ulp is 2^(floor(log2 |s|) - 23),
               floored at 2^-149.  Error model of any fp32 evaluation through exp2(x * log2 e): the rounded argument x * log2 e is at most
               127 in magnitude (beyond it the exponential is 0 or inf in fp32), so rounding it to fp32 moves it by at most 2^-18 (half an
               ulp of a number below 128, plus the half ulp of log2 e's own rounding times x: 2^-18 in all) -- a relative error of
               2^-18 ln 2 in the exponential, under 22 fp32 ulps, and it reaches silu(g) = g * sigmoid(g) in full only where
               sigmoid(-g) ~ 1.  The exponential instruction, the addition of 1 and the division add about one ulp each, and the rest of
               the 32 is slack.  Off the margin every such evaluation rounds to ONE T value, which the test demands; a near-tie gate is
               still launched and must give one of the two adjacent T values (`Ref.alt`).  `near_tie_share` asserts from the reference
               alone that near-tie gates are at most 1 % of the finite nonzero gates (recorded: fp16 332 of 63486, 0.52 %; bf16 268 of
               65278, 0.41 %, most of the bf16 ones tiny gates where silu(g) = g / 2 sits exactly on a subnormal tie).
  up values    `up_pool`: +-1 and full-width odd mantissas at every exponent of [2^-6, 2^6), both signs; fp16 adds values at 2^9, 2^12 and
               2^15 that overflow the product (the result must be +-inf, not 65504) and at 2^-14, 2^-11, 2^-8 that push it into fp16's
               subnormals (one round-to-nearest-even from the exact fp32 product).  `check_products` asserts that every s_T * u_T, for
               both T values a near-tie gate may give, is exact in fp32: zero, or of magnitude >= 2^-126 and finite.  bf16 has fp32's
               exponent range, so there a gate's up values are scaled by 2^k, k chosen from the gate's own silu values, to keep the
               product in that range (`lift`); the last cast is then the only rounding of the product.
  two-hot      the GEMM sites take the gate as a sum.  K is cut into mains [0, inter), ups [inter, inter + 256) and residues behind them.
               Gate weight row n is +1 at main column a_n and, where a_n has one, +1 at a's residue column; up weight row n is +-1 at
               a_n's up column; everything else 0.  a_n is a permutation per expert / per draw and the sign a draw per row, so a gate / up
               swap, a wrong row, a wrong column or another expert each lands on another value.  The mains of a row of h carry the gates,
               `grp` = inter / 256 neighbouring mains share an up column (gates of one run of `grp` consecutive bit patterns: the one
               power of two of `lift` serves them all), and the residue columns carry 0 (sweep launches) or +-3/8 ulp_T(main) (rounding
               launches): the fp32 sum main + residue is exact (asserted) but no T value, so a launch that does not round the gate
               computes silu of another number -- `check_rounding` asserts that this changes s_T for at least a quarter of the gates that
               carry a residue.  Main and residue columns lie in different 256-k chunks, so the sum crosses a chunk boundary.  No inf or
               NaN enters a GEMM operand (0 * inf would poison a row).  Runs are dealt round the rows (run j to row j mod rows), so
               every row meets the whole range, tiny and huge gates alike.
  formats      a weight of +-1 or 0 exists in all five weight formats: the model dtype, MXFP4 (code +-1.0, e8m0 2^0), INT4 / INT8
               (q - z = +-1 with varied zero points, scale 1) and block FP8 (e4m3 +-1.0, scale 1).  `checkpoint_forms` writes them in the
               conventions gemm_planting / moe_planting / quant_planting restate and asserts, through the dequantisers restated here, that
               every format's dequantised weight is exactly the planted matrix.

Faults (`faulty`): silu_not_rounded, gate_not_rounded, up_not_rounded, exp_in_T, exp_sign, gate_up_swapped, last_cast_truncates,
last_cast_saturates (fp16), no_overflow_zero (NaN where exp(-g) overflows), exp_of_plus_g_overflow (NaN for g > 88.7), other_activation
(x sigmoid(1.702 x)).  `self_check` requires of each that it changes at least 5 % of the compared outputs it touches and at least 100 of
them (a floor against vacuous faults; under equality one changed output fails the GPU test); an output counts as changed only if the
fault's value is NEITHER of the values the test accepts."""
import math

import numpy as np
import torch

import gemm_planting as G
import moe_planting as MP
from gemm_planting import KC, MANT, as_t, rounded, truncated

F64 = torch.float64
DTYPES = G.DTYPES
LOG_FLT_MAX = math.log(float(np.finfo(np.float32).max))          # 88.7228...: exp(-g) overflows fp32 for -g above it
MARGIN_ULPS = 32
NEAR_TIE_CAP = 0.01
EMIN = {torch.float16: -14, torch.bfloat16: -126}                 # exponent of the smallest normal value
UP_COLS = 256
CURVE = (2.0 ** -6, 32.0)                                         # |g| range in which the curve itself decides the stored value
FAULTS = ("silu_not_rounded", "gate_not_rounded", "up_not_rounded", "exp_in_T", "exp_sign", "gate_up_swapped", "last_cast_truncates",
          "last_cast_saturates", "no_overflow_zero", "exp_of_plus_g_overflow", "other_activation")
MIN_SHARE, MIN_CHANGED = 0.05, 100

# ---- the cases of tests/test_gpu_silu_curve.py (tests/test_silu_planting_cpu.py builds every one of them) ------------------------------------
DIRECT_ROWS, DIRECT_INTER = 8, 65536
PARTIALS_ROWS, PARTIALS_INTER, PARTIALS_N = 8, 8192, (1, 3)
DENSE_K, DENSE_INTER = 2048, 1024
DENSE_ROWS = (64, 16, 32, 48)                                    # 64: the whole sweep; the others a strided quarter, phase = their index
NORM_ROWS = (5, 8, 9, 16)
NORM_EPS = 0.5                                                   # ssq = K / 2 in tile 0: mean + eps = 0.5 + 0.5 = 1.0f exactly
MOE_HIDDEN, MOE_INTER, MOE_E, MOE_K = 1024, 512, 4, 2
MOE_KINDS = ("rows64", "rows16")
WIDE_ROWS = 192
FORMATS = (None, "mxfp4", "int4g128", "int8g128", "fp8b128")


# ---- the model dtype's values -----------------------------------------------------------------------------------------------------------------
def sweep(dtype):
    """float64 [65536]: the value of every bit pattern of `dtype`, index = the pattern"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).to(F64)


def bits_of(x, dtype):
    """int64 bit pattern of float64 T values"""
    return x.to(dtype).view(torch.int16).to(torch.int64) & 0xFFFF


_VALUES = {}


def t_values(dtype):
    """float64, ascending: every finite value of `dtype` once (+-0 merged)"""
    if dtype not in _VALUES:
        v = sweep(dtype)
        _VALUES[dtype] = torch.unique(v[torch.isfinite(v)])
    return _VALUES[dtype]


def ulp_t(v, dtype):
    """spacing of `dtype` at |v| (float64; the subnormal spacing below the smallest normal value)"""
    _, e = torch.frexp(v.abs())
    return torch.ldexp(torch.ones_like(v), (e - 1).clamp(min=EMIN[dtype]) - MANT[dtype])


def ulp_f32(s):
    """2^(floor(log2 |s|) - 23), floored at 2^-149 (also for s = 0)"""
    _, e = torch.frexp(s.abs())
    e = torch.where(s == 0, torch.full_like(e, -200), e)
    return torch.ldexp(torch.ones_like(s), (e - 1 - 23).clamp(min=-149))


def differs(a, b):
    """the test's inequality: stored values differ (+-0 equal), or only one of them is NaN"""
    return ~((a == b) | (torch.isnan(a) & torch.isnan(b)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def silu_ref(g):
    s = g / (1.0 + torch.exp(-g))
    return torch.where(torch.isfinite(g) & (-g > LOG_FLT_MAX), torch.full_like(g, -0.0), s)


def brackets(s, dtype):
    """(lo, hi): adjacent values of `dtype` with lo <= s <= hi for finite s within the dtype's range; lo == hi == s where s is a value"""
    vals = t_values(dtype)
    i = torch.searchsorted(vals, s.contiguous()).clamp(max=len(vals) - 1)
    hi = vals[i]
    return torch.where(hi == s, hi, vals[(i - 1).clamp(min=0)]), hi


class Curve:
    """per bit pattern of the gate: s_T, the other admissible T value `alt` (= s_T off the margin) and the near-tie mask"""

    def __init__(self, dtype):
        g = sweep(dtype)
        s = silu_ref(g)
        fin = torch.isfinite(s)
        assert bool((s[fin].abs() <= torch.finfo(dtype).max).all())                   # |silu(g)| <= |g|
        sf = torch.where(fin, s, torch.zeros_like(s))
        lo, hi = brackets(sf, dtype)
        self.s_T = rounded(s, dtype)
        self.near = fin & (lo != hi) & ((sf - (lo + hi) / 2.0).abs() <= MARGIN_ULPS * ulp_f32(sf))
        assert bool(((self.s_T == lo) | (self.s_T == hi))[fin].all())
        self.alt = torch.where(self.near, torch.where(self.s_T == lo, hi, lo), self.s_T)
        self.gate, self.silu = g, s


_CURVES = {}


def curve(dtype):
    if dtype not in _CURVES:
        _CURVES[dtype] = Curve(dtype)
    return _CURVES[dtype]


def near_tie_share(dtype):
    """(share, count, gates): near-tie gates among the finite nonzero gates; asserted <= NEAR_TIE_CAP"""
    c = curve(dtype)
    live = torch.isfinite(c.gate) & (c.gate != 0)
    n, tot = int((c.near & live).sum()), int(live.sum())
    assert not bool((c.near & ~live).any()) and n / tot <= NEAR_TIE_CAP, (dtype, n, tot)
    return n / tot, n, tot


class Ref:
    """what a launch must store for exact gate / up sums (float64, any shape): `want`; `alt` differs from it only where the gate is
    near-tie (`near`), and there either value is right"""

    def __init__(self, gate, up, dtype):
        c = curve(dtype)
        self.g_T, self.u_T = rounded(gate, dtype), rounded(up, dtype)
        i = bits_of(self.g_T, dtype)
        self.s_T, self.s_alt, self.near = c.s_T[i], c.alt[i], c.near[i]
        self.want, self.alt = rounded(self.s_T * self.u_T, dtype), rounded(self.s_alt * self.u_T, dtype)


def faulty(gate, up, dtype, fault):
    """the stored tensor of a launch with one named fault"""
    if fault == "gate_up_swapped":
        gate, up = up, gate
    g = gate if fault == "gate_not_rounded" else rounded(gate, dtype)
    u = up if fault == "up_not_rounded" else rounded(up, dtype)
    fin = torch.isfinite(g)
    nan = torch.full_like(g, float("nan"))
    if fault == "exp_in_T":
        s = g / (1.0 + rounded(torch.exp(-g), dtype))
    elif fault == "exp_sign":
        s = g / (1.0 + torch.exp(g))
    elif fault == "other_activation":
        s = g / (1.0 + torch.exp(-1.702 * g))
    elif fault == "no_overflow_zero":
        s = torch.where(fin & (-g > LOG_FLT_MAX), nan, silu_ref(g))
    elif fault == "exp_of_plus_g_overflow":
        s = torch.where(fin & (g > LOG_FLT_MAX), nan, silu_ref(g))
    else:
        s = silu_ref(g)
    if fault == "silu_not_rounded":                               # the fp32 value goes into the product, the fp32 product into the cast
        return rounded((s.float().double() * u).float().double(), dtype)
    p = rounded(s, dtype) * u
    if fault == "last_cast_truncates":
        return truncated(p, dtype)
    out = rounded(p, dtype)
    if fault == "last_cast_saturates":
        m = torch.finfo(dtype).max
        out = torch.where(torch.isinf(out), out.sign() * m, out)
    return out


def touched(gate, up, dtype, fault):
    """the compared outputs a fault can reach"""
    g_T, u_T = rounded(gate, dtype), rounded(up, dtype)
    fin = torch.isfinite(g_T) & torch.isfinite(u_T)
    on_curve = fin & (g_T.abs() >= CURVE[0]) & (g_T.abs() <= CURVE[1])
    if fault == "gate_not_rounded":
        return on_curve & (g_T != gate)
    if fault == "up_not_rounded":
        return fin & (u_T != up)
    if fault == "last_cast_saturates":
        return torch.isinf(Ref(gate, up, dtype).want) & fin
    if fault == "no_overflow_zero":
        return fin & (-g_T > LOG_FLT_MAX)
    if fault == "exp_of_plus_g_overflow":
        return fin & (g_T > LOG_FLT_MAX)
    return on_curve


def self_check(gate, up, dtype, need):
    """every fault of `need` changes >= MIN_SHARE of the outputs it touches and >= MIN_CHANGED of them; returns {fault: (changed, touched)}"""
    ref = Ref(gate, up, dtype)
    out = {}
    for f in need:
        assert f in FAULTS, f
        wrong, t = faulty(gate, up, dtype, f), touched(gate, up, dtype, f)
        changed = int((differs(wrong, ref.want) & differs(wrong, ref.alt) & t).sum())
        n = int(t.sum())
        assert n > 0 and changed >= MIN_CHANGED and changed >= MIN_SHARE * n, (f, dtype, changed, n)
        out[f] = (changed, n)
    return out


# ---- gates and up values ----------------------------------------------------------------------------------------------------------------------
def finite_runs(dtype, grp, curve_only=False):
    """float64 [R, grp]: the finite gates in bit-pattern order (+0 .. +max, -0 .. -max), cut into runs of `grp` neighbours; curve_only:
    the runs that lie in CURVE, 2^-6 <= |g| <= 32, where rounding the gate moves silu(g) across roundings of T"""
    v = sweep(dtype)
    v = v[torch.isfinite(v)]
    assert len(v) % grp == 0
    runs = v.view(-1, grp)
    return runs[((runs.abs() >= CURVE[0]) & (runs.abs() <= CURVE[1])).all(1)] if curve_only else runs


def slot_gates(dtype, rows, inter, grp, start=0, stride=1, curve_only=False):
    """float64 [rows, inter]: run (start + floor(stride j)) mod R goes to row j mod rows, slots grp (j div rows) .. + grp - 1"""
    runs = finite_runs(dtype, grp, curve_only)
    j = torch.arange(rows * inter // grp)
    return runs[(start + torch.floor(stride * j.double()).long()) % len(runs)].view(inter // grp, rows, grp).permute(1, 0, 2).reshape(rows, inter)


def up_pool(dtype):
    """float64: +-1, then one full-width odd mantissa per exponent of [2^-6, 2^6) and sign; fp16: + the overflowing and the subnormal-making ones"""
    rng = np.random.default_rng(MANT[dtype])
    m = MANT[dtype]
    exps = list(range(-6, 6)) + ([9, 12, 15, -14, -11, -8] if dtype == torch.float16 else [])
    vals = [1.0, -1.0]
    for e in exps:
        for sign in (1.0, -1.0):
            mant = 2 ** m + 2 * int(rng.integers(0, 2 ** (m - 1))) + 1                # odd, all m + 1 bits in use
            vals.append(sign * mant * 2.0 ** (e - m))
    pool = as_t(np.array(vals))
    assert torch.equal(rounded(pool, dtype), pool) and bool(torch.isfinite(pool).all()) and pool.abs().max().item() <= torch.finfo(dtype).max
    return pool


def lift(gates, dtype):
    """float64 [..., 1] power of two per run of gates [..., grp] that keeps s_T * u inside fp32's normal range for every |u| in [2^-6, 2^6):
    1 for fp16 (22-bit products between 2^-38 and 2^32 are always exact); bf16: 2^k from the run's own silu values"""
    if dtype == torch.float16:
        return torch.ones(gates.shape[:-1] + (1,), dtype=F64)
    c = curve(dtype)
    i = bits_of(gates, dtype)
    mags = torch.stack((c.s_T[i].abs(), c.alt[i].abs()), dim=-1).flatten(-2)
    big = mags.max(-1).values
    small = torch.where(mags > 0, mags, torch.full_like(mags, float("inf"))).min(-1).values
    small = torch.where(torch.isinf(small), torch.ones_like(small), small)
    big = torch.where(big == 0, torch.ones_like(big), big)
    e_small, e_big = torch.frexp(small)[1] - 1, torch.frexp(big)[1] - 1              # floor(log2)
    up_k, down_k = (-126 + 6 - e_small).clamp(min=0), (127 - 7 - e_big).clamp(max=0)
    assert bool(((up_k == 0) | (down_k == 0)).all())
    return torch.ldexp(torch.ones_like(small), up_k + down_k)[..., None]


def check_products(ref, dtype):
    """every s_T * u_T (both admissible s_T) is exact in fp32: zero, or of magnitude >= 2^-126 and finite in fp32"""
    for s in (ref.s_T, ref.s_alt):
        p = s * ref.u_T
        p = p[torch.isfinite(s) & torch.isfinite(ref.u_T)]
        assert torch.equal(p.float().double(), p), "a product that fp32 does not hold"
        nz = p[p != 0].abs()
        assert nz.min().item() >= 2.0 ** -126 and nz.max().item() <= float(np.finfo(np.float32).max), (nz.min().item(), nz.max().item())


def residues(main, dtype, flip):
    """+-3/8 ulp_T(main) (sign by `flip`), 0 where that is no value of the dtype or main is 0"""
    r = 0.375 * ulp_t(main, dtype) * torch.where(flip, -1.0, 1.0)
    ok = (rounded(r, dtype) == r) & (main != 0) & torch.isfinite(main)
    return torch.where(ok, r, torch.zeros_like(r))


def check_rounding(gate, dtype):
    """the rounding launches: every exact gate sum is an fp32 value; of those in CURVE that are no T value at least a quarter give
    another s_T when the gate is not rounded (outside CURVE silu(g) is g, g / 2 or 0 up to one rounding, and rounding the gate first or
    the result alone stores the same value).  Returns that share."""
    assert torch.equal(gate.float().double(), gate)
    off = (rounded(gate, dtype) != gate) & (gate.abs() >= CURVE[0]) & (gate.abs() <= CURVE[1])
    assert bool(off.any())
    g = gate[off]
    share = differs(rounded(silu_ref(g), dtype), rounded(silu_ref(rounded(g, dtype)), dtype)).double().mean().item()
    assert share >= 0.25, (dtype, share)
    return share


# ---- the direct entry point -------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def direct_case(dtype):
    """samd_silu_mul on T inputs: row m = the sweep rotated by m elements (every gate meets each of the 8 lanes of a vector), inf and NaN
    included; ups from the pool, another one per row"""
    pool, v = up_pool(dtype), sweep(dtype)
    i = (torch.arange(DIRECT_INTER)[None, :] + torch.arange(DIRECT_ROWS)[:, None]) % 65536
    gate = v[i]
    fin = torch.where(torch.isfinite(gate), gate, torch.ones_like(gate))
    up = pool[(i + 5 * torch.arange(DIRECT_ROWS)[:, None]) % len(pool)] * lift(fin[..., None], dtype)[..., 0]
    assert torch.equal(rounded(up, dtype), up) and bool(torch.isfinite(up).all()) and bool((up != 0).all())
    lanes = (torch.arange(65536)[None, :] - torch.arange(DIRECT_ROWS)[:, None]) % 8       # the lane of pattern p in row m
    assert bool((lanes.sort(0).values == torch.arange(8)[:, None]).all())                   # every pattern in every lane
    ref = Ref(gate, up, dtype)
    check_products(ref, dtype)
    return Case(dtype=dtype, gate=gate, up=up, ref=ref)


def partials_case(dtype, n_partials):
    """samd_silu_mul on fp32 partials [n][rows][2 inter]: the finite sweep with a residue on EVERY gate and EVERY up, split over the
    partials so that every partial sum in any order is exact in fp32 (main, 1/4 ulp, 1/8 ulp)"""
    rows, inter = PARTIALS_ROWS, PARTIALS_INTER
    gate_m = slot_gates(dtype, rows, inter, 1)
    pool = up_pool(dtype)
    t, m = torch.arange(inter)[None, :], torch.arange(rows)[:, None]
    up_m = pool[(7 * t + 3 * m) % len(pool)] * lift(gate_m[..., None], dtype)[..., 0]
    parts = torch.zeros((n_partials, rows, 2 * inter), dtype=F64)
    main = torch.cat((gate_m, up_m), dim=1)
    r = residues(main, dtype, ((t + m) % 2 == 1).repeat(1, 2))
    if n_partials == 1:
        parts[0] = main + r
    else:
        parts[0], parts[1], parts[2] = main, r / 1.5, r / 3.0              # 1/4 and 1/8 ulp, exactly
    assert torch.equal(parts.float().double(), parts)
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0))[:1 if n_partials == 1 else 3]:      # any order of adding is exact
        acc = torch.zeros_like(main)
        for k in order[:n_partials]:
            acc = (acc + parts[k]).float().double()
        assert torch.equal(acc, main + r)
    exact = main + r
    gate, up = exact[:, :inter], exact[:, inter:]
    ref = Ref(gate, up, dtype)
    # (main - 3/8 ulp of a power of two rounds to the value below it: the spacing halves there)
    assert bool((ref.g_T == gate_m).double().mean() > 0.99) and bool((rounded(up, dtype) != up).double().mean() > 0.9)
    check_products(ref, dtype)
    share = check_rounding(gate, dtype)
    return Case(dtype=dtype, parts=parts, gate=gate, up=up, ref=ref, rounding_share=share)


# ---- the two-hot planting ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """columns of h: mains [0, inter), ups [inter, inter + 256), residues behind; main a shares up column a div grp with its neighbours and
    has the residue column res_of[a] (-1: none)"""

    def __init__(self, K, inter):
        self.K, self.inter, self.grp = K, inter, inter // UP_COLS
        n_res = K - inter - UP_COLS
        assert inter % KC == 0 and n_res >= KC and n_res % UP_COLS == 0 and n_res <= inter and K % KC == 0
        per = n_res // UP_COLS                                    # residue columns per run
        a = np.arange(inter)
        self.up_of = inter + a // self.grp
        self.res_of = np.where(a % self.grp < per, inter + UP_COLS + (a // self.grp) * per + a % self.grp, -1)
        held = self.res_of[self.res_of >= 0]
        assert len(set(held.tolist())) == len(held) == n_res and held.max() == K - 1
        assert bool((held // KC != a[self.res_of >= 0] // KC).all())                # main and residue in different chunks


def two_hot_weights(seed, L, experts):
    """(Wg, Wu float64 [experts, inter, K], a [experts, inter]): gate row n +1 at main a_n (+1 at its residue column), up row n +-1 at
    a_n's up column; a_n a permutation and the signs a draw per expert"""
    rng = np.random.default_rng(seed)
    Wg, Wu = np.zeros((experts, L.inter, L.K)), np.zeros((experts, L.inter, L.K))
    a = np.stack([rng.permutation(L.inter) for _ in range(experts)])
    n = np.arange(L.inter)
    for e in range(experts):
        Wg[e, n, a[e]] = 1.0
        has = L.res_of[a[e]] >= 0
        Wg[e, n[has], L.res_of[a[e]][has]] = 1.0
        Wu[e, n, L.up_of[a[e]]] = rng.integers(0, 2, L.inter) * 2.0 - 1.0
    assert bool(((Wg != 0).sum(-1) <= 2).all()) and bool(((Wu != 0).sum(-1) == 1).all())
    return as_t(Wg), as_t(Wu), a


def two_hot_rows(dtype, L, rows, rounding, start=0, stride=1):
    """h float64 [rows, K]: gates in the mains, pool values (lifted per run) in the ups, 0 or +-3/8 ulp in the residues"""
    # (a rounding launch draws its gates from CURVE alone, every one of them as often as the slots allow, each time with another up)
    gates = slot_gates(dtype, rows, L.inter, L.grp, start, 1 if rounding else stride, rounding)
    pool = up_pool(dtype)
    c, m = torch.arange(UP_COLS)[None, :], torch.arange(rows)[:, None]
    ups = pool[(7 * c + 3 * m + start) % len(pool)] * lift(gates.view(rows, UP_COLS, L.grp), dtype)[..., 0]
    h = torch.zeros((rows, L.K), dtype=F64)
    h[:, :L.inter], h[:, L.inter:L.inter + UP_COLS] = gates, ups
    if rounding:
        has = torch.from_numpy(L.res_of >= 0)
        t = torch.arange(L.inter)[None, :]
        r = residues(gates, dtype, (t + m) % 2 == 1)
        h[:, torch.from_numpy(L.res_of[L.res_of >= 0])] = r[:, has]
    assert torch.equal(rounded(h, dtype), h) and bool(torch.isfinite(h).all())       # no inf or NaN in a GEMM operand
    return h


def covers_finite_sweep(cases, dtype):
    """the rounded gates of `cases` together are every finite bit pattern of the dtype"""
    seen = torch.zeros(65536, dtype=torch.bool)
    for c in cases:
        seen[bits_of(c.ref.g_T[torch.isfinite(c.ref.g_T)], dtype)] = True
    seen[0x8000] |= seen[0]                                       # (a sum of products with zeros in it is +0: -0 is the direct case's)
    return bool((seen == torch.isfinite(sweep(dtype))).all())


def _finish(c, dtype, rounding):
    c.ref = Ref(c.gate, c.up, dtype)
    check_products(c.ref, dtype)
    assert torch.equal(c.gate.float().double(), c.gate) and torch.equal(rounded(c.up, dtype), c.up)
    c.rounding_share = check_rounding(c.gate, dtype) if rounding else None
    if not rounding:
        assert torch.equal(rounded(c.gate, dtype), c.gate)
    return c


def dense_plan(rows):
    """(start, stride) of a dense launch: the whole sweep at 64 rows; a strided quarter with phase = the row count's index otherwise"""
    return (0, 1) if rows == 64 else (DENSE_ROWS.index(rows), 4)


def dense_case(dtype, rows, rounding, plan=None, seed=0):
    """samd_gemm_skinny_silu / samd_gemm_pairs_silu (/ _norm, where only rows < `rows` of the 16 count): Case(h [rows, K], Wg, Wu
    [inter, K], gate, up [rows, inter], ref)"""
    L = Layout(DENSE_K, DENSE_INTER)
    Wg, Wu, a = two_hot_weights(MP.seed_of(MANT[dtype], rows, seed, 41), L, 1)
    h = two_hot_rows(dtype, L, rows, rounding, *(plan or dense_plan(rows)))
    c = Case(dtype=dtype, rows=rows, L=L, h=h, Wg=Wg[0], Wu=Wu[0], a=a[0], gate=h @ Wg[0].t(), up=h @ Wu[0].t())
    return _finish(c, dtype, rounding)


def norm_plan(rows, dtype):
    """(start, stride) of the NORM entry point's launches: the (fractional) stride that spreads rows x inter slots evenly over the whole
    sweep (12.4 at 5 rows, 3.9 at 16), the start another one per row count"""
    L = Layout(DENSE_K, DENSE_INTER)
    return NORM_ROWS.index(rows), len(finite_runs(dtype, L.grp)) / (rows * L.inter // L.grp)


def identity_case(dtype, rows):
    """the precondition of the NORM entry point: gates 24 .. 63 and up = 1 -- silu(g) = g, the output is +-g bit for bit if the launch's
    own scale (rsqrt(mean + eps) with mean + eps = 1.0f, norm weight 1) is exactly 1"""
    L = Layout(DENSE_K, DENSE_INTER)
    Wg, Wu, a = two_hot_weights(MP.seed_of(MANT[dtype], rows, 43), L, 1)
    h = torch.zeros((rows, L.K), dtype=F64)
    h[:, :L.inter] = 24.0 + (torch.arange(L.inter)[None, :] + 3 * torch.arange(rows)[:, None]) % 40
    h[:, L.inter:L.inter + UP_COLS] = 1.0
    gate, up = h @ Wg[0].t(), h @ Wu[0].t()
    G.assert_silu(gate, up.abs(), dtype)
    want = gate * up
    assert torch.equal(Ref(gate, up, dtype).want, want)
    return Case(dtype=dtype, rows=rows, L=L, h=h, Wg=Wg[0], Wu=Wu[0], want=want)


def norm_ssq(K):
    """fp32 [K / 16][16] tile-major sums of squares whose total is K (1 - NORM_EPS), all of it in tile 0"""
    s = torch.zeros((K // 16, 16), dtype=torch.float32)
    s[0] = K * (1.0 - NORM_EPS)
    assert np.float32(np.float32(s[0, 0].item()) * np.float32(1.0 / K)) + np.float32(NORM_EPS) == np.float32(1.0)
    return s


# ---- mixture of experts -----------------------------------------------------------------------------------------------------------------------
def moe_routing(kind):
    """(idx int32 [rows, 2], rows): rows64 -- every row two distinct experts, all four in use; rows16 -- expert 3 empty and expert 2 holding
    a single pair; wide -- 192 rows, lists of 130, 96, 96 and 62 pairs (three, two, two tiles and one partly filled tile)"""
    if kind == "rows64":
        r = np.arange(64)
        idx = np.stack([r % 4, (r % 4 + 1 + (r // 4) % 3) % 4], axis=1)
    elif kind == "rows16":
        idx = np.stack([np.zeros(16, dtype=np.int64), np.ones(16, dtype=np.int64)], axis=1)
        idx[0, 1] = 2
    elif kind == "wide":
        r = np.arange(WIDE_ROWS)
        idx = np.stack([np.where(r < 130, 0, 3), 1 + r % 2], axis=1)
    else:
        raise ValueError(kind)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    lists = MP.python_lists(idx, len(idx), MOE_E)
    counts = [len(lists.get(e, ())) for e in range(MOE_E)]
    assert bool((idx[:, 0] != idx[:, 1]).all()) and sum(counts) == idx.size
    assert {"rows64": min(counts) > 0, "rows16": counts == [16, 15, 1, 0], "wide": counts == [130, 96, 96, 62]}[kind], counts
    return idx, lists


def moe_plans(kind):
    """[(start, stride)] of the launches that make up the sweep: two halves at 64 rows (a row's two experts read the same h row, so a
    launch holds 64 x 512 different gates), one launch of every 7th run at 16 rows, one launch of the whole sweep at 192 rows"""
    runs = 64 * MOE_INTER // (MOE_INTER // UP_COLS)
    return {"rows64": [(0, 1), (runs, 1)], "rows16": [(3, 7)], "wide": [(0, 1)]}[kind]


def moe_weights(dtype):
    L = Layout(MOE_HIDDEN, MOE_INTER)
    Wg, Wu, a = two_hot_weights(MP.seed_of(MANT[dtype], 47), L, MOE_E)
    assert all(bool((a[e] != a[f]).mean() > 0.9) for e in range(MOE_E) for f in range(e))
    return L, Wg, Wu


def moe_case(dtype, kind, rounding, plan, weights=None):
    """Case(h [rows, hidden], Wg, Wu [E, inter, hidden], idx, lists, gate, up [rows k, inter] of the pair p = row k + slot, ref)"""
    L, Wg, Wu = weights or moe_weights(dtype)
    idx, lists = moe_routing(kind)
    rows = len(idx)
    h = two_hot_rows(dtype, L, rows, rounding, *plan)
    gate, up = torch.empty((rows * MOE_K, L.inter), dtype=F64), torch.empty((rows * MOE_K, L.inter), dtype=F64)
    for e, lst in lists.items():
        src = h[[p // MOE_K for p in lst]]
        gate[lst], up[lst] = src @ Wg[e].t(), src @ Wu[e].t()
    c = Case(dtype=dtype, kind=kind, rows=rows, L=L, h=h, Wg=Wg, Wu=Wu, idx=idx, lists=lists, gate=gate, up=up)
    return _finish(c, dtype, rounding)


# ---- weight formats ---------------------------------------------------------------------------------------------------------------------------
E4M3_ONE = 0x38                                                  # e4m3fn 1.0: exponent field 7 (bias 7), mantissa 0; sign in bit 7


def dequant_int(q, z, s, four_bit):
    """(q - z) * s with one zero point and scale per 128 along k; 4-bit codes two per byte, low nibble = the even element"""
    if four_bit:
        q = np.stack([q & 15, q >> 4], axis=-1).reshape(q.shape[:-1] + (2 * q.shape[-1],))
    return (q.astype(np.float64) - z.astype(np.float64).repeat(128, axis=-1)) * s.repeat(128, axis=-1)


def dequant_fp8(q, s):
    """e4m3fn byte value times the scale of its 128 x 128 block (the bytes used here: 0, +-1.0)"""
    v = np.select([q == 0, q == E4M3_ONE, q == (E4M3_ONE | 0x80)], [0.0, 1.0, -1.0], np.nan)
    return v * s.astype(np.float64).repeat(128, axis=-2).repeat(128, axis=-1)


def checkpoint_forms(W):
    """{format: arrays} of W float64 [E, N, K] with entries in {-1, 0, 1}, each asserted to dequantise to exactly W:
         mxfp4     q uint8 [E, N, K/2], e8 uint8 [E, N, K/32] (all 127), exps int64 zeros (for moe_planting.encode's callers)
         int4g128  q uint8 [E, N, K/2], z uint8 [E, N, K/128] in 1..14, s float64 ones
         int8g128  q uint8 [E, N, K],   z uint8 [E, N, K/128] in 1..254, s float64 ones
         fp8b128   q uint8 [E, N, K] e4m3fn bytes, s float32 [E, N/128, K/128] ones"""
    Wn = W.numpy()
    E, N, K = Wn.shape
    assert set(np.unique(Wn).tolist()) <= {-1.0, 0.0, 1.0}
    out = {}
    exps = np.zeros((E, N, K // 32), dtype=np.int64)
    q, e8 = MP.encode(Wn, exps, torch.float16)
    assert np.array_equal(MP.decode(q, e8), Wn) and bool((e8 == 127).all())
    out["mxfp4"] = dict(q=q, e8=e8, exps=exps)
    n, g = np.arange(N)[None, :, None], np.arange(K // 128)[None, None, :]
    for name, four, z in (("int4g128", True, 1 + (n + g) % 14), ("int8g128", False, 1 + (37 * n + g) % 254)):
        z = np.broadcast_to(z, (E, N, K // 128)).astype(np.uint8)
        codes = (Wn + z.repeat(128, axis=-1)).astype(np.uint8)
        assert codes.max() <= (15 if four else 255)
        q = np.ascontiguousarray(codes[..., 0::2] | (codes[..., 1::2] << 4)) if four else codes
        s = np.ones((E, N, K // 128))
        assert np.array_equal(dequant_int(q, z, s, four), Wn)
        out[name] = dict(q=q, z=z, s=s)
    q = np.where(Wn == 0, 0, np.where(Wn > 0, E4M3_ONE, E4M3_ONE | 0x80)).astype(np.uint8)
    s = np.ones((E, N // 128, K // 128), dtype=np.float32)
    assert np.array_equal(dequant_fp8(q, s), Wn)
    out["fp8b128"] = dict(q=q, s=s)
    return out


# ---- which faults a case can show ---------------------------------------------------------------------------------------------------------------
CURVE_FAULTS = ("silu_not_rounded", "exp_in_T", "exp_sign", "gate_up_swapped", "last_cast_truncates", "other_activation")
RANGE_FAULTS = ("no_overflow_zero", "exp_of_plus_g_overflow")


def faults_of(dtype, ups_rounded=False):
    """the faults that one GPU test must show: those of the curve, of the ends of the range and of the gate's rounding; the partials
    input (residues on the ups as well) also the up's rounding"""
    ends = RANGE_FAULTS + (("last_cast_saturates",) if dtype == torch.float16 else ())
    return CURVE_FAULTS + ends + ("gate_not_rounded",) + (("up_not_rounded",) if ups_rounded else ())


def direct_faults(dtype):
    """the direct entry point takes T gates: nothing there to round"""
    return tuple(f for f in faults_of(dtype) if f != "gate_not_rounded")


def check_launches(cases, dtype, ups_rounded=False):
    """self_check over the launches of ONE GPU test taken together (its sweep launches and its rounding launches: the test fails if any of
    them stores a wrong value); returns {fault: (changed, touched)}"""
    gate, up = torch.cat([c.gate.reshape(-1) for c in cases]), torch.cat([c.up.reshape(-1) for c in cases])
    return self_check(gate, up, dtype, faults_of(dtype, ups_rounded))
