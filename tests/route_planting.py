"""Planted integer logits for the mixture-of-experts router, its float64 reference, a lane-by-lane model of the kernel's selection and the
named faults that the planted set must expose (numpy + torch only; no product import).

k_moe_route (csrc/gemm_kernels.hip) runs behind samd_moe_route (<= 64 rows) and samd_moe_wide_route (one-pass prefill): one workgroup of
16 waves per row.  Restated from the code:

  logits    wave w computes experts e0 .. e0 + 3 for e0 = 4 w, 4 w + 64, ... (ROUND e0 / 64); an index at or past E is clamped to E - 1
            for the loads and its sum is not stored.  Lane l adds the 16-byte units u = l, l + 64, ... < H / 8 (8 elements each, fmaf in
            fp32, `#pragma unroll 4`), then a 6-step xor tree adds the lanes.
  selection wave 0 alone: expert e sits in lane e % 64, slot e / 64 (4 slots; slots at or past E hold -inf and are skipped).  k times:
            every lane scans its slots in ascending order (`>` replaces, `==` replaces only for a lower expert), a 6-step xor tree
            (offsets 32 .. 1; `ov > bv || (ov == bv && oi < bi)` replaces) leaves the winner in every lane, and the lane that owns it sets
            that slot to -inf.  Lane 0 writes.
  weights   mx = max, se = sum of expf(v - mx) over all E (<= 3 rounded in-lane adds, 6 tree adds), p_j = expf(bv - mx) / se,
            sum_sel = sum of the k p_j in slot order (<= 7 adds), w_j = norm_topk ? p_j / sum_sel : p_j, ONE rounding to the model dtype.
  rows >= *d_n get index -1 and weight 0.

EXACT LOGITS.  h and the router hold integers that the model dtype represents.  Expert e owns column e (COARSE, weight P) and, where
H >= 2 E, column E + e (FINE, weight 1); the other columns carry sparse noise in h (-3 .. 3, at least one element of every 16-byte unit
of every row, at a within-unit position that moves with the row) and in the router (-2 .. 2).  With N[r][e] = the noise part of the dot
product, computed on the host in int64, h[r][e] = (target - N) div P and h[r][E + e] = (target - N) mod P plant any integer target.  P = 32
where there is a fine column: bf16 holds integers up to 256 only, so 256 x 32 reaches the magnitudes (>= 4096) at which neither fp16 (step
4) nor bf16 (step 32) can tell two logits one apart; the fine column supplies the low bits that a power-of-two weight alone cannot.  P = 1
at H < 2 E (H = E = 256: no noise, |target| <= 256).  check_case asserts max_e sum_c |h[r][c]| |W[e][c]| < 2^24 -- every partial sum of
the fp32 fma chain and of the tree is then an integer below 2^24, exact in any order -- and that every planted value survives the cast.
All logits but the deliberately low ones (30 .. 80 below the row's maximum, never selected) lie within 80 of the maximum, so every
probability that counts is a normal fp32 number.

WEIGHTS.  The reference is float64 on the exact logits: softmax over all E, the k selected probabilities, division by their sum when
norm_topk, one rounding (round_to: half-even on the dtype's grid, in numpy).  The kernel does the same in fp32; counting 1 ulp per
rounded operation where 1/2 would do, from the code above: the exponent's argument is an exact integer and expf costs <= 2 ulps; se adds
positive terms of that error with <= 3 in-lane and 6 tree adds: <= 11; p_j = expf / se, one division: <= 2 + 11 + 1 = 14; sum_sel, <= 7
adds of such terms: <= 21; the second division: <= 14 + 21 + 1 = 36 fp32 ulps.  36 <= 48, so the margin is the next power of two, 64: a
weight whose float64 value lies within MARGIN_ULPS fp32 ulps (of the value) of a ROUNDING BOUNDARY of the dtype -- the midpoint of two
neighbouring dtype values -- may store either neighbour (`band`); every other weight is compared by equality.  A weight whose float64
value IS a dtype value (1/E, 1/k for powers of two: the plateaus) is half a dtype ulp from every boundary and never in the band.  At most
BAND_CAP of a case's compared weights may be in the band: a condition on the planted set, asserted from the reference alone in
tests/test_route_planting_cpu.py and again on the GPU (a case that misses it gets another seed in SEEDS, never a wider cap).  One plant
gives way for it: 1/65 lies 63 fp32 ulps from an fp16 boundary, so at E = 65 the plateau over all E is planted as a plateau of k.

FAULTS are flags of the Python model only (model_route); no defective kernel is ever built."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

DTYPES = (torch.float16, torch.bfloat16)
MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126}          # exponent of the smallest normal number
MARGIN_ULPS = 64
BAND_CAP = 0.05
COARSE = 32                                                   # P where the shape has a fine column
BIG_LOGIT = 4096                                              # from here on fp16 steps by 4 and bf16 by 32
LANES, SLOTS, WAVES = 64, 4, 16
NINF = float("-inf")
POISON_IDX = 12345
NO_EXPERT = 0x7fffffff

# (E, k, H, rows_pad, n) of samd_moe_route and what each reaches
ROUTE_SHAPES = (
    (256, 8, 256, 64, 64),       # no noise columns; 32 units: half a wave is idle in the dot product
    (128, 8, 2048, 64, 64),      # the product's own geometry
    (128, 8, 768, 48, 37),       # 96 units: the tail of the unroll by 4; n < rows_pad
    (8, 2, 512, 16, 9),          # fewer experts than lanes, and than waves x 4
    (5, 5, 256, 16, 16),         # k == E; E % 4 != 0: the clamped loads run
    (1, 1, 256, 16, 1),          # the smallest legal E and k
    (65, 8, 512, 32, 32),        # one lane holds a second slot; E % 4 != 0
    (67, 3, 512, 32, 32),        # three lanes do
    (255, 7, 512, 16, 16),       # an unfilled last slot, an odd k
    (192, 4, 512, 16, 16),       # no fourth slot at all
)
# (E, k, H, rows, n) of samd_moe_wide_route + samd_moe_wide_lists
WIDE_SHAPES = ((128, 8, 512, 65, 65), (128, 8, 512, 200, 173), (67, 3, 256, 130, 130))
EMPTY_SHAPE = (67, 3, 512, 32, 0)                             # n = 0: every row -1 / 0, no active expert
# shape -> seed, where the seed that _seed derives from the shape leaves more than BAND_CAP of the weights in the band (none does today)
SEEDS = {}

KINDS = ("spaced", "tie_kth", "tie_above", "plateau_all", "plateau_k", "ramp", "all_negative", "resolution")
PAIR_KINDS = ("same_lane_64", "same_lane_128", "same_lane_192", "neighbour_even", "neighbour_odd", "lanes_31_32", "lanes_0_63", "waves_rounds",
              "first_last")

FAULTS = {
    "tie_to_higher": "ties go to the higher expert, in the lane scan and in the tree",
    "lane_slot_order": "the in-lane scan keeps the later slot on a tie",
    "shuffle_tie_keeps_own": "ov == bv never replaces in the shuffle tree",
    "no_removal_upper_slots": "a winner in slot i >= 1 is not set to -inf: it is picked again",
    "pad_zero": "lanes and slots at or past E hold 0 and take part",
    "last_group_dropped": "the experts of an incomplete group of four are not computed (their logit reads 0)",
    "tail_units_dropped": "the units past a lane's last full group of four steps are skipped",
    "logits_in_dtype": "logits rounded to the model dtype",
    "softmax_over_selected": "the softmax runs over the selected experts only",
    "renorm_always": "renormalised whatever norm_topk says",
    "renorm_never": "never renormalised",
    "weights_rounded_twice": "the probability rounded to the dtype before the renormalising division",
    "rows_past_n_kept": "rows >= n are left as they were",
}

Case = namedtuple("Case", "name E k H rows n P h W target kinds pairs")
Case.__doc__ = """h int64 [n][H], W int64 [E][H], target int64 [n][E] = h @ W.T; rows: rows of the launch's buffers (rows_pad, or the wide call's
rows); kinds[r]: the plant of row r; pairs[r]: (pair kind, a, b, decisive) of a tie_kth row -- decisive: the tie is between a and b alone
and the cut runs between them -- else None"""


# ---- number formats -----------------------------------------------------------------------------------------------------------------------
def _ulp(p, mant, min_exp):
    """the spacing of a format with `mant` mantissa bits at p > 0 (the subnormal spacing below 2^min_exp); 1 where p == 0"""
    p = np.asarray(p, np.float64)
    e = np.floor(np.log2(np.where(p > 0, p, 1.0)))
    return np.exp2(np.maximum(e, min_exp) - mant)


def round_to(p, dtype):
    """p >= 0 (float64) rounded half-even to the dtype's grid, as float64"""
    u = _ulp(p, MANT[dtype], MIN_EXP[dtype])
    return np.rint(np.asarray(p, np.float64) / u) * u


def neighbours(p, dtype):
    """the dtype values below (or at) and above p"""
    u = _ulp(p, MANT[dtype], MIN_EXP[dtype])
    lo = np.floor(np.asarray(p, np.float64) / u) * u
    return lo, lo + u


def in_band(p, dtype):
    """p lies within MARGIN_ULPS fp32 ulps of the midpoint of its two dtype neighbours"""
    lo, hi = neighbours(p, dtype)
    return np.abs(np.asarray(p, np.float64) - (lo + hi) / 2) <= MARGIN_ULPS * _ulp(p, 23, -126)


def cast_exact(x, dtype):
    """every integer of x survives the cast to dtype"""
    t = torch.from_numpy(np.asarray(x, np.int64))
    return bool((t.to(dtype).to(torch.int64) == t).all())


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "idx p w band")
Ref.__doc__ = """idx int64 [n][k]; p float64 [n][k]: the unrounded weights; w: round_to(p); band: either neighbour allowed"""


def reference(logits, k, norm_topk, dtype):
    """float64 on exact logits: value descending, ties ascending by index; softmax over all E; renormalisation; one rounding"""
    x = np.asarray(logits, np.float64)
    idx = np.argsort(-x, axis=1, kind="stable")[:, :k]        # stable: equal values keep ascending expert order
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = np.take_along_axis(e / e.sum(axis=1, keepdims=True), idx, axis=1)
    if norm_topk:
        p = p / p.sum(axis=1, keepdims=True)
    return Ref(idx, p, round_to(p, dtype), in_band(p, dtype))


def lists_reference(idx, n, k):
    """samd_moe_route's lists from the reference indices: (n_active, active experts ascending, counts, per expert its entries
    p = row * k + slot ascending)"""
    per = {}
    for r in range(n):
        for j in range(k):
            per.setdefault(int(idx[r][j]), []).append(r * k + j)
    active = sorted(per)
    return len(active), active, [len(per[e]) for e in active], [per[e] for e in active]


# ---- the model of the kernel, with one named fault at a time ---------------------------------------------------------------------------------
def lane_steps(H):
    """steps of the unit loop per lane: units u = l, l + 64, .. < H / 8"""
    return (H // 8 - np.arange(LANES) + LANES - 1) // LANES


def model_logits(case, dtype, fault=None):
    """the logits the selection sees, float64 [n][E]"""
    h = case.h
    if fault == "tail_units_dropped":
        unit = np.arange(case.H) // 8
        kept = (unit // LANES) < (lane_steps(case.H)[unit % LANES] // 4) * 4
        h = h * kept
    x = (h @ case.W.T).astype(np.float64)
    if fault == "last_group_dropped" and case.E % 4:
        x[:, case.E // 4 * 4:] = 0.0
    if fault == "logits_in_dtype":
        x = torch.from_numpy(x).to(dtype).double().numpy()
    return x


def model_select(x, k, fault=None):
    """the k picks of wave 0, all rows at once: v [R][slot][lane], every lane keeps its own (bv, bi) through the tree and removes by
    its own bi; lane 0 reports.  -> (idx [R][k], -1 where the pick is no expert; the picked values)"""
    R, E = x.shape
    e_of = LANES * np.arange(SLOTS)[:, None] + np.arange(LANES)[None, :]
    real = e_of < E
    v = np.full((R, SLOTS, LANES), 0.0 if fault == "pad_zero" else NINF)
    v[:, real] = x
    live = real | (fault == "pad_zero")
    lanes = np.arange(LANES)
    idx, val = np.full((R, k), -1, np.int64), np.full((R, k), NINF)
    for j in range(k):
        bv, bi = np.full((R, LANES), NINF), np.full((R, LANES), NO_EXPERT, np.int64)
        for i in range(SLOTS):
            s, e = v[:, i, :], e_of[i][None, :]
            if fault == "lane_slot_order":
                tie = (s == bv) & (s > NINF)
            elif fault == "tie_to_higher":
                tie = (s == bv) & (e > bi) & (s > NINF) & (bi != NO_EXPERT)
            else:
                tie = (s == bv) & (e < bi) & (s > NINF)
            take = live[i][None, :] & ((s > bv) | tie)
            bv, bi = np.where(take, s, bv), np.where(take, e, bi)
        for o in (32, 16, 8, 4, 2, 1):
            ov, oi = bv[:, lanes ^ o], bi[:, lanes ^ o]
            if fault == "shuffle_tie_keeps_own":
                take = ov > bv
            elif fault == "tie_to_higher":
                take = (ov > bv) | ((ov == bv) & (oi > bi) & (oi != NO_EXPERT))
            else:
                take = (ov > bv) | ((ov == bv) & (oi < bi))
            bv, bi = np.where(take, ov, bv), np.where(take, oi, bi)
        for i in range(SLOTS):
            if i >= 1 and fault == "no_removal_upper_slots":
                continue
            v[:, i, :] = np.where(bi == e_of[i][None, :], NINF, v[:, i, :])
        ok = bi[:, 0] < E
        idx[:, j], val[:, j] = np.where(ok, bi[:, 0], -1), np.where(ok, bv[:, 0], NINF)
    return idx, val


def model_route(case, norm_topk, dtype, fault=None):
    """what the launch leaves in topk_idx / topk_w [rows][k] (weights as float64 holding dtype values), from buffers poisoned with
    POISON_IDX / NaN.  The arithmetic is float64: without a fault this is the reference, reached the kernel's way."""
    assert fault is None or fault in FAULTS
    idx = np.full((case.rows, case.k), POISON_IDX, np.int64)
    w = np.full((case.rows, case.k), np.nan)
    if fault != "rows_past_n_kept":
        idx[case.n:], w[case.n:] = -1, 0.0
    if case.n == 0:
        return idx, w
    x = model_logits(case, dtype, fault)
    sel, val = model_select(x, case.k, fault)
    mx = x.max(axis=1, keepdims=True)
    p = np.exp(val - mx)                                      # (exp(-inf) = 0: a pick that is no expert weighs nothing)
    se = p.sum(axis=1, keepdims=True) if fault == "softmax_over_selected" else np.exp(x - mx).sum(axis=1, keepdims=True)
    p = p / se
    norm = fault == "renorm_always" or (bool(norm_topk) and fault != "renorm_never")
    if norm:
        total = p.sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):                   # (a faulted row that picked no expert at all: 0 / 0, as on the device)
            p = (round_to(p, dtype) if fault == "weights_rounded_twice" else p) / total
    idx[:case.n], w[:case.n] = sel, round_to(p, dtype)
    return idx, w


# ---- the plants ---------------------------------------------------------------------------------------------------------------------------
def expert_place(e):
    """(lane, slot) of the selection and (wave, round) of the dot product"""
    return e % LANES, e // LANES, (e // 4) % WAVES, e // (4 * WAVES)


def pair_kinds(E):
    """the pair kinds an expert count can hold"""
    out = []
    for off in (64, 128, 192):
        if E > off:
            out.append(f"same_lane_{off}")
    if E >= 2:
        out.append("neighbour_even")
    if E >= 3:
        out.append("neighbour_odd")
    if E > 32:
        out.append("lanes_31_32")
    if E >= 64:
        out.append("lanes_0_63")
    if E > 64 + 4:
        out.append("waves_rounds")
    if E >= 2:
        out.append("first_last")
    return out


def make_pair(kind, E, rng):
    if kind.startswith("same_lane_"):
        off = int(kind[len("same_lane_"):])
        a = int(rng.integers(0, E - off))
        pair = (a, a + off)
        assert expert_place(pair[0])[0] == expert_place(pair[1])[0] and expert_place(pair[0])[1] != expert_place(pair[1])[1]
    elif kind in ("neighbour_even", "neighbour_odd"):
        first = 0 if kind == "neighbour_even" else 1
        a = int(rng.choice([a for a in range(first, E - 1, 2) if a % LANES != LANES - 1]))     # (63 | 64 are lanes 63 and 0: another kind)
        pair = (a, a + 1)
    elif kind == "lanes_31_32":
        s = int(rng.integers(0, (E - 33) // LANES + 1))
        pair = (31 + LANES * s, 32 + LANES * s)
    elif kind == "lanes_0_63":
        pair = (63, 64) if E > 64 and rng.integers(0, 2) else (0, 63)
    elif kind == "waves_rounds":
        a = int(rng.integers(0, 64))
        b = int(rng.choice([b for b in range(64, E) if expert_place(b)[2] != expert_place(a)[2]]))
        pair = (a, b)
        assert expert_place(a)[3] != expert_place(b)[3]
    else:
        pair = (0, E - 1)
    assert 0 <= pair[0] < pair[1] < E, (kind, E, pair)
    return pair


def _lows(row, top, rng):
    """everything still unset: 30 .. 80 below the maximum"""
    unset = row == np.iinfo(np.int64).min
    row[unset] = top - rng.integers(30, 81, int(unset.sum()))
    return row


def _descending(top, m, rng):
    """m values from `top` down with gaps 1 .. 3"""
    return top - np.concatenate(([0], np.cumsum(rng.integers(1, 4, m - 1)))) if m else np.zeros(0, np.int64)


def plant_row(kind, E, k, fine, rng, variant):
    """(targets int64 [E], kind as planted, pair record).  A plant the shape cannot hold falls back to `spaced`."""
    row = np.full(E, np.iinfo(np.int64).min, np.int64)
    top = int(rng.integers(-20, 61))
    pair = None
    if kind == "tie_kth" and E < 2:
        kind = "spaced"
    if kind == "resolution" and (not fine or E < 2):
        kind = "spaced"
    if kind == "plateau_all" and any(bool(in_band(1.0 / E, dt)) for dt in DTYPES):
        kind = "plateau_k"                                    # 1/E inside the band (E = 65, fp16: 63 fp32 ulps from a boundary) would count k times per row
    if kind in ("spaced", "all_negative"):
        if kind == "all_negative":
            top = -int(rng.integers(6, 60))
        m = min(k + 2, E)
        row[rng.choice(E, m, replace=False)] = _descending(top, m, rng)
    elif kind == "tie_kth":
        kinds = pair_kinds(E)
        pk = kinds[variant % len(kinds)]
        a, b = make_pair(pk, E, rng)
        decisive = (variant // len(kinds)) % 2 == 0 or E < 4
        tied = [a, b]
        if not decisive:
            others = [e for e in range(E) if e not in (a, b)]
            tied += rng.choice(others, min(int(rng.integers(1, 5)), len(others), max(0, E - 2)), replace=False).tolist()
        tied = sorted(tied)
        if k >= E:
            above = E - len(tied)                             # k == E: no cut, the tie fills the last places in ascending order
        elif decisive:
            above = k - 1
        else:
            above = k - int(rng.integers(1, min(len(tied), k + 1)))        # 1 .. |T| - 1 of the tied are taken
            above = max(above, k - len(tied) + 1, 0)
        above = min(above, E - len(tied))
        free = [e for e in range(E) if e not in tied]
        up = rng.choice(free, above, replace=False) if above else np.zeros(0, np.int64)
        row[up] = _descending(top, above, rng)
        row[tied] = top if above == 0 else row[up].min() - int(rng.integers(1, 4))
        pair = (pk, a, b, bool(decisive and k < E))
    elif kind == "tie_above":
        row[rng.choice(E, min(k + 3, E), replace=False)] = top
    elif kind == "plateau_all":
        row[:] = top
    elif kind == "plateau_k":
        row[rng.choice(E, k, replace=False)] = top
    elif kind == "ramp":
        e = np.arange(E)
        row[:] = top + np.maximum(-80, (e - (E - 1)) if variant % 2 == 0 else -e)
    elif kind == "resolution":
        # B and B + 1 at a magnitude where the dtype cannot tell them apart; the LOWER expert holds the smaller one and must lose
        base = BIG_LOGIT + 32 * int(rng.integers(4, 40))
        a, b = sorted(rng.choice(E, 2, replace=False).tolist())
        above = min(k - 1, E - 2)
        free = [e for e in range(E) if e not in (a, b)]
        up = rng.choice(free, above, replace=False) if above else np.zeros(0, np.int64)
        row[a], row[b] = base, base + 1
        row[up] = base + 1 + np.cumsum(rng.integers(1, 4, above))
        top = int(row[up].max()) if above else base + 1
    else:
        raise KeyError(kind)
    return _lows(row, top, rng), kind, pair


def build_case(E, k, H, rows, n, seed, kind_offset=0, name=None):
    """the planted rows of one shape: plants cycle over the rows, the tie pairs cycle from kind_offset on"""
    rng = np.random.default_rng(seed)
    fine = H >= 2 * E
    P = COARSE if fine else 1
    c0 = 2 * E if fine else E
    W = np.zeros((E, H), np.int64)
    W[np.arange(E), np.arange(E)] = P
    if fine:
        W[np.arange(E), E + np.arange(E)] = 1
    W[:, c0:] = rng.integers(-2, 3, (E, H - c0)) * (rng.random((E, H - c0)) < 0.25)
    for c in range(c0, H):                                    # every noise column reaches some expert
        if not W[:, c].any():
            W[c % E, c] = 1 + c % 2
    h = np.zeros((n, H), np.int64)
    if H > c0 and n:
        nz = rng.integers(-3, 4, (n, H - c0)) * (rng.random((n, H - c0)) < 0.25)
        col = np.arange(c0, H)
        forced = (col[None, :] % 8) == ((col[None, :] // 8 + np.arange(n)[:, None]) % 8)      # one element of every unit, moving with the row
        fill = np.where(rng.random((n, H - c0)) < 0.5, -1, 1) * rng.integers(1, 4, (n, H - c0))
        h[:, c0:] = np.where(forced & (nz == 0), fill, nz)
    N = h[:, c0:] @ W[:, c0:].T
    target = np.zeros((n, E), np.int64)
    kinds, pairs = [], []
    for r in range(n):
        t, kind, pair = plant_row(KINDS[r % len(KINDS)], E, k, fine, rng, r // len(KINDS) + kind_offset)
        target[r] = t
        kinds.append(kind)
        pairs.append(pair)
    d = target - N
    h[:, :E] = d // P                                         # (floor division: the fine column holds 0 .. P - 1)
    if fine:
        h[:, E:2 * E] = d - (d // P) * P
    case = Case(name or f"E{E}_k{k}_H{H}_rows{rows}_n{n}", E, k, H, rows, n, P, h, W, target, tuple(kinds), tuple(pairs))
    check_case(case)
    return case


def check_case(case):
    """the logits are the targets, exactly, in any order of summation, and in both dtypes"""
    assert np.array_equal(case.h @ case.W.T, case.target)
    if case.n:
        assert int((np.abs(case.h) @ np.abs(case.W).T).max()) < 2 ** 24
    for dt in DTYPES:
        assert cast_exact(case.h, dt) and cast_exact(case.W, dt), (case.name, dt)
    for r in range(case.n):
        t = case.target[r]
        low = t < t.max() - 29
        assert int((~low).sum()) >= min(case.k, case.E) and bool((t >= t.max() - 80).all()), (case.name, r, case.kinds[r])
        if case.kinds[r] == "all_negative":
            assert t.max() < -5
        if case.kinds[r] == "resolution":
            assert t.max() >= BIG_LOGIT
    if case.H > (2 * case.E if case.P > 1 else case.E) and case.n >= 8:
        c0 = 2 * case.E if case.P > 1 else case.E
        assert bool((case.h[:, c0:] != 0).any(axis=0).all()) and bool((case.W[:, c0:] != 0).any(axis=0).all())       # every noise element is used


def _seed(shape):
    return SEEDS.get(shape, 1000 + sum(int(x) * m for x, m in zip(shape, (1, 257, 3, 11, 7))))


@lru_cache(maxsize=None)
def route_case(shape):
    """the planted case of one (E, k, H, rows, n), built once (callers must not write into it)"""
    shapes = ROUTE_SHAPES + WIDE_SHAPES + (EMPTY_SHAPE,)
    E, k, H, rows, n = shape
    return build_case(E, k, H, rows, n, _seed(shape), kind_offset=3 * shapes.index(shape) if shape in shapes else 0)


def all_cases():
    return [route_case(s) for s in ROUTE_SHAPES + WIDE_SHAPES + (EMPTY_SHAPE,)]


def tensors(case, dtype, device="cpu", rows_alloc=None):
    """(h [rows_alloc or case.rows][H] with NaN in every row >= n, router [E][H]) in `dtype`"""
    rows = case.rows if rows_alloc is None else rows_alloc
    h = torch.full((rows, case.H), float("nan"), dtype=torch.float64)
    h[:case.n] = torch.from_numpy(case.h).double()
    return h.to(dtype).to(device), torch.from_numpy(case.W).to(dtype).to(device)


# ---- comparing a launch's outputs with the reference ---------------------------------------------------------------------------------------
def compare(case, ref, got_idx, got_w, dtype):
    """got_idx int [rows][k], got_w float64 [rows][k] against the reference: indices by equality on every row, weights by equality
    outside the band and either neighbour inside, rows >= n -1 / 0.  -> (weights in the band, of them stored as the other neighbour);
    raises AssertionError naming the row's plant."""
    got_idx, got_w = np.asarray(got_idx, np.int64), np.asarray(got_w, np.float64)
    n = case.n
    assert bool((got_idx[n:] == -1).all()) and bool((got_w[n:] == 0).all()), (case.name, "rows >= n must read -1 / 0")
    bad = np.nonzero((got_idx[:n] != ref.idx).any(axis=1))[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{case.name} row {r} ({case.kinds[r]}, {case.pairs[r]}): indices {got_idx[r].tolist()}, expected {ref.idx[r].tolist()}; "
                             f"{len(bad)} rows differ")
    lo, hi = neighbours(ref.p, dtype)
    ok = np.where(ref.band, (got_w[:n] == lo) | (got_w[:n] == hi), got_w[:n] == ref.w)
    bad = np.nonzero(~ok.all(axis=1))[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{case.name} row {r} ({case.kinds[r]}): weights {got_w[r].tolist()}, expected {ref.w[r].tolist()} (band {ref.band[r].tolist()}); "
                             f"{len(bad)} rows differ")
    return int(ref.band.sum()), int((ref.band & (got_w[:n] != ref.w)).sum())


def band_share(ref):
    return float(ref.band.mean()) if ref.band.size else 0.0


def exact_plateau(case, r, norm_topk):
    """the float64 weights of row r are dtype values by construction: 1/E on a plateau over a power-of-two E, 1/k after renormalising
    k equal leaders for a power-of-two k"""
    pow2 = lambda x: x & (x - 1) == 0                         # noqa: E731
    if case.kinds[r] not in ("plateau_all", "plateau_k"):
        return False
    if norm_topk:
        return pow2(case.k)
    return case.kinds[r] == "plateau_all" and pow2(case.E)
