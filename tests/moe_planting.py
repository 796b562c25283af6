"""Exact-integer inputs for the five mixture-of-experts kernels (k_moe_gate_up_silu, k_moe_down, k_moe4_gate_up_silu, k_moe4_down,
k_moe_combine), their float64 references and named faults (numpy + torch only; no product import).  The method is tests/gemm_planting.py's:
every exact sum is an integer below 2^24, so the value a kernel must store is determined bit for bit and comparisons are equalities.

  routings     pinned [rows_pad, top_k] int32 with n <= rows_pad live rows, and the per-expert lists computed here from the header's rule
               (entries p = row * top_k + slot ascending; rows >= n, indices outside [0, E) and a repeated expert within a row left out):
               one_expert (expert 0 takes slot 0 of every row: count = the row tile), distinct (every (row, slot) its own expert: count 1
               everywhere), grid_bound (distinct at E = 128, k = 8, 16 rows: n k = min(E, rows_pad k), the y extent of the grid), random
               (n = rows_pad - 3, junk in the rows behind), counts (expert counts 1, 15, 16, 17, 33, 47, 48, 63 as far as they fit in the
               bucket: both sides of every 16-row MFMA tile edge are live; four more experts share the slots left over), excluded (out-of-range and repeated slots).
  down         small sums: act rows in {-1, 0, 1} at gemm_planting.density, weights dense +-1 drawn per expert (`small_draws` with rows =
               live_rows = the expert's count; draws are added per expert until its own rows cover every k column), every exact |y| < BAR.
               large sums: `large_case` per expert; `check_large` on the y of the case.
  gate|up      the silu planting per expert: h rows from `silu_draws` (bias column 0, Q other nonzeros), every expert's own gate / up
               weights from `silu_draws`; act[p] = round(g * u) and `assert_silu` holds from the reference.
  MXFP4        the same three with weights e2m1 x e8m0 holds exactly.  small: +-1 = (code +-1.0, exponent 0) in even 32-k blocks and
               (code +-0.5, exponent 1) in odd ones.  silu: the bias is the first 32-k block (h = 1 across it, gate weights uniform 1.5
               (bf16: 32 x 1.5 = 48) or 8 = 2 x 2^2 (fp16: 256), up weights +-1), gate range GATE_RANGE4.  large: codes uniform over all 16
               values, block exponents 1 and 2 alternating along k and along the rows (every weight an integer, the odd ones included),
               activations dense in [-amax, amax] with amax from (K, dtype) so that the sums reach LARGE_SIGMA (`large4_amax` says why
               the activations are widened and not the weights' level).
  combine      w[row][j] from {1/4, 1/2, 1, 2} (index (row + j) mod 4); out = rounded(sum_j w * rounded(y_exact)): products and sums are
               exact in fp32 (multiples of 1/4 below 2^22).
  rows         `independence_cases`: one row alone at 16 rows against the same row as row 40 of 64, with the same references.
  slot order   terms w_j y_j = (+2^15, +2^-10, -2^15, +2^-11) rotated by the row; y comes from the down launch itself (one-hot act rows
               against integer weight columns); the fp32 reference is an explicit sequential np.float32 loop.

References are float64 with roundings only where the header documents them: act through `silu_ref`, y = rounded(exact), out as above.
Faults recompute a reference with one named change and say which outputs they touch (`_check`: a fault changes >= half of them).  Three
are shares of another kind, each with its reason where it is asserted: the truncating casts (more than a quarter of the large sums, 2 %
of the silu products) and the combine in the model dtype (a double rounding: more than 1/8 of the outputs whose partial sums round).
Layouts: `pack_experts` restates samd_moe_pack_experts, `gate_up_row_order` the MXFP4 row permutation, `encode` / `decode` MXFP4 itself."""
import math

import numpy as np
import torch

import gemm_planting as G
from gemm_planting import LARGE_SIGMA, as_t, assert_silu, check_large, chunk_products, rounded, silu_ref, small_draws, truncated

F64 = torch.float64
KC = G.KC
DTYPES = G.DTYPES
ROWS = (16, 32, 48, 64)
FORMS = (None, "mxfp4")
COUNTS = (1, 15, 16, 17, 33, 47, 48, 63)
KINDS = ("one_expert", "distinct", "random", "counts")
COMBINE_W = (0.25, 0.5, 1.0, 2.0)
# restated from samd_hip/mxfp4.py (tests/test_moe_planting_cpu.py cross-checks): the e2m1 grid and the block exponents exact in a dtype
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
EXPONENT_RANGE = {torch.float16: (-23, 13), torch.bfloat16: (-125, 125)}
# the MXFP4 silu planting: 32 x the block-0 gate weight is the gate bias; bf16 holds every integer up to 256
GATE4 = {torch.float16: (8.0, 2), torch.bfloat16: (1.5, 0)}          # (weight, block exponent)
GATE_RANGE4 = {torch.float16: (24, 512), torch.bfloat16: (24, 128)}
DEPTH4 = {16: 8, 32: 3, 48: 2, 64: 3}                                # pipeline depths of the MXFP4 form (2 everywhere in the model-dtype form)
# ... and of the other quantised forms (restated from csrc/gemm_kernels.hip: MoeW4Depth, MoeI8Depth, Moe8Depth), rows_pad -> depth
DEPTHS = {"mxfp4": DEPTH4, "int4g128": DEPTH4, "int8g128": {16: 4, 32: 3, 48: 2, 64: 1}, "fp8b128": {16: 4, 32: 4, 48: 4, 64: 3}}


def seed_of(*xs):
    s = 0
    for x in xs:
        s = (s * 1000003 + int(x) + 7) % (2 ** 31 - 1)
    return s


def chunk_sweep(form, rows_pad):
    """streams shorter than, at and above every depth; odd counts through the per-block refill of the 48 / 64-row kernels"""
    depth = 2 if form is None else DEPTHS[form][rows_pad]
    if form in (None, "mxfp4"):
        sweep = tuple(range(1, 8)) if form is None else tuple(range(1, depth + 3)) if rows_pad == 16 else (1, 2, 3, 4, 5, 7)
    else:                                                        # (one of depth + 1, depth + 2 is the odd count above the depth)
        sweep = tuple(range(1, depth + 3))
    assert {max(1, depth - 1), depth, depth + 1, depth + 2} <= set(sweep) and any(c % 2 and c > depth for c in sweep)
    return sweep


def exact_sweep(form):
    """[(K, rows_pad)] of the exact-integer tests of a quantised form's expert kernels: chunk_sweep and the stream lengths 1, 3, 9 that
    those tests ran before the sweep (K = 256 / 768 / 2304), at every row tile"""
    return [(KC * c, r) for r in ROWS for c in sorted(set(chunk_sweep(form, r)) | {1, 3, 9})]


# ---- routings -------------------------------------------------------------------------------------------------------------------------------
def python_lists(idx, n, E):
    """{expert: [p, ...]} in ascending expert order, from the header's rule"""
    RP, k = idx.shape
    lists = {}
    for p in range(min(n, RP) * k):
        r, j = divmod(p, k)
        e = int(idx[r, j])
        if 0 <= e < E and e not in idx[r, :j].tolist():
            lists.setdefault(e, []).append(p)
    return dict(sorted(lists.items()))


class Routing:
    def __init__(self, name, E, k, rows_pad, n, idx):
        self.name, self.E, self.k, self.rows_pad, self.n = name, E, k, rows_pad, n
        self.idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert self.idx.shape == (rows_pad, k) and 0 <= n <= rows_pad and k <= min(8, E) and rows_pad in ROWS
        self.lists = python_lists(self.idx, n, E)
        self.named = sorted(p for lst in self.lists.values() for p in lst)
        self.valid = np.zeros((rows_pad, k), dtype=bool)             # the slots that add to a row's output
        self.valid.reshape(-1)[self.named] = True
        assert all(len(lst) <= rows_pad for lst in self.lists.values()) and len(self.lists) <= min(E, rows_pad * k)

    @property
    def counts(self):
        return [len(lst) for lst in self.lists.values()]

    def entry_mask(self, ps, width):
        m = torch.zeros((self.rows_pad * self.k, width), dtype=torch.bool)
        m[list(ps)] = True
        return m

    def row_mask(self, ps, width):
        m = torch.zeros((self.rows_pad, width), dtype=torch.bool)
        m[sorted({p // self.k for p in ps})] = True
        return m


def routing(kind, rows_pad, seed=0):
    rng = np.random.default_rng(seed_of(rows_pad, len(kind), seed))
    r = np.arange(rows_pad)
    if kind == "one_expert":                                     # expert 0: slot 0 of every row; the other slots spread over experts 1 .. 7
        E, k, n = 8, 4, rows_pad
        idx = np.stack([np.zeros(rows_pad, dtype=np.int64)] + [1 + (r + 2 * j) % 7 for j in range(1, k)], axis=1)
    elif kind in ("distinct", "grid_bound"):                     # n k = E experts of one entry each; valid indices in the rows behind n
        E, k, n = (8, 4, 2) if kind == "distinct" else (128, 8, 16)
        assert kind == "distinct" or (rows_pad == 16 and n * k == min(E, rows_pad * k))
        idx = (np.arange(rows_pad * k).reshape(rows_pad, k)) % E
    elif kind == "random":
        E, k, n = 8, 4, rows_pad - 3
        idx = np.stack([rng.permutation(E)[:k] for _ in range(rows_pad)])
    elif kind == "counts":                                       # expert i has the i-th count; a row's experts fill its slots in ascending order,
        counts = [c for c in COUNTS if c <= rows_pad]            # the four experts after them take the slots left over: every row has k products
        E, k, n = len(counts) + 4, 4, rows_pad
        idx, load = np.full((rows_pad, k), -1, dtype=np.int64), np.zeros(rows_pad, dtype=np.int64)
        for e in sorted(range(len(counts)), key=lambda i: -counts[i]):
            rows = np.argsort(load, kind="stable")[:counts[e]]
            assert load[rows].max() < k
            idx[rows, load[rows]] = e
            load[rows] += 1
        idx = np.sort(np.where(idx < 0, E, idx), axis=1)         # ascending within a row, the free slots last
        idx = np.where(idx == E, len(counts) + (r[:, None] + np.arange(k)[None, :]) % 4, idx)
    elif kind == "excluded":                                     # random with out-of-range indices and repeated experts
        E, k, n = 8, 4, rows_pad - 3
        idx = np.stack([rng.permutation(E)[:k] for _ in range(rows_pad)])
        idx[0, 2], idx[3, 1], idx[5, 3], idx[7, 0], idx[8, 3], idx[9, 2] = E + 3, idx[3, 0], 4096, -7, idx[8, 1], E
    else:
        raise ValueError(kind)
    R = Routing(kind, E, k, rows_pad, n, idx)
    if kind == "counts":
        assert [len(R.lists[e]) for e in range(len(counts))] == counts and bool(R.valid.all()), R.counts
    if kind == "one_expert":
        assert R.counts[0] == rows_pad
    if kind in ("distinct", "grid_bound"):
        assert R.counts == [1] * (n * k)
    return R


def combine_weights(R):
    """[rows_pad, k]: w[row][j] = COMBINE_W[(row + j) % 4] -- neighbouring slots and neighbouring rows differ"""
    return torch.tensor(COMBINE_W, dtype=F64)[(torch.arange(R.rows_pad)[:, None] + torch.arange(R.k)[None, :]) % 4]


# ---- MXFP4 ----------------------------------------------------------------------------------------------------------------------------------
def encode(W, exps, dtype):
    """(q uint8 [..., K / 2], e8 uint8 [..., K / 32]) of W [..., K] with block exponents exps [..., K / 32]; every W / 2^e must be on the grid"""
    W, exps = np.asarray(W, dtype=np.float64), np.asarray(exps, dtype=np.int64)
    lo, hi = EXPONENT_RANGE[dtype]
    assert lo <= exps.min() and exps.max() <= hi
    mag = np.abs(W).reshape(exps.shape + (32,)) / np.exp2(exps)[..., None]
    code = np.minimum(np.searchsorted(GRID, mag), 7)
    assert np.array_equal(GRID[code], mag), "a weight that e2m1 x e8m0 does not hold"
    code = (code | ((W.reshape(mag.shape) < 0) << 3)).reshape(W.shape).astype(np.uint8)
    return np.ascontiguousarray(code[..., 0::2] | (code[..., 1::2] << 4)), (exps + 127).astype(np.uint8)


def decode(q, e8):
    """float64 W [..., K]: low nibble = the even element, sign in bit 3, magnitude GRID[code & 7] * 2^(e8 - 127)"""
    code = np.stack([q & 15, q >> 4], axis=-1).reshape(q.shape[:-1] + (2 * q.shape[-1],))
    v = np.where(code & 8, -1.0, 1.0) * GRID[code & 7]
    return (v.reshape(e8.shape + (32,)) * np.exp2(e8.astype(np.int64) - 127)[..., None]).reshape(v.shape)


def pm1_exponents(N, K):
    """the small regime's block exponents: 0 in even 32-k blocks (+-1 = code +-1.0), 1 in odd ones (code +-0.5)"""
    return np.broadcast_to(np.arange(K // 32) % 2, (N, K // 32)).copy()


LARGE4_EXPONENTS = (1, 2)                                        # block exponents of the MXFP4 large regime: neighbours differ by 1
LARGE4_WMAX = 6 * 2 ** max(LARGE4_EXPONENTS)
SIGNED_GRID = np.concatenate([GRID, -GRID])                      # the value of every 4-bit code: sign in bit 3
CODE_VAR = float((SIGNED_GRID ** 2).mean())


def large4_amax(K, dtype):
    """the activation range [-amax, amax] of the MXFP4 large regime.  The weights stay at the lowest integer level (block exponents 1 and
    2: the odd weights 1 and 3 exist) and the ACTIVATIONS are widened until the sums reach LARGE_SIGMA: with the weights raised instead
    (block exponents L, L + 1 for the same sigma) every sum is a multiple of 2^(L - 1), which the dtype then mostly holds exactly, and
    check_large fails (fp16, K = 256, L = 5: 0.3 % of the sums inexact; bf16, L = 3: a truncating cast differs on 24.9 % < 25 %)."""
    var_w = CODE_VAR * float(np.mean([4.0 ** e for e in LARGE4_EXPONENTS]))
    var = LARGE_SIGMA[dtype] ** 2 / (var_w * K)                  # var of a uniform integer in [-a, a] is a (a + 1) / 3
    amax = max(8, int(math.ceil((math.sqrt(1.0 + 12.0 * var) - 1.0) / 2.0)))
    assert amax <= 256 and amax * LARGE4_WMAX * K < 2 ** 24      # every activation is exact in bf16; every partial sum in fp32
    return amax


def large4_weights(rng, N, K, dtype):
    pat = LARGE4_EXPONENTS
    exps = np.array(pat)[(np.arange(K // 32)[None, :] + np.arange(N)[:, None]) % len(pat)]
    assert exps.min() >= 1 and bool((np.abs(np.diff(exps, axis=1)) == 1).all())
    code = rng.integers(0, 16, (N, K), dtype=np.uint8)
    W = (SIGNED_GRID[code].reshape(N, K // 32, 32) * np.exp2(exps)[:, :, None]).reshape(N, K)
    assert np.array_equal(W, np.round(W))
    return W, exps


def nibbles_swapped(W):
    return W.reshape(W.shape[:-1] + (-1, 2)).flip(-1).reshape(W.shape)


def neighbour_exponent(W, exps):
    """every block scaled by block b ^ 1's exponent instead of its own"""
    e = torch.from_numpy(np.asarray(exps, dtype=np.float64))
    nb = e[..., torch.arange(e.shape[-1]) ^ 1]
    return (W.reshape(e.shape + (32,)) * torch.exp2(nb - e)[..., None]).reshape(W.shape)


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def _sources(lst, fault):
    return lst[1:] + lst[:1] if fault == "list_entry_next" else lst      # tile row r reads list entry r + 1 (the last one: entry 0)


def _weights(W, e, fault, exps=None):
    """float64 [N, K] of expert e as the launch with `fault` reads them (the 4-bit faults need the block exponents)"""
    We = W[(e + 1) % W.shape[0] if fault == "neighbour_expert" else e].double()
    if fault == "nibbles_swapped":
        return nibbles_swapped(We)
    return neighbour_exponent(We, exps[e]) if fault == "neighbour_exponent" else We


def combine_ref(R, y, w, dtype, fault=None):
    """out [rows_pad, N] float64: rounded(sum over the valid slots j ascending of w[row][j] * y[row k + j]); rows >= n are zero"""
    RP, k, n = R.rows_pad, R.k, R.n
    N = y.shape[1]
    y3 = (torch.roll(y[:n * k], -1, 0) if fault == "y_next_row" else y[:n * k]).reshape(n, k, N)
    acc = torch.zeros((n, N), dtype=F64)
    valid = torch.from_numpy(R.valid[:n])
    for j in range(k):
        wj = w[:n, (j + 1) % k] if fault == "w_next_slot" else (torch.ones(n, dtype=F64) if fault == "w_not_applied" else w[:n, j])
        term = torch.where(valid[:, j:j + 1], wj[:, None] * y3[:, j], torch.zeros((), dtype=F64))
        acc = rounded(acc + rounded(term, dtype), dtype) if fault == "combine_in_dtype" else acc + term
    out = torch.zeros((RP, N), dtype=F64)
    out[:n] = (truncated if fault == "truncate_out" else rounded)(acc, dtype)
    return out


def combine_in_dtype_touched(R, y, w, dtype):
    """[rows_pad, N] bool: the outputs a combine in the model dtype can change -- a partial sum BEFORE the row's last valid slot is inexact
    in the dtype (where only the last addition rounds, both orders of rounding round the same exact sum once)"""
    n, k = R.n, R.k
    valid = torch.from_numpy(R.valid[:n])
    terms = torch.where(valid[:, :, None], w[:n, :, None] * y[:n * k].reshape(n, k, -1), torch.zeros((), dtype=F64))
    part = terms.cumsum(1)[:, :k - 1]
    more = valid.flip(1).cumsum(1).flip(1)[:, 1:] > 0              # a valid slot follows
    touched = torch.zeros((R.rows_pad, y.shape[1]), dtype=torch.bool)
    touched[:n] = ((rounded(part, dtype) != part) & more[:, :, None]).any(1)
    return touched


def assert_combine_exact(R, y, w):
    """every product and every partial sum of the combine is exact in fp32: multiples of 1/4 whose absolute values sum below 2^22"""
    n, k = R.n, R.k
    terms = torch.where(torch.from_numpy(R.valid[:n])[:, :, None], w[:n, :, None] * y[:n * k].reshape(n, k, -1), torch.zeros((), dtype=F64))
    assert bool((4.0 * terms == (4.0 * terms).round()).all()) and 4.0 * terms.abs().sum(1).max().item() < 2 ** 24


def down_ref(R, W, act, w, dtype, fault=None, exps=None):
    """(y_exact, y, out): y [rows_pad k, N] is NaN in the rows that no list names"""
    y_exact = torch.full((R.rows_pad * R.k, W.shape[1]), float("nan"), dtype=F64)
    for e, lst in R.lists.items():
        y_exact[lst] = act[_sources(lst, fault)] @ _weights(W, e, fault, exps).t()
    y = (truncated if fault == "truncate_y" else rounded)(y_exact, dtype)
    return y_exact, y, combine_ref(R, y, w, dtype, fault)


def gate_up_ref(R, Wg, Wu, h, dtype, fault=None, exps=(None, None)):
    """(gate, up, act) [rows_pad k, inter]: NaN in the rows that no list names; the source row of entry p is p / top_k.  h is [rows_pad, K],
    or [draws, rows_pad, K] for every draw of a case at once (the outputs then lead with the draw as well)"""
    gate = torch.full(h.shape[:-2] + (R.rows_pad * R.k, Wg.shape[1]), float("nan"), dtype=F64)
    up = gate.clone()
    for e, lst in R.lists.items():
        a = h[..., [p % R.n if fault == "source_row_p" else p // R.k for p in _sources(lst, fault)], :]
        gate[..., lst, :], up[..., lst, :] = a @ _weights(Wg, e, fault, exps[0]).t(), a @ _weights(Wu, e, fault, exps[1]).t()
    return gate, up, act_ref(gate, up, dtype, fault)


def act_ref(gate, up, dtype, fault=None):
    """silu_ref, or with the last cast truncating"""
    if fault == "truncate_act":
        return truncated(rounded(rounded(gate, dtype) / (1.0 + torch.exp(-rounded(gate, dtype))), dtype) * rounded(up, dtype), dtype)
    return silu_ref(gate, up, dtype, fault)


def assert_silu4(gate, up, dtype):
    """the MXFP4 silu planting's conditions from the reference alone (gemm_planting.assert_silu with this module's gate range)"""
    lo, hi = GATE_RANGE4[dtype]
    assert bool((gate == gate.round()).all()) and gate.min().item() >= lo and gate.max().item() <= hi
    assert torch.equal(rounded(gate, dtype), gate)
    assert bool((up == up.round()).all()) and up.abs().min().item() >= 1 and up.abs().max().item() <= G.UP_MAX
    assert torch.equal(silu_ref(gate, up, dtype), rounded(gate * up, dtype))
    assert bool(((1.0 + torch.exp(-gate.float())) == 1.0).all())


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """the inputs of one launch sequence and what it must store, draw by draw"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _check(want, wrongs):
    """gemm_planting.self_check's rule over whole-case stored tensors: {name: (wrong, touched)}, each a tensor or a tuple of them like `want`;
    every fault changes >= half of the values it touches, and at least one.  Returns the names."""
    def flat(t):
        return torch.cat([x.reshape(-1) for x in (t if isinstance(t, tuple) else (t,))])
    for name, (wrong, touched) in wrongs.items():
        changed = (flat(wrong) != flat(want))[flat(touched)]
        assert changed.numel() > 0 and changed.double().mean().item() >= 0.5, (name, changed.numel(), changed.double().mean().item())
    return list(wrongs)


def _expert_rows(R, rows_of, total_rows, K):
    """scatter per-expert row blocks {e: [count, K]} into [total_rows, K], NaN elsewhere"""
    A = torch.full((total_rows, K), float("nan"), dtype=F64)
    for e, lst in R.lists.items():
        A[lst] = rows_of[e]
    return A


def down_weights(dtype, R, N, chunks, regime, form=None):
    """(W float64 [E, N, K], exps or None, {active expert: [its rows of act, draw by draw]}) of one down case.  An expert without entries
    gets weights of the same recipe (the neighbouring-expert fault reads them) and no activations"""
    K, E = KC * chunks, R.E
    seed = seed_of(G.MANT[dtype], R.rows_pad, N, chunks, regime == "small", form is not None, len(R.name), 17)
    rng = np.random.default_rng(seed)
    W = torch.empty((E, N, K), dtype=F64)
    exps = None if form is None else np.zeros((E, N, K // 32), dtype=np.int64)
    per_expert = {}
    for e in range(E):
        cnt = len(R.lists.get(e, ()))
        if regime == "small":
            if cnt:
                per_expert[e], W[e] = small_draws(seed + 1 + e, cnt, N, K, dtype, cnt)
                assert G.uncovered_share(per_expert[e], cnt) == 0.0
            else:
                W[e] = torch.from_numpy(rng.integers(0, 2, (N, K), dtype=np.int8) * 2 - 1)
            if form:
                exps[e] = pm1_exponents(N, K)
            continue
        for attempt in range(8 if cnt else 1):                   # (a draw whose largest sum overflows the dtype is drawn again: fp16, about one in 10^3)
            erng = np.random.default_rng(seed + 1 + e + 1000 * attempt)
            if form:
                We, exps[e] = large4_weights(erng, N, K, dtype)
                A, We = as_t(erng.integers(-large4_amax(K, dtype), large4_amax(K, dtype) + 1, (cnt, K))), as_t(We)
            else:
                A, We = G.large_case(seed + 1 + e + 1000 * attempt, cnt, N, K, dtype)
            if not cnt or (A @ We.t()).abs().max().item() <= torch.finfo(dtype).max:
                break
        W[e] = We
        if cnt:
            per_expert[e] = [A]
    assert max(-W.min().item(), W.max().item()) <= 2 ** (G.MANT[dtype] + 1)      # integers of so many bits: the dtype holds every weight
    return W, exps, per_expert


def down_case(dtype, R, N, chunks, regime, form=None, check=True):
    """Case(W float64 [E, N, K], exps or None, w, draws = [(act [rows_pad k, K], y, out), ...]) of the down launch
    and the combine"""
    W, exps, per_expert = down_weights(dtype, R, N, chunks, regime, form)
    K = W.shape[2]
    w = combine_weights(R)
    draws = []
    for d in range(max(len(v) for v in per_expert.values())):
        act = _expert_rows(R, {e: v[d % len(v)] for e, v in per_expert.items()}, R.rows_pad * R.k, K)
        assert torch.equal(rounded(act, dtype).nan_to_num(7.0), act.nan_to_num(7.0))
        y_exact, y, out = down_ref(R, W, act, w, dtype)
        live = y_exact[R.named]
        assert_combine_exact(R, y, w)
        if regime == "small":
            G.assert_small(live, dtype)
        else:
            check_large(live, dtype)
            assert bool((combine_ref(R, y, w, dtype, "combine_in_dtype") != out).any())      # adding in the model dtype stores another value
        draws.append((act, y, out))
    c = Case(dtype=dtype, R=R, N=N, K=K, W=W, exps=exps, w=w, draws=draws, regime=regime, form=form)
    if check:
        c.checked = down_faults(c)
    return c


def down_faults(c):
    """self check of the first draw against every named fault that applies; returns the names"""
    R, dtype = c.R, c.dtype
    act, y, out = c.draws[0]
    N = c.N
    named, multi = R.named, [p for lst in R.lists.values() if len(lst) >= 2 for p in lst]
    ym, om = lambda ps: R.entry_mask(ps, N), lambda ps: R.row_mask(ps, N)
    none_y = torch.zeros_like(y, dtype=torch.bool)
    ref = lambda f: down_ref(R, c.W, act, c.w, dtype, f, c.exps)[1:]
    comb = lambda f: (y, combine_ref(R, y, c.w, dtype, f))         # the faults of the combine alone: y as it is
    wrongs = {"neighbour_expert": (ref("neighbour_expert"), (ym(named), om(named)))}
    if multi:
        wrongs["list_entry_next"] = (ref("list_entry_next"), (ym(multi), om(multi)))
    for f in ("w_next_slot", "y_next_row", "w_not_applied"):
        wrongs[f] = (comb(f), (none_y, om(named)))
    if c.form:
        wrongs["nibbles_swapped"] = (ref("nibbles_swapped"), (ym(named), om(named)))
        wrongs["neighbour_exponent"] = (ref("neighbour_exponent"), (ym(named), om(named)))
    done = _check((y, out), wrongs)
    if c.regime == "large":                                      # truncating casts: more than a quarter of the stored values (check_large's bar)
        G.rounding_share(y[ym(named)], ref("truncate_y")[0][ym(named)], 0.25)
        G.rounding_share(out[om(named)], comb("truncate_out")[1][om(named)], 0.25)
        done += ["truncate_y", "truncate_out"]
        # the combine in the model dtype is a double rounding: it stores another value only where an earlier rounding error carries the
        # sum over a rounding boundary of the last one.  An error uniform in half a unit either way against a sum uniform between two
        # boundaries does so for 1/4 of them, for 1/8 where the last sum has moved up a binade: more than 1/8 of the touched outputs
        sel = combine_in_dtype_touched(R, y, c.w, dtype)
        c.combine_in_dtype_share = G.rounding_share(out[sel], comb("combine_in_dtype")[1][sel], 0.125)
        done.append("combine_in_dtype")
    else:                                                        # faults of a few units, on the expert with the most rows
        e = max(R.lists, key=lambda x: len(R.lists[x]))
        A, We = act[R.lists[e]], c.W[e]
        if len(A) == 1:                                          # (product_faults pairs rows: a second row, another entry's)
            A = torch.cat((A, act[[p for p in named if p != R.lists[e][0]][:1]]))
        A = A[:len(A) // 2 * 2]
        P = chunk_products(A, We)
        faults = G.product_faults(seed_of(N, c.K, 3), A, We, P, 1)
        done += G.self_check(lambda p: rounded(p[0], dtype), P.sum(0)[None], {f: faults[f] for f in G.EXACT_ONLY}, True)
    return done


def silu4_draws(seed, rows, K, dtype):
    """h draws of the MXFP4 silu planting: 1 across the first 32-k block, Q other +-1 per row; block d rows + m of one permutation of the
    other columns: ceil((K - 32) / (Q rows)) draws use every column"""
    rng = np.random.default_rng(seed)
    q = G.SILU_Q[dtype]
    perm = 32 + rng.permutation(K - 32)
    draws = []
    for d in range(-(-(K - 32) // (q * rows))):
        a = np.zeros((rows, K), dtype=np.int64)
        a[:, :32] = 1
        for m in range(rows):
            a[m, perm[(np.arange(q) + q * (d * rows + m)) % (K - 32)]] = rng.integers(0, 2, q) * 2 - 1
        draws.append(as_t(a))
    return draws


def silu4_weights(rng, inter, K, dtype):
    """(Wg, Wu, exps_g, exps_u): +-1 in the small regime's coding, block 0 = the bias (gate: uniform GATE4 weight, up: one sign per row)"""
    Wg, Wu = (torch.from_numpy(rng.integers(0, 2, (inter, K), dtype=np.int8) * 2 - 1).double() for _ in range(2))
    eg, eu = pm1_exponents(inter, K), pm1_exponents(inter, K)
    Wg[:, :32], eg[:, 0] = GATE4[dtype]
    Wu[:, :32] = as_t(rng.integers(0, 2, inter) * 2 - 1)[:, None]
    return Wg, Wu, eg, eu


def gate_up_weights(dtype, R, inter, chunks, form=None):
    """(hs = [h rows [n, K], draw by draw], Wg, Wu float64 [E, inter, K], (exps_g, exps_u) or None) of one gate|up case"""
    K, E, n = KC * chunks, R.E, R.n
    seed = seed_of(G.MANT[dtype], R.rows_pad, inter, chunks, form is not None, len(R.name), 23)
    Wg, Wu = torch.empty((E, inter, K), dtype=F64), torch.empty((E, inter, K), dtype=F64)
    exps = None
    if form is None:
        hs = G.silu_draws(seed, n, 1, K, dtype)[0]
        for e in range(E):
            _, Wg[e], Wu[e] = G.silu_draws(seed + 1 + e, 1, inter, K, dtype)
    else:
        hs = silu4_draws(seed, n, K, dtype)
        exps = (np.zeros((E, inter, K // 32), dtype=np.int64), np.zeros((E, inter, K // 32), dtype=np.int64))
        for e in range(E):
            Wg[e], Wu[e], exps[0][e], exps[1][e] = silu4_weights(np.random.default_rng(seed + 1 + e), inter, K, dtype)
    assert G.uncovered_share(hs, n) == 0.0
    # integers (the MXFP4 gate bias of bf16: 3 halves) of at most this many bits: the dtype holds every weight
    assert max(-Wg.min().item(), Wg.max().item(), -Wu.min().item(), Wu.max().item()) <= 2 ** (G.MANT[dtype] + 1)
    return hs, Wg, Wu, exps


def gate_up_case(dtype, R, inter, chunks, form=None, check=True):
    """Case(Wg, Wu float64 [E, inter, K], exps, sums = (gate, up) of the first draw, draws = [(h [rows_pad, K], act [rows_pad k, inter]), ...])
    of the gate|up launch"""
    hs, Wg, Wu, exps = gate_up_weights(dtype, R, inter, chunks, form)
    h = torch.full((len(hs), R.rows_pad, Wg.shape[2]), float("nan"), dtype=F64)
    h[:, :R.n] = torch.stack(hs)
    gate, up, act = gate_up_ref(R, Wg, Wu, h, dtype)               # every draw at once
    (assert_silu if form is None else assert_silu4)(gate[:, R.named], up[:, R.named], dtype)
    assert torch.equal(act[:, R.named], rounded(gate[:, R.named] * up[:, R.named], dtype))
    c = Case(dtype=dtype, R=R, inter=inter, K=Wg.shape[2], Wg=Wg, Wu=Wu, exps=exps,
             draws=list(zip(h, act)), sums=(gate[0], up[0]), form=form)
    if check:
        c.checked = gate_up_faults(c)
    return c


def gate_up_faults(c):
    R, dtype, inter = c.R, c.dtype, c.inter
    h, act = c.draws[0]
    named, multi = R.named, [p for lst in R.lists.values() if len(lst) >= 2 for p in lst]
    am = lambda ps: R.entry_mask(ps, inter)
    gate, up = c.sums                                              # of the first draw
    ref = lambda f: gate_up_ref(R, c.Wg, c.Wu, h, dtype, f, c.exps or (None, None))[2]
    wrongs = {"neighbour_expert": (ref("neighbour_expert"), am(named)),
              # (silu(u) = u as well for u >= 24: a swap shows on the columns whose up value is below that)
              "gate_up_swapped": (act_ref(gate, up, dtype, "gate_up_swapped"), am(named) & (up < 24))}
    moved = [p for p in named if p % R.n != p // R.k]
    if moved:
        wrongs["source_row_p"] = (ref("source_row_p"), am(moved))
    if multi:
        wrongs["list_entry_next"] = (ref("list_entry_next"), am(multi))
    if c.form:
        wrongs["nibbles_swapped"] = (ref("nibbles_swapped"), am(named))
        wrongs["neighbour_exponent"] = (ref("neighbour_exponent"), am(named))
    done = _check(act, wrongs)
    # a truncating last cast: the products g * u are multiples of their factors' powers of two, so fewer of them are inexact than of the
    # large sums (check_large's quarter); every stored value is compared, so a share of 2 % of some thousand outputs is ample
    G.rounding_share(act[named], act_ref(gate, up, dtype, "truncate_act")[named], 0.02)
    done.append("truncate_act")
    e = max(R.lists, key=lambda x: len(R.lists[x]))                # faults of a few units, on the expert with the most rows
    A, We = h[[p // R.k for p in R.lists[e]]], torch.cat((c.Wg[e], c.Wu[e]))
    if len(A) == 1:                                              # (product_faults pairs rows: a second row of h)
        A = torch.cat((A, h[[(R.lists[e][0] // R.k + 1) % R.n]]))
    A = A[:len(A) // 2 * 2]
    P = chunk_products(A, We)
    faults = G.product_faults(seed_of(inter, c.K, 5), A, We, P, 1)
    return done + G.self_check(lambda p: G.finish_silu(p, dtype), P.sum(0)[None], {f: faults[f] for f in G.EXACT_ONLY}, True)


# ---- row independence -----------------------------------------------------------------------------------------------------------------------
def independence_cases(dtype, form=None, check=False, row=40, chunks=3):
    """(gate|up at 64 rows, the same row alone, down at 64 rows, the same row alone): expert 0 holds all 64 rows and the row's other experts
    are shared too; alone the row is row 0 of a 16-row routing whose other rows name no expert, and carries the same h / act rows, the
    same weights and the same combine weights, so the references of its k entries are those of entries 40 k .. 40 k + k - 1 of the
    64-row case (asserted here); the launches must store the same bits"""
    R64 = routing("one_expert", 64)
    k = R64.k
    idx1 = np.full((16, k), -1)
    idx1[0] = R64.idx[row]
    R1 = Routing("alone", R64.E, k, 16, 1, idx1)
    mine = slice(row * k, (row + 1) * k)
    gu = gate_up_case(dtype, R64, 256, chunks, form, check)
    h64, act64 = gu.draws[-1]
    h1 = torch.full((16, gu.K), float("nan"), dtype=F64)
    h1[0] = h64[row]
    gate1, up1, act1 = gate_up_ref(R1, gu.Wg, gu.Wu, h1, dtype)
    assert torch.equal(act1[:k], act64[mine]) and bool(torch.isnan(act1[k:]).all())
    gu1 = Case(dtype=dtype, R=R1, inter=256, K=gu.K, Wg=gu.Wg, Wu=gu.Wu, exps=gu.exps, draws=[(h1, act1)], sums=(gate1, up1), form=form)
    dn = down_case(dtype, R64, 256, chunks, "large", form, check)
    a64, y64, out64 = dn.draws[-1]
    a1 = torch.full((16 * k, dn.K), float("nan"), dtype=F64)
    a1[:k] = a64[mine]
    w1 = torch.zeros((16, k), dtype=F64)
    w1[0] = dn.w[row]
    _, y1, out1 = down_ref(R1, dn.W, a1, w1, dtype)
    assert torch.equal(y1[:k], y64[mine]) and torch.equal(out1[0], out64[row]) and bool((out1[1:] == 0).all())
    dn1 = Case(dtype=dtype, R=R1, N=256, K=dn.K, W=dn.W, exps=dn.exps, w=w1, draws=[(a1, y1, out1)], regime="large", form=form)
    if check:
        gu1.checked, dn1.checked = gate_up_faults(gu1), down_faults(dn1)
    return gu, gu1, dn, dn1


# ---- slot order -----------------------------------------------------------------------------------------------------------------------------
ORDER_TERMS = (2.0 ** 15, 2.0 ** -10, -2.0 ** 15, 2.0 ** -11)        # w_j * y_j
ORDER_W = (16.0, 2.0 ** -10, 16.0, 2.0 ** -11)
ORDER_Y = (2048.0, 1.0, -2048.0, 1.0)
ORDER_BLOCKS = ((2048.0, 9), (1.0, 0), (-2048.0, 9))                 # (weight, block exponent) of the 32-k blocks 0, 1, 2 of every expert


def f32_sum(terms, order="ascending"):
    """the fp32 sum of `terms` as an explicit sequential np.float32 loop (or a pairwise tree)"""
    t = [np.float32(x) for x in terms]
    if order == "pairwise":
        while len(t) > 1:
            t = [np.float32(t[i] + t[i + 1]) for i in range(0, len(t), 2)]
        return float(t[0])
    acc = np.float32(0.0)
    for x in (t if order == "ascending" else t[::-1]):
        acc = np.float32(acc + x)
    return float(acc)


def order_facts(k):
    """the four facts that separate the documented order from each alternative, for the unrotated pattern"""
    terms = [ORDER_TERMS[j % 4] for j in range(k)]
    asc, desc, pair, exact = f32_sum(terms), f32_sum(terms, "descending"), f32_sum(terms, "pairwise"), math.fsum(terms)
    assert (asc, desc, pair, exact) == (2.0 ** -11, 0.0, 0.0, (k // 4) * (2.0 ** -10 + 2.0 ** -11)), (asc, desc, pair, exact)
    return asc, desc, pair, exact


def order_case(dtype, k, form=None):
    """16 rows, E = 8, hidden = moe_inter = 256: slot j of row r goes to expert (r + j) % 8 and carries term (r + j) % 4 of the pattern (the
    pattern rotated by the row).  Expert e holds ORDER_BLOCKS' weight of block b in column 32 b + e of every output row; the act row of
    entry p is one-hot at the column that makes y[p] the wanted factor.  Case(W, exps, act, w, y, out)"""
    RP, E, N, K = 16, 8, 256, 256
    order_facts(k)
    r, j = np.arange(RP)[:, None], np.arange(k)[None, :]
    R = Routing("slot_order", E, k, RP, RP, (r + j) % E)
    W = torch.zeros((E, N, K), dtype=torch.float32)
    exps = np.zeros((E, N, K // 32), dtype=np.int64)
    for e in range(E):
        for b, (v, ex) in enumerate(ORDER_BLOCKS):
            W[e, :, 32 * b + e], exps[e, :, b] = v, ex
    block_of = (0, 1, 2, 1)                                      # the block whose weight is ORDER_Y[t]
    act = torch.zeros((RP * k, K), dtype=F64)
    w = torch.zeros((RP, k), dtype=F64)
    out = torch.zeros((RP, N), dtype=F64)
    for row in range(RP):
        for s in range(k):
            t, e = (row + s) % 4, (row + s) % E
            act[row * k + s, 32 * block_of[t] + e] = 1.0
            w[row, s] = ORDER_W[t]
        out[row] = f32_sum([ORDER_TERMS[(row + s) % 4] for s in range(k)])
    y_exact, y, _ = down_ref(R, W, act, torch.ones_like(w), dtype)
    assert torch.equal(y_exact, y) and all(bool((y[row * k + s] == ORDER_Y[(row + s) % 4]).all()) for row in range(RP) for s in range(k))
    assert torch.equal(rounded(w, dtype), w) and torch.equal(rounded(out, dtype), out)
    assert out[0, 0].item() == 2.0 ** -11 and len(set(out[:4, 0].tolist())) >= 2
    return Case(dtype=dtype, R=R, N=N, K=K, W=W, exps=exps if form else None, w=w, act=act, y=y, out=out, form=form)


# ---- layout restatements (from the header comments) -----------------------------------------------------------------------------------------
def gate_up_row_order(moe_inter):
    """source row of every packed gate|up row of one expert: packed row 128 t + r is gate row 64 t + r for r < 64 and up row
    moe_inter + 64 t + r - 64 otherwise"""
    p = np.arange(2 * moe_inter)
    t, r = p // 128, p % 128
    return np.where(r < 64, 64 * t + r, moe_inter + 64 * t + r - 64)


def pack_experts(W, gate_up):
    """samd_moe_pack_experts: W [E, N, K] -> per expert gemm_planting.pack_weights' tile layout, experts end to end; gate_up: N = 2 moe_inter
    and every 128-row tile holds 64 gate rows followed by the 64 up rows they multiply"""
    E, N, K = W.shape
    order = gate_up_row_order(N // 2) if gate_up else np.arange(N)
    return np.concatenate([G.pack_weights(np.ascontiguousarray(W[e][order])) for e in range(E)])


# ---- the sweeps of tests/test_gpu_moe_exact.py (tests/test_moe_planting_cpu.py builds every one of these cases) --------------------------------
def gate_up_sweep(form, rows_pad):
    """[(routing kind, moe_inter, chunks)]: 4 and 8 tile columns (moe_inter 256 / 512), hidden = 256 chunks.  The cross product (routing x
    moe_inter x chunks) is cut to one case per chunk count: the routing kind and moe_inter step with the chunk index (the kind starting at
    rows_pad / 16), so every kind meets every fourth chunk count of a row bucket and the four buckets start on different kinds; the
    `counts` routing (both sides of every 16-row tile edge) therefore runs at a quarter of the chunk counts per bucket"""
    cases = [(KINDS[(i + rows_pad // 16) % 4], (256, 512)[i % 2], c) for i, c in enumerate(chunk_sweep(form, rows_pad))]
    return cases + ([("grid_bound", 256, 1)] if rows_pad == 16 else [])


def down_sweep(form, rows_pad):
    """[(routing kind, hidden, chunks, regime)]: both regimes at every chunk count, hidden 256 / 512 (2 / 4 tile columns; the launch takes
    hidden % 256 == 0 only) alternating against them.  Cut like gate_up_sweep: the routing kind steps with chunk index + regime, so a
    kind meets a chunk count in one regime and the next count in the other, never the same count in both"""
    cases = [(KINDS[(i + r + rows_pad // 16) % 4], (256, 512)[(i + r) % 2], c, regime)
             for i, c in enumerate(chunk_sweep(form, rows_pad)) for r, regime in enumerate(("small", "large"))]
    return cases + ([("grid_bound", 256, 2, "small")] if rows_pad == 16 else [])
