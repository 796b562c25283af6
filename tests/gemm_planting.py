"""Exact-integer inputs for the model-dtype weight-streaming GEMMs, their exact references and named faults (numpy + torch only; no
product import).

The kernels compute sum_k A[m][k] * W[n][k] in fp32.  With integer A and W whose every partial sum stays below 2^24 the fp32 result is
the exact integer in any summation order and at any split, so the value a kernel must store is fully determined: the exact sum, rounded
ONCE to the model dtype T (or not at all for fp32 split-K partials).  Comparisons are therefore equalities, and one wrong product fails.

  small sums   W dense +-1, A in {-1, 0, +1} with P(nonzero) = min(1, (BAR_T / 6)^2 / K), BAR = 2^8 (bf16) / 2^11 (fp16): every exact
               output has |sum| < BAR_T (asserted from the reference, no output left out), a range in which every integer and its
               neighbours are representable -- a sum that is off by any amount stores another value.  Where A is sparse (bf16, K > 1792)
               `small_draws` keeps drawing fresh A until every k column has carried a nonzero activation in a live row of some draw.
  large sums   A dense in [-8, 8], W dense in [-wmax, wmax]; wmax (>= 8) is chosen from (K, T) so that the sums have a standard deviation
               of 2^11.5 (bf16) / 2^13.5 (fp16): at W in [-8, 8] and K = 256 most sums are exactly representable (fp16: all of them) and
               the conditions below could not hold.  |sum| <= 8 wmax K < 2^24.  want = exact.to(T), one round-to-nearest-even;
               `check_large` asserts from the reference that it holds inexact outputs, exact ties, no overflow, and that a truncating
               cast differs on more than a quarter of the outputs.
  silu         gate sums are integers in [24, 64] (bf16) / [24, 512] (fp16), up sums nonzero integers with |u| <= 64: column 0 of A is a
               bias of 1 against a constant gate weight G0 / an up weight +-34, every row of A carries exactly Q other nonzeros (+-1,
               Q = 20 / 30) against dense +-1 weights, so the ranges hold by construction.  For g >= 24, 1 + exp(-g) is 1 in fp32:
               silu(g) = g and the output is the single rounding of the exact product g * u (the float64 reference with HF's roundings
               gives the same value; asserted).  The nonzero positions of draw d, row m are block d * rows + m of one random
               permutation of the columns: ceil((K - 1) / (Q rows)) draws use every column.
  rope         cos | sin per (row, j) from {(1, 0), (0, 1), (-1, 0), (0, -1)}, index (row + j) mod 4: neighbouring rows and neighbouring
               j differ, and every rotated output is exactly +-x1 or +-x2 of the rounded sums.

References are float64 (exact below 2^53) with roundings where the kernels document them: projection output to T; residual sum to T;
squares of the stored values; silu(gate.to(T)).to(T) * up.to(T) rounded; q|k|v sums to T before the rotation.

Faults: `product_faults` recomputes the per-split exact sums with one named fault each and says which outputs it touches; `self_check`
pushes both through the entry point's epilogue and requires that the fault changes at least half of the outputs it touches, and at
least one, under the equality the test uses.

The three packed layouts are restated from their header comments (`pack_weights`, `pack_groups`, `pack_qkv`), not from the pack kernels."""
import math

import numpy as np
import torch

F64 = torch.float64
KC = 256                                               # k elements per chunk
DTYPES = (torch.float16, torch.bfloat16)
BAR = {torch.float16: 2 ** 11, torch.bfloat16: 2 ** 8}
MANT = {torch.float16: 10, torch.bfloat16: 7}
LARGE_SIGMA = {torch.float16: 2.0 ** 13.5, torch.bfloat16: 2.0 ** 11.5}
GATE_RANGE = {torch.float16: (24, 512), torch.bfloat16: (24, 64)}
SILU_Q = {torch.float16: 30, torch.bfloat16: 20}       # nonzeros per row of A besides the bias column
UP_BIAS, UP_MAX = 34, 64
MAX_DRAWS = 64

# ---- the cases of tests/test_gpu_gemm_exact.py (tests/test_gemm_planting_cpu.py runs the helper's conditions at every one of them) ----------
ROWS = (16, 32, 48, 64)
SKINNY_N = (128, 384)
CHUNK_SPLITS = ((1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (7, 1), (2, 2), (3, 2), (5, 2), (7, 3), (8, 8), (9, 4), (10, 3))
SILU_CHUNKS = tuple(range(1, 8))
CS_ROWS = (16, 8)
CS_N = (16, 48)
CS_CHUNKS = tuple(range(1, 27)) + (43,)
CS_LARGE_CHUNKS = 20                                   # K = 5120: three chunks per wave through the refill branch
ROPE_CHUNKS = tuple(range(1, 10)) + (16,)
ROPE_HEADS = ((5, 5), (2, 2), (8, 1), (4, 1))          # (H, Hkv): 48-column tiles straddling heads and q | k, 48, 64 (1280 % 48 != 0), GQA at 48
ROPE_MAX_LEN = 96


def rounded(x, dtype):
    """float64 tensor of the values `x` takes in `dtype` (one round-to-nearest-even)"""
    return x.to(dtype).to(F64)


def truncated(x, dtype):
    """float64 tensor of `x` cast to `dtype` by truncation (round toward zero)"""
    r = x.to(dtype)
    over = r.to(F64).abs() > x.abs()
    back = (r.view(torch.int16) - 1).view(dtype)        # sign-magnitude: one step toward zero
    return torch.where(over, back, r).to(F64)


def ulp(v, dtype):
    """spacing of `dtype` at |v| for normal values (float64)"""
    _, e = torch.frexp(v.abs().clamp(min=2.0 ** -14))
    return torch.ldexp(torch.ones_like(v), e - 1 - MANT[dtype])


def as_t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ---- input recipes --------------------------------------------------------------------------------------------------------------------------
def density(K, dtype):
    return min(1.0, (BAR[dtype] / 6.0) ** 2 / K)


def small_draws(seed, rows, N, K, dtype, live_rows=None):
    """([A_0, A_1, ...], W): W [N, K] dense +-1; every A [rows, K] in {-1, 0, 1} at `density`; draws are added until every k column carries
    a nonzero activation in one of the first `live_rows` rows of some draw"""
    rng = np.random.default_rng(seed)
    live = rows if live_rows is None else live_rows
    W = as_t(rng.integers(0, 2, (N, K)) * 2 - 1)
    p, draws, covered = density(K, dtype), [], np.zeros(K, dtype=bool)
    while not covered.all():
        assert len(draws) < MAX_DRAWS, (rows, K, dtype)
        a = (rng.integers(0, 2, (rows, K)) * 2 - 1) * (rng.random((rows, K)) < p)
        covered |= (a[:live] != 0).any(0)
        draws.append(as_t(a))
    return draws, W


def uncovered_share(draws, live_rows=None):
    """share of the k columns that no live row of any draw multiplies with a nonzero activation"""
    used = torch.zeros(draws[0].shape[1], dtype=torch.bool)
    for a in draws:
        used |= (a[:live_rows] != 0).any(0)
    return 1.0 - used.double().mean().item()


def assert_small(exact, dtype):
    """the small-sum condition, from the reference alone: EVERY exact output is an integer with |sum| < BAR (cap on excluded outputs: 0)"""
    assert bool((exact == exact.round()).all()) and exact.abs().max().item() < BAR[dtype], exact.abs().max().item()


def large_wmax(K, dtype):
    var = LARGE_SIGMA[dtype] ** 2 / (24.0 * K)          # var of a uniform integer in [-8, 8] is 24, in [-w, w] it is w (w + 1) / 3
    return max(8, int(math.ceil((math.sqrt(1.0 + 12.0 * var) - 1.0) / 2.0)))


def large_case(seed, rows, N, K, dtype):
    """(A [rows, K] dense in [-8, 8], W [N, K] dense in [-wmax, wmax])"""
    rng = np.random.default_rng(seed)
    w = large_wmax(K, dtype)
    assert 8 * w * K < 2 ** 24
    return as_t(rng.integers(-8, 9, (rows, K))), as_t(rng.integers(-w, w + 1, (N, K)))


def check_large(exact, dtype):
    """the rounding-regime conditions, from the reference alone; returns (inexact share, tie share, share a truncating cast changes)"""
    assert exact.abs().max().item() < 2 ** 24
    want, tr = rounded(exact, dtype), truncated(exact, dtype)
    assert bool(torch.isfinite(want).all())
    inexact = tr != exact
    tie = inexact & (2.0 * (exact - tr).abs() == ulp(tr, dtype))
    differs = (tr != want).double().mean().item()
    assert bool(inexact.any()) and bool(tie.any()) and differs > 0.25, (inexact.double().mean().item(), tie.double().mean().item(), differs)
    up = tie & (want != tr)
    assert bool(up.any()) and bool((tie & (want == tr)).any())          # ties go both ways under round-to-nearest-even
    return inexact.double().mean().item(), tie.double().mean().item(), differs


def silu_draws(seed, rows, inter, K, dtype):
    """([A_0, ...], Wg [inter, K], Wu [inter, K]) of the silu planting (module docstring)"""
    rng = np.random.default_rng(seed)
    q = SILU_Q[dtype]
    lo, hi = GATE_RANGE[dtype]
    g0 = (lo + hi) // 2
    assert g0 - q >= lo and g0 + q <= hi and UP_BIAS - q > 0 and UP_BIAS + q <= UP_MAX
    Wg, Wu = rng.integers(0, 2, (inter, K)) * 2 - 1, rng.integers(0, 2, (inter, K)) * 2 - 1
    Wg[:, 0] = g0
    Wu[:, 0] = UP_BIAS * (rng.integers(0, 2, inter) * 2 - 1)
    perm = 1 + rng.permutation(K - 1)
    draws = []
    for d in range(-(-(K - 1) // (q * rows))):
        a = np.zeros((rows, K), dtype=np.int64)
        a[:, 0] = 1
        for m in range(rows):
            cols = perm[(np.arange(q) + q * (d * rows + m)) % (K - 1)]
            a[m, cols] = rng.integers(0, 2, q) * 2 - 1
        draws.append(as_t(a))
    return draws, as_t(Wg), as_t(Wu)


def assert_silu(gate, up, dtype):
    """the silu planting's conditions from the reference alone: ranges, and the float64 reference with HF's roundings == round(g * u)"""
    lo, hi = GATE_RANGE[dtype]
    assert bool((gate == gate.round()).all()) and gate.min().item() >= lo and gate.max().item() <= hi
    assert bool((up == up.round()).all()) and up.abs().min().item() >= 1 and up.abs().max().item() <= UP_MAX
    assert torch.equal(silu_ref(gate, up, dtype), rounded(gate * up, dtype))
    assert bool(((1.0 + torch.exp(-gate.float())) == 1.0).all())         # 1 + exp(-g) in fp32


def rope_cs(rows):
    """float32 [64][128] cos | sin rows (the layout of samd_rope_rows): (cos, sin) of (row, j) = the ((row + j) mod 4)-th of
    (1, 0), (0, 1), (-1, 0), (0, -1); rows >= `rows` are NaN"""
    idx = (torch.arange(rows)[:, None] + torch.arange(64)[None, :]) % 4
    cs = torch.full((64, 128), float("nan"), dtype=torch.float32)
    cs[:rows, :64] = torch.tensor([1.0, 0.0, -1.0, 0.0])[idx]
    cs[:rows, 64:] = torch.tensor([0.0, 1.0, 0.0, -1.0])[idx]
    return cs


# ---- exact references -----------------------------------------------------------------------------------------------------------------------
def chunk_products(A, W):
    """float64 [chunks, rows, N]: the exact sums over every 256-wide k chunk"""
    rows, K = A.shape
    return torch.einsum("mck,nck->cmn", A.view(rows, K // KC, KC), W.view(W.shape[0], K // KC, KC))


def split_range(s, chunks, splits):
    return s * chunks // splits, (s + 1) * chunks // splits


def split_sums(P, splits):
    """float64 [splits, rows, N]: the exact sum of every split over ITS OWN chunk range [s chunks / splits, (s + 1) chunks / splits)"""
    chunks = P.shape[0]
    return torch.stack([P[slice(*split_range(s, chunks, splits))].sum(0) for s in range(splits)])


def finish_skinny(parts, dtype, trunc=False):
    """what samd_gemm_skinny stores: the sum in T for one split, the fp32 partials (exact) otherwise"""
    if parts.shape[0] > 1:
        assert parts.abs().max().item() < 2 ** 24
        return parts
    return (truncated if trunc else rounded)(parts[0], dtype)


def silu_ref(gate, up, dtype, fault=None):
    """LlamaMLP act_fn(gate_proj(x)) * up_proj(x) with the model dtype's roundings, in float64"""
    if fault == "gate_up_swapped":
        gate, up = up, gate
    g, u = rounded(gate, dtype), rounded(up, dtype)
    return rounded(rounded(g / (1.0 + torch.exp(-g)), dtype) * u, dtype)


def finish_silu(parts, dtype, fault=None):
    """parts [1, rows, 2 inter] = gate | up sums"""
    inter = parts.shape[2] // 2
    return silu_ref(parts[0][:, :inter], parts[0][:, inter:], dtype, fault)


def tree_ssq(x):
    """fp32 [rows, N / 16]: sums of 16 squares in the order of a 4-step xor butterfly over the 16 columns (fp32 throughout)"""
    q = x.float() * x.float()
    q = q.view(x.shape[0], -1, 16)
    for _ in range(4):
        q = q[..., 0::2] + q[..., 1::2]
    return q[..., 0]


def cs_residual_ref(exact, x0, dtype, fault=None):
    """(x, ssq): x = (x0 + proj.to(T)).to(T) in float64, ssq fp32 [rows, N / 16] of the stored values"""
    o = exact if fault == "no_proj_round" else (truncated if fault == "truncate" else rounded)(exact, dtype)
    x = (truncated if fault == "truncate" else rounded)(x0 + o, dtype)
    return x, tree_ssq(x)


def rope_ref(exact, cs, H, Hkv, dtype, fault=None):
    """float64 (q [rows, H, 128], k [rows, Hkv, 128], v [rows, Hkv, 128]) of the q|k|v sums `exact` [rows, (H + 2 Hkv) 128]: sums rounded
    to T, q and k heads rotated (HF rotate_half: columns j and j + 64 are a pair), every output rounded to T"""
    rows = exact.shape[0]
    y = rounded(exact, dtype).view(rows, H + 2 * Hkv, 128)
    c, s = cs[:rows, None, :64].double(), cs[:rows, None, 64:].double()
    if fault == "cs_neighbour_row":
        nb = torch.arange(rows) ^ 1
        nb = torch.where(nb < rows, nb, torch.arange(rows))
        c, s = c[nb], s[nb]
    if fault == "sine_sign":
        s = -s
    x1, x2 = y[:, :H + Hkv, :64], y[:, :H + Hkv, 64:]
    if fault == "partner_xor32":
        x2 = x1[..., torch.arange(64) ^ 32]
    rot = rounded(torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1), dtype)
    return rot[:, :H], rot[:, H:], y[:, H + Hkv:]


def rope_partner_touched(cs, rows, heads):
    """outputs of the rotated heads whose formula reads the partner x2 with a nonzero coefficient: [rows, heads, 128]"""
    c, s = cs[:rows, None, :64], cs[:rows, None, 64:]
    return torch.cat((s != 0, c != 0), dim=-1).expand(rows, heads, 128)


# ---- named faults ---------------------------------------------------------------------------------------------------------------------------
EXACT_ONLY = ("product_dropped", "product_doubled", "vec8_dropped")        # faults of a few units: visible where integers are stored exactly


def product_faults(seed, A, W, P, splits, samples=16):
    """{name: (wrong [splits, rows, N] float64 exact sums with the fault, touched bool mask)} for the faults of the product itself"""
    rng = np.random.default_rng(seed)
    rows, K = A.shape
    N, chunks = W.shape[0], P.shape[0]
    parts = split_sums(P, splits)
    split_of = np.zeros(chunks, dtype=np.int64)
    for s in range(splits):
        split_of[slice(*split_range(s, chunks, splits))] = s
    out = {}

    def fresh():
        return parts.clone(), torch.zeros_like(parts, dtype=torch.bool)

    for name, sign in (("product_dropped", -1.0), ("product_doubled", 1.0)):            # one product at a sampled (m, n, k)
        wrong, touched = fresh()
        for _ in range(samples):
            m, n = int(rng.integers(rows)), int(rng.integers(N))
            nz = torch.nonzero(A[m] * W[n]).view(-1)
            if len(nz) == 0:
                continue
            k = int(nz[int(rng.integers(len(nz)))])
            wrong[split_of[k // KC], m, n] += sign * A[m, k] * W[n, k]
            touched[split_of[k // KC], m, n] = True
        out[name] = (wrong, touched)
    wrong, touched = fresh()                                                            # one 8-element vector of one lane (column n, all rows)
    live = (A.view(rows, K // 8, 8) != 0).any(-1)                                       # [rows, K / 8]: a row the vector multiplies with only zeros
    vecs = torch.nonzero(live.any(0)).view(-1)                                          # computes the same sum without it
    for _ in range(samples):
        n, k0 = int(rng.integers(N)), 8 * int(vecs[int(rng.integers(len(vecs)))])
        wrong[split_of[k0 // KC], :, n] -= A[:, k0:k0 + 8] @ W[n, k0:k0 + 8]
        touched[split_of[k0 // KC], :, n] |= live[:, k0 // 8]
    out["vec8_dropped"] = (wrong, touched)
    c = int(rng.integers(chunks))                                                        # k block b ^ 1 of the A tile in one chunk
    wrong, touched = fresh()
    a_sw = A[:, KC * c:KC * (c + 1)].view(rows, 4, 64)[:, [1, 0, 3, 2]].reshape(rows, KC)
    wrong[split_of[c]] += a_sw @ W[:, KC * c:KC * (c + 1)].t() - P[c]
    touched[split_of[c]] = True
    out["kblock_xor1"] = (wrong, touched)
    perm = torch.arange(rows) ^ 1                                                        # A row m ^ 1
    out["row_xor1"] = (parts[:, perm], torch.ones_like(parts, dtype=torch.bool))
    if chunks >= 2:                                                                      # chunk c against the A tile of chunk c - 1
        c = int(rng.integers(1, chunks))
        wrong, touched = fresh()
        wrong[split_of[c]] += A[:, KC * (c - 1):KC * c] @ W[:, KC * c:KC * (c + 1)].t() - P[c]
        touched[split_of[c]] = True
        out["stale_a_tile"] = (wrong, touched)
    s = int(rng.integers(max(1, splits - 1)))                                            # a split boundary off by one chunk
    c1 = split_range(s, chunks, splits)[1]
    for name, delta in (("chunk_dropped", -P[c1 - 1]), ("chunk_twice", P[c1] if c1 < chunks else P[c1 - 1])):
        wrong, touched = fresh()
        wrong[s] += delta
        touched[s] = True
        out[name] = (wrong, touched)
    return out


def self_check(finish, parts, faults, exact_integers, extra=None):
    """every fault that applies must change >= half of the outputs it touches, and at least one, under equality.  finish(parts) -> the
    stored tensor (or a tuple of tensors); `extra` = {name: (wrong stored tensors, touched masks)} for faults of the epilogue itself.
    Returns the names checked."""
    def flat(t):
        return torch.cat([x.reshape(-1).double() for x in (t if isinstance(t, tuple) else (t,))])
    want = flat(finish(parts))
    done = []
    for name, (wrong, touched) in faults.items():
        if name in EXACT_ONLY and not exact_integers:
            continue
        big = torch.where(touched, torch.full_like(parts, 3000.5), torch.zeros_like(parts))
        t_out = flat(finish(parts + big)) != want                   # the stored outputs that depend on a touched sum
        changed = (flat(finish(wrong)) != want)[t_out]
        assert changed.numel() > 0 and bool(changed.any()) and changed.double().mean().item() >= 0.5, (name, changed.double().mean().item())
        done.append(name)
    for name, (wrong, touched) in (extra or {}).items():
        changed = (flat(wrong) != want)[flat(touched).bool()]
        assert changed.numel() > 0 and bool(changed.any()) and changed.double().mean().item() >= 0.5, (name, changed.double().mean().item())
        done.append(name)
    return done


# ---- layout restatements (from the header comments) -----------------------------------------------------------------------------------------
def pack_weights(W):
    """samd_gemm_pack_weights: block (tile t = 128 rows, chunk c = 256 k) is 4096 units of 8 elements at (t K/256 + c) 4096; unit
    (2 b + j) 512 + tid holds W[128 t + 16 w + n][256 c + 64 b + 16 g + 8 j .. + 7] for tid = 64 w + 16 g + n"""
    N, K = W.shape
    v = W.reshape(N // 128, 8, 16, K // KC, 4, 4, 2, 8)                       # [t][w][n][c][b][g][j][e]
    return np.ascontiguousarray(v.transpose(0, 3, 4, 6, 1, 5, 2, 7)).reshape(-1)


def pack_groups(W):
    """samd_gemm_pack_groups: (group gi = 16 rows, chunk c) is 512 units at (gi K/256 + c) 512; unit (2 b + j) 64 + lane holds
    W[16 gi + n][256 c + 64 b + 16 g + 8 j .. + 7] for lane = 16 g + n"""
    N, K = W.shape
    v = W.reshape(N // 16, 16, K // KC, 4, 4, 2, 8)                            # [gi][n][c][b][g][j][e]
    return np.ascontiguousarray(v.transpose(0, 2, 3, 5, 4, 1, 6)).reshape(-1)


def qkv_tile_groups(heads_total, n_cu):
    """column groups (of 16) per tile of samd_gemm_pack_qkv64 / samd_gemm_qkv_rope: 3 (48 columns) when 48 divides the matrix and 48-column
    tiles need no more rounds of workgroups over the CUs than 64-column tiles, else 4"""
    N = heads_total * 128
    if N % 48:
        return 4
    rounds = lambda t: -(-t // n_cu)
    return 3 if rounds(N // 48) * 48 < rounds(N // 64) * 64 else 4


def qkv_row_permutation(heads_total, cg):
    """rotate_half row permutation: pairs are numbered head by head (pair P = 64 head + j = head columns j and 64 + j); tile t holds pairs
    [8 cg t, 8 cg (t + 1)); packed row 16 cg t + q = the FIRST column of pair 8 cg t + q for q < 8 cg, else the SECOND of pair 8 cg t + q - 8 cg"""
    pp = 8 * cg
    r = np.arange(heads_total * 128)
    t, q = r // (2 * pp), r % (2 * pp)
    pair = pp * t + q % pp
    return 128 * (pair // 64) + pair % 64 + 64 * (q >= pp)


def pack_qkv(W, cg):
    """samd_gemm_pack_qkv64 with tiles of 16 cg columns: block (tile t, chunk c) is 512 cg units at (t K/256 + c) 512 cg; unit
    (2 bl + j) 128 cg + x holds Wperm[16 cg t + 16 g_c + n][256 c + 64 (2 kh + bl) + 16 g + 8 j .. + 7] for x = 64 (cg kh + g_c) + 16 g + n"""
    N, K = W.shape
    v = W[qkv_row_permutation(N // 128, cg)].reshape(N // (16 * cg), cg, 16, K // KC, 2, 2, 4, 2, 8)     # [t][g_c][n][c][kh][bl][g][j][e]
    return np.ascontiguousarray(v.transpose(0, 3, 5, 7, 4, 1, 6, 2, 8)).reshape(-1)


def pair_shares(n_pairs, n_cu):
    """(grid, set of pairs per workgroup) of samd_gemm_pairs_silu: one workgroup per CU with an even share of the pairs, more workgroups
    (a CU count at a time) only while a share would exceed 4 pairs"""
    grid = min(n_pairs, n_cu)
    while -(-n_pairs // grid) > 4:
        grid += n_cu
    return grid, {(b + 1) * n_pairs // grid - b * n_pairs // grid for b in range(grid)}


def share_pairs(n_cu):
    """pair counts whose workgroups hold 1 (one and three workgroups), 1, 1-2, 2-3, 3-4, exactly 4 pairs, and 2-3 on a grid of two
    workgroups per CU; all but the first two are multiples of 4 (inter % 64 == 0)"""
    r4 = lambda x: max(4, int(x) // 4 * 4)
    return [(1, {1}, 1), (3, {1}, 1), (r4(n_cu), {1}, 1), (r4(n_cu * 1.17), {1, 2}, 1), (r4(n_cu * 2.73), {2, 3}, 1), (r4(n_cu * 3.9), {3, 4}, 1),
            (4 * n_cu, {4}, 1), (r4(n_cu * 5.08), {2, 3}, 2)]


# ---- cases: inputs, conditions and self check in one place (the CPU file builds every one of them, the GPU file builds and launches) --------
def _seed(*xs):
    s = 0
    for x in xs:
        s = (s * 1000003 + int(x) + 7) % (2 ** 31 - 1)
    return s


def _draws(seed, rows, N, K, dtype, regime, live_rows=None):
    if regime == "small":
        draws, W = small_draws(seed, rows, N, K, dtype, live_rows)
        assert uncovered_share(draws, live_rows) == 0.0
    else:
        A, W = large_case(seed, rows, N, K, dtype)
        draws = [A]
    assert torch.equal(rounded(W, dtype), W) and all(torch.equal(rounded(a, dtype), a) for a in draws)
    return draws, W


def rounding_share(want, wrong, more_than):
    share = (want != wrong).double().mean().item()
    assert share > more_than, share
    return share


def skinny_case(dtype, rows, N, chunks, splits, regime):
    """(W, [(A, stored), ...]): stored = the T output (float64 values) for one split, the exact fp32 partials [splits, rows, N] otherwise"""
    seed = _seed(MANT[dtype], rows, N, chunks, splits, regime == "small")
    draws, W = _draws(seed, rows, N, KC * chunks, dtype, regime)
    out = []
    for i, A in enumerate(draws):
        P = chunk_products(A, W)
        parts = split_sums(P, splits)
        if regime == "small":
            assert_small(P.sum(0), dtype)
        elif splits == 1:
            check_large(parts[0], dtype)
        if i == 0:
            done = self_check(lambda p: finish_skinny(p, dtype), parts, product_faults(seed + 1, A, W, P, splits), regime == "small" or splits > 1)
            assert len(done) >= (4 if chunks == 1 else 5)
        out.append((A, finish_skinny(parts, dtype)))
    return W, out


def silu_case(dtype, rows, inter, chunks):
    """(Wg, Wu, [(A, stored [rows, inter]), ...])"""
    seed = _seed(MANT[dtype], rows, inter, chunks, 11)
    draws, Wg, Wu = silu_draws(seed, rows, inter, KC * chunks, dtype)
    assert uncovered_share(draws) == 0.0
    W = torch.cat((Wg, Wu))
    assert torch.equal(rounded(W, dtype), W)
    out = []
    for i, A in enumerate(draws):
        P = chunk_products(A, W)
        parts = P.sum(0)[None]
        assert_silu(parts[0][:, :inter], parts[0][:, inter:], dtype)
        want = finish_silu(parts, dtype)
        if i == 0:
            # (silu(u) = u as well for u >= 24: a swap shows on the columns whose up value is below that)
            extra = {"gate_up_swapped": (finish_silu(parts, dtype, "gate_up_swapped"), parts[0][:, inter:] < GATE_RANGE[dtype][0])}
            self_check(lambda p: finish_silu(p, dtype), parts, product_faults(seed + 1, A, W, P, 1), True, extra)
        out.append((A, want))
    return Wg, Wu, out


def cs_case(dtype, rows, N, chunks, regime):
    """(W, x0 [16, N], [(A [16, K], x [rows, N], ssq fp32 [rows, N / 16]), ...]); only rows < `rows` of A are live"""
    seed = _seed(MANT[dtype], rows, N, chunks, regime == "small", 5)
    draws, W = _draws(seed, 16, N, KC * chunks, dtype, regime, rows)
    rng = np.random.default_rng(seed + 2)
    x0 = rounded(as_t(rng.integers(-16, 17, (16, N)) if regime == "small" else rng.integers(-4096, 4097, (16, N))), dtype)
    fin = lambda p, f=None: cs_residual_ref(p[0], x0[:rows], dtype, f)
    out = []
    for i, A in enumerate(draws):
        P = chunk_products(A[:rows], W)
        parts = P.sum(0)[None]
        x, ssq = fin(parts)
        if regime == "small":
            assert_small(parts[0], dtype)
            assert x.abs().max().item() <= BAR[dtype] and bool((x == x0[:rows] + parts[0]).all())
            exact_ssq = (x * x).view(rows, N // 16, 16).sum(-1)
            assert exact_ssq.max().item() <= 2 ** 24 and torch.equal(ssq.double(), exact_ssq)
        else:
            check_large(parts[0], dtype)
            rounding_share(x, fin(parts, "truncate")[0], 0.25)
            rounding_share(x, fin(parts, "no_proj_round")[0], 0.02)
        if i == 0:
            self_check(fin, parts, product_faults(seed + 1, A[:rows], W, P, 1), regime == "small")
        out.append((A, x, ssq))
    return W, x0, out


ROPE_FAULTS = ("partner_xor32", "sine_sign", "cs_neighbour_row")


def rope_case(dtype, rows, H, Hkv, chunks, regime):
    """(W, cs fp32 [64, 128], [(A, q [rows, H, 128], k [rows, Hkv, 128], v [rows, Hkv, 128]), ...])"""
    seed = _seed(MANT[dtype], rows, H, Hkv, chunks, regime == "small", 3)
    N = (H + 2 * Hkv) * 128
    draws, W = _draws(seed, rows, N, KC * chunks, dtype, regime)
    cs = rope_cs(rows)
    fin = lambda p, f=None: rope_ref(p[0], cs, H, Hkv, dtype, f)
    out = []
    for i, A in enumerate(draws):
        if i == 0:
            P = chunk_products(A, W)
            parts = P.sum(0)[None]
        else:
            parts = (A @ W.t())[None]
        (assert_small if regime == "small" else check_large)(parts[0], dtype)
        q, k, v = fin(parts)
        if i == 0:
            none = torch.zeros_like(v, dtype=torch.bool)
            sine = torch.cat((cs[:rows, None, 64:] != 0,) * 2, dim=-1)
            touched = {"partner_xor32": (rope_partner_touched(cs, rows, H), rope_partner_touched(cs, rows, Hkv), none),
                       "sine_sign": (sine.expand(rows, H, 128), sine.expand(rows, Hkv, 128), none),
                       "cs_neighbour_row": (torch.ones_like(q, dtype=torch.bool), torch.ones_like(k, dtype=torch.bool), none)}
            extra = {f: (fin(parts, f), touched[f]) for f in ROPE_FAULTS}
            self_check(fin, parts, product_faults(seed + 1, A, W, P, 1), regime == "small", extra)
        out.append((A, q, k, v))
    return W, cs, out
