"""Exact-integer inputs for the five dense weight-only streaming GEMMs (samd_gemm_skinny_f8, _f8b, _f4, _i4, _i8) at every stream length,
their float64 references and the named faults of a software-pipelined stream (numpy + torch only; no product import).  The method is
tests/gemm_planting.py's: every weight is (code - zero) * 2^e, every activation an integer, and sum_k |A| |W| stays below 2^24 quanta, so
the fp32 sum over ANY set of chunks in ANY order is exact.  What a launch must store is then determined bit for bit: the exact sum of a
split's own chunks as an fp32 partial, or its single rounding to the model dtype at one split.  Every comparison is an equality.

  stream plan  the stream length L of a workgroup is the number of 256-k chunks of its split, c1 - c0 with c0 = split * chunks // splits
               (`split_lengths`).  LENGTHS = 1 .. 18 run as whole launches (K = 256 L, one split), and SPLIT_PLANS puts every length beside
               a split of another length: (2 L + 1, 2) gives L | L + 1; (18, 18) all ones; the three-way plans are uneven in all three
               positions; gemm_planting.CHUNK_SPLITS are the plans of the model-dtype sweep.  LONG_CHUNKS = 56 (K = 14336) runs whole and
               at the product's own split count.  `assert_plan` proves both coverages.  The kernels static_assert DEPTH <= 8, so 1 .. 18
               reaches 2 DEPTH + 2 whatever a depth is retuned to: the plan does not rest on the DEPTH table below.
  weights      codes over their whole range where the 2^24 bound allows it: INT4 / INT8 codes and zero points over all 16 / 256 values,
               all 16 e2m1 codes, the integer e4m3 values up to a `qmax` that `weights` lowers with K (see `_fp8_codes`).
  side data    scales are powers of two, 2^(EMIN + level).  Group- and block-scaled formats (i4, i8: per row and 128 k; f4: per row and
               32 k): level = (i + row + r[row][chunk]) mod 4 for the i-th group or block of a chunk with r drawn per (row, chunk) --
               neighbours inside a chunk always differ, chunks and rows differ where r does.  f8b (per 128-row tile and 128 k):
               level = (block + 5 tile) mod 11, so the two blocks of a chunk, the tiles, and chunks up to 9 apart (block distance 2 d,
               11 odd) ALL differ -- a workgroup sees two scales per chunk and both must be visible.  f8 has one scale per row (level =
               row mod 4) and no side data that changes along k.
  activations  dense integers in [-amax, amax], amax = min(AMAX_CAP, (2^24 - 1) // max_n sum_k |W[n][k]| / quantum): the bound then
               holds for ANY activations in the range, and `check_case` asserts it on the drawn ones.
  quantum      2^EMIN = 2^-9 for every format (e2m1's half steps sit on block exponents from EMIN + 1): 2^24 quanta = 2^15, so every
               output is finite in fp16 as well.

`stream_faults` recomputes the per-split exact sums with one named fault of the pipeline each (a chunk dropped at either end, counted
twice, multiplied by the weights or widened with the side data of chunk c + DEPTH, multiplied by the A chunk that held its ring buffer
before, or handed to the neighbouring split); `fault_shares` requires that each changes at least half of the outputs it touches, and at
least one, under the equality the GPU test uses.  DEPTH restates the kernels' pipeline depths for these faults only."""
import numpy as np
import torch

import gemm_planting as G
import moe_planting as MP
from gemm_planting import KC, as_t, rounded

F64 = torch.float64
DTYPES = G.DTYPES
FORMATS = ("f8", "f8b", "f4", "i4", "i8")
ROWS = (16, 32, 48, 64)
N = 256                                                  # two 128-column tiles: the second one's weight offset is exercised
EMIN = -9
QUANTUM = 2.0 ** EMIN
AMAX_CAP = 16
LEVELS = 4                                               # scale levels of f8, f4, i4, i8
F8B_PERIOD = 11                                          # scale levels of f8b (module docstring)
F8_QMAX = (448, 128, 32, 8, 3)                           # candidate bounds on the integer e4m3 values, widest first
F8_AMIN = 4                                              # ... the widest whose amax reaches this is taken
MAX_DISTANCE = 9                                         # chunk c differs from chunks c +- 1 .. 9: DEPTH <= 8, ring of DEPTH + 1 buffers
# restated from csrc/gemm_kernels.hip for the faults only (rows -> pipeline depth)
DEPTH = {"f8": {16: 4, 32: 4, 48: 4, 64: 3}, "f8b": {16: 4, 32: 3, 48: 4, 64: 3}, "f4": {16: 8, 32: 4, 48: 5, 64: 3},
         "i4": {16: 8, 32: 4, 48: 5, 64: 3}, "i8": {16: 4, 32: 4, 48: 4, 64: 3}}

# ---- the stream plan ------------------------------------------------------------------------------------------------------------------------
LENGTHS = tuple(range(1, 19))
LONG_CHUNKS = 56                                         # K = 14336


def split_lengths(chunks, splits):
    """stream length of every split: c1 - c0 with c0 = split * chunks // splits, the kernels' rule"""
    return [(s + 1) * chunks // splits - s * chunks // splits for s in range(splits)]


def _unique(seq):
    return tuple(dict.fromkeys(seq))


SPLIT_PLANS = _unique(tuple((2 * L + 1, 2) for L in range(1, 18)) + ((18, 18),) + ((4, 3), (5, 3), (7, 3), (8, 3), (25, 3), (26, 3))
                      + tuple(G.CHUNK_SPLITS))             # (chunks, splits)
WHOLE_CHUNKS = LENGTHS + (LONG_CHUNKS,)
ALL_CHUNKS = tuple(sorted(set(WHOLE_CHUNKS) | {c for c, _ in SPLIT_PLANS}))


def assert_plan():
    """every length 1 .. 18 runs as a whole launch, and as one split of a launch that has a split of another length beside it"""
    assert set(LENGTHS) == set(range(1, 19)) and set(LENGTHS) <= set(WHOLE_CHUNKS)
    beside = set()
    for chunks, splits in SPLIT_PLANS:
        ls = split_lengths(chunks, splits)
        assert sum(ls) == chunks and min(ls) >= 1 and splits <= chunks
        if splits > 1 and len(set(ls)) > 1:
            beside |= set(ls)
    assert set(LENGTHS) <= beside, sorted(set(LENGTHS) - beside)
    assert (18, 18) in SPLIT_PLANS and set(G.CHUNK_SPLITS) <= set(SPLIT_PLANS)
    return sorted(beside)


# ---- per-format recipes ---------------------------------------------------------------------------------------------------------------------
_E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()      # the value of every e4m3fn byte (NaN: 0x7f, 0xff)


def _fp8_codes(rng, shape, qmax):
    """(bytes uint8, values float64): uniform over the e4m3fn bytes whose value is an integer with |v| <= qmax (both zeros among them).  The
    integers keep the quantum at the scale's own 2^e; qmax = 448 is every integer the format holds."""
    ok = np.flatnonzero(np.isfinite(_E4M3) & (_E4M3 == np.round(_E4M3)) & (np.abs(_E4M3) <= qmax)).astype(np.uint8)
    b = ok[rng.integers(0, len(ok), shape)]
    return b, _E4M3[b]


def _row_levels(rng, chunks, per):
    """[N, chunks * per] levels (i + row + r[row][chunk]) mod LEVELS"""
    r = rng.integers(0, LEVELS, (N, chunks, 1))
    lv = (np.arange(per)[None, None, :] + np.arange(N)[:, None, None] + r) % LEVELS
    return lv.reshape(N, chunks * per)


def seed_of(fmt, chunks, what=0):
    return MP.seed_of(FORMATS.index(fmt), chunks, what, 59)


def weights(fmt, chunks, qmax=None):
    """(ckpt, W, quantum) of one [N, K = 256 chunks] matrix.  ckpt: the checkpoint-form arrays the product's pack call takes --
         f8   q uint8 [N, K] (e4m3fn bytes), scale float64 [N]
         f8b  q uint8 [N, K], s float64 [N / 128, K / 128]
         f4   q uint8 [N, K / 2], e8 uint8 [N, K / 32]
         i4   q uint8 [N, K / 2] (low nibble = even k), z uint8 [N, K / 128], s float64 [N, K / 128]
         i8   q uint8 [N, K], z, s as i4
    (every scale a power of two: exact in fp32, fp16 and bf16) plus `codes` float64 [N, K], the VALUE of every code before its side data
    (q for i4 / i8, the e2m1 / e4m3 value otherwise).  W float64 [N, K] is the exact dequantised matrix, quantum = 2^EMIN."""
    K = KC * chunks
    rng = np.random.default_rng(seed_of(fmt, chunks))
    if fmt in ("f8", "f8b"):
        q, codes = _fp8_codes(rng, (N, K), F8_QMAX[0] if qmax is None else qmax)
        if fmt == "f8":
            e = EMIN + np.arange(N) % LEVELS
            ckpt = dict(q=q, scale=np.exp2(e.astype(np.float64)), codes=codes)
            W = codes * ckpt["scale"][:, None]
        else:
            e = EMIN + (np.arange(K // 128)[None, :] + 5 * np.arange(N // 128)[:, None]) % F8B_PERIOD
            ckpt = dict(q=q, s=np.exp2(e.astype(np.float64)), codes=codes)
            W = codes * ckpt["s"].repeat(128, 0).repeat(128, 1)
    elif fmt == "f4":
        exps = EMIN + 1 + _row_levels(rng, chunks, 8)                       # e2m1's half steps: the quantum is 2^(e - 1)
        idx = rng.integers(0, 16, (N, K))
        codes = MP.SIGNED_GRID[idx]
        W = codes * np.exp2(exps.astype(np.float64)).repeat(32, 1)
        q, e8 = MP.encode(W, exps, torch.float16)
        neg0 = (idx == 8).astype(np.uint8)                                  # the sixteenth code, -0: `encode` writes every zero as +0
        q = q | (neg0[:, 0::2] << 3) | (neg0[:, 1::2] << 7)
        assert np.array_equal(MP.decode(q, e8), W)
        ckpt = dict(q=q, e8=e8, codes=codes)
    elif fmt in ("i4", "i8"):
        top = 16 if fmt == "i4" else 256
        codes = rng.integers(0, top, (N, K))
        z = rng.integers(0, top, (N, K // 128))
        s = np.exp2((EMIN + _row_levels(rng, chunks, 2)).astype(np.float64))
        W = (codes - z.repeat(128, 1)).astype(np.float64) * s.repeat(128, 1)
        q8 = codes.astype(np.uint8)
        ckpt = dict(q=np.ascontiguousarray(q8[:, 0::2] | (q8[:, 1::2] << 4)) if fmt == "i4" else q8, z=z.astype(np.uint8), s=s,
                    codes=codes.astype(np.float64))
    else:
        raise ValueError(fmt)
    return ckpt, as_t(W), QUANTUM


def side_elements(fmt, ckpt, K):
    """(z_el, s_el) float64 [N, K]: the zero point and the scale of every element, W = (codes - z_el) * s_el"""
    zero = np.zeros((N, K))
    if fmt == "f8":
        return zero, np.broadcast_to(ckpt["scale"][:, None], (N, K))
    if fmt == "f8b":
        return zero, ckpt["s"].repeat(128, 0).repeat(128, 1)
    if fmt == "f4":
        return zero, np.exp2(ckpt["e8"].astype(np.float64) - 127).repeat(32, 1)
    return ckpt["z"].astype(np.float64).repeat(128, 1), ckpt["s"].repeat(128, 1)


def side_tables(fmt, ckpt, chunks):
    """{name: array [owners, chunks, entries per chunk]} of the side data that changes along k (none for f8)"""
    if fmt == "f8":
        return {}
    if fmt == "f8b":
        return {"s": ckpt["s"].reshape(N // 128, chunks, 2)}
    if fmt == "f4":
        return {"e8": ckpt["e8"].reshape(N, chunks, 8)}
    return {"s": ckpt["s"].reshape(N, chunks, 2), "z": ckpt["z"].reshape(N, chunks, 2)}


class Case:
    """one (format, chunks): ckpt, W float64 [N, K], quantum, amax, A float64 [64, K], P float64 [chunks, 64, N] (the exact sums over every
    chunk); rows r of a launch are A[:r] and P[:, :r]"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def parts(self, rows, splits):
        return G.split_sums(self.P[:, :rows], splits)

    def chunk(self, c):
        return slice(KC * c, KC * (c + 1))

    def side(self):
        if not hasattr(self, "_side"):
            self._side = side_elements(self.fmt, self.ckpt, self.K)
        return self._side


def case(fmt, chunks):
    K = KC * chunks
    for qmax in (F8_QMAX if fmt in ("f8", "f8b") else (None,)):
        ckpt, W, quantum = weights(fmt, chunks, qmax)
        col = (W.abs() / quantum).sum(1).max().item()
        amax = int(min(AMAX_CAP, (2 ** 24 - 1) // col))
        if amax >= (F8_AMIN if qmax is not None and qmax != F8_QMAX[-1] else 2):
            break
    assert amax >= 2, (fmt, chunks, amax)
    rng = np.random.default_rng(seed_of(fmt, chunks, 1))
    A = as_t(rng.integers(-amax, amax + 1, (max(ROWS), K)))
    return Case(fmt=fmt, chunks=chunks, K=K, ckpt=ckpt, W=W, quantum=quantum, amax=amax, qmax=qmax, A=A, P=G.chunk_products(A, W))


# ---- conditions, from the inputs and the float64 reference alone (cap on excluded outputs: 0) ---------------------------------------------------
def inexact_share(exact, dtype):
    return (rounded(exact, dtype) != exact).double().mean().item()


def check_case(c):
    """every condition of the module docstring that does not depend on the row tile; returns {dtype: share of the 64-row outputs that the
    single rounding changes}"""
    fmt, chunks, W, q = c.fmt, c.chunks, c.W, c.quantum
    z_el, s_el = c.side()
    assert np.array_equal((c.ckpt["codes"] - z_el) * s_el, W.numpy())
    for dtype in DTYPES:                                         # the i4 / i8 widening rounds (q - z) * s to the dtype: it must round nothing
        assert torch.equal(rounded(W, dtype), W) and torch.equal(rounded(c.A, dtype), c.A), (fmt, chunks, dtype)
        assert all(torch.equal(rounded(as_t(v), dtype), as_t(v)) for k, v in c.ckpt.items() if k in ("s", "scale"))
    units = W / q
    assert bool((units == units.round()).all()) and c.A.abs().max().item() <= c.amax
    assert (c.A.abs() @ W.abs().t()).max().item() < 2 ** 24 * q      # every partial sum in any order and at any split is exact in fp32
    exact = c.P.sum(0)
    assert torch.equal(exact.float().double(), exact) and exact.abs().max().item() < torch.finfo(torch.float16).max
    assert bool(torch.isfinite(exact.to(torch.float16)).all())
    # chunk c against chunks c +- d: more than half of the weights, and of every side table, differ
    Wc = W.view(N, chunks, KC)
    tables = side_tables(fmt, c.ckpt, chunks)
    for d in range(1, min(MAX_DISTANCE, chunks - 1) + 1):
        assert (Wc[:, d:] != Wc[:, :-d]).double().mean((0, 2)).min().item() > 0.5, (fmt, chunks, d)
        for name, t in tables.items():
            assert (t[:, d:] != t[:, :-d]).mean((0, 2)).min() > 0.5, (fmt, chunks, name, d)
    # scales: the groups / blocks of every chunk differ pairwise next to each other; neighbouring rows / tiles differ in more than half
    sc = {"f8": c.ckpt.get("scale"), "f8b": c.ckpt.get("s"), "f4": c.ckpt.get("e8"), "i4": c.ckpt.get("s"), "i8": c.ckpt.get("s")}[fmt]
    if fmt == "f8":
        assert bool((sc[1:] != sc[:-1]).all())
    else:
        per = sc.shape[1] // chunks
        t = sc.reshape(sc.shape[0], chunks, per)
        assert bool((t[:, :, 1:] != t[:, :, :-1]).all()), (fmt, chunks)
        assert (sc[1:] != sc[:-1]).mean() > 0.5, (fmt, chunks)
    return {dtype: inexact_share(exact, dtype) for dtype in DTYPES}


def check_rows(c, rows):
    """the rounding condition per row tile: visible on more than 5 % of the outputs in bf16 at every length, in fp16 at LONG_CHUNKS"""
    exact = c.P[:, :rows].sum(0)
    shares = {dtype: inexact_share(exact, dtype) for dtype in DTYPES}
    assert shares[torch.bfloat16] > 0.05, (c.fmt, c.chunks, rows, shares)
    if c.chunks == LONG_CHUNKS:
        assert shares[torch.float16] > 0.05, (c.fmt, c.chunks, rows, shares)
    return shares


def finish(parts, dtype):
    """what a launch stores: the single rounding to the dtype at one split, the fp32 partials (exact) otherwise"""
    return rounded(parts[0], dtype) if parts.shape[0] == 1 else parts


# ---- named faults ---------------------------------------------------------------------------------------------------------------------------
def stream_faults(c, rows, splits, dtype, depth=None):
    """{name: (wrong [splits, rows, N] float64 per-split sums with the fault, touched bool mask)}.  The faulty split and chunk are the
    first that the fault can happen to; a fault that needs a longer stream than the plan has is left out."""
    depth = DEPTH[c.fmt][rows] if depth is None else depth
    A, W, P = c.A[:rows], c.W, c.P[:, :rows]
    parts = G.split_sums(P, splits)
    ranges = [G.split_range(s, c.chunks, splits) for s in range(splits)]
    out = {}

    def put(name, s, delta):
        wrong, touched = parts.clone(), torch.zeros_like(parts, dtype=torch.bool)
        wrong[s] += delta
        touched[s] = True
        out[name] = (wrong, touched)

    s, (c0, c1) = max(enumerate(ranges), key=lambda x: x[1][1] - x[1][0])          # the longest split
    put("first_chunk_dropped", s, -P[c0])
    put("last_chunk_dropped", s, -P[c1 - 1])
    put("chunk_twice", s, P[(c0 + c1) // 2])
    if c1 - c0 > depth:                                          # the refill of chunk c0 + depth landing while chunk c0 is consumed
        a = A[:, c.chunk(c0)]
        put("early_refill", s, a @ W[:, c.chunk(c0 + depth)].t() - P[c0])
        if c.fmt != "f8":
            z_el, s_el = c.side()
            other = c.chunk(c0 + depth)
            w = as_t((c.ckpt["codes"][:, c.chunk(c0)] - z_el[:, other]) * s_el[:, other])
            put("side_data_ahead", s, a @ (rounded(w, dtype) if c.fmt in ("i4", "i8") else w).t() - P[c0])
    if c1 - c0 > depth + 1:                                      # ring of depth + 1 A buffers: chunk c's buffer held chunk c - (depth + 1)
        cc = c0 + depth + 1
        put("stale_ring_buffer", s, A[:, c.chunk(c0)] @ W[:, c.chunk(cc)].t() - P[cc])
    if splits > 1:                                               # the boundary chunk handed to the neighbouring split: the total is unchanged
        s = min(s, splits - 2)
        b = ranges[s][1]
        wrong, touched = parts.clone(), torch.zeros_like(parts, dtype=torch.bool)
        wrong[s] -= P[b - 1]
        wrong[s + 1] += P[b - 1]
        touched[s], touched[s + 1] = True, True
        out["boundary_chunk_to_neighbour"] = (wrong, touched)
    return out


def fault_shares(c, rows, splits, dtype, depth=None):
    """every fault changes at least half of the stored values it touches, and at least one, under the equality of the GPU test; the
    boundary fault leaves the sum of the partials as it was (which is why the partials are compared one by one).  Returns {name: share}."""
    parts = c.parts(rows, splits)
    want = finish(parts, dtype)
    shares = {}
    for name, (wrong, touched) in stream_faults(c, rows, splits, dtype, depth).items():
        got = finish(wrong, dtype)
        changed = (got != want)[touched[0] if splits == 1 else touched]
        shares[name] = changed.double().mean().item()
        assert changed.numel() > 0 and bool(changed.any()) and shares[name] >= 0.5, (c.fmt, c.chunks, rows, splits, dtype, name, shares[name])
        if name == "boundary_chunk_to_neighbour":
            assert torch.equal(wrong.sum(0), parts.sum(0))
    return shares
