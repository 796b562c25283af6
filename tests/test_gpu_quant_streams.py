"""Exact sums at every stream length for the five dense weight-only streaming GEMMs (samd_gemm_skinny_f8, _f8b, _f4, _i4, _i8) on the inputs
of tests/quant_planting.py.  Every comparison is torch.equal against the float64 reference; every output and partial buffer starts
NaN-filled; weights go through the product's own pack kernels.

The plan (quant_planting's docstring has the reasons).  Both dtypes, rows 16 / 32 / 48 / 64, N = 256 (two column tiles).
  whole launches   K = 256 L for every L = 1 .. 18 and K = 14336 (56 chunks) at one split: out == exact.to(dtype), one rounding.
  split launches   (2 L + 1, 2) for L = 1 .. 17 (neighbouring splits of length L and L + 1), (18, 18), the three-way plans (4, 3) (5, 3)
                   (7, 3) (8, 3) (25, 3) (26, 3), gemm_planting.CHUNK_SPLITS, and 56 chunks at samd_gemm_splits' own count (8): EVERY fp32
                   partial equals the exact sum over its own chunks, so a chunk handed to the neighbouring split fails although the sum
                   of the partials is unchanged; every element of the partial buffer is written (a NaN never compares equal).
The pipeline depths the sweep crosses (rows 16 / 32 / 48 / 64): f8 4 4 4 3, f4 and i4 8 4 5 3, i8 4 4 4 3, f8b 4 3 4 3; lengths 1 .. 18 reach
2 DEPTH + 2 for any depth the kernels admit (DEPTH <= 8).

Measured on the references (tests/test_quant_planting_cpu.py prints them), lowest over every case of the plan and all four row tiles:
  outputs the single rounding changes   bf16, every length: f8 0.932, f8b 0.947, f4 0.842, i4 0.721, i8 0.967
                                        fp16, 56 chunks:    f8 0.689, f8b 0.965, f4 0.838, i4 0.851, i8 0.941
  share of the touched outputs a named fault changes (lowest fault of the format): f8 0.985 (last chunk dropped), f8b 0.558 (first chunk
  dropped, at one split: the rounding to the dtype hides part of a chunk that carries the lowest scale levels), f4 0.680 (side data of chunk c + DEPTH: a quarter of
  the rows draw the same levels), i4 0.976, i8 0.976; the boundary chunk given to the neighbouring split changes >= 0.996 of both partials
  and leaves their sum unchanged.

Proof that the file bites (once, in a scratch copy of csrc/gemm_kernels.hip that was never committed): one deterministic, memory-safe defect
per dense body, every load, wait and barrier left as it is --
  f8    the last chunk of a stream of exactly DEPTH + 1 chunks is not accumulated
  w4    (f4 and i4) the refill requests the side data of the chunk being consumed instead of chunk c + DEPTH's
  i8    chunk c0 + DEPTH + 1, the first to reuse a ring buffer, is accumulated twice
  f8b   in a stream of exactly DEPTH chunks the last chunk takes the scales of the chunk before it
Against that build all 80 tests failed.  Launch by launch (2160 launches: 5 formats x 2 dtypes x 4 row tiles x 54 plans), 844 failed, and they
were exactly the launches in which some split has a length the defect needs -- f8 length DEPTH + 1 (4 or 5 launches per row tile: (5, 1),
(9, 2), (11, 2) at depth 4), f4 / i4 any length above DEPTH (23 launches at 16 rows, depth 8; 38 at 64 rows, depth 3), i8 any length
>= DEPTH + 2 (31 / 34), f8b length DEPTH (5 / 8) -- with no launch failing or passing against that prediction.  On the real build
all 80 pass; the file takes 6.5 s on an MI355X (80 tests, 2160 launches), the references of a format are built once and shared by its tests."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gemm_planting as G
import quant_planting as Q
import test_gpu_fp8_gemm as T8
import test_gpu_fp8b_gemm as T8B
import test_gpu_int4_gemm as TI4
import test_gpu_int8_gemm as TI8
import test_gpu_mxfp4_gemm as TF4
from samd_hip import lib

DTYPES = list(Q.DTYPES)
N = Q.N
_cases, _packed = {}, {}


def case(fmt, chunks):
    """(A float64 [64, K], P float64 [chunks, 64, N], ckpt): built once per (format, K) and left unchanged"""
    if (fmt, chunks) not in _cases:
        c = Q.case(fmt, chunks)
        _cases[fmt, chunks] = (c.A, c.P, c.ckpt)
    return _cases[fmt, chunks]


def packed(fmt, chunks, dtype):
    """the launch's weight arguments, through the product's own pack kernel: cached per (format, K, dtype)"""
    key = (fmt, chunks, dtype)
    if key not in _packed:
        ck = case(fmt, chunks)[2]
        t = lambda name, dt=None: (torch.from_numpy(ck[name]) if dt is None else torch.from_numpy(ck[name]).to(dt)).cuda().contiguous()
        if fmt == "f8":
            _packed[key] = (T8.pack(t("q").view(torch.float8_e4m3fn)), t("scale", torch.float32))
        elif fmt == "f8b":
            _packed[key] = (T8.pack(t("q").view(torch.float8_e4m3fn)), t("s", torch.float32))
        elif fmt == "f4":
            _packed[key] = (TF4.pack(t("q"), t("e8")),)
        else:
            _packed[key] = ((TI4 if fmt == "i4" else TI8).pack(t("q"), t("z"), t("s", dtype)),)
    return _packed[key]


def launch(fmt, A, w, rows, K, splits, dtype):
    """the dtype output [rows, N] at one split, else the fp32 partials [splits, rows, N]; from NaN-filled buffers, synchronised"""
    if fmt == "f8":
        return T8.run(A, w[0], w[1], N, K, rows, splits, dtype)
    if fmt == "f8b":
        return T8B.run(A, w[0], w[1], N, K, rows, splits, dtype)
    return {"f4": TF4, "i4": TI4, "i8": TI8}[fmt].run(A, w[0], N, K, rows, splits, dtype)


def compare(got, want, fmt, dtype, rows, chunks, splits):
    want = want.cuda()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = torch.nonzero(~(got == want))
    i = tuple(bad[0].tolist())
    split, m, n = (0,) + i if splits == 1 else i
    lengths = Q.split_lengths(chunks, splits)
    pytest.fail(f"{fmt} {dtype} rows {rows} chunks {chunks} splits {splits} (lengths {lengths}): {len(bad)} of {got.numel()} stored values differ, "
                f"in splits {sorted(set(bad[:, 0].tolist())) if splits > 1 else [0]}; first in split {split} (length {lengths[split]}) at "
                f"(m, n) = ({m}, {n}): got {got[i].item()!r}, want {want[i].item()!r}")


def run_plan(fmt, dtype, rows, plans):
    for chunks, splits in plans:
        A, P, _ = case(fmt, chunks)
        parts = G.split_sums(P[:, :rows], splits)
        want = parts[0].to(dtype) if splits == 1 else parts.float()          # one rounding of the exact sum | the exact fp32 partials
        got = launch(fmt, A[:rows].to(dtype).cuda().contiguous(), packed(fmt, chunks, dtype), rows, G.KC * chunks, splits, dtype)
        compare(got, want, fmt, dtype, rows, chunks, splits)


@pytest.mark.parametrize("rows", Q.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_whole_launches_store_the_rounded_exact_sum_at_every_length(fmt, dtype, rows):
    Q.assert_plan()
    run_plan(fmt, dtype, rows, [(chunks, 1) for chunks in Q.WHOLE_CHUNKS])


@pytest.mark.parametrize("rows", Q.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_every_split_stores_the_exact_sum_of_its_own_chunks(fmt, dtype, rows):
    own = lib().samd_gemm_splits(N, G.KC * Q.LONG_CHUNKS, rows)
    assert 1 < own <= Q.LONG_CHUNKS
    run_plan(fmt, dtype, rows, list(Q.SPLIT_PLANS) + [(Q.LONG_CHUNKS, own)])
