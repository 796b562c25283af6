"""tests/quant_planting.py on the CPU: the stream plan, every recipe condition at every case tests/test_gpu_quant_streams.py launches, every
named fault under the equality that file uses, and the recipes against the package's own dequantize_* (no GPU, no library call)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gemm_planting as G
import quant_planting as Q

WHOLE = [(c, 1) for c in Q.WHOLE_CHUNKS]
LONG_SPLITS = 8                                          # samd_gemm_splits(256, 14336, rows): min(256 / 2 column tiles, cap 8, 56 chunks)
SPLIT = list(Q.SPLIT_PLANS) + [(Q.LONG_CHUNKS, LONG_SPLITS)]


def test_the_plan_puts_every_length_alone_and_beside_another_length():
    assert Q.assert_plan() == list(range(1, 19))
    assert Q.split_lengths(7, 3) == [2, 2, 3] and Q.split_lengths(18, 18) == [1] * 18 and Q.split_lengths(35, 2) == [17, 18]
    for chunks, splits in Q.SPLIT_PLANS:                 # the rule restated: c0 = split * chunks // splits
        assert Q.split_lengths(chunks, splits) == [b - a for a, b in (G.split_range(s, chunks, splits) for s in range(splits))]
    assert max(max(d.values()) for d in Q.DEPTH.values()) <= 8 and max(Q.LENGTHS) >= 2 * 8 + 2
    assert Q.MAX_DISTANCE >= max(max(d.values()) for d in Q.DEPTH.values()) + 1
    assert {c for c, _ in WHOLE + SPLIT} == set(Q.ALL_CHUNKS)


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_every_case_meets_the_conditions_and_shows_every_fault(fmt):
    """every (chunks) of the plan: the exactness conditions, the rounding shares per row tile, and every fault at every (rows, splits,
    dtype) the GPU file launches it at"""
    low = {dt: 1.0 for dt in Q.DTYPES}
    fault_low, seen = {}, set()
    for chunks in Q.ALL_CHUNKS:
        c = Q.case(fmt, chunks)
        shares = Q.check_case(c)
        for rows in Q.ROWS:
            for dt, s in Q.check_rows(c, rows).items():
                if dt == torch.bfloat16 or chunks == Q.LONG_CHUNKS:
                    low[dt] = min(low[dt], s)
            for ch, splits in WHOLE + SPLIT:
                if ch != chunks:
                    continue
                for dtype in Q.DTYPES:
                    for name, s in Q.fault_shares(c, rows, splits, dtype).items():
                        fault_low[name] = min(fault_low.get(name, 1.0), s)
                        seen.add((name, rows))
        assert shares[torch.bfloat16] > 0.05
    print(f"{fmt}: lowest inexact share bf16 (every length) {low[torch.bfloat16]:.3f}, fp16 (56 chunks) {low[torch.float16]:.3f}; "
          "lowest share of the touched outputs a fault changes: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(fault_low.items())))
    names = {"first_chunk_dropped", "last_chunk_dropped", "chunk_twice", "early_refill", "stale_ring_buffer", "boundary_chunk_to_neighbour"}
    names |= set() if fmt == "f8" else {"side_data_ahead"}
    assert {(n, r) for n in names for r in Q.ROWS} <= seen       # every fault ran at every row tile (each has its own depth)


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_a_retuned_depth_is_still_covered(fmt):
    """the plan does not rest on the DEPTH table: at every depth 1 .. 8 some whole launch and some split launch show every fault"""
    cases = {ch: Q.case(fmt, ch) for ch in (18, 35)}
    for depth in range(1, 9):
        for ch, splits in ((18, 1), (35, 2)):
            got = Q.fault_shares(cases[ch], 16, splits, torch.bfloat16, depth)
            assert {"early_refill", "stale_ring_buffer"} <= set(got), (depth, ch, splits)


def test_the_recipes_are_what_the_package_dequantises():
    from samd_hip import fp8 as F8
    from samd_hip import int4 as I4
    from samd_hip import int8 as I8
    from samd_hip import mxfp4 as MX
    assert np.array_equal(np.asarray(MX.GRID), Q.MP.GRID)
    for chunks in (1, 3, 18):
        for dtype in Q.DTYPES:
            ck, W, _ = Q.weights("i4", chunks)
            got = I4.dequantize_groups(torch.from_numpy(ck["q"]), torch.from_numpy(ck["z"]), torch.from_numpy(ck["s"]).to(dtype))
            assert torch.equal(got.double(), W)
            I4.check_groups(torch.from_numpy(ck["q"]), torch.from_numpy(ck["z"]), torch.from_numpy(ck["s"]).to(dtype), dtype)
            ck, W, _ = Q.weights("i8", chunks)
            got = I8.dequantize_groups(torch.from_numpy(ck["q"]), torch.from_numpy(ck["z"]), torch.from_numpy(ck["s"]).to(dtype))
            assert torch.equal(got.double(), W)
            I8.check_groups(torch.from_numpy(ck["q"]), torch.from_numpy(ck["z"]), torch.from_numpy(ck["s"]).to(dtype), dtype)
            ck, W, _ = Q.weights("f4", chunks)
            MX.check_exponents(torch.from_numpy(ck["e8"]), dtype)
            assert torch.equal(MX.dequantize_blocks(torch.from_numpy(ck["q"]), torch.from_numpy(ck["e8"])).double(), W)
        for qmax in Q.F8_QMAX:
            ck, W, _ = Q.weights("f8", chunks, qmax)
            q8 = torch.from_numpy(ck["q"]).view(torch.float8_e4m3fn)
            assert torch.equal(F8.dequantize_rows(q8, torch.from_numpy(ck["scale"]).float()).double(), W)
            ck, W, _ = Q.weights("f8b", chunks, qmax)
            q8, s = torch.from_numpy(ck["q"]).view(torch.float8_e4m3fn), torch.from_numpy(ck["s"]).float()
            assert torch.equal(F8.dequantize_blocks(q8, s).double(), W)
            F8.check_block_scales(q8, s)
    # whole code ranges where the bound allows: every INT4 / INT8 code and zero point, every e2m1 code, every integer e4m3 byte
    assert set(np.unique(Q.weights("i4", 1)[0]["codes"])) == set(range(16)) and set(np.unique(Q.weights("i4", 4)[0]["z"])) == set(range(16))
    assert set(np.unique(Q.weights("i8", 1)[0]["codes"])) == set(range(256)) and set(np.unique(Q.weights("i8", 18)[0]["z"])) == set(range(256))
    q4 = Q.weights("f4", 1)[0]["q"]
    assert set(np.unique(q4 & 15)) == set(range(16)) and set(np.unique(q4 >> 4)) == set(range(16))
    assert Q.case("f8", 1).qmax == 448 and np.abs(Q.weights("f8", 1)[0]["codes"]).max() == 448


def test_the_expert_sweeps_cross_every_depth_of_the_quantised_forms():
    assert set(Q.MP.DEPTHS) == {"mxfp4", "int4g128", "int8g128", "fp8b128"}
    for form, depths in Q.MP.DEPTHS.items():
        cases = Q.MP.exact_sweep(form)
        for rows_pad, depth in depths.items():
            chunks = {K // 256 for K, r in cases if r == rows_pad}
            assert {max(1, depth - 1), depth, depth + 1, depth + 2, 1, 3, 9} <= chunks and any(c % 2 and c > depth for c in chunks)
            assert set(Q.MP.chunk_sweep(form, rows_pad)) <= chunks
    assert Q.MP.chunk_sweep("mxfp4", 32) == (1, 2, 3, 4, 5, 7) and Q.MP.chunk_sweep(None, 16) == tuple(range(1, 8))      # as before
