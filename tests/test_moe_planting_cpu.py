"""tests/moe_planting.py on the CPU: every case tests/test_gpu_moe_exact.py launches is built here, which runs the helper's conditions from the
references alone -- ranges (|y| < BAR with no output left out, gate and up ranges), column coverage with zero uncovered columns, check_large,
assert_silu / assert_silu4, the combine's exactness, and every named fault through gemm_planting.self_check -- plus the restatements
against the package: the Python lists' rule, the MXFP4 coding against samd_hip.mxfp4, the gate|up row permutation against samd_hip.moe.
The sweeps, the excluded-slot cases and the row-independence cases (the row alone included) are built with their faults checked; the
slot-order case has its own four facts.  Recorded on 8 CPU cores: 56 tests in 39 s (most of it drawing the weights, E N K float64 a case)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gemm_planting as G
import moe_planting as M

DOWN_COMMON = {"neighbour_expert", "w_next_slot", "y_next_row", "w_not_applied"}
GU_COMMON = {"neighbour_expert", "gate_up_swapped", "truncate_act", "product_dropped", "product_doubled", "vec8_dropped"}
FOUR_BIT = {"nibbles_swapped", "neighbour_exponent"}


@pytest.mark.parametrize("rows_pad", M.ROWS)
def test_routings_and_their_lists(rows_pad):
    kinds = M.KINDS + (("grid_bound", "excluded") if rows_pad == 16 else ())
    for kind in kinds:
        R = M.routing(kind, rows_pad)
        flat = R.idx.reshape(-1).tolist()
        seen = set()
        for e, lst in R.lists.items():                             # the header's rule, stated once more entry by entry
            assert 0 <= e < R.E and lst == sorted(lst) and len(lst) > 0
            for p in lst:
                r, j = divmod(p, R.k)
                assert r < R.n and flat[p] == e and e not in flat[r * R.k:p] and p not in seen
                seen.add(p)
        for p in range(R.rows_pad * R.k):                          # and nothing that belongs in a list is missing
            r, j = divmod(p, R.k)
            if r < R.n and 0 <= flat[p] < R.E and flat[p] not in flat[r * R.k:p]:
                assert p in seen
        assert list(R.lists) == sorted(R.lists)
        w = M.combine_weights(R)
        assert bool((w[:, 1:] != w[:, :-1]).all()) and bool((w[1:] != w[:-1]).all())
    counts = M.routing("counts", rows_pad).counts
    assert set(counts) >= {c for c in M.COUNTS if c <= rows_pad}
    assert M.routing("one_expert", rows_pad).counts[0] == rows_pad and M.routing("random", rows_pad).n < rows_pad
    if rows_pad == 16:
        R = M.routing("grid_bound", 16)
        assert len(R.lists) == R.n * R.k == min(R.E, R.rows_pad * R.k) == 128
        R = M.routing("excluded", 16)
        assert int((~R.valid[:R.n]).sum()) == 6                    # two repetitions and four indices outside [0, E)


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("rows_pad", M.ROWS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_gate_up_cases(dtype, rows_pad, form):
    seen = set()
    for kind, inter, chunks in M.gate_up_sweep(form, rows_pad):
        c = M.gate_up_case(dtype, M.routing(kind, rows_pad), inter, chunks, form)
        need = GU_COMMON | (FOUR_BIT if form else set())
        if max(c.R.counts) >= 2:
            need = need | {"list_entry_next", "source_row_p"}
        assert need <= set(c.checked), (kind, inter, chunks, need - set(c.checked))
        seen |= set(c.checked)
        for h, act in c.draws:
            assert bool(torch.isnan(h[c.R.n:]).all()) and int(torch.isnan(act).any(1).sum()) == c.R.rows_pad * c.R.k - len(c.R.named)
    assert {"list_entry_next", "source_row_p"} <= seen


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("rows_pad", M.ROWS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_down_cases(dtype, rows_pad, form):
    seen = set()
    for kind, hidden, chunks, regime in M.down_sweep(form, rows_pad):
        c = M.down_case(dtype, M.routing(kind, rows_pad), hidden, chunks, regime, form)
        need = DOWN_COMMON | (FOUR_BIT if form else set())
        need |= {"truncate_y", "truncate_out", "combine_in_dtype"} if regime == "large" else set(G.EXACT_ONLY)
        if max(c.R.counts) >= 2:
            need = need | {"list_entry_next"}
        assert need <= set(c.checked), (kind, hidden, chunks, regime, need - set(c.checked))
        seen |= set(c.checked)
        for act, y, out in c.draws:
            assert bool((out[c.R.n:] == 0).all()) and not bool(torch.isnan(out).any())
            assert int(torch.isnan(y).any(1).sum()) == c.R.rows_pad * c.R.k - len(c.R.named)
    assert "list_entry_next" in seen


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_slot_order_case_separates_the_orders(dtype, k, form):
    asc, desc, pair, exact = M.order_facts(k)
    assert asc == 2.0 ** -11 and desc == 0.0 and pair == 0.0 and exact == (k // 4) * (2.0 ** -10 + 2.0 ** -11)
    assert M.f32_sum(M.ORDER_TERMS) == 2.0 ** -11 and M.f32_sum(M.ORDER_TERMS, "descending") == 0.0
    assert M.f32_sum(M.ORDER_TERMS, "pairwise") == 0.0 and sum(M.ORDER_TERMS) == 2.0 ** -10 + 2.0 ** -11
    c = M.order_case(dtype, k, form)
    terms = lambda row: [M.ORDER_TERMS[(row + s) % 4] for s in range(k)]
    for row in range(16):
        assert c.out[row, 0].item() == M.f32_sum(terms(row)) and bool((c.out[row] == c.out[row, 0]).all())
        assert [c.w[row, s].item() * c.y[row * k + s, 0].item() for s in range(k)] == terms(row)
    # the documented order against each alternative, on stored values: most rows tell them apart
    for other in ("descending", "pairwise"):
        assert sum(G.rounded(torch.tensor([M.f32_sum(terms(r), other)], dtype=torch.float64), dtype).item() != c.out[r, 0].item() for r in range(16)) >= 8
    assert all(G.rounded(torch.tensor([sum(terms(r))], dtype=torch.float64), dtype).item() != c.out[r, 0].item() for r in range(16))
    if form:
        q, e8 = M.encode(c.W.numpy(), c.exps, dtype)
        assert np.array_equal(M.decode(q, e8), c.W.double().numpy())


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_excluded_slot_cases(dtype, form):
    """the three launches of the excluded-slots test, faults checked; the reference equals that of a routing with those slots marked empty"""
    R = M.routing("excluded", 16)
    clean = M.Routing("clean", R.E, R.k, 16, R.n, np.where(R.valid, R.idx, -1))
    assert clean.lists == R.lists
    four = FOUR_BIT if form else set()
    gu = M.gate_up_case(dtype, R, 256, 2, form)
    assert GU_COMMON | four | {"list_entry_next", "source_row_p"} <= set(gu.checked)
    for h, act in gu.draws:
        assert int(torch.isnan(act).any(1).sum()) == 16 * R.k - len(R.named) == 3 * R.k + 6
    for regime in ("small", "large"):
        c = M.down_case(dtype, R, 256, 2, regime, form)
        need = DOWN_COMMON | four | {"list_entry_next"} | ({"truncate_y", "truncate_out", "combine_in_dtype"} if regime == "large" else set(G.EXACT_ONLY))
        assert need <= set(c.checked), need - set(c.checked)
        for act, y, out in c.draws:
            assert torch.equal(M.down_ref(clean, c.W, act, c.w, dtype)[2], out) and bool((out[R.n:] == 0).all())


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_row_independence_cases(dtype, form):
    """the four launches of the row-independence test, faults checked: alone, the row's references are those it has as row 40 of 64"""
    gu, gu1, dn, dn1 = M.independence_cases(dtype, form, check=True)
    four = FOUR_BIT if form else set()
    assert GU_COMMON | four | {"list_entry_next", "source_row_p"} <= set(gu.checked) and GU_COMMON | four <= set(gu1.checked)
    large = DOWN_COMMON | four | {"truncate_y", "truncate_out", "combine_in_dtype"}
    assert large | {"list_entry_next"} <= set(dn.checked) and large <= set(dn1.checked)
    k = gu.R.k
    assert gu1.R.lists == {int(e): [j] for j, e in sorted(enumerate(gu.R.idx[40]), key=lambda t: t[1])} and gu1.R.n == 1
    assert torch.equal(gu1.draws[0][1][:k], gu.draws[-1][1][40 * k:41 * k])
    assert torch.equal(dn1.draws[0][1][:k], dn.draws[-1][1][40 * k:41 * k]) and torch.equal(dn1.draws[0][2][0], dn.draws[-1][2][40])


def test_mxfp4_restatement_against_the_package():
    from samd_hip import moe as MOE
    from samd_hip import mxfp4 as MX
    assert tuple(M.GRID) == MX.GRID
    for dtype in M.DTYPES:
        assert M.EXPONENT_RANGE[dtype] == tuple(MX.exponent_range(dtype))
    rng = np.random.default_rng(1)
    q = rng.integers(0, 256, (8, 64), dtype=np.uint8)
    e8 = rng.integers(100, 140, (8, 4), dtype=np.uint8)
    assert np.array_equal(M.decode(q, e8), MX.dequantize_blocks(torch.from_numpy(q), torch.from_numpy(e8)).double().numpy())
    for inter in (128, 256, 320, 768):
        assert np.array_equal(M.gate_up_row_order(inter), MOE.gate_up_tile_order(inter).numpy())


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_every_planted_mxfp4_weight_round_trips_through_the_package(dtype):
    """a recipe's coding of a weight depends on (k block, dtype) alone, not on the routing, the expert or the row bucket: the three recipes'
    weights (M.down_weights / M.gate_up_weights, the builders of every case, without the references) at every K of the sweeps, two experts of
    128 rows each, and the slot-order case"""
    from samd_hip import mxfp4 as MX

    def trip(W, exps):
        q, e8 = M.encode(W.numpy(), exps, dtype)
        MX.check_exponents(torch.from_numpy(e8), dtype)
        back = MX.dequantize_blocks(torch.from_numpy(q.reshape(-1, q.shape[-1])), torch.from_numpy(e8.reshape(-1, e8.shape[-1])))
        assert torch.equal(back.reshape(W.shape).double(), W.double()) and np.array_equal(M.decode(q, e8), W.double().numpy())
        assert torch.equal(back.to(dtype).float(), back)
    R = M.Routing("two", 2, 2, 16, 2, np.tile([[0, 1]], (16, 1)))
    for chunks in range(1, 11):
        for regime in ("small", "large"):
            W, exps, _ = M.down_weights(dtype, R, 128, chunks, regime, "mxfp4")
            trip(W, exps)
            assert bool((np.abs(np.diff(exps, axis=-1)) == 1).all()) and (regime == "small" or exps.min() >= 1)
        _, Wg, Wu, exps = M.gate_up_weights(dtype, R, 128, chunks, "mxfp4")
        trip(Wg, exps[0]), trip(Wu, exps[1])
        assert float(Wg[0, 0, :32].sum()) == {torch.float16: 256.0, torch.bfloat16: 48.0}[dtype]
    c = M.order_case(dtype, 4, "mxfp4")
    trip(c.W, c.exps)


def test_pack_experts_restatement_is_a_permutation_with_the_interleave():
    E, inter, K = 2, 320, 256
    W = np.arange(E * 2 * inter * K, dtype=np.int64).reshape(E, 2 * inter, K)
    p = M.pack_experts(W, 1)
    assert np.array_equal(np.sort(p), W.reshape(-1))
    # tile t of expert e, chunk 0, unit 0 (b = 0, j = 0), lane tid = 64 w + 16 g + n: row 16 w + n of the tile, k = 16 g .. + 7
    per = 2 * inter * K
    for e, t, tid in ((0, 0, 0), (1, 4, 5 + 64 * 3), (1, 4, 5 + 64 * 4), (0, 2, 511)):
        w, g, n = tid // 64, (tid // 16) % 4, tid % 16
        q = 16 * w + n
        row = 64 * t + q if q < 64 else inter + 64 * t + q - 64
        assert np.array_equal(p[e * per + t * 128 * K + 8 * tid:][:8], W[e, row, 16 * g:16 * g + 8])
    assert np.array_equal(M.pack_experts(W[:, :256], 0), np.concatenate([G.pack_weights(W[e, :256]) for e in range(E)]))
