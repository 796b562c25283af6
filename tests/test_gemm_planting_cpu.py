"""tests/gemm_planting.py on the CPU: every case tests/test_gpu_gemm_exact.py launches is built here too -- its range bars, its zero
uncovered share, every fault visible with the required margin, the rounding-regime conditions (each builder asserts them) -- plus the
recipe's table, the rounding helpers and the three layout restatements against a slow element-by-element reading of their comments."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gemm_planting as G

DTYPES = list(G.DTYPES)
REGIMES = ["small", "large"]
N_CU = 256                                  # the pair counts of the share sweep on an MI355X (the GPU file computes them from the device)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,rows", [(256, 64), (2560, 64), (6656, 16), (11008, 64), (6656, 8)])
def test_small_sum_recipe_keeps_every_output_below_the_bar(dtype, K, rows):
    draws, W = G.small_draws(K + rows, rows, 384, K, dtype)
    assert G.uncovered_share(draws) == 0.0
    for A in draws:
        G.assert_small(A @ W.t(), dtype)
    dense = G.density(K, dtype) == 1.0
    assert dense == (dtype == torch.float16 or K <= 1792) and (len(draws) == 1) >= dense
    if dtype == torch.bfloat16 and (K, rows) == (6656, 8):
        assert 0.04 < G.uncovered_share(draws[:1]) < 0.12            # one draw leaves ~8 % of the columns unused: further draws matter


@pytest.mark.parametrize("dtype", DTYPES)
def test_rounding_helpers(dtype):
    one = 2.0 ** -G.MANT[dtype]
    x = torch.tensor([1.0 + one / 2, 1.0 + 3 * one / 2, -(1.0 + one / 2), -(1.0 + 3 * one / 2), 1.0 + one / 4, 1.0 + 3 * one / 4, 257.0, 259.0, -3.0],
                     dtype=G.F64)
    assert G.rounded(x, dtype).tolist() == [1.0, 1.0 + 2 * one, -1.0, -(1.0 + 2 * one), 1.0, 1.0 + one, 257.0 if dtype == torch.float16 else 256.0,
                                            259.0 if dtype == torch.float16 else 260.0, -3.0]
    assert G.truncated(x, dtype).tolist() == [1.0, 1.0 + one, -1.0, -(1.0 + one), 1.0, 1.0, 257.0 if dtype == torch.float16 else 256.0,
                                              259.0 if dtype == torch.float16 else 258.0, -3.0]
    assert G.ulp(torch.tensor([1.0, 1.5, 2.0, 300.0], dtype=G.F64), dtype).tolist() == [one, one, 2 * one, 256 * one]
    if dtype == torch.bfloat16:                                      # every odd sum in [256, 512) is a tie
        odd = torch.arange(257, 512, 2, dtype=G.F64)
        assert bool((2 * (odd - G.truncated(odd, dtype)).abs() == G.ulp(odd, dtype)).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_sum_conditions_fail_where_nothing_rounds(dtype):
    """check_large is a condition, not a formality: W in [-8, 8] at K = 256 leaves (nearly) every sum representable in fp16"""
    rng = np.random.default_rng(0)
    A, W = G.as_t(rng.integers(-8, 9, (64, 256))), G.as_t(rng.integers(-8, 9, (384, 256)))
    with pytest.raises(AssertionError):
        G.check_large(A @ W.t(), dtype)
    A, W = G.large_case(1, 64, 384, 256, dtype)
    inexact, tie, differs = G.check_large(A @ W.t(), dtype)
    assert inexact > 0.5 and tie > 0 and differs > 0.25


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rows", G.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_skinny_cases(dtype, rows, regime):
    for N in G.SKINNY_N:
        for chunks, splits in G.CHUNK_SPLITS:
            W, draws = G.skinny_case(dtype, rows, N, chunks, splits, regime)
            assert draws[0][1].shape == ((rows, N) if splits == 1 else (splits, rows, N))


def test_split_sums_cover_every_chunk_once():
    P = torch.arange(10, dtype=G.F64).view(10, 1, 1)
    for splits in range(1, 11):
        ranges = [G.split_range(s, 10, splits) for s in range(splits)]
        assert ranges[0][0] == 0 and ranges[-1][1] == 10 and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ranges, ranges[1:] + [(10, 11)]))
        assert G.split_sums(P, splits).sum().item() == 45.0
    assert [G.split_range(s, 10, 3) for s in range(3)] == [(0, 3), (3, 6), (6, 10)]


@pytest.mark.parametrize("rows", G.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_cases(dtype, rows):
    for chunks in G.SILU_CHUNKS:
        Wg, Wu, draws = G.silu_case(dtype, rows, 64, chunks)
        assert len(draws) == -(-(256 * chunks - 1) // (G.SILU_Q[dtype] * rows))
    for rows_s, K in ((16, 256), (64, 512)):
        if rows_s == rows:
            for pairs, shares, rounds in G.share_pairs(N_CU):
                assert G.pair_shares(pairs, N_CU) == (min(pairs, N_CU) if rounds == 1 else rounds * N_CU, shares)
                G.silu_case(dtype, rows, 16 * pairs, K // 256)


def test_share_pairs_on_256_cus():
    assert [p for p, _, _ in G.share_pairs(256)] == [1, 3, 256, 296, 696, 996, 1024, 1300]
    assert G.pair_shares(688, 256) == (256, {2, 3})                # Vicuna-7B's 11008


@pytest.mark.parametrize("rows", G.CS_ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cs_residual_cases(dtype, rows):
    for N in G.CS_N:
        for chunks in G.CS_CHUNKS:
            W, x0, draws = G.cs_case(dtype, rows, N, chunks, "small")
            assert all(bool((A[:rows] != 0).any()) for A, _, _ in draws)
    G.cs_case(dtype, rows, 48, G.CS_LARGE_CHUNKS, "large")
    # chunks per wave: wave w takes chunks w, w + 8, ...
    per_wave = {c: {(c - w + 7) // 8 for w in range(8)} for c in G.CS_CHUNKS}
    assert per_wave[1] == {0, 1} and per_wave[8] == {1} and per_wave[12] == {1, 2} and per_wave[20] == {2, 3} and per_wave[26] == {3, 4}
    assert per_wave[43] == {5, 6}


@pytest.mark.parametrize("heads", G.ROPE_HEADS)
@pytest.mark.parametrize("rows", G.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_cases(dtype, rows, heads):
    for chunks in G.ROPE_CHUNKS:
        for regime in REGIMES:
            G.rope_case(dtype, rows, heads[0], heads[1], chunks, regime)
    assert G.qkv_tile_groups(heads[0] + 2 * heads[1], N_CU) == (4 if heads == (8, 1) else 3)


def test_rope_reference_matches_rotate_half():
    """rope_ref against HF's apply_rotary_pos_emb written out (q * cos + rotate_half(q) * sin) on generic cos | sin"""
    rng = np.random.default_rng(2)
    rows, H, Hkv = 5, 2, 1
    y = G.rounded(G.as_t(rng.standard_normal((rows, (H + 2 * Hkv) * 128))), torch.float16)
    ang = G.as_t(rng.uniform(0, 6.28, (rows, 64)))
    cs = torch.zeros((64, 128), dtype=torch.float32)
    cs[:rows, :64], cs[:rows, 64:] = ang.cos().float(), ang.sin().float()
    q, k, v = G.rope_ref(y, cs, H, Hkv, torch.float16)
    x = y.view(rows, H + 2 * Hkv, 128)
    cos, sin = torch.cat((cs[:rows, :64],) * 2, -1).double()[:, None], torch.cat((cs[:rows, 64:],) * 2, -1).double()[:, None]
    rot_half = torch.cat((-x[..., 64:], x[..., :64]), dim=-1)
    want = G.rounded(x * cos + rot_half * sin, torch.float16)
    assert torch.equal(q, want[:, :H]) and torch.equal(k, want[:, H:H + Hkv]) and torch.equal(v, x[:, H + Hkv:])
    planted = G.rope_cs(7)
    assert bool(((planted[:7, :64] ** 2 + planted[:7, 64:] ** 2) == 1).all()) and bool(torch.isnan(planted[7:]).all())
    pair = torch.stack((planted[:7, :64], planted[:7, 64:]), dim=-1)                              # (cos, sin) per (row, j)
    assert not bool((pair[:6] == pair[1:]).all(-1).any()) and not bool((pair[:, :63] == pair[:, 1:]).all(-1).any())      # neighbours differ


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------------
def is_permutation(packed, W):
    return packed.shape == (W.size,) and np.array_equal(np.sort(packed), np.sort(W.reshape(-1)))


def test_pack_weights_restatement():
    N, K = 256, 768
    W = np.arange(N * K, dtype=np.int64).reshape(N, K)
    out = G.pack_weights(W)
    assert is_permutation(out, W)
    for u in np.random.default_rng(0).integers(0, N * K // 8, 4000):
        blk, inn = divmod(int(u), 4096)
        t, c = divmod(blk, K // 256)
        bj, tid = divmod(inn, 512)
        b, j = divmod(bj, 2)
        w, g, n = tid // 64, (tid // 16) % 4, tid % 16
        row, col = 128 * t + 16 * w + n, 256 * c + 64 * b + 16 * g + 8 * j
        assert np.array_equal(out[8 * u:8 * u + 8], W[row, col:col + 8])


def test_pack_groups_restatement():
    N, K = 48, 768
    W = np.arange(N * K, dtype=np.int64).reshape(N, K)
    out = G.pack_groups(W)
    assert is_permutation(out, W)
    for u in range(N * K // 8):
        blk, inn = divmod(u, 512)
        gi, c = divmod(blk, K // 256)
        bj, lane = divmod(inn, 64)
        b, j = divmod(bj, 2)
        g, n = divmod(lane, 16)
        row, col = 16 * gi + n, 256 * c + 64 * b + 16 * g + 8 * j
        assert np.array_equal(out[8 * u:8 * u + 8], W[row, col:col + 8])


@pytest.mark.parametrize("heads,cg", [(6, 3), (10, 4), (3, 3), (1, 4)])
def test_pack_qkv_restatement(heads, cg):
    N, K = heads * 128, 512
    W = np.arange(N * K, dtype=np.int64).reshape(N, K)
    out = G.pack_qkv(W, cg)
    assert is_permutation(out, W)
    perm = G.qkv_row_permutation(heads, cg)
    assert np.array_equal(np.sort(perm), np.arange(N))
    pp = 8 * cg
    for u in range(0, N * K // 8, 3):
        blk, inn = divmod(u, 512 * cg)
        t, c = divmod(blk, K // 256)
        blj, x = divmod(inn, 128 * cg)
        bl, j = divmod(blj, 2)
        wv, g, n = x // 64, (x // 16) % 4, x % 16
        kh, gc = divmod(wv, cg)
        q = 16 * gc + n                                            # packed row 16 cg t + q
        pair = pp * t + (q if q < pp else q - pp)
        head, jj = divmod(pair, 64)
        row = 128 * head + jj + (0 if q < pp else 64)              # pair P = head columns j and 64 + j
        col = 256 * c + 64 * (2 * kh + bl) + 16 * g + 8 * j
        assert np.array_equal(out[8 * u:8 * u + 8], W[row, col:col + 8])
    # a tile holds complete rotate_half pairs: its first half of rows are columns j < 64 of a head, the second half their partners
    rows = perm.reshape(-1, 2, pp)
    assert np.array_equal(rows[:, 0] + 64, rows[:, 1]) and bool((rows[:, 0] % 128 < 64).all())


def test_qkv_tile_rule():
    assert G.qkv_tile_groups(96, 256) == 3 and G.qkv_tile_groups(120, 256) == 4          # 12288 = 256 x 48; 15360 = 320 x 48 (two rounds) or 240 x 64
    assert G.qkv_tile_groups(10, 256) == 4 and G.qkv_tile_groups(6, 256) == 3 and G.qkv_tile_groups(15, 256) == 3
