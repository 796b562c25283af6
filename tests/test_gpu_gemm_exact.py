"""Exact-integer parity of the model-dtype weight-streaming GEMMs (csrc/gemm_kernels.hip) on inputs planted by tests/gemm_planting.py: every
product and partial sum is an integer below 2^24, so what a kernel must store is determined bit for bit and every comparison below is
torch.equal on the stored tensor against the float64 reference (-0 and +0 compare equal; a NaN never does).  Outputs and partials start
NaN-filled.  Every case runs the helper's self check (each named fault would change >= half of the outputs it touches) before it launches.

  entry point                      inputs                                    compared (all by equality)
  samd_gemm_skinny, _groups        small and large sums; rows 16-64,         T output (one split); EVERY fp32 partial against the exact sum
                                   N 128 / 384, 13 (chunks, splits)          over its own chunk range; the two layouts against each other;
                                                                             rows < n unchanged when rows >= n of A are NaN
  samd_gemm_pairs_silu,            silu planting (silu(g) = g, output =      T output = round(g * u); the two kernels against each other
  samd_gemm_skinny_silu            round(g * u)); chunks 1-7; inter so that  where inter % 64 == 0
                                   workgroups hold 1, 1-2, 2-3, 3-4, 4
                                   pairs and two workgroups share a CU
  samd_gemm_cs_residual            small sums + integer residuals, chunks    x; ssq (exact integer sums of 16 squares); at 8 rows: rows
                                   1-26 and 43, rows 16 / 8, N 16 / 48;      8..15 of x and ssq untouched with rows 8..15 of A NaN
                                   one large-sum case per row count          (large sums: x through both roundings, ssq in the kernel's
                                                                             butterfly order)
  samd_gemm_qkv_rope, _vt          small and large sums, planted cos | sin;  q rows, K rows (exactly +-x1 / +-x2 of the rounded sums), V rows
                                   rows 16-64, chunks 1-9 and 16, four head  / V^T columns (the rounded sums); everything else untouched,
                                   layouts, n < and == rows, three L         rows past the cache included
  samd_gemm_pack_groups, _qkv64    2-byte counter payload                    the numpy restatements of the header comments

Recorded on an MI355X: samd_device_info reports 256 CUs, so the share sweep ran at inter = 16 x {1, 3, 256, 296, 696, 996, 1024, 1300}.
SiLU epilogue: the device's __expf and fp32 divide deliver silu(g) = g exactly for every planted gate (g in [24, 64] bf16, [24, 512] fp16):
the outputs equal round(g * u) bit for bit, no fallback to a 1-ulp bar was needed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import gemm_planting as G
import samd_hip
from samd_hip import _ptr as P, check, current_stream, torch_dtype_code

DTYPES = list(G.DTYPES)
REGIMES = ["small", "large"]
NAN = float("nan")


def dev(x, dtype):
    return x.to(dtype).cuda().contiguous()


def cu_count():
    info = np.zeros(4, dtype=np.int64)
    check(samd_hip.lib().samd_device_info(P(info)))
    return int(info[1])


def same(got, want, what):
    """equality of the stored values, with the first mismatch in the message"""
    want = want.to(got.device)
    if got.shape == want.shape and torch.equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = torch.nonzero(~(got == want))
    i = tuple(bad[0].tolist())
    pytest.fail(f"{what}: {len(bad)} of {got.numel()} stored values differ; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


def untouched(t, what):
    assert bool(torch.isnan(t).all()), what


def packed(fn, W, *shape):
    out = torch.empty_like(W)
    check(fn(P(W), P(out), *shape, current_stream()))
    return out


def launch_skinny(fn, A, Wp, rows, N, K, splits, dtype):
    if splits == 1:
        out = torch.full((rows, N), NAN, device="cuda", dtype=dtype)
        check(fn(P(A), P(Wp), rows, N, K, 1, None, P(out), torch_dtype_code(dtype), current_stream()))
    else:
        out = torch.full((splits, rows, N), NAN, device="cuda", dtype=torch.float32)
        check(fn(P(A), P(Wp), rows, N, K, splits, P(out), None, torch_dtype_code(dtype), current_stream()))
    return out


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rows", G.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_skinny_and_groups_store_the_exact_sums(dtype, rows, regime):
    L = samd_hip.lib()
    for N in G.SKINNY_N:
        for chunks, splits in G.CHUNK_SPLITS:
            K = G.KC * chunks
            W, draws = G.skinny_case(dtype, rows, N, chunks, splits, regime)
            Wd = dev(W, dtype)
            layouts = ((L.samd_gemm_skinny, packed(L.samd_gemm_pack_weights, Wd, N, K)), (L.samd_gemm_skinny_groups, packed(L.samd_gemm_pack_groups, Wd, N, K)))
            what = f"N={N} chunks={chunks} splits={splits}"
            for A, want in draws:
                Ad = dev(A, dtype)
                outs = [launch_skinny(fn, Ad, w, rows, N, K, splits, dtype) for fn, w in layouts]
                torch.cuda.synchronize()
                # one split: the exact sum rounded once to T; else every fp32 partial = the exact sum over ITS chunk range
                same(outs[0], want.to(dtype) if splits == 1 else want.float(), "samd_gemm_skinny " + what)
                same(outs[1], outs[0], "samd_gemm_skinny_groups vs samd_gemm_skinny " + what)
            # row independence: rows >= n of A are NaN, rows < n keep their values
            n = rows - 5
            An = Ad.clone()
            An[n:] = NAN
            for (fn, w), full in zip(layouts, outs):
                got = launch_skinny(fn, An, w, rows, N, K, splits, dtype)
                torch.cuda.synchronize()
                same(got[..., :n, :], full[..., :n, :], f"rows < {n} with NaN rows behind them, " + what)
                assert bool(torch.isnan(got[..., n:, :]).all())


def interleave(wg, wu, group):
    inter, K = wg.shape
    return torch.stack([wg.view(inter // group, group, K), wu.view(inter // group, group, K)], dim=1).reshape(2 * inter, K).contiguous()


@pytest.mark.parametrize("rows", G.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_epilogues_store_the_rounded_product(dtype, rows):
    """samd_gemm_pairs_silu and samd_gemm_skinny_silu: the output is the single rounding of the exact product g * u"""
    L, dc = samd_hip.lib(), torch_dtype_code(dtype)
    cases = [(64, c) for c in G.SILU_CHUNKS]                        # depth 3 at 16 / 32 rows, depth 2 at 48 / 64
    n_cu = cu_count()
    for rows_s, K in ((16, 256), (64, 512)):                        # shares of 1 .. 4 pairs and a grid past one workgroup per CU
        if rows_s == rows:
            for pairs, shares, rounds in G.share_pairs(n_cu):
                assert G.pair_shares(pairs, n_cu) == (min(pairs, n_cu) if rounds == 1 else rounds * n_cu, shares), (pairs, n_cu)
                cases.append((16 * pairs, K // G.KC))
    for inter, chunks in cases:
        K = G.KC * chunks
        Wg, Wu, draws = G.silu_case(dtype, rows, inter, chunks)
        wg, wu = dev(Wg, dtype), dev(Wu, dtype)
        w16 = packed(L.samd_gemm_pack_groups, interleave(wg, wu, 16), 2 * inter, K)
        w64 = packed(L.samd_gemm_pack_weights, interleave(wg, wu, 64), 2 * inter, K) if inter % 64 == 0 else None
        what = f"inter={inter} chunks={chunks}"
        for A, want in draws:
            Ad = dev(A, dtype)
            out = torch.full((rows, inter), NAN, device="cuda", dtype=dtype)
            check(L.samd_gemm_pairs_silu(P(Ad), P(w16), rows, inter, K, P(out), dc, current_stream()))
            torch.cuda.synchronize()
            same(out, want.to(dtype), "samd_gemm_pairs_silu " + what)
            if w64 is not None:
                ref = torch.full((rows, inter), NAN, device="cuda", dtype=dtype)
                check(L.samd_gemm_skinny_silu(P(Ad), P(w64), rows, 2 * inter, K, P(ref), dc, current_stream()))
                torch.cuda.synchronize()
                same(ref, want.to(dtype), "samd_gemm_skinny_silu " + what)
                assert torch.equal(out, ref)


@pytest.mark.parametrize("rows", G.CS_ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cs_residual_stores_the_exact_rows_and_sums_of_squares(dtype, rows):
    L, dc = samd_hip.lib(), torch_dtype_code(dtype)
    cases = [(N, chunks, "small") for N in G.CS_N for chunks in G.CS_CHUNKS] + [(48, G.CS_LARGE_CHUNKS, "large")]
    for N, chunks, regime in cases:
        K = G.KC * chunks
        W, x0, draws = G.cs_case(dtype, rows, N, chunks, regime)
        Wp = packed(L.samd_gemm_pack_groups, dev(W, dtype), N, K)
        what = f"N={N} chunks={chunks} {regime}"
        for A, x, ssq in draws:
            Ad = dev(A, dtype)
            if rows == 8:
                Ad[8:] = NAN                                        # the 8-row form reads rows 0..7 only
            xd = dev(x0, dtype)
            sd = torch.full((N // 16, 16), NAN, device="cuda", dtype=torch.float32)
            check(L.samd_gemm_cs_residual(P(Ad), P(Wp), rows, N, K, P(xd), P(sd), dc, current_stream()))
            torch.cuda.synchronize()
            same(xd[:rows], x.to(dtype), "x " + what)
            same(sd[:, :rows], ssq.t().contiguous(), "ssq " + what)
            if rows == 8:
                same(xd[8:], x0[8:].to(dtype), "rows 8..15 of x " + what)
                untouched(sd[:, 8:], "rows 8..15 of ssq " + what)


@pytest.mark.parametrize("heads", G.ROPE_HEADS)
@pytest.mark.parametrize("rows", G.ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_qkv_rope_stores_the_exact_rotated_rows(dtype, rows, heads):
    L, dc = samd_hip.lib(), torch_dtype_code(dtype)
    H, Hkv = heads
    max_len = G.ROPE_MAX_LEN
    assert G.qkv_tile_groups(H + 2 * Hkv, cu_count()) == (4 if heads == (8, 1) else 3)         # 64-column tiles for 1280 columns, 48 otherwise
    for i, chunks in enumerate(G.ROPE_CHUNKS):
        for r, regime in enumerate(REGIMES):
            K = G.KC * chunks
            W, cs, draws = G.rope_case(dtype, rows, H, Hkv, chunks, regime)
            W64 = packed(L.samd_gemm_pack_qkv64, dev(W, dtype), H + 2 * Hkv, K)
            n = rows if i % 2 else rows - 3                          # n == rows_pad / n < rows_pad
            Lc = (0, 37, max_len - n + 2)[(i + r) % 3]               # L = 0, odd, and L + n > max_len (the last two rows fall past the cache)
            live = min(n, max_len - Lc)
            d_L = torch.tensor([Lc], dtype=torch.int32, device="cuda")
            d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
            csd = cs.cuda()
            what = f"chunks={chunks} {regime} n={n} L={Lc}"
            for A, q, k, v in draws:
                Ad = dev(A, dtype)
                for vt in (False, True):
                    qd = torch.full((rows, H, 128), NAN, device="cuda", dtype=dtype)
                    kc = torch.full((Hkv, max_len, 128), NAN, device="cuda", dtype=dtype)
                    vc = torch.full((Hkv, 128, max_len) if vt else (Hkv, max_len, 128), NAN, device="cuda", dtype=dtype)
                    fn = L.samd_gemm_qkv_rope_vt if vt else L.samd_gemm_qkv_rope
                    check(fn(P(Ad), P(W64), rows, K, P(csd), P(d_L), P(d_n), P(qd), P(kc), P(vc), H, Hkv, 128, max_len, dc, current_stream()))
                    torch.cuda.synchronize()
                    w = what + (" vt" if vt else "")
                    same(qd[:live], q[:live].to(dtype), "q " + w)
                    same(kc[:, Lc:Lc + live], k[:live].transpose(0, 1).to(dtype), "K rows " + w)
                    vrows = vc.transpose(1, 2) if vt else vc          # [Hkv, max_len, 128] either way
                    same(vrows[:, Lc:Lc + live], v[:live].transpose(0, 1).to(dtype), "V rows " + w)
                    untouched(qd[live:], "q rows >= n " + w)
                    untouched(kc[:, :Lc], "K cache below L " + w)
                    untouched(kc[:, Lc + live:], "K cache past L + n " + w)
                    untouched(vrows[:, :Lc], "V cache below L " + w)
                    untouched(vrows[:, Lc + live:], "V cache past L + n " + w)


def counter(N, K):
    return torch.arange(N * K, dtype=torch.int32).to(torch.int16).view(N, K)          # any 2-byte payload


def test_pack_groups_is_the_documented_permutation():
    N, K = 48, 768
    W = counter(N, K)
    out = packed(samd_hip.lib().samd_gemm_pack_groups, W.cuda(), N, K)
    assert np.array_equal(out.cpu().numpy().reshape(-1), G.pack_groups(W.numpy()))


@pytest.mark.parametrize("heads,cg", [(6, 3), (10, 4)])
def test_pack_qkv64_is_the_documented_permutation(heads, cg):
    """48-column tiles at 6 heads, 64-column tiles at 10 (1280 columns are no multiple of 48), with the rotate_half row permutation"""
    N, K = heads * 128, 512
    assert G.qkv_tile_groups(heads, cu_count()) == cg
    W = counter(N, K)
    out = packed(samd_hip.lib().samd_gemm_pack_qkv64, W.cuda(), heads, K)
    assert np.array_equal(out.cpu().numpy().reshape(-1), G.pack_qkv(W.numpy(), cg))
