"""GPU parity of the dense block-scaled FP8 projection (samd_gemm_pack_f8 + samd_gemm_skinny_f8b):
out[m][n] = sum_b s[n / 128][b] * sum_{k in block b} A[m][k] * q[n][k], q OCP e4m3fn, s fp32 [N / 128][K / 128] as the checkpoint has it, A in the
model dtype.  Exact-integer cases pin every scale index at every split count, one-hot rows pin the layout element by element, random cases use
test_gpu_fp8_gemm.py's tolerance.  Every launch starts from NaN-filled outputs."""
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import fp8 as F8
from test_gpu_fp8_gemm import TOL, one_hot_ks, pack

DTYPES = [torch.float16, torch.bfloat16]
SMALL = [(16, 128, 256), (32, 256, 768), (48, 384, 2816), (64, 256, 4096)]          # (rows, N, K): every row tile, 1-3 tiles, 1-16 chunks, odd chunk counts
LONG = (16, 128, 25600)                                                             # 200 k blocks in one scale row (Qwen3-32B's down projection)


def run(A, qp, sinv, N, K, rows_pad, splits, dtype):
    """(the dtype output [rows_pad, N] for splits == 1 | the fp32 partials [splits, rows_pad, N]), from NaN-filled buffers"""
    if splits == 1:
        out = torch.full((rows_pad, N), float("nan"), device="cuda", dtype=dtype)
        check(lib().samd_gemm_skinny_f8b(_ptr(A), _ptr(qp), _ptr(sinv), rows_pad, N, K, 1, None, _ptr(out), torch_dtype_code(dtype), current_stream()))
    else:
        out = torch.full((splits, rows_pad, N), float("nan"), device="cuda", dtype=torch.float32)
        check(lib().samd_gemm_skinny_f8b(_ptr(A), _ptr(qp), _ptr(sinv), rows_pad, N, K, splits, _ptr(out), None, torch_dtype_code(dtype), current_stream()))
    torch.cuda.synchronize()
    return out


def split_counts(N, K, rows_pad):
    chunks = K // 256
    return sorted({1, 2, 3, lib().samd_gemm_splits(N, K, rows_pad), chunks} & set(range(1, chunks + 1)))


def expand(s):
    return s.repeat_interleave(128, 0).repeat_interleave(128, 1)


# ------------------------------------------------------------------------------------------------ exact integers
@functools.lru_cache(maxsize=None)
def exact_case(rows, N, K):
    """integer A in [-4, 4], integer codes in [-8, 8] (exact in e4m3fn), scales 2^e with e = ((3 i + 2 j) mod 7) - 3 for block (i, j): neighbouring
    blocks differ in both directions.  Every block sum is an integer below 2^12, every scaled partial sum a multiple of 2^-3 below 2^21: the fp32
    result is exact in any order and at any split.  Returns (A fp32, packed codes, s, the per-k-block sums [K / 128, rows, N] in float64)."""
    g = torch.Generator(device="cuda").manual_seed(rows + N + K)
    A = torch.randint(-4, 5, (rows, K), generator=g, device="cuda").float()
    q = torch.randint(-8, 9, (N, K), generator=g, device="cuda").float()
    i, j = torch.arange(N // 128, device="cuda")[:, None], torch.arange(K // 128, device="cuda")[None, :]
    s = torch.exp2((((3 * i + 2 * j) % 7) - 3).float()).contiguous()
    blocks = torch.einsum("mbk,nbk->bmn", A.double().view(rows, K // 128, 128), q.double().view(N, K // 128, 128))
    return A, pack(q.to(torch.float8_e4m3fn)), s, blocks


def scaled_sum(blocks, s):
    """sum_j s[n / 128][j] * blocks[j][m][n] in float64 (exact here)"""
    return torch.einsum("bmn,nb->mn", blocks, s.double().repeat_interleave(128, 0))


FAULTS = {
    "the scale of the next k block": lambda s: s.roll(-1, 1),
    "the scale of the next tile": lambda s: s.roll(-1, 0),
    "one scale for both blocks of a chunk": lambda s: s[:, 0::2].repeat_interleave(2, 1),
    "no scale": lambda s: torch.ones_like(s),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,N,K", SMALL + [LONG])
def test_exact_integers_at_every_split(dtype, rows, N, K):
    A, qp, s, blocks = exact_case(rows, N, K)
    exact = scaled_sum(blocks, s)
    assert exact.abs().max().item() < 2 ** 21 and bool((exact * 8 == (exact * 8).round()).all())
    assert exact.abs().max().item() < 65504                                       # nothing overflows fp16
    want = exact.to(dtype)
    Ad = A.to(dtype)
    for splits in split_counts(N, K, rows):
        got = run(Ad, qp, s, N, K, rows, splits, dtype)
        if splits == 1:
            assert torch.equal(got, want), (splits, (got.double() - exact).abs().max().item())
        else:
            assert torch.isfinite(got).all(), splits                              # every partial written
            assert torch.equal(got.double().sum(0), exact), (splits, (got.double().sum(0) - exact).abs().max().item())
    # the named faults, recomputed: each changes more than half of the outputs it touches, so equality cannot pass by accident
    for name, f in FAULTS.items():
        if name == "the scale of the next tile" and N == 128:
            continue                                                              # (one tile: nothing to confuse)
        wrong = scaled_sum(blocks, f(s))
        miss16 = (wrong.to(dtype) != want).float().mean().item()
        miss32 = (wrong != exact).float().mean().item()
        print(f"{name}: changes {miss32:.4f} of the fp32 sums, {miss16:.4f} of the {dtype} outputs")
        assert miss16 > 0.5 and miss32 > 0.5, (name, miss16, miss32)


# ------------------------------------------------------------------------------------------------ one-hot rows
def spread_scales(N, K, seed):
    """block scales 2^(e_i + u_ij): e_i spread over -18 .. 1 across the tiles (permuted), u_ij uniform in -2 .. 1 per block -- 2^-20 .. 2^2 overall,
    neighbouring blocks differ in both directions"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    nt, nb = N // 128, K // 128
    e = torch.linspace(-18, 1, nt, device="cuda")[torch.randperm(nt, generator=g, device="cuda")] if nt > 1 else torch.tensor([-3.0], device="cuda")
    return torch.exp2(e[:, None] + torch.rand((nt, nb), generator=g, device="cuda") * 3 - 2).contiguous()


@functools.lru_cache(maxsize=None)
def random_case(N, K):
    g = torch.Generator(device="cuda").manual_seed(N + K)
    W = torch.randn((N, K), generator=g, device="cuda") * 0.05 * (1 + torch.rand((N, 1), generator=g, device="cuda") * 8)
    q, _ = F8.quantize_blocks(W)
    return q, pack(q), spread_scales(N, K, 7 * N + K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_pad,N,K", [(16, 256, 512), (32, 384, 2816), (48, 128, 768), (64, 256, 4096)])
def test_one_hot_rows_pick_single_weights(dtype, rows_pad, N, K):
    """A row m = e_{k_m}: out[m][n] must equal round(s[n / 128][k_m / 128] * float(q[n][k_m])) exactly (one nonzero product, one exact-or-once-
    rounded fp32 FMA, exact zeros from every other block and split, one rounding to the model dtype), at one_hot_ks and at both sides of every
    128-k block seam"""
    q, qp, s = random_case(N, K)
    ks = sorted(set(one_hot_ks(K)) | {128 * j - 1 for j in range(1, K // 128)} | {128 * j for j in range(K // 128)})
    qf, S = q.float(), expand(s)
    for at in range(0, len(ks), rows_pad):
        group = (ks[at:at + rows_pad] + ks[:rows_pad])[:rows_pad]
        A = torch.zeros((rows_pad, K), device="cuda", dtype=dtype)
        A[torch.arange(rows_pad), torch.tensor(group)] = 1
        want32 = qf[:, group].t() * S[:, group].t()
        want = want32.to(dtype)
        for splits in sorted({1, 2, K // 256}):
            got = run(A, qp, s, N, K, rows_pad, splits, dtype)
            if splits > 1:
                assert torch.isfinite(got).all()
                assert torch.equal(got.sum(0), want32), (splits, at)
                got = got.sum(0).to(dtype)
            assert torch.equal(got, want), (splits, at, (got.float() - want.float()).abs().max().item())
        faults = {
            "k + 1": qf[:, [k + 1 if k < K - 1 else k - 1 for k in group]].t() * S[:, group].t(),
            "k +- 16 (lane group)": qf[:, [k ^ 16 for k in group]].t() * S[:, group].t(),
            "the other block of the chunk": qf[:, group].t() * S[:, [k ^ 128 for k in group]].t(),
            "no scale": qf[:, group].t(),
        }
        for name, f in faults.items():
            miss = (f.to(dtype).float() != want.float()).float().mean().item()
            assert miss > 0.5, (name, miss)


# ------------------------------------------------------------------------------------------------ random
def check_random(dtype, rows_pad, N, K, splits_list):
    q, qp, s = random_case(N, K)
    g = torch.Generator(device="cuda").manual_seed(N + K + rows_pad)
    A = (torch.randn((rows_pad, K), generator=g, device="cuda") / 8).to(dtype)        # (sums stay below fp16's max at scale 4)
    want = A.double() @ F8.dequantize_blocks(q, s).double().t()
    tile = want.abs().view(rows_pad, N // 128, 128).amax((0, 2)).repeat_interleave(128)        # each 128-column tile's own magnitude
    sub = 2.0 ** -24 if dtype == torch.float16 else 0.0                                # fp16 subnormal spacing at the smallest tiles
    bound = TOL[dtype] * tile[None, :] + sub
    for splits in splits_list:
        got = run(A, qp, s, N, K, rows_pad, splits, dtype)
        assert torch.isfinite(got).all(), splits
        got = got.double() if splits == 1 else got.double().sum(0)
        ratio = ((got - want).abs() / bound).max().item()
        print(f"{dtype} rows {rows_pad} {N}x{K} splits {splits}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, (splits, ratio)
    if N > 128:                                                                        # the next tile's scales miss by orders of magnitude
        wrong = A.double() @ F8.dequantize_blocks(q, s.roll(-1, 0)).double().t()
        assert ((wrong - want).abs().view(rows_pad, N // 128, 128).amax((0, 2)) > 50 * bound.view(N // 128, 128).amax(1)).float().mean().item() > 0.8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_pad,N,K", SMALL)
def test_random_small_shapes_within_tolerance_of_each_tiles_magnitude(dtype, rows_pad, N, K):
    check_random(dtype, rows_pad, N, K, split_counts(N, K, rows_pad))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_pad", [16, 32, 48, 64])
@pytest.mark.parametrize("N,K", [(6144, 4096), (4096, 12288)])
def test_random_model_shapes_within_tolerance_of_each_tiles_magnitude(dtype, rows_pad, N, K):
    check_random(dtype, rows_pad, N, K, sorted({1, lib().samd_gemm_splits(N, K, rows_pad)}))


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_are_rejected():
    L, st = lib(), current_stream()
    N, K = 256, 512
    q, qp, s = random_case(N, K)
    A = torch.zeros((64, K), device="cuda", dtype=torch.float16)
    out = torch.zeros((64, N), device="cuda", dtype=torch.float16)
    part = torch.zeros((2, 64, N), device="cuda", dtype=torch.float32)
    odd = torch.ones(N // 128 * (K // 128) + 1, device="cuda")[1:]                     # a table that is only 4-byte aligned
    ok = lambda **kw: dict(dict(A=A, W=qp, s=s, rows=16, N=N, K=K, sp=1, part=None, out=out, dt=0), **kw)
    call = lambda a: L.samd_gemm_skinny_f8b(_ptr(a["A"]), _ptr(a["W"]), _ptr(a["s"]), a["rows"], a["N"], a["K"], a["sp"], _ptr(a["part"]), _ptr(a["out"]), a["dt"], st)
    assert call(ok()) == 0
    for bad in (dict(rows=24), dict(rows=128), dict(N=192), dict(N=0), dict(K=384), dict(K=0), dict(s=None), dict(A=None), dict(W=None),
                dict(sp=0), dict(sp=3), dict(sp=2, part=None), dict(out=None), dict(dt=2), dict(s=odd)):
        assert call(ok(**bad)) == -1, bad                             # SAMD_E_INVALID
    assert call(ok(sp=2, part=part, out=None)) == 0
    torch.cuda.synchronize()
