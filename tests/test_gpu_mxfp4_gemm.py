"""GPU parity of the MXFP4 weight-only projection (samd_gemm_pack_f4 + samd_gemm_skinny_f4):
out[m][n] = sum_k A[m][k] * fp4(q[n][k]) * 2^(e8[n][k/32] - 127), A in the model dtype.  Tolerances are test_gpu_gemm.py's (fp32 accumulation,
one rounding); the planted cases pin the layout, the nibble order, the block-scale index and the conversion element by element, exactly, and
decide the lower end of fp16's exponent range (samd_hip/mxfp4.py: FP16_EMIN)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import mxfp4 as MX
from test_gpu_fp8_gemm import SHAPES, one_hot_ks
from test_mxfp4_weights_cpu import packed_f4_np

TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}          # test_gpu_gemm.py's


def pack(q, e8):
    N, K = q.shape[0], 2 * q.shape[1]
    out = torch.full((MX.packed_bytes(N, K),), 0x5A, dtype=torch.uint8, device="cuda")
    check(lib().samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(out), N, K, current_stream()))
    return out


def run(A, qp, N, K, rows_pad, splits, dtype):
    """(the dtype output [rows_pad, N] for splits == 1 | the fp32 partials [splits, rows_pad, N]), from NaN-filled buffers"""
    if splits == 1:
        out = torch.full((rows_pad, N), float("nan"), device="cuda", dtype=dtype)
        check(lib().samd_gemm_skinny_f4(_ptr(A), _ptr(qp), rows_pad, N, K, 1, None, _ptr(out), torch_dtype_code(dtype), current_stream()))
    else:
        out = torch.full((splits, rows_pad, N), float("nan"), device="cuda", dtype=torch.float32)
        check(lib().samd_gemm_skinny_f4(_ptr(A), _ptr(qp), rows_pad, N, K, splits, _ptr(out), None, torch_dtype_code(dtype), current_stream()))
    torch.cuda.synchronize()
    return out


def weights(N, K, seed, dtype=None):
    """rows of differing magnitude whose 32-k blocks differ as well (x 2^{0..5} per block): neighbouring blocks carry different exponents"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = torch.randn((N, K), generator=g, device="cuda") * 0.05 * (1 + torch.rand((N, 1), generator=g, device="cuda") * 8)
    blk = torch.exp2(torch.randint(0, 6, (N, K // 32), generator=g, device="cuda").float()).repeat_interleave(32, dim=1)
    return MX.quantize_blocks(W * blk, dtype)


@pytest.mark.parametrize("N,K", [(128, 256), (384, 768), (4096, 11008), (6144, 4096)])
def test_pack_matches_numpy_layout(N, K):
    g = torch.Generator(device="cuda").manual_seed(N + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g, device="cuda", dtype=torch.uint8)
    e8 = torch.randint(0, 256, (N, K // 32), generator=g, device="cuda", dtype=torch.uint8)
    got = pack(q, e8).cpu().numpy()
    assert np.array_equal(got, packed_f4_np(q.cpu().numpy(), e8.cpu().numpy()))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows_pad", [16, 32, 48, 64])
@pytest.mark.parametrize("N,K", SHAPES)
def test_mxfp4_gemm_matches_float64_reference(dtype, rows_pad, N, K):
    q, e8 = weights(N, K, N + K, dtype)
    qp = pack(q, e8)
    g = torch.Generator(device="cuda").manual_seed(N + K + rows_pad)
    A = torch.randn((rows_pad, K), generator=g, device="cuda").to(dtype)
    want = A.double() @ MX.dequantize_blocks(q, e8).double().t()
    bound = TOL[dtype] * max(1.0, want.abs().max().item())
    chunks = K // 256
    for splits in sorted({1, 2, 3, lib().samd_gemm_splits(N, K, rows_pad), chunks} & set(range(1, chunks + 1))):
        got = run(A, qp, N, K, rows_pad, splits, dtype)
        assert torch.isfinite(got).all(), splits                      # every element (or partial) written
        got = got.double() if splits == 1 else got.double().sum(0)
        err = (got - want).abs().max().item()
        assert err <= bound, (splits, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
def planted_ks(K):
    """one_hot_ks of the FP8 test plus both sides of every 32-k block seam (first and last chunk in full)"""
    ks = set(one_hot_ks(K))
    for base in (0, K - 256):
        for s in range(0, 256, 32):
            ks |= {base + s, base + s + 31}
    return sorted(ks)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows_pad,N,K", [(16, 256, 512), (32, 384, 2816), (48, 128, 768), (64, 256, 4096), (64, 4096, 11008)])
def test_one_hot_rows_pick_single_weights(dtype, rows_pad, N, K):
    """A row m = e_{k_m}: out[m][n] must equal fp4(q[n][k_m]) * 2^e exactly (one nonzero product of a weight that is exact in the model
    dtype) -- for every split count the partials hold it in one split and exact zeros elsewhere.  The k set is larger than a launch has
    rows, so it goes through in passes.  Faults (nibbles swapped, a dword off, the neighbouring block's scale, the next column's scale, no
    scale) miss on more than half the elements."""
    q, e8 = weights(N, K, 7 * N + K, dtype)
    ex = e8.int() - 127
    assert (ex[:, 1:] != ex[:, :-1]).float().mean().item() > 0.5      # neighbouring blocks differ in exponent: the seam faults are visible
    assert (ex[1:] != ex[:-1]).float().mean().item() > 0.5            # and so do neighbouring columns
    qp = pack(q, e8)
    W = MX.dequantize_blocks(q, e8)
    assert torch.equal(W.to(dtype).float(), W)
    all_ks = planted_ks(K)
    all_ks += all_ks[:(-len(all_ks)) % rows_pad]
    raw = MX.dequantize_blocks(q, torch.full_like(e8, 127))           # the bare fp4 values
    scale = torch.exp2(ex.float())                                    # [N, K/32]
    miss = {}
    for p0 in range(0, len(all_ks), rows_pad):
        ks = all_ks[p0:p0 + rows_pad]
        A = torch.zeros((rows_pad, K), device="cuda", dtype=dtype)
        A[torch.arange(rows_pad), torch.tensor(ks)] = 1
        want = W[:, ks].t().to(dtype)
        for splits in sorted({1, 2, K // 256}):
            got = run(A, qp, N, K, rows_pad, splits, dtype)
            if splits > 1:
                assert torch.isfinite(got).all()
                got = got.sum(0).to(dtype)
            assert torch.equal(got, want), (splits, ks, (got.float() - want.float()).abs().max().item())
        kb = [k // 32 for k in ks]
        faults = {
            "k ^ 1 (nibbles swapped)": W[:, [k ^ 1 for k in ks]].t(),
            "k ^ 8 (dword off)": W[:, [k ^ 8 for k in ks]].t(),
            "k ^ 32 (the neighbouring block's scale)": (raw[:, ks] * scale[:, [b ^ 1 for b in kb]]).t(),
            "column + 1 scale": (raw[:, ks] * scale.roll(1, dims=0)[:, kb]).t(),
            "no scale": raw[:, ks].t(),
        }
        for name, f in faults.items():
            miss.setdefault(name, []).append((f.float() != want.float()).float().mean().item())
    for name, m in miss.items():
        print(f"fault {name}: misses {np.mean(m):.3f} of the elements")
        assert np.mean(m) > 0.5, (name, np.mean(m))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_every_code_and_every_exponent_converts_exactly(dtype):
    """Column c holds code (c + k) mod 16 at k, and block (c, b) has exponent lo + (c + b) mod (hi - lo + 1): with one-hot rows over ALL k of
    the first two chunks plus seams of the last, every code passes at every nibble, byte, dword and lane position, every exponent of the
    dtype's range is some block's scale, and every product must come out exact.  This decides fp16's lower bound: the exponents
    -23 .. -14 produce fp16 subnormals, and FP16_EMIN is -23 exactly when the instruction delivers them exactly, else -13 -- whichever the
    module declares, the other outcome fails here; an error is never tolerated inside the declared range."""
    lo, hi = (-23, 13) if dtype == torch.float16 else (-125, 125)         # the widest candidate range
    N, K, rows = 256, 1024, 64
    c = torch.arange(N, device="cuda")[:, None]
    k = torch.arange(K, device="cuda")[None, :]
    codes = ((c + k) % 16).to(torch.uint8)
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    ex = lo + (c + torch.arange(K // 32, device="cuda")[None, :]) % (hi - lo + 1)
    e8 = (ex + 127).to(torch.uint8)
    assert set(ex.unique().tolist()) == set(range(lo, hi + 1))
    qp = pack(q, e8)
    W = MX.dequantize_blocks(q, e8)
    ks_all = list(range(512)) + [K - 256, K - 225, K - 224, K - 33, K - 32, K - 1] + list(range(600, 658))
    assert len(ks_all) % rows == 0
    exact = torch.ones((N, K // 32), dtype=torch.bool, device="cuda")   # per block: every planted element came out exact
    seen = torch.zeros(16, dtype=torch.bool, device="cuda")
    for p0 in range(0, len(ks_all), rows):
        ks = ks_all[p0:p0 + rows]
        A = torch.zeros((rows, K), device="cuda", dtype=dtype)
        A[torch.arange(rows), torch.tensor(ks)] = 1
        got = run(A, qp, N, K, rows, 1, dtype).double().t()             # [N, rows]
        ok = got == W[:, ks].double()
        for i, kk in enumerate(ks):
            exact[:, kk // 32] &= ok[:, i]
        seen[codes[:, ks].unique().long()] = True
    assert bool(seen.all())
    bad_ex = sorted(set(ex[~exact].tolist()))
    print(f"{dtype}: exponents with an inexact product: {bad_ex}")
    dlo, dhi = MX.exponent_range(dtype)
    inside = (ex >= dlo) & (ex <= dhi)
    assert bool(exact[inside].all()), bad_ex                              # exact over the declared range, no tolerance
    if dtype == torch.float16:
        sub = (ex < -13)
        if MX.FP16_EMIN == -23:
            assert bool(exact[sub].all()), bad_ex
        else:                                                             # the -13 bound is declared because the subnormals are NOT exact
            assert MX.FP16_EMIN == -13 and not bool(exact[sub].all())
    # all codes x a dense row, mid-range exponents: the fp32 sums over K of exact products
    e8m = torch.full_like(e8, 127)
    A1 = torch.ones((16, K), device="cuda", dtype=dtype)
    got = run(A1, pack(q, e8m), N, K, 16, 4, dtype).sum(0)
    assert torch.allclose(got.double(), MX.dequantize_blocks(q, e8m).double().sum(1)[None, :].expand(16, N), rtol=1e-6, atol=1e-3)


def test_bad_arguments_are_rejected():
    L, st = lib(), current_stream()
    N, K = 256, 512
    q, e8 = weights(N, K, 1)
    qp = pack(q, e8)
    A = torch.zeros((64, K), device="cuda", dtype=torch.float16)
    out = torch.zeros((64, N), device="cuda", dtype=torch.float16)
    part = torch.zeros((2, 64, N), device="cuda", dtype=torch.float32)
    ok = lambda **kw: dict(dict(A=A, W=qp, rows=16, N=N, K=K, sp=1, part=None, out=out, dt=0), **kw)
    call = lambda a: L.samd_gemm_skinny_f4(_ptr(a["A"]), _ptr(a["W"]), a["rows"], a["N"], a["K"], a["sp"], _ptr(a["part"]), _ptr(a["out"]), a["dt"], st)
    assert call(ok()) == 0
    for bad in (dict(rows=24), dict(rows=128), dict(N=192), dict(N=0), dict(K=384), dict(K=0), dict(A=None), dict(W=None),
                dict(sp=0), dict(sp=3), dict(sp=2, part=None), dict(out=None), dict(dt=2)):
        assert call(ok(**bad)) == -1, bad                             # SAMD_E_INVALID
    assert call(ok(sp=2, part=part, out=None)) == 0
    assert L.samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(q), N, K, st) == -1
    assert L.samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(e8), N, K, st) == -1
    assert L.samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(qp), 100, K, st) == -1
    assert L.samd_gemm_pack_f4(_ptr(q), _ptr(e8), _ptr(qp), N, 300, st) == -1
    assert L.samd_gemm_pack_f4(None, _ptr(e8), _ptr(qp), N, K, st) == -1
    assert L.samd_gemm_pack_f4(_ptr(q), None, _ptr(qp), N, K, st) == -1
    torch.cuda.synchronize()
