"""GPU parity of the FP8 weight-only projection (samd_gemm_pack_f8 + samd_gemm_skinny_f8): out[m][n] = scale[n] * sum_k A[m][k] * q[n][k]
with OCP e4m3fn q, fp32 column scales and A in the model dtype.  Tolerances are test_gpu_gemm.py's (fp32 accumulation, one rounding);
the planted cases pin the layout, the scale index and the conversion element by element, exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import fp8 as F8
from test_fp8_weights_cpu import packed_f8_np

TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}


def pack(q):
    N, K = q.shape
    out = torch.full((N * K,), 0x5A, dtype=torch.uint8, device="cuda")
    check(lib().samd_gemm_pack_f8(_ptr(q), _ptr(out), N, K, current_stream()))
    return out


def run(A, qp, scale, N, K, rows_pad, splits, dtype):
    """(the dtype output [rows_pad, N] for splits == 1 | the fp32 partials [splits, rows_pad, N]), from NaN-filled buffers"""
    if splits == 1:
        out = torch.full((rows_pad, N), float("nan"), device="cuda", dtype=dtype)
        check(lib().samd_gemm_skinny_f8(_ptr(A), _ptr(qp), _ptr(scale), rows_pad, N, K, 1, None, _ptr(out), torch_dtype_code(dtype), current_stream()))
    else:
        out = torch.full((splits, rows_pad, N), float("nan"), device="cuda", dtype=torch.float32)
        check(lib().samd_gemm_skinny_f8(_ptr(A), _ptr(qp), _ptr(scale), rows_pad, N, K, splits, _ptr(out), None, torch_dtype_code(dtype), current_stream()))
    torch.cuda.synchronize()
    return out


def weights(N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = torch.randn((N, K), generator=g, device="cuda") * 0.05 * (1 + torch.rand((N, 1), generator=g, device="cuda") * 8)
    return F8.quantize_rows(W)


@pytest.mark.parametrize("N,K", [(128, 256), (384, 768), (4096, 11008), (6144, 4096)])
def test_pack_matches_numpy_layout(N, K):
    g = torch.Generator(device="cuda").manual_seed(N + K)
    qb = torch.randint(0, 256, (N, K), generator=g, device="cuda", dtype=torch.uint8)
    got = pack(qb.view(torch.float8_e4m3fn)).cpu().numpy()
    assert np.array_equal(got, packed_f8_np(qb.cpu().numpy()))


SHAPES = [(128, 256), (4096, 4096), (1024, 768), (12288, 4096), (4096, 11008), (256, 512), (32000, 4096), (22016, 4096), (128, 2816),
          (6144, 4096), (28672, 4096), (4096, 14336)]          # test_gpu_gemm.py's, then Llama-3-8B's q|k|v, gate|up, down


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows_pad", [16, 32, 48, 64])
@pytest.mark.parametrize("N,K", SHAPES)
def test_fp8_gemm_matches_float64_reference(dtype, rows_pad, N, K):
    q, scale = weights(N, K, N + K)
    qp = pack(q)
    g = torch.Generator(device="cuda").manual_seed(N + K + rows_pad)
    A = torch.randn((rows_pad, K), generator=g, device="cuda").to(dtype)
    want = A.double() @ F8.dequantize_rows(q, scale).double().t()
    bound = TOL[dtype] * max(1.0, want.abs().max().item())
    chunks = K // 256
    for splits in sorted({1, 2, 3, lib().samd_gemm_splits(N, K, rows_pad), chunks} & set(range(1, chunks + 1))):
        got = run(A, qp, scale, N, K, rows_pad, splits, dtype)
        assert torch.isfinite(got).all(), splits                      # every element (or partial) written
        got = got.double() if splits == 1 else got.double().sum(0)
        err = (got - want).abs().max().item()
        assert err <= bound, (splits, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
def one_hot_ks(K):
    """k positions a wrong lane / block / chunk mapping would confuse: chunk starts and ends, both sides of every 64-k block seam of the first
    and last chunk, the 16-k lane-group and 8-k half-vector edges, and the last k"""
    ks = set()
    for c in range(K // 256):
        ks |= {256 * c, 256 * c + 255}
    for base in (0, K - 256):
        for s in range(0, 256, 64):
            ks |= {base + s, base + s + 63, base + s + 8, base + s + 7, base + s + 16, base + s + 15, base + s + 24, base + s + 40}
    ks.add(K - 1)
    return sorted(k for k in ks if 0 <= k < K)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows_pad,N,K", [(16, 256, 512), (32, 384, 2816), (48, 128, 768), (64, 256, 4096), (64, 4096, 11008)])
def test_one_hot_rows_pick_single_weights(dtype, rows_pad, N, K):
    """A row m = e_{k_m}: out[m][n] must equal round(scale[n] * float(q[n][k_m])) exactly (one nonzero product, an exact fp32 multiply, one
    rounding) -- for every split count the partials hold it in one split and exact zeros elsewhere.  Faults (a neighbouring k, a lane group
    or half-vector off, the wrong column's scale, no scale) miss by a wide margin."""
    q, scale = weights(N, K, 7 * N + K)
    qp = pack(q)
    ks = one_hot_ks(K)
    ks = (ks * (rows_pad // len(ks) + 1))[:rows_pad] if len(ks) < rows_pad else ks[:rows_pad - 2] + [K - 1, ks[len(ks) // 2]]
    A = torch.zeros((rows_pad, K), device="cuda", dtype=dtype)
    A[torch.arange(rows_pad), torch.tensor(ks)] = 1
    qf = q.float()
    want = (qf[:, ks].t() * scale[None, :]).to(dtype)
    for splits in sorted({1, 2, K // 256}):
        got = run(A, qp, scale, N, K, rows_pad, splits, dtype)
        if splits > 1:
            assert torch.isfinite(got).all()
            got = got.sum(0).to(dtype)
        assert torch.equal(got, want), (splits, (got.float() - want.float()).abs().max().item())
    faults = {
        "k + 1": (qf[:, [min(k + 1, K - 1) if k < K - 1 else k - 1 for k in ks]].t() * scale[None, :]),
        "k +- 8 (half vector)": (qf[:, [k ^ 8 for k in ks]].t() * scale[None, :]),
        "k +- 16 (lane group)": (qf[:, [k ^ 16 for k in ks]].t() * scale[None, :]),
        "column + 1 scale": (qf[:, ks].t() * scale.roll(1)[None, :]),
        "no scale": qf[:, ks].t(),
    }
    for name, f in faults.items():
        miss = (f.to(dtype).float() != want.float()).float().mean().item()
        assert miss > 0.5, (name, miss)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_every_finite_code_converts_exactly(dtype):
    """a 256-column matrix whose column c holds code (c + k) mod 256 at k (the two NaN codes replaced by 0): with one-hot rows and scale 1
    every finite e4m3fn code passes through the conversion at every lane / byte position and must come out as its exact value"""
    N, K, rows = 256, 1024, 64
    c = torch.arange(N, device="cuda")[:, None]
    k = torch.arange(K, device="cuda")[None, :]
    codes = ((c + k) % 256).to(torch.uint8)
    codes[(codes == 0x7F) | (codes == 0xFF)] = 0
    q = codes.view(torch.float8_e4m3fn)
    qp = pack(q)
    scale = torch.ones(N, device="cuda")
    ks = list(range(0, K, K // rows))[:rows - 3] + [1, 255, K - 1]
    A = torch.zeros((rows, K), device="cuda", dtype=dtype)
    A[torch.arange(rows), torch.tensor(ks)] = 1
    got = run(A, qp, scale, N, K, rows, 1, dtype)
    want = q.float()[:, ks].t()
    assert torch.equal(got.float(), want)
    assert set(np.unique(codes[:, ks].cpu().numpy()).tolist()) >= set(range(256)) - {0x7F, 0xFF}
    # all codes x a dense row: the fp32 sums over K of exact products
    A1 = torch.ones((16, K), device="cuda", dtype=dtype)
    got = run(A1, qp, scale, N, K, 16, 4, dtype).sum(0)
    assert torch.allclose(got.double(), q.float().double().sum(1)[None, :].expand(16, N), rtol=1e-6, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("splits", [1, 4])
def test_column_scales_across_2_to_the_minus_20_to_4(dtype, splits):
    """per-column scales spread over 2^-20 .. 2^2: each column within tolerance of ITS OWN magnitude (a scale applied to the wrong column
    would be off by orders of magnitude)"""
    N, K, rows = 1024, 4096, 32
    q, _ = weights(N, K, 11)
    scale = torch.exp2(torch.linspace(-20, 2, N, device="cuda"))[torch.randperm(N, device="cuda")]
    qp = pack(q)
    A = (torch.randn((rows, K), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda") / 8).to(dtype)   # (sums stay below fp16's max at scale 4)
    want = A.double() @ F8.dequantize_rows(q, scale).double().t()
    got = run(A, qp, scale, N, K, rows, splits, dtype)
    got = got.double() if splits == 1 else got.double().sum(0)
    col = want.abs().amax(0)
    sub = 2.0 ** -24 if dtype == torch.float16 else 0.0                # fp16 subnormal spacing at the smallest columns
    assert bool(((got - want).abs() <= TOL[dtype] * col[None, :] + sub).all())
    wrong = A.double() @ F8.dequantize_rows(q, scale.roll(1)).double().t()
    assert ((wrong - want).abs().amax(0) > 50 * (TOL[dtype] * col + sub)).float().mean().item() > 0.8     # (per column: its worst element)


def test_bad_arguments_are_rejected():
    L, st = lib(), current_stream()
    N, K = 256, 512
    q, scale = weights(N, K, 1)
    qp = pack(q)
    A = torch.zeros((64, K), device="cuda", dtype=torch.float16)
    out = torch.zeros((64, N), device="cuda", dtype=torch.float16)
    part = torch.zeros((2, 64, N), device="cuda", dtype=torch.float32)
    ok = lambda **kw: dict(dict(A=A, W=qp, s=scale, rows=16, N=N, K=K, sp=1, part=None, out=out, dt=0), **kw)
    call = lambda a: L.samd_gemm_skinny_f8(_ptr(a["A"]), _ptr(a["W"]), _ptr(a["s"]), a["rows"], a["N"], a["K"], a["sp"], _ptr(a["part"]), _ptr(a["out"]), a["dt"], st)
    assert call(ok()) == 0
    for bad in (dict(rows=24), dict(rows=128), dict(N=192), dict(N=0), dict(K=384), dict(K=0), dict(s=None), dict(A=None), dict(W=None),
                dict(sp=0), dict(sp=3), dict(sp=2, part=None), dict(out=None), dict(dt=2)):
        assert call(ok(**bad)) == -1, bad                             # SAMD_E_INVALID
    assert call(ok(sp=2, part=part, out=None)) == 0
    assert L.samd_gemm_pack_f8(_ptr(q), _ptr(q), N, K, st) == -1
    assert L.samd_gemm_pack_f8(_ptr(q), _ptr(qp), 100, K, st) == -1
    assert L.samd_gemm_pack_f8(_ptr(q), _ptr(qp), N, 300, st) == -1
    assert L.samd_gemm_pack_f8(None, _ptr(qp), N, K, st) == -1
    torch.cuda.synchronize()
