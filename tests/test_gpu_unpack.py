"""samd_gemm_unpack_f8 / _f8b / _f4 / _i4 / _i8: a packed projection back to row-major [N][K] in the model dtype, bit for bit the Python
helper of each format (samd_hip/int4.py, int8.py, mxfp4.py, fp8.py) with one rounding to the dtype where the helper returns fp32.  Every
comparison is torch.equal; every output buffer starts NaN-filled; the weights go through the product's own pack kernels.

  shapes   (128, 256) the minimum; (256, 512) two tiles x two chunks (f8b: 2 x 4 scale blocks); (384, 768) three x three.
  codes    uniform over the format's codes with every code value planted at a random place besides: all 16 nibbles (i4, f4), all 256 bytes
           (i8), the 254 e4m3fn bytes that are numbers (f8, f8b: 0x7f and 0xff are NaN, which no equality can hold; the importers produce
           none).
  side     a DISTINCT scale per group (i4, i8: consecutive bit patterns of the dtype, shuffled), per row (f8) and per block (f8b); zero
           points that differ between neighbouring groups and rows; f4 exponents that differ between neighbouring blocks and rows and span
           the dtype's whole exact range (samd_hip/mxfp4.py EXPONENT_RANGE).  A group, block or row read from the wrong place then shows.
  fp16     the integer formats' scales start inside fp16's subnormals (2^-15), so (q - z) * s is subnormal for small |q - z|: the widening's
           v_pk_mul_f16 must deliver them; f8's smallest products (2^-9 * scale) are subnormal in fp16 as well.
One tie to the streaming kernels per format on the exact-integer inputs of tests/quant_planting.py (16 rows, one split):
samd_gemm_skinny_* == A @ unpack(W).T in fp32 (exact there: every partial sum stays below 2^24 quanta), rounded once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import quant_planting as Q
import test_gpu_fp8_gemm as T8
import test_gpu_fp8b_gemm as T8B
import test_gpu_int4_gemm as TI4
import test_gpu_int8_gemm as TI8
import test_gpu_mxfp4_gemm as TF4
from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import fp8 as F8
from samd_hip import int4 as I4
from samd_hip import int8 as I8
from samd_hip import mxfp4 as MX

E_INVALID = -1
DTYPES = [torch.float16, torch.bfloat16]
SHAPES = [(128, 256), (256, 512), (384, 768)]
FORMATS = ("f8", "f8b", "f4", "i4", "i8")


def _codes(rng, shape, values):
    """uniform over `values`, and every value planted once at a random place"""
    values = np.asarray(values, dtype=np.uint8)
    a = values[rng.integers(0, len(values), shape)]
    flat = a.reshape(-1)
    flat[rng.permutation(flat.size)[:len(values)]] = values
    assert set(np.unique(a).tolist()) == set(values.tolist())
    return a


def _distinct_scales(rng, n, dtype):
    """n distinct positive scales of `dtype`: consecutive bit patterns from 2^-15 up (fp16: subnormal scales first), shuffled"""
    first = 0x0200 if dtype == torch.float16 else 0x3800
    bits = (first + rng.permutation(n)).astype(np.int16)
    s = torch.from_numpy(bits).view(dtype)
    assert s.float().unique().numel() == n and bool((s.float() > 0).all())
    return s


def make(fmt, N, K, dtype):
    """((the packed buffer, then the scales of f8 / f8b), the contract's weights in `dtype`)"""
    rng = np.random.default_rng(1000 * FORMATS.index(fmt) + N + K + (dtype == torch.bfloat16))
    dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda().contiguous()
    if fmt in ("i4", "i8"):
        top = 16 if fmt == "i4" else 256
        codes = _codes(rng, (N, K), range(top))
        g = np.arange(N * (K // 128)).reshape(N, K // 128)
        z = dev(((g * (7 if fmt == "i4" else 37) + 3 + np.arange(N)[:, None]) % top).astype(np.uint8))
        assert bool((z[:, 1:] != z[:, :-1]).all()) and bool((z[1:] != z[:-1]).all())
        s = dev(_distinct_scales(rng, g.size, dtype).reshape(N, K // 128))
        if fmt == "i4":
            q = dev(codes[:, 0::2] | (codes[:, 1::2] << 4))
            want = I4.dequantize_groups(q, z, s)
            packed = (TI4.pack(q, z, s),)
        else:
            q = dev(codes)
            want = I8.dequantize_groups(q, z, s)
            packed = (TI8.pack(q, z, s),)
        if dtype == torch.float16:                               # subnormal products occur, and not only zeros
            w16 = want.to(dtype)
            assert bool(((w16 != 0) & (w16.abs() < torch.finfo(dtype).tiny)).any())
        return packed, want.to(dtype)
    if fmt == "f4":
        codes = _codes(rng, (N, K), range(16))
        lo, hi = MX.exponent_range(dtype)
        e = lo + (11 * np.arange(N)[:, None] + 5 * np.arange(K // 32)[None, :]) % (hi - lo + 1)
        assert bool((e[:, 1:] != e[:, :-1]).all()) and bool((e[1:] != e[:-1]).all()) and e.min() == lo and e.max() == hi
        q, e8 = dev(codes[:, 0::2] | (codes[:, 1::2] << 4)), dev((e + 127).astype(np.uint8))
        MX.check_exponents(e8, dtype)
        want = MX.dequantize_blocks(q, e8)
        assert torch.equal(want.to(dtype).float(), want)         # exact inside the range the runner enforces
        return (TF4.pack(q, e8),), want.to(dtype)
    numbers = [b for b in range(256) if b & 0x7f != 0x7f]
    q = dev(_codes(rng, (N, K), numbers)).view(torch.float8_e4m3fn)
    if fmt == "f8":
        scale = dev((0.001 + 0.0007 * rng.permutation(N)).astype(np.float32))
        assert scale.unique().numel() == N
        return (T8.pack(q), scale), F8.dequantize_rows(q, scale).to(dtype)
    s = dev((0.001 + 0.0013 * rng.permutation((N // 128) * (K // 128))).astype(np.float32).reshape(N // 128, K // 128))
    assert s.unique().numel() == s.numel()
    return (T8.pack(q), s), F8.dequantize_blocks(q, s).to(dtype)


def call(fmt, packed, N, K, out, dtype_code):
    """the raw status of the entry point (no exception)"""
    fn = getattr(lib(), "samd_gemm_unpack_" + fmt)
    side = [_ptr(packed[1])] if fmt in ("f8", "f8b") else []
    return fn(_ptr(packed[0]), *side, N, K, _ptr(out), dtype_code, current_stream())


def unpack(fmt, packed, N, K, dtype):
    out = torch.full((N, K), float("nan"), dtype=dtype, device="cuda")
    rc = call(fmt, packed, N, K, out, torch_dtype_code(dtype))
    check(rc)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_unpack_is_the_python_helper_bit_for_bit(fmt, dtype, N, K):
    packed, want = make(fmt, N, K, dtype)
    before = [p.clone() for p in packed]
    got = unpack(fmt, packed, N, K, dtype)
    assert got.dtype == want.dtype == dtype and bool(torch.isfinite(want.float()).all())
    if not torch.equal(got, want):
        bad = torch.nonzero(~(got == want))
        r, c = bad[0].tolist()
        pytest.fail(f"{fmt} {dtype} ({N}, {K}): {len(bad)} of {got.numel()} weights differ; first at row {r} (tile {r // 128}), k {c} "
                    f"(chunk {c // 256}): got {got[r, c].item()!r}, want {want[r, c].item()!r}")
    assert all(torch.equal(a, b) for a, b in zip(before, packed)), "the packed buffer is read, never written"


@pytest.mark.parametrize("fmt", FORMATS)
def test_bad_arguments_are_invalid_and_launch_nothing(fmt):
    N, K, dtype = 256, 512, torch.float16
    packed, want = make(fmt, N, K, dtype)
    out = torch.full((N, K), float("nan"), dtype=dtype, device="cuda")
    code = torch_dtype_code(dtype)
    fn = getattr(lib(), "samd_gemm_unpack_" + fmt)
    side = [_ptr(packed[1])] if fmt in ("f8", "f8b") else []
    st = current_stream()
    bad = {"null packed buffer": lambda: fn(None, *side, N, K, _ptr(out), code, st),
           "null output": lambda: fn(_ptr(packed[0]), *side, N, K, None, code, st),
           "N % 128": lambda: call(fmt, packed, N - 64, K, out, code),
           "N < 128": lambda: call(fmt, packed, 0, K, out, code),
           "K % 256": lambda: call(fmt, packed, N, K - 128, out, code),
           "K < 256": lambda: call(fmt, packed, N, 0, out, code),
           "d_out == d_packed": lambda: fn(_ptr(packed[0]), *side, N, K, _ptr(packed[0]), code, st),
           "unknown dtype (fp32)": lambda: call(fmt, packed, N, K, out, 2),
           "unknown dtype (7)": lambda: call(fmt, packed, N, K, out, 7)}
    if side:
        bad["null scales"] = lambda: fn(_ptr(packed[0]), None, N, K, _ptr(out), code, st)
    keep = packed[0].clone()
    for what, f in bad.items():
        assert f() == E_INVALID, (fmt, what)
        msg = lib().samd_last_error().decode()
        assert "samd_gemm_unpack_" + fmt + ":" in msg and "N % 128 == 0" in msg, (fmt, what, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and torch.equal(packed[0], keep), "a rejected call must not launch"
    assert call(fmt, packed, N, K, out, code) == 0               # and the same arguments, valid, run
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_streaming_launch_multiplies_by_the_unpacked_weights(fmt, dtype):
    """exact-integer inputs (quant_planting: two chunks, N = 256): the unpacked matrix is the exact W, and the 16-row launch at one split
    stores A @ unpack(W).T -- an exact fp32 sum -- rounded once"""
    chunks, rows = 2, 16
    c = Q.case(fmt, chunks)
    Q.check_case(c)
    K, ck = c.K, c.ckpt
    t = lambda name, dt=None: (torch.from_numpy(ck[name]) if dt is None else torch.from_numpy(ck[name]).to(dt)).cuda().contiguous()
    A = c.A[:rows].to(dtype).cuda().contiguous()
    if fmt == "f8":
        packed = (T8.pack(t("q").view(torch.float8_e4m3fn)), t("scale", torch.float32))
        got = T8.run(A, packed[0], packed[1], Q.N, K, rows, 1, dtype)
    elif fmt == "f8b":
        packed = (T8.pack(t("q").view(torch.float8_e4m3fn)), t("s", torch.float32))
        got = T8B.run(A, packed[0], packed[1], Q.N, K, rows, 1, dtype)
    elif fmt == "f4":
        packed = (TF4.pack(t("q"), t("e8")),)
        got = TF4.run(A, packed[0], Q.N, K, rows, 1, dtype)
    else:
        mod = TI4 if fmt == "i4" else TI8
        packed = (mod.pack(t("q"), t("z"), t("s", dtype)),)
        got = mod.run(A, packed[0], Q.N, K, rows, 1, dtype)
    W = unpack(fmt, packed, Q.N, K, dtype)
    assert torch.equal(W.double().cpu(), c.W), "the unpacked weights are the planted ones"
    # fp32 on the host: every partial sum is an integer number of quanta below 2^24 of them, so the fp32 product is exact in any order
    want = (A.float().cpu() @ W.float().cpu().t()).to(dtype)
    assert torch.equal(want.double(), c.P[:, :rows].sum(0).to(dtype).double())
    assert torch.equal(got.cpu(), want)
