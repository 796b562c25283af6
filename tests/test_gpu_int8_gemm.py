"""GPU parity of the INT8 weight-only projection (samd_gemm_pack_i8 + samd_gemm_skinny_i8):
out[m][n] = sum_k A[m][k] * rne_dtype((q[n][k] - z[n][k/128]) * s[n][k/128]), A and s in the model dtype.  Tolerances are test_gpu_gemm.py's
(fp32 accumulation, one rounding); the planted cases pin the layout, the byte order, the group index of scale and zero point and the
widening element by element, exactly -- including fp16 products that are subnormal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import int8 as I8
from test_gpu_int4_gemm import planted_ks as planted_ks_i4
from test_int8_weights_cpu import packed_i8_np, s_bits_np

TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}          # test_gpu_gemm.py's
DTYPES = [torch.float16, torch.bfloat16]
SHAPES = [(128, 256), (256, 512), (1024, 768), (128, 2816), (4096, 4096)]      # one block; ...; fewer chunks than DEPTH; 11 chunks, ragged against every DEPTH


def pack(q, z, s):
    N, K = q.shape
    out = torch.full((I8.packed_bytes(N, K),), 0x5A, dtype=torch.uint8, device="cuda")
    check(lib().samd_gemm_pack_i8(_ptr(q), _ptr(z), _ptr(s), _ptr(out), N, K, torch_dtype_code(s.dtype), current_stream()))
    return out


def run(A, qp, N, K, rows_pad, splits, dtype):
    """(the dtype output [rows_pad, N] for splits == 1 | the fp32 partials [splits, rows_pad, N]), from NaN-filled buffers"""
    if splits == 1:
        out = torch.full((rows_pad, N), float("nan"), device="cuda", dtype=dtype)
        check(lib().samd_gemm_skinny_i8(_ptr(A), _ptr(qp), rows_pad, N, K, 1, None, _ptr(out), torch_dtype_code(dtype), current_stream()))
    else:
        out = torch.full((splits, rows_pad, N), float("nan"), device="cuda", dtype=torch.float32)
        check(lib().samd_gemm_skinny_i8(_ptr(A), _ptr(qp), rows_pad, N, K, splits, _ptr(out), None, torch_dtype_code(dtype), current_stream()))
    torch.cuda.synchronize()
    return out


def weights(N, K, seed, dtype):
    """random codes and zero points 0..255, random scales in [0.0002, 0.002): neighbouring groups and columns differ in both"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randint(0, 256, (N, K), generator=g, device="cuda", dtype=torch.uint8)
    z = torch.randint(0, 256, (N, K // 128), generator=g, device="cuda", dtype=torch.uint8)
    s = (0.0002 + 0.0018 * torch.rand((N, K // 128), generator=g, device="cuda")).to(dtype)
    return q, z, s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K", [(128, 256), (384, 768), (4096, 11008)])
def test_pack_matches_numpy_layout(dtype, N, K):
    q, z, s = weights(N, K, N + K, dtype)
    got = pack(q, z, s).cpu().numpy()                                  # (every byte of the 0x5A-filled buffer is written)
    assert np.array_equal(got, packed_i8_np(q.cpu().numpy(), z.cpu().numpy(), s_bits_np(s.cpu()), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_pad", [16, 32, 48, 64])
@pytest.mark.parametrize("N,K", SHAPES)
def test_int8_gemm_matches_float64_reference(dtype, rows_pad, N, K):
    q, z, s = weights(N, K, N + K, dtype)
    qp = pack(q, z, s)
    g = torch.Generator(device="cuda").manual_seed(N + K + rows_pad)
    A = torch.randn((rows_pad, K), generator=g, device="cuda").to(dtype)
    want = A.double() @ I8.dequantize_groups(q, z, s).double().t()
    bound = TOL[dtype] * max(1.0, want.abs().max().item())
    chunks = K // 256
    for splits in sorted({1, 2, 3, lib().samd_gemm_splits(N, K, rows_pad), chunks} & set(range(1, chunks + 1))):
        got = run(A, qp, N, K, rows_pad, splits, dtype)
        assert torch.isfinite(got).all(), splits                      # every element (or partial) written
        got = got.double() if splits == 1 else got.double().sum(0)
        err = (got - want).abs().max().item()
        print(f"{dtype} rows {rows_pad} ({N}, {K}) splits {splits}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (splits, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
def planted_ks(K):
    """planted_ks of the INT4 test (chunk ends, 32-k seams, 128-k group seams of the first and last chunk) plus both sides of every 16-k unit
    seam of the first and last chunk"""
    ks = set(planted_ks_i4(K))
    for base in (0, K - 256):
        for s in range(0, 256, 16):
            ks |= {base + s, base + s + 15}
    return sorted(ks)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_pad,N,K", [(16, 256, 512), (32, 384, 2816), (48, 128, 768), (64, 256, 4096), (16, 128, 256), (64, 256, 256)])
def test_one_hot_rows_pick_single_weights(dtype, rows_pad, N, K):
    """A row m = e_{k_m}: out[m][n] must equal W[n][k_m] exactly (one nonzero product of a weight that is a value of the model dtype) -- for
    every split count the partials hold it in one split and exact zeros elsewhere.  The k set is larger than a launch has rows, so it goes
    through in passes.  Planted faults (bytes swapped within a pair, a dword off, the neighbouring group's scale or zero point, the next
    column's scale, no zero point) each miss on more than half the elements."""
    q, z, s = weights(N, K, 7 * N + K, dtype)
    # the condition under which the seam faults are visible, on the inputs: neighbouring groups and columns differ in both s and z
    for t in (s.float(), z.int()):
        assert (t[:, 1:] != t[:, :-1]).float().mean().item() > 0.5
        assert (t[1:] != t[:-1]).float().mean().item() > 0.5
    qp = pack(q, z, s)
    W = I8.dequantize_groups(q, z, s)
    assert torch.equal(W.to(dtype).float(), W)
    codes = q.float()
    rne = lambda x: x.to(dtype).float()
    all_ks = planted_ks(K)
    all_ks += all_ks[:(-len(all_ks)) % rows_pad]
    miss = {}
    for p0 in range(0, len(all_ks), rows_pad):
        ks = all_ks[p0:p0 + rows_pad]
        A = torch.zeros((rows_pad, K), device="cuda", dtype=dtype)
        A[torch.arange(rows_pad), torch.tensor(ks)] = 1
        want = W[:, ks].t().to(dtype)
        for splits in sorted({1, 2, K // 256} & set(range(1, K // 256 + 1))):
            got = run(A, qp, N, K, rows_pad, splits, dtype)
            if splits > 1:
                assert torch.isfinite(got).all()
                chunks = K // 256
                for m, k in enumerate(ks):                              # exact zeros in every split but the one that owns k's chunk
                    own = [sp for sp in range(splits) if sp * chunks // splits <= k // 256 < (sp + 1) * chunks // splits]
                    assert len(own) == 1
                    others = [sp for sp in range(splits) if sp != own[0]]
                    assert not bool(got[others, m].any()), (splits, k)
                got = got.sum(0).to(dtype)
            assert torch.equal(got, want), (splits, ks, (got.float() - want.float()).abs().max().item())
        kg = [k // 128 for k in ks]
        ng = [g ^ 1 for g in kg]
        c, zf, sf = codes[:, ks], z.float(), s.float()
        faults = {
            "k ^ 1 (bytes swapped within a pair)": W[:, [k ^ 1 for k in ks]].t(),
            "k ^ 4 (dword off)": W[:, [k ^ 4 for k in ks]].t(),
            "the neighbouring group's scale": rne((c - zf[:, kg]) * sf[:, ng]).t(),
            "the neighbouring group's zero": rne((c - zf[:, ng]) * sf[:, kg]).t(),
            "column + 1 scale": rne((c - zf[:, kg]) * sf.roll(1, dims=0)[:, kg]).t(),
            "no zero point": rne(c * sf[:, kg]).t(),
        }
        for name, f in faults.items():
            miss.setdefault(name, []).append((f.float() != want.float()).float().mean().item())
    for name, m in miss.items():
        print(f"fault {name}: misses {np.mean(m):.3f} of the elements")
        assert np.mean(m) > 0.5, (name, np.mean(m))


def scale_spread(dtype, count):
    """`count` scales across the dtype's admitted range, as bit patterns: for every exponent a power of two and odd mantissas (one ulp,
    alternating bits, all ones); fp16 from its smallest subnormal (bits 0x0001) up -- so that products (q - z) * s are subnormal, straddle
    the normal boundary, and need rounding -- bf16 from its smallest normal, both to the largest s with 255 * s finite (fp16: 256.75, bits
    0x5C03).  Evenly thinned, so both ends of the range stay."""
    if dtype == torch.float16:
        bits = [(e << 10) | m for e in range(0, 24) for m in (0x000, 0x001, 0x0AA, 0x155, 0x1FF, 0x200, 0x2AB, 0x333, 0x3AB, 0x3FE, 0x3FF)]
        bits += list(range(0x5C00, 0x5C10))                          # (every value around the upper end)
    else:
        bits = [(e << 7) | m for e in range(1, 248) for m in (0x00, 0x01, 0x2B, 0x55, 0x7F)] + list(range(246 << 7, 249 << 7))
    s = torch.tensor(sorted(set(bits)), dtype=torch.int16).view(dtype)
    s = s[(s.float() > 0) & (255.0 * s.float() <= torch.finfo(dtype).max)]
    assert s.numel() >= count // 4
    if dtype == torch.float16:
        assert s[0].view(torch.int16).item() == 0x0001 and s[-1].item() == 256.75
    nxt = (s[-1:].view(torch.int16) + 1).view(dtype)                 # the next value up no longer holds 255 * s
    assert 255.0 * nxt.float().item() > torch.finfo(dtype).max
    if s.numel() > count:
        return s[torch.linspace(0, s.numel() - 1, count).round().long()]
    return s.repeat((count + s.numel() - 1) // s.numel())[:count]


def one_hot_equals_contract(q, z, s, dtype, label):
    """every weight, fetched by one-hot rows over ALL k, equals dequantize_groups: no tolerance"""
    N, K = q.shape
    rows = 64
    W = I8.dequantize_groups(q, z, s)
    qp = pack(q, z, s)
    bad = 0
    for p0 in range(0, K, rows):
        ks = list(range(p0, p0 + rows))
        A = torch.zeros((rows, K), device="cuda", dtype=dtype)
        A[torch.arange(rows), torch.tensor(ks)] = 1
        got = run(A, qp, N, K, rows, 1, dtype).float().t()              # [N, rows]
        wrong = got != W[:, ks]
        if bool(wrong.any()) and bad == 0:
            n_, i_ = [int(x[0]) for x in torch.nonzero(wrong, as_tuple=True)]
            print(f"{label} {dtype}: k {ks[i_]} column {n_}: got {got[n_, i_].item()!r}, want {W[n_, ks[i_]].item()!r}, q {int(q[n_, ks[i_]])} "
                  f"z {int(z[n_, ks[i_] // 128])} s {s[n_, ks[i_] // 128].item()!r}")
        bad += int(wrong.sum())
    assert bad == 0, (label, bad)
    return W


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_code_zero_pair_and_every_difference_at_every_scale(dtype):
    """Two N = 512, K = 1024 matrices, one-hot rows over ALL k, every weight equal to dequantize_groups with no tolerance.
    First: column c has zero point c % 256 and code (k + c // 16) % 256 at k, so every (q, z) pair of 0..255 x 0..255 occurs four times in
    column c and four times in column c + 256; occurrence (c // 256, k // 256) has scale number 4 (c // 256) + k // 256 of an 8-scale spread.
    Second: group number gid = 8 c + g has scale number gid % 256 of a 256-scale spread; the 16 groups of one scale lie in columns c % 32
    fixed, i = c // 32 = 0..15, whose zero point is ZL[i // 2] and whose codes are the half 128 (i % 2) + (k + c) % 128: with ZL starting
    0, 255 every difference -255..255 meets every scale.  Both coverages are asserted on the inputs."""
    N, K = 512, 1024
    G = K // 128
    c = torch.arange(N, device="cuda")[:, None]
    k = torch.arange(K, device="cuda")[None, :]
    g = torch.arange(G, device="cuda")[None, :]
    # --- every (q, z) pair, each at 8 scales
    q = ((k + c // 16) % 256).to(torch.uint8).contiguous()
    z = (c % 256).to(torch.uint8).expand(N, G).contiguous()
    spread8 = scale_spread(dtype, 8).cuda()
    sidx = 4 * (c // 256) + g // 2                                            # (k // 256 == g // 2)
    s = spread8[sidx.reshape(-1)].reshape(N, G).contiguous()
    I8.check_groups(q, z, s, dtype, "pairs")
    seen = torch.zeros((256, 256, 8), dtype=torch.bool, device="cuda")
    seen[q.long(), z.long().repeat_interleave(128, 1), sidx.repeat_interleave(128, 1).expand(N, K)] = True
    assert bool(seen.all()), "every (q, z) pair at each of the 8 scales"
    one_hot_equals_contract(q, z, s, dtype, "pairs")
    # --- every difference at every one of 256 scales
    ZL = torch.tensor([0, 255, 1, 254, 127, 128, 85, 200], device="cuda")
    i = c // 32
    q2 = (128 * (i % 2) + (k + c) % 128).to(torch.uint8).contiguous()
    z2 = ZL[(i // 2).reshape(-1)].reshape(N, 1).to(torch.uint8).expand(N, G).contiguous()
    spread = scale_spread(dtype, 256).cuda()
    sidx2 = (8 * c + g) % 256
    s2 = spread[sidx2.reshape(-1)].reshape(N, G).contiguous()
    I8.check_groups(q2, z2, s2, dtype, "differences")
    seen2 = torch.zeros((511, 256), dtype=torch.bool, device="cuda")
    seen2[(q2.long() - z2.long().repeat_interleave(128, 1)) + 255, sidx2.repeat_interleave(128, 1)] = True
    assert bool(seen2.all()), "every difference -255..255 at each of the 256 scales"
    W2 = one_hot_equals_contract(q2, z2, s2, dtype, "differences")
    if dtype == torch.float16:
        sub = (W2 != 0) & (W2.abs() < 2.0 ** -14)
        assert int(sub.sum()) >= 1000, "the spread must produce subnormal fp16 products"
    exact = (q2.double() - z2.double().repeat_interleave(128, 1)) * s2.double().repeat_interleave(128, 1)
    assert bool((W2.double() != exact).any()), "some products must need the rounding"
    # a dense row: the fp32 sum over K of the rounded weights (a mid-range scale so that the sum is well inside fp32)
    s1 = torch.full_like(s, 0.00123)
    A1 = torch.ones((16, K), device="cuda", dtype=dtype)
    got = run(A1, pack(q, z, s1), N, K, 16, 4, dtype).sum(0)
    assert torch.allclose(got.double(), I8.dequantize_groups(q, z, s1).double().sum(1)[None, :].expand(16, N), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_pad,N,K", [(16, 256, 512), (32, 128, 2816), (48, 384, 768), (64, 512, 4096)])
def test_exact_integers(dtype, rows_pad, N, K):
    """power-of-two scales (2^-3 .. 2^0 per group) and integer A in [-4, 4]: every weight is a multiple of 1/8 that the dtype holds (|q - z|
    <= 255: 8 significant bits), every product and every partial sum a multiple of 1/8 below 2^24 / 8 (asserted on the reference), so fp32
    accumulation in any order is exact -- every split's partial must equal an int64 reference over its own chunks bit for bit, the one-split
    output its single rounding to the dtype"""
    g = torch.Generator(device="cuda").manual_seed(3 * N + K + rows_pad)
    q = torch.randint(0, 256, (N, K), generator=g, device="cuda", dtype=torch.uint8)
    z = torch.randint(0, 256, (N, K // 128), generator=g, device="cuda", dtype=torch.uint8)
    e = torch.randint(0, 4, (N, K // 128), generator=g, device="cuda")
    s = torch.exp2(e.float() - 3).to(dtype)
    A = torch.randint(-4, 5, (rows_pad, K), generator=g, device="cuda").to(dtype)
    w8 = (q.long() - z.long().repeat_interleave(128, 1)) * (2 ** e.long()).repeat_interleave(128, 1)      # 8 W, integers
    assert torch.equal(I8.dequantize_groups(q, z, s).double() * 8, w8.double())
    a8, w8c = A.long().cpu(), w8.cpu()
    ref8 = a8 @ w8c.t()                                                      # [rows, N] int64
    assert int((a8.abs() @ w8c.abs().t()).max()) < 2 ** 24                   # |ref| and every partial sum in any order: exact in fp32
    qp = pack(q, z, s)
    chunks = K // 256
    for splits in sorted({1, 2, lib().samd_gemm_splits(N, K, rows_pad), chunks} & set(range(1, chunks + 1))):
        got = run(A, qp, N, K, rows_pad, splits, dtype)
        if splits == 1:
            assert torch.equal(got.cpu(), (ref8.double() / 8).to(dtype)), splits
        else:
            assert torch.equal(got.double().sum(0).cpu(), ref8.double() / 8), splits      # (the fp64 sum of exact fp32 partials is exact)
            for sp in range(splits):                                         # each split's partial is the exact sum over its own chunks
                c0, c1 = sp * chunks // splits, (sp + 1) * chunks // splits
                part8 = a8[:, 256 * c0:256 * c1] @ w8c[:, 256 * c0:256 * c1].t()
                assert torch.equal(got[sp].double().cpu(), part8.double() / 8), (splits, sp)


def test_bad_arguments_are_rejected():
    L, st = lib(), current_stream()
    N, K = 256, 512
    q, z, s = weights(N, K, 1, torch.float16)
    qp = pack(q, z, s)
    A = torch.zeros((64, K), device="cuda", dtype=torch.float16)
    out = torch.zeros((64, N), device="cuda", dtype=torch.float16)
    part = torch.zeros((2, 64, N), device="cuda", dtype=torch.float32)
    ok = lambda **kw: dict(dict(A=A, W=qp, rows=16, N=N, K=K, sp=1, part=None, out=out, dt=0), **kw)
    call = lambda a: L.samd_gemm_skinny_i8(_ptr(a["A"]), _ptr(a["W"]), a["rows"], a["N"], a["K"], a["sp"], _ptr(a["part"]), _ptr(a["out"]), a["dt"], st)
    assert call(ok()) == 0
    for bad in (dict(rows=24), dict(rows=128), dict(N=192), dict(N=0), dict(K=384), dict(K=0), dict(A=None), dict(W=None),
                dict(sp=0), dict(sp=3), dict(sp=2, part=None), dict(out=None), dict(dt=2)):
        assert call(ok(**bad)) == -1, bad                             # SAMD_E_INVALID
    assert call(ok(sp=2, part=part, out=None)) == 0
    pk = lambda q_, z_, s_, o_, n_=N, k_=K, dt_=0: L.samd_gemm_pack_i8(_ptr(q_), _ptr(z_), _ptr(s_), _ptr(o_), n_, k_, dt_, st)
    assert pk(q, z, s, qp) == 0
    assert pk(q, z, s, q) == -1 and pk(q, z, s, z) == -1 and pk(q, z, s, s) == -1
    assert pk(q, z, s, qp, n_=100) == -1 and pk(q, z, s, qp, k_=300) == -1 and pk(q, z, s, qp, dt_=2) == -1
    assert pk(None, z, s, qp) == -1 and pk(q, None, s, qp) == -1 and pk(q, z, None, qp) == -1 and pk(q, z, s, None) == -1
    torch.cuda.synchronize()
