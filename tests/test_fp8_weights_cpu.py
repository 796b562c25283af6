"""FP8 (OCP e4m3fn) weight-only decoding, host side: the per-row quantiser of samd_hip/fp8.py against a numpy restatement of e4m3fn
round-to-nearest-even, the checkpoint importer on hand-built modules, and the packed layout of samd_gemm_pack_f8 restated in numpy."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from samd_hip import SamdError
from samd_hip import fp8 as F8


def e4m3_rne(x):
    """float64 -> the nearest e4m3fn value (ties to even), saturated at +-448: 3 mantissa bits, exponents -6..8, subnormal step 2^-9"""
    x = np.clip(np.asarray(x, dtype=np.float64), -448.0, 448.0)
    a = np.abs(x)
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    step = np.exp2(np.maximum(e, -6.0) - 3.0)
    return np.sign(x) * np.rint(a / step) * step          # np.rint rounds half to even; a carry into the next binade stays exact


def q_values(q):
    return q.float().numpy().astype(np.float64)


def test_quantiser_per_row_scales_and_saturation():
    g = torch.Generator().manual_seed(0)
    W = torch.randn((6, 512), generator=g) * torch.tensor([1e-3, 0.02, 1.0, 30.0, 5e3, 0.5])[:, None]
    W[2, 17] = -9.0                                        # a row whose absmax is negative
    q, scale = F8.quantize_rows(W)
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and scale.shape == (6,)
    absmax = W.abs().amax(1)
    assert torch.equal(scale, absmax / 448.0)
    qv = q_values(q)
    assert np.abs(qv).max() <= 448.0
    for r in range(6):                                     # the absmax element maps to the largest finite code, with its sign
        i = int(W[r].abs().argmax())
        assert qv[r, i] == 448.0 * np.sign(W[r, i].item())
    # per-element: exactly the RNE of W / scale (computed in fp32, as the quantiser does)
    want = e4m3_rne((W.float() / scale[:, None]).numpy())
    assert np.array_equal(qv, want)


def test_quantiser_zero_rows_and_subnormals():
    W = torch.zeros((3, 256))
    W[1, :8] = torch.tensor([448.0, 2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 2.0 ** -7 + 2.0 ** -10, -2.0 ** -9])
    W[2, :3] = torch.tensor([-448.0, 7 * 2.0 ** -9, 2.0 ** -6])
    q, scale = F8.quantize_rows(W)
    assert scale[0].item() == 1.0 and not q_values(q)[0].any()       # a zero row: scale 1, all codes zero
    assert scale[1].item() == 1.0 and scale[2].item() == 1.0
    qv = q_values(q)
    # 2^-9 and 3 x 2^-9 are subnormal codes; 2^-10 ties between 0 and 2^-9 -> 0 (even); 1.5 x 2^-9 -> 2 x 2^-9; 2.5 x 2^-9 -> 2 x 2^-9
    assert qv[1, :8].tolist() == [448.0, 2.0 ** -9, 3 * 2.0 ** -9, 0.0, 2 * 2.0 ** -9, 2 * 2.0 ** -9, 2.0 ** -7, -2.0 ** -9]
    assert qv[2, :3].tolist() == [-448.0, 7 * 2.0 ** -9, 2.0 ** -6]
    assert np.array_equal(qv, e4m3_rne(W.numpy()))


def test_quantiser_rounds_to_nearest_even_like_torch_and_numpy():
    """every tie between two neighbouring codes of one binade, and random values: the quantiser's bytes equal both torch's cast of W / scale
    and the numpy RNE restatement"""
    codes = torch.arange(0, 126, dtype=torch.uint8).view(torch.float8_e4m3fn).float()      # 0 .. 448, finite positive codes
    mids = (codes[:-1] + codes[1:]) / 2
    W = torch.zeros((2, 256))
    W[0, :125] = mids
    W[0, 125] = 448.0
    W[1, :125] = -mids
    W[1, 125] = -448.0
    q, scale = F8.quantize_rows(W)
    assert torch.equal(scale, torch.ones(2))
    assert np.array_equal(q_values(q), e4m3_rne(W.numpy()))
    lo, hi = codes[:-1].numpy(), codes[1:].numpy()
    bits = torch.arange(0, 126, dtype=torch.uint8).numpy()
    even_is_lo = (bits[:-1] % 2 == 0)
    assert np.array_equal(q_values(q)[0, :125], np.where(even_is_lo, lo, hi))
    g = torch.Generator().manual_seed(1)
    R = torch.randn((64, 1024), generator=g) * torch.logspace(-4, 3, 64)[:, None]
    q, scale = F8.quantize_rows(R)
    assert torch.equal(q.view(torch.uint8), (R / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    assert np.array_equal(q_values(q), e4m3_rne((R / scale[:, None]).numpy()))


def test_quantiser_error_bound_for_normal_values():
    """|W - float(q) * scale| <= 2^-4 x the row's absmax wherever q is a normal e4m3 value (3 mantissa bits: half a step is 2^-4 of the value)"""
    g = torch.Generator().manual_seed(2)
    W = torch.randn((128, 2048), generator=g) * 0.02
    W[5] *= 1e4
    q, scale = F8.quantize_rows(W)
    deq = F8.dequantize_rows(q, scale)
    normal = q.float().abs() >= 2.0 ** -6
    err = (deq - W).abs()
    bound = W.abs().amax(1, keepdim=True) * 2.0 ** -4
    assert bool((err <= bound)[normal].all())
    assert bool((err <= (W.abs() * 2.0 ** -4 + 1e-30))[normal].all())       # (and relative to the element itself)


def test_fusing_before_or_after_quantising_gives_the_same_bytes():
    g = torch.Generator().manual_seed(3)
    parts = [torch.randn((n, 512), generator=g) * s for n, s in ((256, 0.02), (128, 0.5), (128, 3.0))]
    q_all, s_all = F8.quantize_rows(torch.cat(parts, 0).to(torch.float16))
    q_cat, s_cat = F8.fuse_fp8([F8.quantize_rows(p.to(torch.float16)) for p in parts], "cpu")
    assert torch.equal(q_all.view(torch.uint8), q_cat.view(torch.uint8)) and torch.equal(s_all, s_cat)


# ---------------------------------------------------------------------------------------------------------------------
def fp8_linear(N=256, K=512, scale_shape="row", seed=0, dtype=torch.float8_e4m3fn):
    lin = torch.nn.Linear(K, N, bias=False)
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((N, K), generator=g) * 0.05
    q, s = F8.quantize_rows(w)
    lin.weight = torch.nn.Parameter(q.float().to(dtype) if dtype != torch.float8_e4m3fn else q, requires_grad=False)
    if scale_shape == "tensor":
        lin.register_buffer("weight_scale", torch.tensor(0.25))
    elif scale_shape == "tensor1":
        lin.register_buffer("weight_scale", torch.tensor([0.25]))
    elif scale_shape == "row":
        lin.register_buffer("weight_scale", s.clone())
    elif scale_shape == "row1":
        lin.register_buffer("weight_scale", s.clone()[:, None])
    elif scale_shape == "block":
        lin.register_buffer("weight_scale_inv", torch.ones((N // 128, K // 128)))
    return lin, q, s


@pytest.mark.parametrize("kind", ["tensor", "tensor1", "row", "row1"])
def test_importer_expands_scales(kind):
    lin, q, s = fp8_linear(scale_shape=kind)
    got_q, got_s = F8.linear_fp8(lin)
    assert torch.equal(got_q.view(torch.uint8), q.view(torch.uint8))
    assert got_s.shape == (256,) and got_s.dtype == torch.float32
    want = torch.full((256,), 0.25) if kind.startswith("tensor") else s
    assert torch.equal(got_s, want)


def test_importer_leaves_plain_linears_alone():
    assert F8.linear_fp8(torch.nn.Linear(512, 256, bias=False)) is None
    assert F8.linear_fp8(torch.nn.Linear(512, 256, bias=False).half()) is None


@pytest.mark.parametrize("dtype,word", [(torch.float8_e4m3fnuz, "float8_e4m3fnuz"), (torch.float8_e5m2, "float8_e5m2")])
def test_importer_rejects_other_fp8_encodings(dtype, word):
    lin, _, _ = fp8_linear(dtype=dtype)
    with pytest.raises(SamdError, match=word):
        F8.linear_fp8(lin, "layers.0.self_attn.q_proj")


def test_importer_rejects_block_scales_and_bad_shapes():
    lin, _, _ = fp8_linear(scale_shape="block")
    with pytest.raises(SamdError, match="block"):
        F8.linear_fp8(lin)
    lin, _, _ = fp8_linear(scale_shape=None)
    with pytest.raises(SamdError, match="without a weight_scale"):
        F8.linear_fp8(lin)
    lin, _, _ = fp8_linear(scale_shape="row")
    lin.weight_scale = torch.ones((2, 4))                              # [N/128, K/128] under the per-row name
    with pytest.raises(SamdError, match="weight_scale of shape"):
        F8.linear_fp8(lin)


def test_importer_rejects_a_mix_of_formats():
    f8, _, _ = fp8_linear()
    plain = torch.nn.Linear(512, 256, bias=False)
    assert F8.checkpoint_is_fp8([("a", f8), ("b", fp8_linear(seed=1)[0])]) is True
    assert F8.checkpoint_is_fp8([("a", plain), ("b", torch.nn.Linear(512, 256, bias=False))]) is False
    with pytest.raises(SamdError, match="mix of FP8 and non-FP8"):
        F8.checkpoint_is_fp8([("layers.0.q_proj", f8), ("layers.0.k_proj", plain)])


# ---------------------------------------------------------------------------------------------------------------------
def packed_f8_np(Wb):
    """numpy restatement of samd_gemm_pack_f8: [N][K] bytes -> packed bytes.  Block (tile t, chunk c) = 32 KiB at (t * K/256 + c);
    inside it the 16-byte unit b * 512 + tid, tid = 64 w + 16 g + n, holds row 128 t + 16 w + n, columns 256 c + 64 b + 16 g .. +15."""
    N, K = Wb.shape
    T, Cc = N // 128, K // 256
    x = Wb.reshape(T, 8, 16, Cc, 4, 4, 16)                 # [t][w][n][c][b][g][16 bytes]
    x = x.transpose(0, 3, 4, 1, 5, 2, 6)                   # [t][c][b][w][g][n][16]
    return np.ascontiguousarray(x).reshape(-1)


@pytest.mark.parametrize("N,K", [(128, 256), (384, 768), (256, 2816)])
def test_packed_layout_is_a_permutation(N, K):
    idx = np.arange(N * K, dtype=np.int64).reshape(N, K)
    # byte -> its packed position, via a matrix of distinct int64 "bytes"
    T, Cc = N // 128, K // 256
    p = np.ascontiguousarray(idx.reshape(T, 8, 16, Cc, 4, 4, 16).transpose(0, 3, 4, 1, 5, 2, 6)).reshape(-1)
    assert np.array_equal(np.sort(p), np.arange(N * K))
    # unit by unit: the formula of the kernel's header comment
    u = np.arange(N * K // 16)
    blk, inner = u // 2048, u % 2048
    b, tid = inner // 512, inner % 512
    w, g, n = tid // 64, (tid // 16) % 4, tid % 16
    t, c = blk // Cc, blk % Cc
    row, col = 128 * t + 16 * w + n, 256 * c + 64 * b + 16 * g
    assert np.array_equal(p.reshape(-1, 16), (row * K + col)[:, None] + np.arange(16)[None, :])
    Wb = np.random.default_rng(0).integers(0, 256, (N, K), dtype=np.uint8)
    assert np.array_equal(np.sort(packed_f8_np(Wb)), np.sort(Wb.reshape(-1)))
