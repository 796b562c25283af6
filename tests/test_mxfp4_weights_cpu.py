"""MXFP4 (e2m1 elements + e8m0 block scales) weight-only decoding, host side: the block quantiser of samd_hip/mxfp4.py against the rules it
documents, the exactness of every code x exponent in the model dtypes, the checkpoint importer on hand-built modules, and the packed layout
of samd_gemm_pack_f4 restated in numpy."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from samd_hip import SamdError
from samd_hip import mxfp4 as MX

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
F4 = torch.float4_e2m1fn_x2
E8 = torch.float8_e8m0fnu


def rows(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, K), generator=g) * 0.02 * (1 + 8 * torch.rand((N, 1), generator=g))


def block_of(values, e=0):
    """one [1, 32] row: `values` then zeros, with a 4 * 2^e element last so that the block's exponent is e"""
    v = list(values) + [0.0] * (31 - len(values)) + [4.0]
    return torch.tensor([v], dtype=torch.float32) * 2.0 ** e


def nibbles(q):
    q = q.to(torch.int32)
    return torch.stack([q & 15, q >> 4], dim=2).reshape(q.shape[0], -1)


def test_sixteen_codes_dequantise_to_the_grid_low_nibble_first():
    codes = torch.arange(16, dtype=torch.uint8)
    q = (codes[0::2] | (codes[1::2] << 4)).repeat(4)[None, :]            # [1, 32] bytes = 64 elements: code k % 16 at k
    e8 = torch.full((1, 2), 127, dtype=torch.uint8)
    W = MX.dequantize_blocks(q, e8)
    want = torch.tensor(GRID + [-g for g in GRID]).repeat(4)[None, :]
    assert torch.equal(W, want)
    assert str(W[0, 8].item()) == "-0.0"                                  # code 8 is -0
    # one byte 0x72: the low nibble (2 -> 1.0) is the even k, the high nibble (7 -> 6.0) the odd one
    q1 = torch.zeros((1, 16), dtype=torch.uint8)
    q1[0, 3] = 0x72
    W1 = MX.dequantize_blocks(q1, torch.tensor([[128]], dtype=torch.uint8))
    assert W1[0, 6].item() == 2.0 and W1[0, 7].item() == 12.0 and W1.abs().sum().item() == 14.0
    # the float4_e2m1fn_x2 view of the same bytes is accepted
    assert torch.equal(MX.dequantize_blocks(q.view(F4), e8.view(E8)), W)


def test_exponent_rule():
    for e in (-8, -3, 0, 5):
        for top in (4.0, 5.0, 7.99, 4.0001):
            W = torch.zeros((1, 32))
            W[0, 5] = -top * 2.0 ** e
            q, e8 = MX.quantize_blocks(W)
            assert e8.item() == e + 127, (e, top)
    # floor(log2(absmax)) - 2 on random rows, against numpy
    W = rows(64, 256, 3)
    q, e8 = MX.quantize_blocks(W)
    absmax = W.view(64, 8, 32).abs().amax(2).double().numpy()
    assert np.array_equal(e8.numpy().astype(np.int64) - 127, np.floor(np.log2(absmax)).astype(np.int64) - 2)
    ex = e8.int() - 127
    assert -8 <= ex.min().item() and ex.max().item() <= -3                # the range the module's docstring quotes for such rows
    rel = ((MX.dequantize_blocks(q, e8) - W).pow(2).sum() / W.pow(2).sum()).sqrt().item()
    assert 0.08 < rel < 0.15, rel                                         # about 11.5 % relative RMS


def test_tie_rounding_saturation_zero_blocks_and_minus_zero():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    q, e8 = MX.quantize_blocks(block_of(ties + [-t for t in ties]))
    got = MX.dequantize_blocks(q, e8)[0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert got[:7].tolist() == want and got[7:14].tolist() == [-w for w in want]
    assert nibbles(q)[0, 7].item() == 0                                   # -0.25 rounds to 0 and becomes +0, not code 8
    # just off the ties: nearest wins
    q, e8 = MX.quantize_blocks(block_of([0.2501, 0.7499, 2.4999, 2.5001, 4.9999, 5.0001]))
    assert MX.dequantize_blocks(q, e8)[0, :6].tolist() == [0.5, 0.5, 2.0, 3.0, 4.0, 6.0]
    # saturation: a clamped exponent leaves elements beyond +-6, which saturate
    W = torch.tensor([[100000.0, -100000.0] + [0.0] * 30])
    q, e8 = MX.quantize_blocks(W, torch.float16)
    assert e8.item() == 13 + 127 and MX.dequantize_blocks(q, e8)[0, :2].tolist() == [6.0 * 2 ** 13, -6.0 * 2 ** 13]
    # 7.99 with exponent 0 rounds (saturates) to 6
    q, e8 = MX.quantize_blocks(torch.tensor([[7.99, -7.99] + [0.0] * 30]))
    assert e8.item() == 127 and MX.dequantize_blocks(q, e8)[0, :2].tolist() == [6.0, -6.0]
    # zero blocks: exponent 0, all codes +0 (from -0.0 inputs too)
    W = torch.zeros((2, 64))
    W[1, :32] = -0.0
    q, e8 = MX.quantize_blocks(W)
    assert bool((q == 0).all()) and bool((e8 == 127).all())
    # a block that underflows the clamped range entirely is a zero block
    q, e8 = MX.quantize_blocks(torch.full((1, 32), 2.0 ** -30), torch.float16)
    assert bool((q == 0).all()) and e8.item() == 127


@pytest.mark.parametrize("dtype", [None, torch.float16, torch.bfloat16])
def test_quantiser_is_idempotent_on_its_own_output(dtype):
    W = rows(128, 512, 5)
    W[3] *= 2.0 ** -14                                                   # rows that meet fp16's lower clamp
    W[4] *= 2.0 ** -19
    W[5] *= 2.0 ** 20
    q, e8 = MX.quantize_blocks(W, dtype)
    q2, e2 = MX.quantize_blocks(MX.dequantize_blocks(q, e8), dtype)
    assert torch.equal(q, q2) and torch.equal(e8, e2)


def test_dequantise_agrees_with_torch_e8m0_and_fp4_views():
    e8 = torch.arange(0, 255, dtype=torch.uint8)[None, :]                # every numeric code
    q = torch.full((1, 255 * 16), 0x22, dtype=torch.uint8)               # every element 1.0
    W = MX.dequantize_blocks(q, e8)
    assert torch.equal(W[0, ::32], e8.view(E8).float()[0])
    assert torch.equal(W[0, ::32], torch.exp2(e8[0].double() - 127).float())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_every_code_times_every_exponent_is_exact_in_the_model_dtype(dtype):
    lo, hi = MX.exponent_range(dtype)
    assert (lo, hi) == ((MX.FP16_EMIN, 13) if dtype == torch.float16 else (-125, 125))
    assert MX.FP16_EMIN in (-23, -13)
    ex = torch.arange(lo, hi + 1)
    e8 = (ex + 127).to(torch.uint8)[:, None]                             # one block per row
    codes = torch.arange(16, dtype=torch.uint8)
    q = (codes[0::2] | (codes[1::2] << 4)).repeat(2)[None, :].expand(len(ex), 16).contiguous()
    W = MX.dequantize_blocks(q, e8)
    assert torch.equal(W.to(dtype).double(), W.double()) and bool(torch.isfinite(W.to(dtype)).all())
    want = torch.tensor(GRID + [-g for g in GRID], dtype=torch.float64).repeat(2)[None, :] * torch.exp2(ex.double())[:, None]
    assert torch.equal(W.double(), want)
    if dtype == torch.float16:                                           # one step past either end is not exact: the range is tight
        for e, val in ((-24, 0.5), (14, 6.0)):
            x = torch.tensor(val * 2.0 ** e, dtype=torch.float64)
            assert x.to(dtype).double().item() != x.item()
        assert float(torch.tensor(0.5 * 2.0 ** -13).half()) == 0.5 * 2.0 ** -13 and 0.5 * 2.0 ** -13 >= 2.0 ** -14     # -13: still normal
    # the quantiser clamps at both ends
    W = torch.zeros((2, 32))
    W[0, 0], W[1, 0] = 4.0 * 2.0 ** (lo - 6), (3.0e38 if dtype == torch.bfloat16 else 4.0 * 2.0 ** (hi + 4))
    q, e8 = MX.quantize_blocks(W, dtype)
    assert e8[1, 0].item() - 127 == hi
    W[0, 0] = 4.0 * 2.0 ** (lo - 1)                                       # 2 * 2^lo after the clamp
    q, e8 = MX.quantize_blocks(W, dtype)
    assert e8[0, 0].item() - 127 == lo and MX.dequantize_blocks(q, e8)[0, 0].item() == 2.0 * 2.0 ** lo
    with pytest.raises(SamdError):
        MX.exponent_range(torch.float32)


def test_fuse_before_quantising_equals_fuse_after():
    parts = [rows(n, 256, seed=n) for n in (128, 64, 64)]
    q_all, e_all = MX.quantize_blocks(torch.cat(parts, dim=0))
    q_cat, e_cat = MX.fuse_mxfp4([MX.quantize_blocks(p) for p in parts], "cpu")
    assert torch.equal(q_all, q_cat) and torch.equal(e_all, e_cat)
    assert q_cat.dtype == torch.uint8 and e_cat.dtype == torch.uint8 and q_cat.is_contiguous()


def mx_linear(N=256, K=512, form="fp4", seed=0, scale_shape=None, scale_dtype=None):
    """an nn.Linear as an MXFP4 checkpoint holds it: form "fp4" = float4_e2m1fn_x2 weight + float8_e8m0fnu scale, "u8" = uint8 + uint8"""
    q, e8 = MX.quantize_blocks(rows(N, K, seed))
    lin = torch.nn.Linear(K, N, bias=False)
    lin.weight = torch.nn.Parameter(q.view(F4) if form == "fp4" else q, requires_grad=False)
    s = e8.view(E8) if form == "fp4" else e8
    if scale_dtype == "e8m0":
        s = e8.view(E8)
    elif scale_dtype == "u8":
        s = e8
    elif scale_dtype is not None:
        s = torch.ones(e8.shape, dtype=scale_dtype)
    if scale_shape is not None:
        s = torch.full(scale_shape, 127, dtype=torch.uint8)
        s = s.view(E8) if form == "fp4" else s
    lin.register_buffer("weight_scale", s)
    return lin, q, e8


@pytest.mark.parametrize("form,scale_dtype", [("fp4", None), ("fp4", "u8"), ("u8", None), ("u8", "e8m0")])
def test_importer_takes_both_forms(form, scale_dtype):
    lin, q, e8 = mx_linear(form=form, scale_dtype=scale_dtype)
    got_q, got_e = MX.linear_mxfp4(lin)
    assert got_q.dtype == torch.uint8 and got_e.dtype == torch.uint8
    assert torch.equal(got_q, q) and torch.equal(got_e, e8)


def test_importer_ignores_other_linears():
    assert MX.linear_mxfp4(torch.nn.Linear(512, 256, bias=False)) is None
    assert MX.linear_mxfp4(torch.nn.Linear(512, 256, bias=False).half()) is None
    lin = torch.nn.Linear(512, 256, bias=False)
    lin.weight = torch.nn.Parameter(torch.zeros((256, 512), dtype=torch.float8_e4m3fn), requires_grad=False)
    assert MX.linear_mxfp4(lin) is None


def test_quantiser_refuses_k_not_a_multiple_of_32():
    with pytest.raises(SamdError, match="32"):
        MX.quantize_blocks(torch.zeros((4, 48)))


@pytest.mark.parametrize("form", ["fp4", "u8"])
def test_importer_rejects_what_the_runner_cannot_run(form):
    name = "layers.0.self_attn.q_proj"
    # K % 32 != 0
    lin = torch.nn.Linear(48, 128, bias=False)
    w = torch.zeros((128, 24), dtype=torch.uint8)
    lin.weight = torch.nn.Parameter(w.view(F4) if form == "fp4" else w, requires_grad=False)
    lin.register_buffer("weight_scale", torch.full((128, 1), 127, dtype=torch.uint8))
    with pytest.raises(SamdError, match="multiple of the MX block"):
        MX.linear_mxfp4(lin, name)
    # a block size of 16
    lin, _, _ = mx_linear(form=form, scale_shape=(256, 32))
    with pytest.raises(SamdError, match="one scale per 32"):
        MX.linear_mxfp4(lin, name)
    # per-row scales
    lin, _, _ = mx_linear(form=form, scale_shape=(256, 1))
    with pytest.raises(SamdError, match="weight_scale of shape"):
        MX.linear_mxfp4(lin, name)
    # a scale that is not e8m0
    lin, _, _ = mx_linear(form=form, scale_dtype=torch.float32)
    with pytest.raises(SamdError, match="e8m0"):
        MX.linear_mxfp4(lin, name)
    lin, _, _ = mx_linear(form=form, scale_dtype=torch.float8_e4m3fn)
    with pytest.raises(SamdError, match="e8m0"):
        MX.linear_mxfp4(lin, name)
    # NVFP4's second-level scales
    for second in ("weight_scale_2", "weight_global_scale"):
        lin, _, _ = mx_linear(form=form)
        lin.register_buffer(second, torch.ones(1))
        with pytest.raises(SamdError, match="NVFP4"):
            MX.linear_mxfp4(lin, name)
    # no scale at all
    lin, _, _ = mx_linear(form=form)
    lin.weight_scale = None
    with pytest.raises(SamdError, match="without a weight_scale"):
        MX.linear_mxfp4(lin, name)
    # the NaN code
    lin, _, e8 = mx_linear(form=form)
    bad = e8.clone()
    bad[7, 3] = 255
    lin.weight_scale = bad.view(E8) if form == "fp4" else bad
    with pytest.raises(SamdError, match="NaN"):
        MX.linear_mxfp4(lin, name)


def test_exponents_outside_the_dtype_range_are_rejected():
    e8 = torch.full((4, 4), 127, dtype=torch.uint8)
    MX.check_exponents(e8, torch.float16)
    MX.check_exponents(e8, torch.bfloat16)
    lo, hi = MX.exponent_range(torch.float16)
    for ex in (lo - 1, hi + 1):
        bad = e8.clone()
        bad[1, 2] = ex + 127
        with pytest.raises(SamdError, match="bfloat16"):                  # the fp16 message names the way out
            MX.check_exponents(bad, torch.float16, "layers.3.mlp.down_proj")
        MX.check_exponents(bad, torch.bfloat16)
    for code in (0, 1, 253, 254):                                         # exponents -127, -126, 126, 127
        bad = e8.clone()
        bad[0, 0] = code
        with pytest.raises(SamdError, match="exact"):
            MX.check_exponents(bad, torch.bfloat16)
    bad = e8.clone()
    bad[0, 0] = 255
    with pytest.raises(SamdError, match="NaN"):
        MX.check_exponents(bad, torch.bfloat16)
    for ok in (2, 252):
        good = e8.clone()
        good[0, 0] = ok
        MX.check_exponents(good, torch.bfloat16)


def test_checkpoint_is_all_or_nothing():
    m4 = mx_linear()[0]
    plain = torch.nn.Linear(512, 256, bias=False)
    assert MX.checkpoint_is_mxfp4([("a", m4), ("b", mx_linear(seed=1, form="u8")[0])]) is True
    assert MX.checkpoint_is_mxfp4([("a", plain), ("b", torch.nn.Linear(512, 256, bias=False))]) is False
    with pytest.raises(SamdError, match="mix of MXFP4"):
        MX.checkpoint_is_mxfp4([("layers.0.q_proj", m4), ("layers.0.k_proj", plain)])


# ---------------------------------------------------------------------------------------------------------------------
def packed_f4_np(q, e8):
    """numpy restatement of samd_gemm_pack_f4: q [N][K/2] bytes, e8 [N][K/32] bytes -> the packed bytes.  Block (tile t, chunk c) = 17408 bytes
    at (t * K/256 + c) * 17408: 1024 element units of 16 bytes, then 1024 scale bytes.  Element unit j * 512 + tid holds the 16 bytes (32
    weights, one MX block) of q[128 t + 16 w + n] at k = 256 c + 128 j + 32 g, for tid = 64 w + 16 g + n; scale byte 2 tid + j is that block's
    e8[128 t + 16 w + n][8 c + 4 j + g]."""
    N, Kh = q.shape
    K = 2 * Kh
    assert N % 128 == 0 and K % 256 == 0 and e8.shape == (N, K // 32)
    n_chunks = K // 256
    out = np.zeros((N // 128, n_chunks, 17408), dtype=np.uint8)
    for j in range(2):
        for tid in range(512):
            w, g, n = tid >> 6, (tid >> 4) & 3, tid & 15
            rows_ = 128 * np.arange(N // 128) + 16 * w + n                            # one row per tile
            for c in range(n_chunks):
                blk = 8 * c + 4 * j + g                                              # the MX block along k
                out[:, c, 16 * (512 * j + tid):16 * (512 * j + tid) + 16] = q[rows_, 16 * blk:16 * blk + 16]
                out[:, c, 16384 + 2 * tid + j] = e8[rows_, blk]
    return out.reshape(-1)


def test_packed_layout_is_a_permutation_with_every_block_beside_its_scale():
    rng = np.random.default_rng(0)
    N, K = 256, 768
    q = rng.integers(0, 256, size=(N, K // 2), dtype=np.uint8)
    e8 = rng.integers(0, 255, size=(N, K // 32), dtype=np.uint8)
    p = packed_f4_np(q, e8)
    assert p.size == MX.packed_bytes(N, K) == N * K // 2 + N * K // 32
    assert np.array_equal(np.sort(p), np.sort(np.concatenate([q.reshape(-1), e8.reshape(-1)])))
    # spot checks written out by hand: tile 1, chunk 2, j = 1, wave 3, lane group 2, column 5
    t, c, j, w, g, n = 1, 2, 1, 3, 2, 5
    tid = 64 * w + 16 * g + n
    base = (t * (K // 256) + c) * 17408
    row, k = 128 * t + 16 * w + n, 256 * c + 128 * j + 32 * g
    assert np.array_equal(p[base + 16 * (512 * j + tid):base + 16 * (512 * j + tid) + 16], q[row, k // 2:k // 2 + 16])
    assert p[base + 16384 + 2 * tid + j] == e8[row, k // 32]
