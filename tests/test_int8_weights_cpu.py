"""INT8 (GPTQ: 8-bit codes, one scale and one 8-bit zero point per 128 along K) weight-only decoding, host side: dequantize_groups on every
difference q - z, the quantiser of samd_hip/int8.py against the rule it documents, the checkpoint importer against an independent packer
written here from the format's public definition, every rejection by its message, and the packed layout of samd_gemm_pack_i8 restated in
numpy (packed_i8_np, which tests/test_gpu_int8_gemm.py imports).

Measured here: the relative RMS weight error of quantize_groups on Gaussian rows is 0.00592 in fp16 and 0.00617 in bf16 (whose one rounding
of the weight to 8 significant bits shows at this step size) -- against 0.0059, the INT4 figure of this repository (0.1006 with 15 steps)
times 15 / 255."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from samd_hip import SamdError
from samd_hip import int4 as I4
from samd_hip import int8 as I8

DTYPES = [torch.float16, torch.bfloat16]


def rows(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, K), generator=g) * 0.02 * (1 + 8 * torch.rand((N, 1), generator=g))


def random_qzs(N, K, seed=0, dtype=torch.float16, groups=None):
    """a random canonical projection: every code, every zero point, scales that differ between groups and columns"""
    g = torch.Generator().manual_seed(seed)
    G = K // 128 if groups is None else groups
    q = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 256, (N, G), generator=g, dtype=torch.uint8)
    s = (0.0001 + 0.002 * torch.rand((N, G), generator=g)).to(dtype)
    return q, z, s


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_groups_on_every_difference_with_one_rounding(dtype):
    # row r: z = r (0..255), codes k: 0..255 over two groups -> every (q, z) pair, every difference -255..255
    q = torch.arange(256, dtype=torch.uint8)[None, :].repeat(256, 1)
    z = torch.arange(256, dtype=torch.uint8)[:, None].repeat(1, 2)
    diff = (q.double() - z[:, :1].double())
    assert diff.min().item() == -255 and diff.max().item() == 255
    inexact = 0
    for sv in (1.0, 0.0123, 3.0e-7 if dtype == torch.float16 else 1.0e-30, 6.1e-5, 0.37, 250.0):
        s = torch.full((256, 2), sv).to(dtype)
        W = I8.dequantize_groups(q, z, s)
        prod = diff * s[:, :1].double()                                      # exact in float64 (9 x 11 significant bits)
        assert torch.equal(prod.float().double(), prod), sv                  # ... and already in fp32: the product itself is not a rounding
        assert torch.equal(W, prod.to(dtype).float()), sv                    # ONE rounding, to the dtype
        assert torch.equal(W.to(dtype).float(), W)
        inexact += int((W.double() != prod).sum())
    assert inexact > 1000                                                    # the rounding is really there
    # the group index is k // 128, and there is one code per byte in k order
    q2, z2, s2 = random_qzs(2, 512, 5, dtype)
    W2 = I8.dequantize_groups(q2, z2, s2)
    for k in (0, 127, 128, 255, 256, 511):
        want = ((q2[:, k].int() - z2[:, k // 128].int()).float() * s2[:, k // 128].float()).to(dtype).float()
        assert torch.equal(W2[:, k], want), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantiser_rule_and_round_trip(dtype):
    tiny, eps = torch.finfo(dtype).tiny, torch.finfo(dtype).eps
    # zero inclusion: an all-positive group still has lo = 0 (z = 0), an all-negative one hi = 0 (z = 255)
    W = torch.zeros((3, 128))
    W[0] = torch.linspace(1.0, 2.0, 128)
    W[1] = -torch.linspace(1.0, 2.0, 128)
    W[2] = torch.linspace(-1.0, 2.0, 128)
    q, z, s = I8.quantize_groups(W, dtype)
    assert s.dtype == dtype and q.dtype == torch.uint8 and z.dtype == torch.uint8 and q.shape == (3, 128)
    lo = torch.tensor([0.0, -2.0, -1.0])
    assert torch.equal(z[:, 0].float(), torch.round(-lo / s[:, 0].float()).clamp(0, 255))     # with the ROUNDED s: bf16's rounds up, so 254
    assert z[:, 0].tolist() == ([0, 255, 85] if dtype == torch.float16 else [0, 254, 85])
    assert torch.equal(s[:, 0], torch.tensor([2.0 / 255, 2.0 / 255, 3.0 / 255]).to(dtype))
    sf = s.float()
    assert torch.equal(q.int(), (torch.round(W / sf) + z.float()).clamp(0, 255).int())     # computed with the ROUNDED s
    assert int(q[0].max()) == (255 if dtype == torch.float16 else 254) and int(q[1].min()) == 0       # (2 / s rounds to 254 with bf16's s)
    # zero is representable: a zero weight dequantises to exactly zero
    Wz = rows(8, 256, 3)
    Wz[:, ::7] = 0.0
    qz, zz, sz = I8.quantize_groups(Wz, dtype)
    assert bool((I8.dequantize_groups(qz, zz, sz)[:, ::7] == 0).all())
    # the all-zero group
    q0, z0, s0 = I8.quantize_groups(torch.zeros((1, 256)), dtype)
    assert s0.tolist() == [[1.0, 1.0]] and z0.tolist() == [[0, 0]] and int(q0.max()) == 0
    # a group of tiny values gets the smallest normal as its scale
    qt, zt, st = I8.quantize_groups(torch.full((1, 128), tiny / 64.0), dtype)
    assert st.float().item() == tiny and zt.item() == 0
    for seed in range(4):
        Wr = rows(32, 512, seed)
        qr, zr, sr = I8.quantize_groups(Wr, dtype)
        lo = Wr.view(32, 4, 128).amin(2).clamp_max(0)
        hi = Wr.view(32, 4, 128).amax(2).clamp_min(0)
        assert torch.equal(sr, ((hi - lo) / 255).clamp_min(tiny).to(dtype))
        assert torch.equal(zr.float(), torch.round(-lo / sr.float()).clamp(0, 255))
        # |W - dequantised| <= s / 2 + one ulp of the dtype wherever no clamp acted (the rounded s can undershoot (hi - lo) / 255)
        srf = sr.float().repeat_interleave(128, dim=1)
        raw = torch.round(Wr / srf) + zr.float().repeat_interleave(128, dim=1)
        free = (raw >= 0) & (raw <= 255)
        assert free.float().mean().item() > 0.99
        D = I8.dequantize_groups(qr, zr, sr)
        bound = 0.5 * srf + eps * D.abs()
        assert bool(((Wr - D).abs() <= bound)[free].all())
    with pytest.raises(SamdError, match="K % 128"):
        I8.quantize_groups(torch.zeros((4, 192)), dtype)
    with pytest.raises(SamdError, match="fp16 or bf16"):
        I8.quantize_groups(torch.zeros((4, 128)), torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_measured_rms_error_on_gaussian_rows(dtype):
    W = rows(256, 4096, 11)
    q, z, s = I8.quantize_groups(W, dtype)
    rel = ((I8.dequantize_groups(q, z, s) - W).pow(2).sum() / W.pow(2).sum()).sqrt().item()
    print(f"{dtype}: relative RMS weight error of quantize_groups on Gaussian rows: {rel:.5f}")
    # the INT4 quantiser of this repository measures 0.1006 on these rows with 15 steps over the same range: 255 steps give 0.1006 * 15 / 255
    want = 0.1006 * 15 / 255
    assert 0.9 * want <= rel <= 1.1 * want, rel


@pytest.mark.parametrize("dtype", DTYPES)
def test_fusing_before_and_after_quantising_gives_the_same_bytes(dtype):
    Wq, Wk, Wv = rows(256, 512, 1), rows(128, 512, 2), rows(128, 512, 3)
    parts = [I8.quantize_groups(w, dtype) for w in (Wq, Wk, Wv)]
    q, z, s = I8.fuse_int8(parts, "cpu", dtype)
    q2, z2, s2 = I8.quantize_groups(torch.cat([Wq, Wk, Wv]), dtype)
    assert torch.equal(q, q2) and torch.equal(z, z2) and torch.equal(s, s2)


# ---------------------------------------------------------------------------------------------------------------------
# an independent packer, from the format's public definition
def pack_bytes_int32(b):
    """b int64 [..., 4] (0..255) -> int32 [...]: byte p at bits 8p .. 8p + 7"""
    v = np.zeros(b.shape[:-1], dtype=np.uint32)
    for p in range(4):
        v |= b[..., p].astype(np.uint32) << np.uint32(8 * p)
    return torch.from_numpy(v.view(np.int32).copy())


def gptq8_tensors(q, z, s, g, stored_offset):
    """-> 8-bit GPTQ (qweight [K/4, N], qzeros [K/g, N/4], scales [K/g, N], g_idx [K]); the stored zero is z - stored_offset"""
    N, K = q.shape
    c = q.numpy()
    by = np.zeros((K // 4, N, 4), dtype=np.int64)
    for r in range(K // 4):
        for p in range(4):
            by[r, :, p] = c[:, 4 * r + p]
    zs = z.numpy().astype(np.int64).T - stored_offset              # [K/g, N]
    assert zs.min() >= 0
    zby = np.zeros((zs.shape[0], N // 4, 4), dtype=np.int64)
    for j in range(N // 4):
        for p in range(4):
            zby[:, j, p] = zs[:, 4 * j + p]
    return pack_bytes_int32(by), pack_bytes_int32(zby), s.t().contiguous(), (torch.arange(K) // g).to(torch.int32)


class QLinear(torch.nn.Module):
    """what a GPTQ loader leaves in place of an nn.Linear: integer buffers, no `weight`"""

    def __init__(self, K, N, qweight, qzeros, scales, g_idx=None, bias=None, bits=None):
        super().__init__()
        self.in_features, self.out_features = K, N
        self.register_buffer("qweight", qweight)
        self.register_buffer("qzeros", qzeros)
        self.register_buffer("scales", scales)
        if g_idx is not None:
            self.register_buffer("g_idx", g_idx)
        self.bias = bias
        if bits is not None:
            self.bits = bits


def gptq8_module(q, z, s, g=128, v2=False, with_g_idx=True, **kw):
    N, K = q.shape
    qw, qz, sc, gi = gptq8_tensors(q, z, s, g, 0 if v2 else 1)
    return QLinear(K, N, qw, qz, sc, gi if with_g_idx else None, **kw)


def gptq4_module(N, K, seed=0):
    """a 4-bit GPTQ module, through test_int4_weights_cpu's independent packer"""
    from test_int4_weights_cpu import gptq_module, random_qzs as random_qzs4, v1_safe as v1_safe4
    q, z, s = random_qzs4(N, K, seed)
    return gptq_module(q, v1_safe4(z), s)


def v1_safe(z):
    """zero points a GPTQ v1 checkpoint can store (z - 1 >= 0)"""
    return z.clamp_min(1)


GPTQ8_CFG = dict(quant_method="gptq", bits=8, group_size=128, desc_act=False)
GPTQ8V2_CFG = dict(GPTQ8_CFG, checkpoint_format="gptq_v2")


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_the_importer_returns_the_known_canonical_projection():
    N, K = 64, 512
    q, z, s = random_qzs(N, K, 3)
    z = v1_safe(z)
    z[0, 0], z[1, 0] = 255, 1
    for got in (I8.linear_int8(gptq8_module(q, z, s), "p", config=GPTQ8_CFG),
                I8.linear_int8(gptq8_module(q, z, s), "p", config=Obj(**GPTQ8_CFG)),           # a config object
                I8.linear_int8(gptq8_module(q, z, s), "p"),                                    # no config: by shape, GPTQ v1
                I8.linear_int8(gptq8_module(q, z, s, bits=8), "p"),                            # the module's own bits
                I8.linear_int8(gptq8_module(q, z, s, with_g_idx=False), "p", config=GPTQ8_CFG),
                I8.linear_int8(gptq8_module(q, z, s, v2=True), "p", config=GPTQ8V2_CFG),
                I8.linear_int8(gptq8_module(q, z, s, v2=True), "p", config=GPTQ8_CFG, zero_offset=0)):
        assert got is not None
        assert torch.equal(got[0], q) and torch.equal(got[1], z) and torch.equal(got[2], s)
    # v2 stores z itself: read as v1 every zero point would be one too high
    zlow = z.clamp_max(254)
    assert torch.equal(I8.linear_int8(gptq8_module(q, zlow, s, v2=True), "p", config=GPTQ8_CFG)[1], zlow + 1)
    # an ordinary Linear is not INT8; which width a quantised module has: config, then the module's bits, then qweight's shape
    assert I8.linear_int8(torch.nn.Linear(8, 8), "p") is None
    m8, m4 = gptq8_module(q, z, s), gptq4_module(N, K)
    assert not I8.is_int8_module(torch.nn.Linear(8, 8)) and I8.is_int8_module(m8) and not I8.is_int8_module(m4)
    assert I4.is_int4_module(m8)                                   # (the INT4 test does not look at the width: the runner asks INT8 first)
    assert I8.is_int8_module(m4, dict(bits=8)) and not I8.is_int8_module(m8, dict(bits=4))
    assert I8.is_int8_module(gptq8_module(q, z, s, bits=8)) and not I8.is_int8_module(gptq8_module(q, z, s, bits=4))


def test_byte_order_by_hand():
    # byte p of qweight[r][n] is k = 4 r + p: plant code 0x9C at row n = 19, k = 7 -> byte 3 of qweight[1][19]
    N, K = 32, 256
    q = torch.zeros((N, K), dtype=torch.uint8)
    q[19, 7] = 0x9C
    z = torch.ones((N, 2), dtype=torch.uint8)
    s = torch.ones((N, 2), dtype=torch.float16)
    qw, qz, sc, gi = gptq8_tensors(q, z, s, 128, 1)
    assert qw[1, 19].item() & 0xFFFFFFFF == 0x9C << 24 and int((qw != 0).sum()) == 1
    assert qw[1, 19].item() < 0                                     # the top byte makes the int32 negative: no sign extension into the code
    got = I8.linear_int8(QLinear(K, N, qw, qz, sc, gi), "p", config=GPTQ8_CFG)
    assert torch.equal(got[0], q) and torch.equal(got[1], z)
    # byte p of qzeros[G][j] is column 4 j + p: zero point 200 (stored 199) of column 14, group 1 -> byte 2 of qzeros[1][3]
    z[14, 1] = 200
    qw, qz, sc, gi = gptq8_tensors(q, z, s, 128, 1)
    assert (qz[1, 3].item() >> 16) & 255 == 199
    assert I8.linear_int8(QLinear(K, N, qw, qz, sc, gi), "p", config=GPTQ8_CFG)[1][14, 1].item() == 200


def test_group_256_512_and_per_channel_are_expanded():
    N, K = 64, 512
    for g, cfg_g in ((256, 256), (512, -1), (512, 512)):
        q, z, s = random_qzs(N, K, 4, groups=K // g)
        z = v1_safe(z)
        got = I8.linear_int8(gptq8_module(q, z, s, g), "p", config=dict(GPTQ8_CFG, group_size=cfg_g))
        assert got[1].shape == (N, K // 128) and got[2].shape == (N, K // 128)
        assert torch.equal(got[0], q)
        assert torch.equal(got[1], z.repeat_interleave(g // 128, dim=1)) and torch.equal(got[2], s.repeat_interleave(g // 128, dim=1))


def test_rejections_by_message():
    N, K = 64, 512
    q, z, s = random_qzs(N, K, 6)
    z = v1_safe(z).clamp_max(254)
    name = "layers.3.o_proj"
    # bit widths other than 8: by config, by the module's bits, by shape (a 4-bit module handed to linear_int8)
    with pytest.raises(SamdError, match=f"{name}: 4-bit"):
        I8.linear_int8(gptq8_module(q, z, s), name, config=dict(GPTQ8_CFG, bits=4))
    with pytest.raises(SamdError, match=f"{name}: 3-bit"):
        I8.linear_int8(gptq8_module(q, z, s, bits=3), name)
    with pytest.raises(SamdError, match=f"{name}: 4-bit quantisation; the INT8 importer takes 8-bit GPTQ"):
        I8.linear_int8(gptq4_module(N, K), name)
    # AWQ
    with pytest.raises(SamdError, match=f"{name}: quant_method 'awq'"):
        I8.linear_int8(gptq8_module(q, z, s), name, config=dict(GPTQ8_CFG, quant_method="awq"))
    # group 64 (and 32)
    for g in (64, 32):
        q6, z6, s6 = random_qzs(N, K, 7, groups=K // g)
        with pytest.raises(SamdError, match=f"{name}: group_size {g} is not supported"):
            I8.linear_int8(gptq8_module(q6, v1_safe(z6), s6, g), name, config=dict(GPTQ8_CFG, group_size=g))
    # act-order
    mod = gptq8_module(q, z, s)
    mod.g_idx = mod.g_idx.flip(0).contiguous()
    with pytest.raises(SamdError, match=f"{name}: act-order"):
        I8.linear_int8(mod, name, config=dict(GPTQ8_CFG, desc_act=True))
    with pytest.raises(SamdError, match=f"{name}: act-order"):
        I8.linear_int8(mod, name)
    with pytest.raises(SamdError, match=f"{name}: act-order \\(desc_act\\)"):
        I8.linear_int8(gptq8_module(q, z, s, with_g_idx=False), name, config=dict(GPTQ8_CFG, desc_act=True))
    # desc_act with the trivial g_idx is the plain order and passes
    assert I8.linear_int8(gptq8_module(q, z, s), name, config=dict(GPTQ8_CFG, desc_act=True)) is not None
    # unknown checkpoint_format
    with pytest.raises(SamdError, match=f"{name}: GPTQ checkpoint_format 'marlin'"):
        I8.linear_int8(gptq8_module(q, z, s), name, config=dict(GPTQ8_CFG, checkpoint_format="marlin"))
    # a stored 255 under GPTQ v1
    z255 = z.clone()
    z255[3, 1] = 255
    with pytest.raises(SamdError, match=f"{name}: a stored zero point of 255"):
        I8.linear_int8(gptq8_module(q, z255, s, v2=True), name, config=GPTQ8_CFG)
    assert I8.linear_int8(gptq8_module(q, z255, s, v2=True), name, config=GPTQ8V2_CFG)[1][3, 1].item() == 255
    # ill-shaped tensors
    bad = gptq8_module(q, z, s)
    bad.qzeros = bad.qzeros[:, :-1].contiguous()
    with pytest.raises(SamdError, match=f"{name}: qzeros of shape"):
        I8.linear_int8(bad, name, config=GPTQ8_CFG)
    bad = gptq8_module(q, z, s)
    bad.qweight = bad.qweight[:-1].contiguous()
    with pytest.raises(SamdError, match=f"{name}: qweight of shape"):
        I8.linear_int8(bad, name, config=GPTQ8_CFG)
    bad = gptq8_module(q, z, s)
    bad.scales = bad.scales[:, :-1].contiguous()
    with pytest.raises(SamdError, match=f"{name}: scales of shape"):
        I8.linear_int8(bad, name, config=GPTQ8_CFG)
    with pytest.raises(SamdError, match=f"{name}: the tensors carry groups of 128"):
        I8.linear_int8(gptq8_module(q, z, s), name, config=dict(GPTQ8_CFG, group_size=256))
    # a bias on o / gate / up / down (q / k / v may carry one: Qwen2)
    for proj in ("o_proj", "gate_proj", "up_proj", "down_proj"):
        with pytest.raises(SamdError, match=f"layers.0.{proj}: a bias"):
            I8.linear_int8(gptq8_module(q, z, s, bias=torch.zeros(N)), f"layers.0.{proj}", config=GPTQ8_CFG)
    assert I8.linear_int8(gptq8_module(q, z, s, bias=torch.zeros(N)), "layers.0.q_proj", config=GPTQ8_CFG) is not None
    # canonical-form checks of the runner
    with pytest.raises(SamdError, match="N % 128 == 0 and K % 256 == 0"):
        I8.check_groups(q, z, s, torch.float16, "p")
    q2, z2, s2 = random_qzs(128, 256, 1)
    I8.check_groups(q2, z2, s2, torch.float16, "p")
    with pytest.raises(SamdError, match="scales of dtype"):
        I8.check_groups(q2, z2, s2, torch.bfloat16, "p")
    with pytest.raises(SamdError, match="zero points .* one per 128"):
        I8.check_groups(q2, z2[:, :1], s2, torch.float16, "p")
    # int4.linear_int4 keeps rejecting the 8-bit module
    with pytest.raises(SamdError, match="8-bit"):
        I4.linear_int4(gptq8_module(q, z, s), "p", config=GPTQ8_CFG)


def test_checkpoint_is_int8_and_mix_detection():
    N, K = 64, 512
    q, z, s = random_qzs(N, K, 6)
    m8, m4, plain = gptq8_module(q, v1_safe(z), s), gptq4_module(N, K), torch.nn.Linear(8, 8)
    assert I8.checkpoint_is_int8([("layers.0.q", m8), ("layers.0.k", m8)]) is True
    assert I8.checkpoint_is_int8([("layers.0.q", m4), ("layers.0.k", plain)]) is False
    assert I8.checkpoint_is_int8([]) is False
    for other in (m4, plain):
        with pytest.raises(SamdError, match="a mix of INT8 and other projections \\(1 of 2 are INT8; e.g. layers.0.k"):
            I8.checkpoint_is_int8([("layers.0.q", m8), ("layers.0.k", other)])
    # the config's bits decide before the shapes do
    assert I8.checkpoint_is_int8([("layers.0.q", m8)], dict(bits=4)) is False
    assert I8.checkpoint_is_int8([("layers.0.q", m8)], GPTQ8_CFG) is True


def test_scale_checks():
    q, z, _ = random_qzs(64, 512, 6)
    # 255 * s must stay finite in fp16, and the message names bf16
    big = torch.full((64, 4), 300.0, dtype=torch.float16)
    with pytest.raises(SamdError, match="255 \\* max\\(scale\\).*overflows torch.float16.*bfloat16"):
        I8.check_scales(big, torch.float16, "p")
    with pytest.raises(SamdError, match="overflows torch.float16.*bfloat16"):
        I8.fuse_int8([(q, z, big)], "cpu", torch.float16)
    with pytest.raises(SamdError, match="a scale of .* overflows torch.float16.*bfloat16"):
        I8.as_scales(torch.full((1, 1), 1.0e6), torch.float16)
    ok = torch.full((1, 1), 256.0, dtype=torch.float16)            # 255 * 256 = 65280 <= 65504
    I8.check_scales(ok, torch.float16)
    with pytest.raises(SamdError, match="overflows"):
        I8.check_scales(torch.full((1, 1), 257.0, dtype=torch.float16), torch.float16)
    I8.check_scales(big.to(torch.bfloat16), torch.bfloat16, "p")
    assert I8.fuse_int8([(q, z, big)], "cpu", torch.bfloat16)[2].dtype == torch.bfloat16
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(SamdError, match="finite and > 0"):
            I8.check_scales(torch.full((1, 1), bad, dtype=torch.float16), torch.float16)
    with pytest.raises(SamdError, match="scales of dtype"):
        I8.as_scales(torch.ones((1, 1), dtype=torch.int32), torch.float16)
    # a bf16 runner rounds each fp16 scale ONCE; an fp16 runner takes them as they are
    s16 = torch.tensor([[0.0123, 0.5, 3.0e-5]], dtype=torch.float16)
    assert torch.equal(I8.as_scales(s16, torch.bfloat16), s16.to(torch.bfloat16)) and torch.equal(I8.as_scales(s16, torch.float16), s16)
    assert not torch.equal(I8.as_scales(s16, torch.bfloat16).float(), s16.float())
    assert I8.packed_bytes(128, 256) == 128 * 256 + 1024 and I8.PROJECTIONS == I4.PROJECTIONS


# ---------------------------------------------------------------------------------------------------------------------
def zero_words_np(z, dtype):
    """the 16-bit word the dtype's widening subtracts: fp16 the bits of 1024 + z (0x6400 | z), bf16 the bits of z itself (exact: 8 bits)"""
    if dtype == torch.float16:
        return z.astype(np.uint16) | np.uint16(0x6400)
    return (z.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def packed_i8_np(q, z, s_bits, dtype):
    """numpy restatement of samd_gemm_pack_i8: q [N][K] bytes, z [N][K/128] bytes, s_bits [N][K/128] uint16 (the scales' bits in the model
    dtype) -> the packed bytes.  Block (tile t, chunk c) = 33792 bytes at (t * K/256 + c) * 33792: 2048 code units of 16 bytes, then 128
    rows x 8 bytes of group data.  Code unit b * 512 + tid holds the 16 codes of q[128 t + 16 w + n] at k = 256 c + 64 b + 16 g .. + 15 in
    k order (inside group 2 c + b // 2), for tid = 64 w + 16 g + n.  Group data of row 16 w + n, as four little-endian 16-bit words:
    s[2c], s[2c+1], zw[2c], zw[2c+1] (zw: zero_words_np)."""
    N, K = q.shape
    T, C = N // 128, K // 256
    assert N % 128 == 0 and K % 256 == 0 and z.shape == (N, K // 128) and s_bits.shape == (N, K // 128) and s_bits.dtype == np.uint16
    u = q.reshape(T, 8, 16, C, 4, 4, 16)                                        # [t, w, n, c, b, g, byte]
    units = np.ascontiguousarray(u.transpose(0, 3, 4, 1, 5, 2, 6))              # [t, c, b, w, g, n, byte]: unit b * 512 + 64 w + 16 g + n
    out = np.zeros((T, C, 33792), dtype=np.uint8)
    out[:, :, :32768] = units.reshape(T, C, 32768)
    gd = np.zeros((T, C, 8, 16, 4), dtype="<u2")                                # [t, c, w, n, word]
    gd[..., 0:2] = s_bits.reshape(T, 8, 16, C, 2).transpose(0, 3, 1, 2, 4)
    gd[..., 2:4] = zero_words_np(z, dtype).reshape(T, 8, 16, C, 2).transpose(0, 3, 1, 2, 4)
    out[:, :, 32768:] = gd.view(np.uint8).reshape(T, C, 1024)
    return out.reshape(-1)


def s_bits_np(s):
    return s.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_layout_by_hand_and_as_a_permutation(dtype):
    N, K = 256, 768
    # one code, one zero point and one scale, each at a known offset: row 128 + 16 * 5 + 9 = 217 (tile 1, wave 5, n 9), k = 256 + 64 * 2 + 16 * 3
    # + 11 = 443 (chunk 1, b 2, g 3, byte 11; group 3 = 2 * 1 + 1)
    q = np.zeros((N, K), dtype=np.uint8)
    z = np.zeros((N, K // 128), dtype=np.uint8)
    sb = np.zeros((N, K // 128), dtype=np.uint16)
    q[217, 443], z[217, 3], sb[217, 3] = 0xAB, 0xC8, 0x1234
    p = packed_i8_np(q, z, sb, dtype)
    base = (1 * 3 + 1) * 33792
    assert p[base + 16 * (2 * 512 + 64 * 5 + 16 * 3 + 9) + 11] == 0xAB
    words = p[base + 32768 + 8 * (16 * 5 + 9):base + 32768 + 8 * (16 * 5 + 9) + 8].copy().view("<u2")
    zero0 = 0x6400 if dtype == torch.float16 else 0x0000             # the word of z = 0
    zero200 = 0x64C8 if dtype == torch.float16 else 0x4348           # 1024 + 200 in fp16; 200.0 in bf16
    assert words.tolist() == [0, 0x1234, zero0, zero200]
    blocks = p.reshape(-1, 33792)
    assert int((blocks[:, :32768] != 0).sum()) == 1 and int((blocks[:, 32768:].copy().view("<u2").reshape(-1, 4)[:, :2] != 0).sum()) == 1
    # the zero word is the dtype's bits of what the widening subtracts
    for zz in (0, 1, 127, 128, 200, 255):
        bits = torch.from_numpy(zero_words_np(np.array([zz], dtype=np.uint8), dtype).view(np.int16).copy()).view(dtype).float().item()
        assert bits == (1024 + zz if dtype == torch.float16 else zz)
    # random: a permutation of the codes block by block, every unit beside its group data
    qt, zt, st = random_qzs(N, K, 9, dtype)
    qn, zn, sn = qt.numpy(), zt.numpy(), s_bits_np(st)
    p = packed_i8_np(qn, zn, sn, dtype)
    assert p.size == I8.packed_bytes(N, K) == N * K + N * K // 32
    blocks = p.reshape(-1, 33792)
    assert np.array_equal(np.bincount(blocks[:, :32768].reshape(-1), minlength=256), np.bincount(qn.reshape(-1), minlength=256))
    gd = blocks[:, 32768:].copy().view("<u2").reshape(-1, 128, 4)
    assert np.array_equal(np.sort(gd[:, :, :2].reshape(-1)), np.sort(sn.reshape(-1)))
    assert np.array_equal(np.sort(gd[:, :, 2:].reshape(-1)), np.sort(zero_words_np(zn, dtype).reshape(-1)))
    W = I8.dequantize_groups(qt, zt, st).numpy()
    rng = np.random.default_rng(1)
    for _ in range(200):
        t, c, b, w, g, n, e = (int(rng.integers(0, hi)) for hi in (N // 128, K // 256, 4, 8, 4, 16, 16))
        tid = 64 * w + 16 * g + n
        base = (t * (K // 256) + c) * 33792
        row, k = 128 * t + 16 * w + n, 256 * c + 64 * b + 16 * g + e
        code = int(p[base + 16 * (512 * b + tid) + e])
        assert code == qn[row, k]
        words = p[base + 32768 + 8 * (16 * w + n):base + 32768 + 8 * (16 * w + n) + 8].copy().view("<u2")
        j = b // 2
        assert k // 128 == 2 * c + j and int(words[j]) == int(sn[row, k // 128])
        sval = torch.from_numpy(words[j:j + 1].copy().view(np.int16)).view(dtype).float().item()
        zval = torch.from_numpy(words[2 + j:3 + j].copy().view(np.int16)).view(dtype).float().item() - (1024 if dtype == torch.float16 else 0)
        assert zval == zn[row, k // 128]
        assert torch.tensor((code - zval) * sval, dtype=torch.float32).to(dtype).float().item() == W[row, k]
