"""Act-order GPTQ at import (samd_hip/int4.py, int8.py, formats.py): the permutation a g_idx implies, the tensors reordered by it, the fold
of down_proj's permutation into gate / up rows, and the rejections by name.  The helpers build act-order modules from NATURAL-order codes
through the independent packers of test_int4_weights_cpu / test_int8_weights_cpu; dequant_natural is the plain definition of the format."""
import pytest

torch = pytest.importorskip("torch")

from samd_hip import SamdError
from samd_hip import int4 as I4
from samd_hip import int8 as I8
from samd_hip.formats import DENSE
from test_int4_weights_cpu import GPTQ_CFG, gptq_module
from test_int8_weights_cpu import GPTQ8_CFG, gptq8_module

ORDERED = {4: I4.linear_int4_ordered, 8: I8.linear_int8_ordered}
QUANT = {4: I4, 8: I8}


def random_g_idx(K, g, seed):
    """every group exactly g members, assigned at random"""
    gen = torch.Generator().manual_seed(seed)
    return (torch.arange(K) // g)[torch.randperm(K, generator=gen)].to(torch.int32)


def random_codes(bits, N, K, g, seed, pow2_scales=False):
    """natural-order codes [N, K], zero points a v1 checkpoint can store and fp16 scales [N, K/g]"""
    gen = torch.Generator().manual_seed(seed)
    top = 1 << bits
    codes = torch.randint(0, top, (N, K), generator=gen, dtype=torch.uint8)
    z = torch.randint(1, top, (N, K // g), generator=gen, dtype=torch.int32).to(torch.uint8)
    if pow2_scales:
        s = torch.exp2(torch.randint(0, 4, (N, K // g), generator=gen).float() - 3).to(torch.float16)
    else:
        s = (0.002 + 0.018 * torch.rand((N, K // g), generator=gen)).to(torch.float16)
    return codes, z, s


def act_order_module(bits, codes, z, s, g_idx, g=128):
    mod = gptq_module(I4.pack_nibbles(codes), z, s, g=g) if bits == 4 else gptq8_module(codes, z, s, g=g)
    mod.g_idx = g_idx.clone()
    return mod


def cfg(bits, g=128):
    return dict(GPTQ_CFG if bits == 4 else GPTQ8_CFG, group_size=g, desc_act=True)


def dequant_natural(codes, z, s, g_idx, dtype):
    """W[n][k] = rne_dtype((codes[n][k] - z[n][g_idx[k]]) * s[n][g_idx[k]]), in the checkpoint's own K order, fp32"""
    gi = g_idx.long()
    return ((codes.int() - z.int()[:, gi]).float() * s.to(dtype).float()[:, gi]).to(dtype).float()


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("K,g", [(512, 128), (1024, 256)])
def test_perm_reconstruction(bits, K, g):
    codes, z, s = random_codes(bits, 128, K, g, seed=K + bits)
    gi = random_g_idx(K, g, seed=bits)
    q, zz, ss, perm = ORDERED[bits](act_order_module(bits, codes, z, s, gi, g), "p", config=cfg(bits, g))
    assert torch.equal(perm, torch.argsort(gi.long(), stable=True)) and torch.equal(gi.long()[perm], torch.arange(K) // g)
    assert tuple(zz.shape) == (128, K // 128)                                  # group sizes above 128 expand after the reorder
    w_perm = QUANT[bits].dequantize_groups(q, zz, ss)
    assert torch.equal(w_perm[:, I4.inverse_perm(perm)], dequant_natural(codes, z, s, gi, torch.float16))
    # the plain order has no permutation, with or without desc_act in the config
    plain = act_order_module(bits, codes, z, s, (torch.arange(K) // g).to(torch.int32), g)
    assert ORDERED[bits](plain, "p", config=cfg(bits, g))[3] is None


class Layer(torch.nn.Module):
    """a dense decoder layer's seven projections, hidden 256, 2 heads of 128, intermediate 384; q|k|v share g_idx, gate|up share one"""

    def __init__(self, bits, seed=0):
        super().__init__()
        self.self_attn, self.mlp = torch.nn.Module(), torch.nn.Module()
        self.parts, hidden, inter = {}, 256, 384
        g_in, g_o, g_mlp, g_down = (random_g_idx(K, 128, seed + i) for i, K in enumerate((hidden, hidden, hidden, inter)))
        for i, (own, name, N, K, gi) in enumerate(((self.self_attn, "q_proj", 256, hidden, g_in), (self.self_attn, "k_proj", 128, hidden, g_in),
                                                   (self.self_attn, "v_proj", 128, hidden, g_in), (self.self_attn, "o_proj", 256, hidden, g_o),
                                                   (self.mlp, "gate_proj", inter, hidden, g_mlp), (self.mlp, "up_proj", inter, hidden, g_mlp),
                                                   (self.mlp, "down_proj", hidden, inter, g_down))):
            codes, z, s = random_codes(bits, N, K, 128, seed=seed + 10 + i)
            setattr(own, name, act_order_module(bits, codes, z, s, gi))
            self.parts[name] = dequant_natural(codes, z, s, gi, torch.float16).double()


@pytest.mark.parametrize("bits", [4, 8])
def test_gate_up_fold_leaves_the_mlp_unchanged(bits):
    fmt = DENSE["int4g128" if bits == 4 else "int8g128"]
    lyr = Layer(bits)
    got = fmt.import_layer(lyr, 0, "cpu", torch.float16, cfg(bits))
    sfx = fmt.raw_keys
    W = {k: QUANT[bits].dequantize_groups(*(got[k + x] for x in sfx)).double() for k in ("wqkv", "wo", "wgu", "wdown")}
    x = torch.randn(3, 256, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    nat = lyr.parts
    silu_mul = lambda gu: torch.nn.functional.silu(gu[:, :384]) * gu[:, 384:]
    want = silu_mul(x @ torch.cat([nat["gate_proj"], nat["up_proj"]]).t()) @ nat["down_proj"].t()
    # float64 sums of <= 384 terms in another order: 384 x 2^-53 = 4e-14 of the largest term; 1e-10 of the largest output is far above
    # that and far below a misplaced row or column, which changes an output by its own size
    same = lambda a, b: float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())
    assert same(silu_mul(x[:, got["perm_mlp"].long()] @ W["wgu"].t()) @ W["wdown"].t(), want)
    # q|k|v and o_proj: the imported matrix against its input in the table's order
    assert same(x[:, got["perm_attn"].long()] @ W["wqkv"].t(), x @ torch.cat([nat["q_proj"], nat["k_proj"], nat["v_proj"]]).t())
    assert same(x[:, got["perm_o"].long()] @ W["wo"].t(), x @ nat["o_proj"].t())
    assert all(got[k].dtype == torch.int32 for k in ("perm_attn", "perm_o", "perm_mlp")) and "perm_down" not in got


@pytest.mark.parametrize("bits", [4, 8])
def test_named_rejections(bits):
    fmt = DENSE["int4g128" if bits == 4 else "int8g128"]
    lyr = Layer(bits)
    lyr.self_attn.k_proj.g_idx = random_g_idx(256, 128, seed=99)
    with pytest.raises(SamdError, match=r"layers\.3\.q_proj: act-order g_idx differs from layers\.3\.k_proj's: q_proj, k_proj, v_proj"):
        fmt.import_layer(lyr, 3, "cpu", torch.float16, cfg(bits))
    lyr = Layer(bits)
    lyr.mlp.up_proj.g_idx = random_g_idx(256, 128, seed=98)
    with pytest.raises(SamdError, match=r"layers\.0\.gate_proj: act-order g_idx differs from layers\.0\.up_proj's"):
        fmt.import_layer(lyr, 0, "cpu", torch.float16, cfg(bits))
    lyr = Layer(bits)
    gi = lyr.self_attn.o_proj.g_idx
    gi[int((gi == 1).nonzero()[0])] = 0                                     # one channel moves from group 1 to group 0
    with pytest.raises(SamdError, match=r"layers\.0\.o_proj: act-order group 0 has 129 input channels, group_size is 128"):
        fmt.import_layer(lyr, 0, "cpu", torch.float16, cfg(bits))
    # an expert's module goes through the plain-order importers, which say why act-order stops there
    plain = {4: I4.linear_int4, 8: I8.linear_int8}[bits]
    with pytest.raises(SamdError, match=r"layers\.1\.mlp\.experts\.5\.up_proj: act-order .* each expert of a sparse layer has its own permutation"):
        plain(Layer(bits).mlp.up_proj, "layers.1.mlp.experts.5.up_proj", config=cfg(bits))
