"""samd_tree_attention at head_dim 64 (k_tree_attention_gqa64 + the 64-wide merge) against a float64 masked softmax.  Inputs and tolerance
as test_tree_attention (tests/test_gpu_verify.py): a 64-long dot product rounds no worse than a 128-long one."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import SamdError, _ptr
from util import random_parents

# (H, Hkv): G = 1, 4, 3 (a head count that is no multiple of 8), 8 (two heads per wave).  (L, n, tree): the first tile alone; total = 64; new
# keys open tile 2; a second 16-row tile; bushy; > 1024 keys (every split's second tile).  Then: two mask words; the cache filled to its last row
SHAPES = [(0, 1, "chain"), (1, 5, "chain"), (63, 1, "chain"), (64, 16, "star"), (130, 17, "random"), (1000, 60, "bushy"), (1030, 9, "random")]
CASES = [(H, Hkv, L, n, t, 64, 2048) for H, Hkv in [(4, 4), (8, 2), (6, 2), (8, 1)] for L, n, t in SHAPES] + [
    (8, 2, 700, 100, "random", 128, 2048), (8, 2, 512 - 33, 33, "bushy", 64, 512)]
TOL = [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)]


def run(fn, dtype, H, Hkv, L, n, tree, n_pad, max_len, extra=(), D=64):
    """(output rows < n of fn on a seeded case, their float64 reference [n][H][D])"""
    rng, g = np.random.default_rng(L * 7 + n + H), torch.Generator(device="cuda").manual_seed(L + n)
    q = torch.randn((n_pad, H, D), generator=g, device="cuda").to(dtype)
    k = torch.randn((Hkv, max_len, D), generator=g, device="cuda").to(dtype)
    v = (torch.randn((Hkv, max_len, D), generator=g, device="cuda") * torch.linspace(0.5, 2.0, D, device="cuda")).to(dtype)
    k[:, L + n:], v[:, L + n:], q[n:] = float("nan"), float("nan"), float("nan")      # stale cache rows and pad query rows must never leak
    anc, vis = random_parents(rng, n, tree), torch.eye(n, dtype=torch.bool)
    for i in range(1, n):
        vis[i] |= vis[anc[i]]                             # (parents precede children)
    rows = [sum(1 << j for j in range(n) if vis[i, j]) for i in range(n)]
    pad = [0] * (samd_hip.MAX_DRAFT - n)                  # [2][MAX_DRAFT] words: low, then high (read only above 64 rows)
    mask = torch.tensor(np.array([r & (2 ** 64 - 1) for r in rows] + pad + [r >> 64 for r in rows] + pad, dtype=np.uint64).view(np.int64), device="cuda")
    bias = torch.zeros((n, L + n), dtype=torch.float64, device="cuda")
    bias[:, L:] = torch.where(vis.cuda(), 0.0, float("-inf"))
    kd, vd = (t[:, :L + n].double().repeat_interleave(H // Hkv, 0) for t in (k, v))
    want = torch.einsum("hnk,hkd->nhd", torch.softmax(torch.einsum("nhd,hkd->hnk", q[:n].double(), kd) / math.sqrt(D) + bias, -1), vd)
    out = torch.full((n_pad, H, D), 7.0, device="cuda").to(dtype)
    ws_bytes = samd_hip.lib().samd_tree_attention_workspace(n_pad, H, D)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    d_L, d_n = (torch.tensor([x], dtype=torch.int32, device="cuda") for x in (L, n))
    samd_hip.check(fn(_ptr(q), _ptr(k), _ptr(v), _ptr(out), samd_hip.torch_dtype_code(dtype), n_pad, H, Hkv, D, max_len, _ptr(mask), _ptr(d_L),
                      _ptr(d_n), 1.0 / math.sqrt(D), _ptr(ws), ws_bytes, *extra, samd_hip.current_stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and (out[n:] == 0).all()
    return out[:n].double(), want


@pytest.mark.parametrize("dtype,tol", TOL)
@pytest.mark.parametrize("H,Hkv,L,n,tree,n_pad,max_len", CASES)
def test_tree_attention_hd64(dtype, tol, H, Hkv, L, n, tree, n_pad, max_len):
    got, want = run(samd_hip.lib().samd_tree_attention, dtype, H, Hkv, L, n, tree, n_pad, max_len)
    assert (got - want).abs().max().item() < tol * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("dtype,tol", TOL)
def test_permuting_merge_hd64(dtype, tol):
    perm = torch.randperm(8 * 64, generator=torch.Generator().manual_seed(5))
    d_inv = torch.argsort(perm).to(torch.int32).cuda()    # the inverse permutation (kept alive across the launch)
    got, want = run(samd_hip.lib().samd_tree_attention_perm, dtype, 8, 2, 130, 17, "random", 64, 2048, extra=(0, _ptr(d_inv), None))
    err = (got.reshape(17, -1) - want.reshape(17, -1)[:, perm.cuda()]).abs().max().item()      # out_perm[r][i] = out[r][perm[i]]
    assert err < tol * max(1.0, want.abs().max().item()), err


def test_other_widths_and_the_transposed_cache_are_errors():
    for fn, kw in ((samd_hip.lib().samd_tree_attention, dict(D=96)), (samd_hip.lib().samd_tree_attention_vt, dict(extra=(None,)))):
        with pytest.raises(SamdError):                    # (an error before any launch: the layout of v is never read)
            run(fn, torch.float16, 8, 2, 10, 3, "chain", 16, 64, **kw)
