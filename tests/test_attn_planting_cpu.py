"""The planted-attention helper (tests/attn_planting.py) checked on CPU in float64, for fp16 and bf16 rounding: the plants do what the GPU
tests rely on them to do, and the visibility matrices are the reference's tree masks."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import attn_planting as P
from util import random_parents

DTYPES = [torch.float16, torch.bfloat16]


def weights(q, k, vis_row):
    s = (k @ q) * P.SCALE
    s = s.masked_fill(~torch.as_tensor(vis_row), float("-inf"))
    return torch.softmax(s, -1)


def planted(dtype, L, n, H, Hkv, seed, kinds=P.KINDS, shape="random"):
    rng = np.random.default_rng(seed)
    rows = P.ancestor_rows(random_parents(rng, n, shape))
    vis = P.tree_visibility(rows, L)
    k = P.rounded(P.unit_rows(rng, (Hkv, L + n)), dtype)
    v = P.rounded(P.value_rows(rng, (Hkv, L + n)), dtype)
    plan = P.make_plan(rng, vis, H, Hkv, P.tree_splits(L + n), seams=P.seam_keys(L, n, L + n), kinds=kinds, anti_prefer=(L + 63, L + 64))
    P.apply_negations(v, plan)
    q = P.rounded(P.plant_queries(plan, k, H), dtype)
    return q, k, v, vis, plan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,n", [(8192 - 64, 64), (1000, 16), (0, 5)])
def test_needles_take_the_weight(dtype, L, n):
    H, Hkv = 8, 2
    q, k, v, vis, plan = planted(dtype, L, n, H, Hkv, L + n, kinds=("needle",))
    for i, h in plan.cells():
        w = weights(q[i, h], k[h // 4], vis[i])
        assert w[plan.keys[i][h][0]] >= 1 - 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_needles_split_the_weight_as_designed(dtype):
    H, Hkv, L, n = 8, 2, 2000, 32
    q, k, v, vis, plan = planted(dtype, L, n, H, Hkv, 3, kinds=("two",))
    cells = plan.cells(("two",))
    assert len(cells) > H * n // 2
    split = P.tree_splits(L + n)
    want_a = 1 / (1 + np.exp(-P.GAP))
    for i, h in cells:
        a, b = plan.keys[i][h]
        assert split[a] != split[b]
        w = weights(q[i, h], k[h // 4], vis[i])
        assert abs(w[a].item() - want_a) < 0.03 and abs(w[b].item() - (1 - want_a)) < 0.03 and w[a] + w[b] > 1 - 1e-6
        assert torch.equal(v[h // 4, b], -v[h // 4, a])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["star", "chain", "random"])
def test_anti_needles_would_take_the_weight_if_unmasked(dtype, shape):
    H, Hkv, L, n = 8, 8, 300, 128
    q, k, v, vis, plan = planted(dtype, L, n, H, Hkv, 5, kinds=("anti",), shape=shape)
    cells = plan.cells(("anti",))
    assert cells and any(plan.keys[i][h][1] in (L + 63, L + 64) for i, h in cells)
    for i, h in cells:
        t, m = plan.keys[i][h]
        assert vis[i, t] and not vis[i, m]
        assert weights(q[i, h], k[h], vis[i])[t] >= 1 - 1e-6
        flipped = vis[i].copy()
        flipped[m] = True
        assert weights(q[i, h], k[h], flipped)[m] > 0.999


@pytest.mark.parametrize("dtype", DTYPES)
def test_spread_rows_reach_the_gap(dtype):
    H, Hkv, L, n = 8, 2, 8000, 16
    q, k, v, vis, plan = planted(dtype, L, n, H, Hkv, 7, kinds=("spread",))
    split = P.tree_splits(L + n)
    for i, h in plan.cells():
        t = plan.keys[i][h][0]
        s = (k[h // 4] @ q[i, h]) * P.SCALE
        s[~torch.as_tensor(vis[i])] = float("-inf")
        others = torch.cat((s[:t], s[t + 1:]))
        assert s[t] - others.max() > 90                                  # every other key and split below 2^-126 in log2 units
        assert (s[t] - others.max()) / np.log(2) > 126
        assert len(set(split[vis[i]].tolist())) == P.SPLITS


@pytest.mark.parametrize("dtype", DTYPES)
def test_faults_are_seen_and_the_right_answer_is_not(dtype):
    """the self-check every GPU test runs: each planted cell's fault misses the reference by > 50x the tolerance"""
    H, Hkv, L, n = 8, 2, 1100, 64
    q, k, v, vis, plan = planted(dtype, L, n, H, Hkv, 11)
    want = P.reference(q, k, v, vis)
    P.self_check(plan, want, P.faulted(q, k, v, vis, plan, P.tree_splits(L + n)), dtype)
    assert not P.failures(want, want, plan, dtype, v)
    with pytest.raises(AssertionError):                                 # the identity is no fault
        P.self_check(plan, want, want, dtype)


def test_split_merge_reference_is_the_softmax_when_nothing_is_flagged():
    rng = np.random.default_rng(1)
    k, v = P.unit_rows(rng, (300,)), P.value_rows(rng, (300,))
    q = P.unit_rows(rng, (4,)) * 30
    q[0] = k[5] * 30                                                    # row 0: split 0 far above split 2
    vis = torch.ones((4, 300), dtype=torch.bool)
    exact = P.attend_head(q, k, v, vis)
    unit = torch.zeros((4, P.SPLITS + 1), dtype=torch.bool)
    unit[0, 2] = True                                                   # row 0 flagged; rows 1..3 must come out exact
    faulty = P.attend_head(q, k, v, vis, P.tree_splits(300), unit)
    assert torch.allclose(faulty[1:], exact[1:], rtol=0, atol=1e-12) and not torch.allclose(faulty[0], exact[0])


@pytest.mark.parametrize("n", [1, 2, 7, 63, 64, 65, 100, 127, 128])
def test_visibility_is_the_reference_tree_mask(n):
    from oracle import sam_oracle as O
    rng = np.random.default_rng(n)
    for shape in ("chain", "star", "bushy", "random"):
        anc = random_parents(rng, n, shape)
        m = O.gen_buffers(anc)["tree_attn_mask"][0, 0]
        L = int(rng.integers(0, 200))
        vis = P.tree_visibility(P.ancestor_rows(anc), L)
        assert vis[:, :L].all() and np.array_equal(vis[:, L:], m)
        words = P.mask_words(P.ancestor_rows(anc)).view(np.uint64)
        for i in range(n):
            bits = int(words[i]) | (int(words[128 + i]) << 64)
            assert [(bits >> j) & 1 for j in range(n)] == m[i].astype(int).tolist()


def test_causal_and_block_visibility():
    vis = P.causal_visibility(5, 3)
    assert vis.shape == (5, 8) and vis[0].tolist() == [True] * 4 + [False] * 4 and vis[4].all()
    b = P.block_visibility([0b101, 0b010], 10, 13)
    assert b[:, :10].all() and b[0, 10:].tolist() == [True, False, True] and b[1, 10:].tolist() == [False, True, False]
