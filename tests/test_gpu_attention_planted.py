"""Attention parity on PLANTED inputs (tests/attn_planting.py): every (row, head) is built so that one key, one mask bit or one merge weight
decides its output -- a needle at a tile seam, an anti-needle on a masked tree node or a future prompt key, two needles in different KV
splits, a needle far above every other key.  Each launch is held per (row, head) to a float64 reference of the dtype-rounded inputs,
|got - want|_inf <= tol * max(|want_row|_inf, 0.25) (fp16 2e-3, bf16 1.6e-2), every needle row must land on its key, and every case first
proves that the fault its plants target would miss that bar by more than 50x.

  samd_tree_attention / _vt          k_tree_attention (row-major V; V^T above SAMD_ATT_DIRECT_ROWS), k_tree_attention_direct, k_attn_combine
  samd_tree_attention_rope           k_tree_attention_rope + k_attn_combine_slots
  samd_attention_block               k_attn_block (also with a visible prefix shorter than the write position)
  samd_prefill_attention / _vt       k_prefill_attention
  SAMD_ATT_DIRECT_ROWS               0, 64 and 128 (clamped to 64: the direct kernel reads one mask word per row), each in a child process"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import attn_planting as P
import samd_hip
from samd_hip import _ptr
from util import random_parents

D = P.D
DTYPES = [torch.float16, torch.bfloat16]


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def expect(got, want, plan, dtype, v, label):
    msgs = P.failures(got, want, plan, dtype, v, label)
    assert not msgs, f"{len(msgs)} bad (row, head) cells; first: " + "\n".join(msgs[:12])


def cache_pair(rng, Hkv, max_len, live, dtype):
    """rounded float64 K (unit rows) and V on the GPU, plus the dtype tensors the kernels read with rows >= live NaN"""
    k = P.rounded(P.unit_rows(rng, (Hkv, max_len)), dtype).cuda()
    v = P.rounded(P.value_rows(rng, (Hkv, max_len)), dtype).cuda()
    return k, v


def to_kernel(x, live, dtype):
    t = x.to(dtype).clone()
    t[:, live:] = float("nan")                 # stale rows beyond the live range must never leak
    return t


def run_tree(q, kc, vc, mask, L, n, n_pad, H, Hkv, max_len, dtype, vt):
    lib, dc = samd_hip.lib(), samd_hip.torch_dtype_code(dtype)
    ws_bytes = lib.samd_tree_attention_workspace(n_pad, H, D)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda")           # NaN partials wherever a split does not write
    out = torch.full((n_pad, H, D), 7.0, device="cuda").to(dtype)
    d_L, d_n = dev([L]), dev([n])
    if vt:
        vtc = vc.transpose(1, 2).contiguous()
        samd_hip.check(lib.samd_tree_attention_vt(_ptr(q), _ptr(kc), _ptr(vtc), _ptr(out), dc, n_pad, H, Hkv, D, max_len, _ptr(mask), _ptr(d_L), _ptr(d_n),
                                                  P.SCALE, _ptr(ws), ws_bytes, None, samd_hip.current_stream()))
    else:
        samd_hip.check(lib.samd_tree_attention(_ptr(q), _ptr(kc), _ptr(vc), _ptr(out), dc, n_pad, H, Hkv, D, max_len, _ptr(mask), _ptr(d_L), _ptr(d_n),
                                               P.SCALE, _ptr(ws), ws_bytes, samd_hip.current_stream()))
    torch.cuda.synchronize()
    return out


def tree_case(dtype, H, Hkv, L, n, n_pad, max_len, shape, seed, plan=None):
    """planted q / K / V of one verify launch: (q64, k64, v64, vis, plan, split_of, mask)"""
    rng = np.random.default_rng(seed)
    anc = random_parents(rng, n, shape)
    rows = P.ancestor_rows(anc)
    K = L + n
    vis = P.tree_visibility(rows, L)
    split_of = P.tree_splits(K)
    k, v = cache_pair(rng, Hkv, max_len, K, dtype)
    if plan is None:
        plan = P.make_plan(rng, vis, H, Hkv, split_of, seams=P.seam_keys(L, n, max_len, (16 * 64 * 2 - 1,)), anti_prefer=(L + 63, L + 64, L + 127, L + n - 1))
    P.apply_negations(v, plan)
    q = P.rounded(P.plant_queries(plan, k, H, n_pad), dtype)
    mask = torch.tensor(P.mask_words(rows), device="cuda")
    return q, k, v, vis, plan, split_of, mask


def check_tree(dtype, H, Hkv, L, n, n_pad, max_len, shape, seed, layouts=(False, True), plan=None, self_check=True):
    q, k, v, vis, plan, split_of, mask = tree_case(dtype, H, Hkv, L, n, n_pad, max_len, shape, seed, plan)
    K = L + n
    want = P.reference(q, k, v, vis)
    if self_check:
        P.self_check(plan, want, P.faulted(q, k, v, vis, plan, split_of), dtype)
    qk = q.to(dtype).cuda()
    qk[n:] = float("nan")                      # padded query rows are ignored and zeroed
    kc, vc = to_kernel(k, K, dtype), to_kernel(v, K, dtype)
    outs = []
    for vt in layouts:
        out = run_tree(qk, kc, vc, mask, L, n, n_pad, H, Hkv, max_len, dtype, vt)
        expect(out[:n], want, plan, dtype, v[:, :K], f"{'V^T' if vt else 'rows'} L={L} n={n}/{n_pad}")
        assert (out[n:] == 0).all()
        outs.append(out)
    return outs


TREE_CASES = [
    # (H, Hkv, L, n, n_pad, max_len, shape)        n_pad <= 16 over V^T: the one-wave kernel; wider: the tiled kernel
    (32, 32, 0, 1, 8, 2048, "chain"), (32, 8, 1, 5, 8, 2048, "chain"), (32, 4, 63, 8, 8, 2048, "bushy"), (32, 8, 64, 16, 16, 2048, "random"),
    (32, 32, 65, 13, 16, 2048, "bushy"), (32, 8, 1023, 16, 16, 2048, "star"), (32, 8, 1024, 30, 32, 2048, "random"), (32, 4, 1025, 48, 48, 2048, "bushy"),
    (32, 8, 2047, 64, 64, 4096, "random"), (32, 8, 4097, 64, 64, 8192, "chain"), (32, 8, 8192 - 16, 16, 16, 8192, "bushy"),
    (32, 8, 8192 - 64, 64, 64, 8192, "random"), (32, 8, 8192 - 128, 128, 128, 8192, "bushy"),      # Llama-3's cache, its last key live
    (8, 2, 1000 - 48, 48, 48, 1000, "random"), (8, 8, 1000 - 16, 16, 16, 1000, "chain"), (4, 4, 0, 64, 64, 64, "bushy"),   # max_len % 64 != 0
    (32, 8, 928, 64, 64, 2048, "star"),        # split 15 holds nodes 32..63 only: rows 1..31 see no key of it
    (32, 8, 900, 128, 128, 2048, "star"), (16, 4, 64, 128, 128, 2048, "random"), (32, 32, 1023, 100, 128, 2048, "chain"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,Hkv,L,n,n_pad,max_len,shape", TREE_CASES)
def test_tree_attention_planted(dtype, H, Hkv, L, n, n_pad, max_len, shape):
    rows_out, vt_out = check_tree(dtype, H, Hkv, L, n, n_pad, max_len, shape, seed=L * 131 + n)
    assert torch.equal(rows_out, vt_out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [1000, 8000])
def test_tree_attention_every_cached_key_is_a_needle(dtype, L):
    """cell (row i, head h) of launch s aims at key (2048 s + 32 i + h) of its row's visible keys: every cached key is some cell's needle"""
    H, Hkv, n, max_len = 32, 8, 64, 8192
    vis = P.tree_visibility(P.ancestor_rows(random_parents(np.random.default_rng(L), n, "random")), L)
    for start in range(0, L, n * H):
        plan = P.every_key_plan(vis, H, start)
        check_tree(dtype, H, Hkv, L, n, n, max_len, "random", seed=L, plan=plan, layouts=(True,) if start else (False, True))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,n,n_pad", [(1500, 16, 16), (1500, 60, 64), (3000, 100, 128), (40, 8, 8)])
def test_tree_attention_score_spread(dtype, L, n, n_pad):
    """KV head 0: plain plants with needles 200 above everything (whole splits more than 90 nat below the best one, their merge weights
    flushed to zero); KV head 1: keys sharing one direction, so that every score of a row sits near -1e4 or near +1e4 with a needle 40
    above the rest -- without the running maximum the exponentials would underflow to 0 / overflow to inf"""
    H, Hkv, max_len = 8, 2, 4096
    rng = np.random.default_rng(L + n)
    rows = P.ancestor_rows(random_parents(rng, n, "bushy"))
    K = L + n
    vis = P.tree_visibility(rows, L)
    split_of = P.tree_splits(K)
    k, v = cache_pair(rng, Hkv, max_len, K, dtype)
    u = torch.full((D,), 1.0 / math.sqrt(D), dtype=torch.float64)
    r = P.unit_rows(rng, (max_len,))
    r = r - (r @ u)[:, None] * u
    r = r / r.norm(dim=-1, keepdim=True)
    k[1] = P.rounded(u + 0.5 * r, dtype).cuda()
    plan = P.make_plan(rng, vis, H, Hkv, split_of, seams=P.seam_keys(L, n, max_len), kinds=("spread", "needle", "two", "anti"))
    base = {}
    for i in range(n):
        for h in range(H // 2, H):
            t = plan.keys[i][h][0]
            plan.kind[i][h], plan.keys[i][h], plan.scores[i][h] = "needle", (t,), (P.NEEDLE,)
            base[(i, h)] = -1e4 if (i + h) % 2 else 1e4
    plan.negate = [x for x in plan.negate if x[0] == 0]
    P.apply_negations(v, plan)
    q = P.plant_queries(plan, k, H, n_pad)
    for (i, h), b in base.items():                   # span of (u, k_t): q . u * scale = b, q . k_t * scale = b + 40
        q[i, h] = P.query_for(torch.stack([u.cuda(), k[1, plan.keys[i][h][0]]]), (b, b + P.NEEDLE))
    q = P.rounded(q, dtype)
    assert q.abs().max().item() < 6e4
    want = P.reference(q, k, v, vis)
    P.self_check(plan, want, P.faulted(q, k, v, vis, plan, split_of), dtype)
    kc, vc = to_kernel(k, K, dtype), to_kernel(v, K, dtype)
    mask = torch.tensor(P.mask_words(rows), device="cuda")
    for vt in (False, True):
        out = run_tree(q.to(dtype).cuda(), kc, vc, mask, L, n, n_pad, H, Hkv, max_len, dtype, vt)
        assert torch.isfinite(out.float()).all()
        expect(out[:n], want, plan, dtype, v[:, :K], f"spread {'V^T' if vt else 'rows'}")


# ---- RoPE entry points: planted in post-RoPE space ----------------------------------------------------------------------------------------
def tables(max_pos):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.outer(torch.arange(max_pos, dtype=torch.float64), inv)
    return ang.cos().float().cuda().contiguous(), ang.sin().float().cuda().contiguous()


def unrotate(x, c, s):
    """float64 pre-RoPE rows whose HF rotate_half RoPE with (c, s) [.., 64] is x [.., 128]"""
    lo, hi = x[..., :64], x[..., 64:]
    return torch.cat((lo * c + hi * s, hi * c - lo * s), -1)


def rotate_like_kernel(x, c, s, dtype):
    """the kernels' fp32 RoPE of dtype rows x, rounded to dtype (arithmetic of k_rope_kv)"""
    x1, x2 = x[..., :64].float(), x[..., 64:].float()
    return torch.cat(((x1 * c - x2 * s).to(dtype), (x2 * c + x1 * s).to(dtype)), -1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,H,Hkv,Lw,vis_len,n,n_pad,shape", [
    ("rope", 32, 8, 1000, None, 60, 64, "bushy"), ("rope", 32, 32, 64, None, 16, 16, "chain"), ("rope", 8, 1, 1025, None, 33, 48, "random"),
    ("rope", 32, 4, 0, None, 8, 8, "star"), ("rope", 8, 2, 2047, None, 64, 64, "star"),
    ("block", 32, 8, 1000, 1000, 60, 64, "bushy"), ("block", 32, 32, 64, 64, 16, 16, "chain"), ("block", 8, 1, 1025, 1025, 33, 48, "random"),
    ("block", 32, 4, 0, 0, 8, 8, "star"), ("block", 32, 8, 777, 737, 16, 16, "bushy"), ("block", 8, 2, 300, 256, 20, 32, "random"),
    ("block", 32, 8, 4101, 4096, 8, 8, "chain")])
def test_rope_attention_entry_points_planted(dtype, kernel, H, Hkv, Lw, vis_len, n, n_pad, shape):
    """samd_tree_attention_rope (row-major V, 16 KV splits + the new keys' slot) and samd_attention_block (V^T; visible prefix vis_len,
    the rows of earlier tree levels at [vis_len, Lw) governed by the mask bits like the new ones)"""
    lib, dc, st = samd_hip.lib(), samd_hip.torch_dtype_code(dtype), samd_hip.current_stream()
    max_len = 8192
    rng = np.random.default_rng(Lw * 7 + n)
    earlier = 0 if vis_len is None else Lw - vis_len
    anc = random_parents(rng, n, shape)
    rows = [(int(sum(1 << j for j in range(earlier) if rng.random() < 0.4))) | (r << earlier) for r in P.ancestor_rows(anc)]
    base = Lw if vis_len is None else vis_len
    depth = [0] * n
    for i in range(1, n):
        depth[i] = depth[anc[i]] + 1
    K = Lw + n
    vis = P.tree_visibility(rows, Lw) if vis_len is None else P.block_visibility(rows, vis_len, K)
    split_of = np.where(np.arange(K) < Lw, (np.arange(K) // P.TILE) % (P.SPLITS if kernel == "rope" else 8), P.SPLITS if kernel == "rope" else 7)
    k, v = cache_pair(rng, Hkv, max_len, K, dtype)        # rows [Lw, Lw + n): the post-RoPE K wanted for the new keys
    plan = P.make_plan(rng, vis, H, Hkv, split_of, seams=P.seam_keys(Lw, n, max_len, (base - 1, base)), anti_prefer=(Lw + n - 1, Lw))
    P.apply_negations(v, plan)
    q_want = P.plant_queries(plan, k, H, n)
    cos, sin = tables(max_len)
    pos = torch.tensor([base + d for d in depth], device="cuda")
    c, s = cos[pos].double()[:, None, :], sin[pos].double()[:, None, :]
    W = (H + 2 * Hkv) * D
    rows_src = max(n_pad, 16)
    qkv = torch.zeros((rows_src, H + 2 * Hkv, D), dtype=torch.float64, device="cuda")
    qkv[:n, :H] = unrotate(q_want, c, s)
    qkv[:n, H:H + Hkv] = unrotate(k[:, Lw:K].transpose(0, 1), c, s)
    qkv[:n, H + Hkv:] = v[:, Lw:K].transpose(0, 1)
    src = qkv.view(rows_src, W).to(dtype)
    n_part = 2 if n % 2 else 0
    if n_part:                                            # fp32 split-K partials summing exactly to the same rows
        src = torch.stack((src.float() / 2, src.float() / 2)).contiguous()
    rel = torch.zeros(64, dtype=torch.int32, device="cuda")
    rel[:n] = torch.tensor(depth, dtype=torch.int32, device="cuda")
    mask = torch.tensor(P.mask_words(rows, 64)[:64], device="cuda")
    kc, vc = to_kernel(k, Lw, dtype), to_kernel(v, Lw, dtype)
    d_L, d_n, d_b = dev([Lw]), dev([n]), dev([base])
    cs = torch.zeros((64, D), dtype=torch.float32, device="cuda")
    samd_hip.check(lib.samd_rope_rows(_ptr(rel), _ptr(d_b), _ptr(cos), _ptr(sin), _ptr(cs), n_pad, D, max_len, st))
    out = torch.full((n_pad, H, D), 3.0, device="cuda").to(dtype)
    stride = rows_src * W if n_part else 0
    if kernel == "rope":
        ws = torch.full((lib.samd_tree_attention_rope_workspace(n_pad, H, D),), 0xFF, dtype=torch.uint8, device="cuda")
        samd_hip.check(lib.samd_tree_attention_rope(_ptr(src), n_part, stride, _ptr(cs), _ptr(kc), _ptr(vc), _ptr(out), dc, n_pad, H, Hkv, D, max_len,
                                                    _ptr(mask), _ptr(d_L), _ptr(d_n), P.SCALE, _ptr(ws), ws.numel(), st))
        v_new = vc[:, Lw:K]
    else:
        vtc = vc.transpose(1, 2).contiguous()
        samd_hip.check(lib.samd_attention_block(_ptr(src), n_part, stride, _ptr(cs), _ptr(kc), _ptr(vtc), _ptr(out), dc, n_pad, H, Hkv, D, max_len,
                                                _ptr(mask), _ptr(d_L), None if vis_len is None else _ptr(d_b), _ptr(d_n), P.SCALE, st))
        v_new = vtc[:, :, Lw:K].transpose(1, 2)
    torch.cuda.synchronize()
    # the reference is built from what the kernel wrote (K rows) and the q rows its RoPE produces; both close to the planted ones
    k_got = k.clone()
    k_got[:, Lw:K] = kc[:, Lw:K].double()
    assert torch.equal(v_new.double(), v[:, Lw:K])
    assert (k_got[:, Lw:K] - k[:, Lw:K]).abs().max().item() < 0.02
    qsrc = (src.sum(0) if n_part else src).to(dtype).view(rows_src, H + 2 * Hkv, D)[:n, :H]
    q = rotate_like_kernel(qsrc, c.float(), s.float(), dtype).double()
    want = P.reference(q, k_got, v, vis)
    P.self_check(plan, want, P.faulted(q, k_got, v, vis, plan, split_of), dtype)
    expect(out[:n], want, plan, dtype, v[:, :K], f"{kernel} Lw={Lw} n={n}")
    assert (out[n:] == 0).all()


# ---- prefill ------------------------------------------------------------------------------------------------------------------------------
def prefill_plan(rng, rows, pos0, H, total):
    """row r (position p = pos0 + r): needles at p, p - 1, 0 and a key of the previous 64-row block; anti-needles at p + 1 and inside the next
    64-key tile (future keys that exist: the prompt's later rows)"""
    plan = P.Plan(rows, H)
    for r in range(rows):
        p = pos0 + r
        for h in range(H):
            kind = (r + 3 * h) % 6
            if kind == 0 or (kind == 1 and p == 0):
                keys = (p,)
            elif kind == 1:
                keys = (p - 1,)
            elif kind == 2:
                keys = (0,)
            elif kind == 3:
                blk = p // 64
                keys = ((blk - 1) * 64 + int(rng.integers(0, 64)),) if blk > 0 else (int(rng.integers(0, p + 1)),)
            else:
                nxt = (p // 64 + 1) * 64 + (h * 7 + r) % 64
                m = p + 1 if kind == 4 else nxt
                if m >= total:
                    m = p + 1
                if m >= total:
                    plan.kind[r][h], plan.keys[r][h], plan.scores[r][h] = "needle", (p,), (P.NEEDLE,)
                    continue
                t = int(rng.integers(0, p + 1))
                plan.kind[r][h], plan.keys[r][h], plan.scores[r][h] = "anti", (t, m), (P.NEEDLE, P.ANTI)
                continue
            plan.kind[r][h], plan.keys[r][h], plan.scores[r][h] = "needle", keys, (P.NEEDLE,)
    plan.negate = []
    return plan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,pos0,H,Hkv,max_len", [(300, 0, 4, 4, 2048), (200, 37, 8, 2, 512), (1000, 0, 8, 8, 1024), (130, 5, 2, 1, 136),
                                                     (4096, 0, 32, 8, 4096), (1100, 64, 32, 32, 2048)])
def test_prefill_attention_planted(dtype, rows, pos0, H, Hkv, max_len):
    lib, dc, st = samd_hip.lib(), samd_hip.torch_dtype_code(dtype), samd_hip.current_stream()
    rng = np.random.default_rng(rows + pos0)
    total = pos0 + rows
    k, v = cache_pair(rng, Hkv, max_len, total, dtype)
    vis = P.causal_visibility(rows, pos0)
    plan = prefill_plan(rng, rows, pos0, H, total)
    q = P.rounded(P.plant_queries(plan, k, H), dtype)
    want = P.reference(q, k, v, vis)
    P.self_check(plan, want, P.faulted(q, k, v, vis, plan), dtype)
    qk, kc, vc = q.to(dtype).cuda(), to_kernel(k, total, dtype), to_kernel(v, total, dtype)
    o_rows, o_t = torch.full((rows, H, D), 7.0, device="cuda").to(dtype), torch.full((rows, H, D), 7.0, device="cuda").to(dtype)
    samd_hip.check(lib.samd_prefill_attention(_ptr(qk), _ptr(kc), _ptr(vc), _ptr(o_rows), dc, rows, pos0, H, Hkv, D, max_len, P.SCALE, st))
    samd_hip.check(lib.samd_prefill_attention_vt(_ptr(qk), _ptr(kc), _ptr(vc.transpose(1, 2).contiguous()), _ptr(o_t), dc, rows, pos0, H, Hkv, D, max_len,
                                                 P.SCALE, st))
    torch.cuda.synchronize()
    expect(o_rows, want, plan, dtype, v[:, :total], f"prefill rows={rows} pos0={pos0}")
    expect(o_t, want, plan, dtype, v[:, :total], f"prefill V^T rows={rows} pos0={pos0}")


# ---- SAMD_ATT_DIRECT_ROWS ------------------------------------------------------------------------------------------------------------------
DIRECT_ROWS_CASES = [(32, 8, 1000, 8, 8, "bushy"), (32, 8, 1025, 16, 16, "random"), (32, 8, 700, 30, 32, "bushy"), (32, 4, 64, 48, 48, "chain"),
                     (32, 8, 928, 64, 64, "star"), (16, 4, 64, 128, 128, "random"), (32, 8, 900, 128, 128, "star")]


def direct_rows_child():
    """run in a fresh process (the variable is read once per process): the planted V^T cases at every row bucket"""
    for dtype in DTYPES:
        for H, Hkv, L, n, n_pad, shape in DIRECT_ROWS_CASES:
            check_tree(dtype, H, Hkv, L, n, n_pad, 2048, shape, seed=L * 131 + n, layouts=(True,), self_check=False)
    print("direct rows child ok", flush=True)


@pytest.mark.parametrize("value", ["0", "64", "128"])
def test_direct_rows_setting_keeps_the_attention_right(value):
    """0: every bucket on the tiled kernel; 64: 32..64-row buckets on the one-wave kernel; 128: must behave like 64 (the one-wave kernel
    reads only the low mask word, so wider drafts may not take it)"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SAMD_ATT_DIRECT_ROWS=value)
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_attention_planted as t; t.direct_rows_child()"
            % (here, os.path.join(os.path.dirname(here), "sam-decoding_amd"), os.path.dirname(here)))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "direct rows child ok" in res.stdout, (res.returncode, res.stdout[-3000:], res.stderr[-3000:])
