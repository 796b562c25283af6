"""Planted attention inputs and their float64 reference (numpy + torch only; no product import).

Random q / k / v give scores of about N(0, 1): the softmax is nearly flat, the output is about the mean of the V rows, and one key dropped,
counted twice or leaked moves it by less than the fp16 / bf16 bars.  Here every (row, head) is PLANTED instead:

  needle       q = c k_t with c * scale = NEEDLE: key t takes >= 1 - 1e-6 of the weight (unit-norm keys: other scores ~ N(0, 3.5^2))
  two          q = c_a k_a + c_b k_b, scores NEEDLE + GAP and NEEDLE: weights ~0.73 / 0.27, a and b in different KV splits where there are
               several, and V[b] = -V[a], so that a wrong merge weight moves the output by a large fraction of its size
  anti         a visible needle at NEEDLE and a MASKED key at ANTI > NEEDLE: one wrong mask bit hands the masked key > 0.999 of the weight
  spread       a needle at SPREAD: every other key lies more than 90 natural-log units below it (weights under 2^-126 in the kernels'
               log2 domain, flushed to zero), and so do whole KV splits in the merge

Every plan also states the fault it is built to expose (`faulted`): the reference recomputed with the needle dropped, the anti-needle's mask
bit flipped, or the splits merged without their rescale factors -- and `self_check` asserts that this wrong answer misses the right one by
more than 50x the tolerance, so each test proves inside itself that it would fail on that fault."""
import math

import numpy as np
import torch

D = 128
SCALE = 1.0 / math.sqrt(D)
TILE, SPLITS = 64, 16
NEEDLE, ANTI, GAP, SPREAD = 40.0, 50.0, 1.0, 200.0
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
FLOOR = 0.25                                   # |want_row|_inf below this is held to tol * FLOOR
KINDS = ("needle", "two", "anti", "spread")


def rounded(x, dtype):
    """float64 tensor of the values `x` takes in `dtype`"""
    return torch.as_tensor(x).to(dtype).double()


def unit_rows(rng, shape):
    """float64 [..., D] rows of norm 1: two different rows have a dot product of about N(0, 1/128)"""
    x = rng.standard_normal(tuple(shape) + (D,))
    return torch.from_numpy(x / np.linalg.norm(x, axis=-1, keepdims=True))


def value_rows(rng, shape):
    """float64 [..., D] V rows: random sign x (1 + U[0, 0.5)) -- two rows differ by >= 2 wherever their signs do"""
    s = np.where(rng.random(tuple(shape) + (D,)) < 0.5, -1.0, 1.0)
    return torch.from_numpy(s * (1.0 + 0.5 * rng.random(tuple(shape) + (D,))))


# ---- visibility matrices: vis[i, k] = query row i may attend key k ------------------------------------------------------------------------
def ancestor_rows(anc):
    """per node the bit set of itself and its ancestors (python ints; bit j = node j), from a parent list (-1 = root)"""
    rows = []
    for i in range(len(anc)):
        r, j = 0, i
        while j >= 0:
            r |= 1 << j
            j = anc[j]
        rows.append(r)
    return rows


def mask_words(rows, n_words_rows=128):
    """u64 words as the kernels read them: the low words of all rows, then the high words (numpy int64 view)"""
    lo = [r & ((1 << 64) - 1) for r in rows] + [0] * (n_words_rows - len(rows))
    hi = [r >> 64 for r in rows] + [0] * (n_words_rows - len(rows))
    return np.array(lo + hi, dtype=np.uint64).view(np.int64)


def tree_visibility(rows, L, n_keys=None):
    """verify attention: every cached key < L, and new key L + j iff bit j of the row (both u64 words)"""
    n = len(rows)
    K = n_keys if n_keys is not None else L + n
    vis = np.zeros((n, K), dtype=bool)
    vis[:, :L] = True
    for i, r in enumerate(rows):
        for j in range(n):
            if (r >> j) & 1:
                vis[i, L + j] = True
    return vis


def block_visibility(rows, n_vis, n_keys):
    """samd_attention_block: keys < n_vis visible to every row, key n_vis + j iff bit j of the row"""
    vis = np.zeros((len(rows), n_keys), dtype=bool)
    vis[:, :n_vis] = True
    for i, r in enumerate(rows):
        for j in range(n_keys - n_vis):
            if (r >> j) & 1:
                vis[i, n_vis + j] = True
    return vis


def causal_visibility(rows, pos0):
    """prefill: the row at position pos0 + r sees keys 0 .. pos0 + r"""
    return np.arange(pos0 + rows)[None, :] <= (pos0 + np.arange(rows))[:, None]


def tree_splits(n_keys):
    """k_tree_attention: key k lies in tile k // 64, tile t in KV split t % 16"""
    return (np.arange(n_keys) // TILE) % SPLITS


# ---- planting -----------------------------------------------------------------------------------------------------------------------------
class Plan:
    """what every (row, head) was built to do: kind[i][h], keys[i][h] (the planted keys, first = the one the output should name),
    scores[i][h] (their designed scores, scale included)"""

    def __init__(self, n, H):
        self.kind = [[None] * H for _ in range(n)]
        self.keys = [[()] * H for _ in range(n)]
        self.scores = [[()] * H for _ in range(n)]

    def cells(self, kinds=KINDS):
        return [(i, h) for i in range(len(self.kind)) for h in range(len(self.kind[0])) if self.kind[i][h] in kinds]


def seam_keys(L, n, max_len, extra=()):
    """keys where tiling and masking go wrong: 0, the 64-key seams, 1024 (split 0's second tile), L - 1, L, L + n - 1, the cache's last"""
    c = [0, 1, 62, 63, 64, 65, 127, 128, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, L - 1, L, L + 1, L + 63, L + 64, L + n - 1, max_len - 1]
    c += list(extra)
    return sorted(set(k for k in c if 0 <= k < L + n))


def make_plan(rng, vis, H, Hkv, split_of=None, seams=(), kinds=KINDS, anti_prefer=()):
    """choose the planted keys of every (row, head) under visibility vis [n, K]: kinds cycle over the cells (so the heads of one GQA group
    get different kinds and targets); needles walk the seam keys first.  A kind that cannot be built (no masked key for an anti-needle,
    one visible key for two needles) falls back to a needle.  split_of[k]: the KV split / slot of key k (two needles go to different ones)."""
    n, K = vis.shape
    plan = Plan(n, H)
    seams = [k for k in seams if k < K]
    group = H // Hkv
    paired = [set() for _ in range(Hkv)]              # keys already in a two-needle pair of that KV head (V rows negated)
    negate = []                                       # (kvh, a, b): V[kvh, b] = -V[kvh, a]
    cursor = 0
    for i in range(n):
        visible = np.flatnonzero(vis[i])
        masked = np.flatnonzero(~vis[i])
        vseams = [k for k in seams if vis[i, k]]
        for h in range(H):
            kvh = h // group
            kind = kinds[(i * H + h + i // 7) % len(kinds)]
            cursor += 1
            t = vseams[cursor % len(vseams)] if vseams and cursor % 3 != 0 else int(rng.choice(visible))
            if kind == "anti" and len(masked) == 0:
                kind = "needle"
            if kind == "two":
                free = [k for k in visible if k not in paired[kvh]]
                if t in paired[kvh] and free:
                    t = int(rng.choice(free))
                others = [k for k in free if k != t]
                if split_of is not None:
                    far = [k for k in others if split_of[k] != split_of[t]]
                    others = far or others
                if t in paired[kvh] or not others:
                    kind = "needle"
                else:
                    b = int(rng.choice(others))
                    paired[kvh].update((t, b))
                    negate.append((kvh, t, b))
                    plan.kind[i][h], plan.keys[i][h], plan.scores[i][h] = kind, (t, b), (NEEDLE + GAP, NEEDLE)
                    continue
            if kind == "anti":
                pref = [k for k in anti_prefer if k < K and not vis[i, k]]
                m = pref[cursor % len(pref)] if pref and cursor % 2 == 0 else int(rng.choice(masked))
                plan.kind[i][h], plan.keys[i][h], plan.scores[i][h] = kind, (t, m), (NEEDLE, ANTI)
                continue
            score = SPREAD if kind == "spread" else NEEDLE
            plan.kind[i][h], plan.keys[i][h], plan.scores[i][h] = kind, (t,), (score,)
    plan.negate = negate
    return plan


def every_key_plan(vis, H, start):
    """needles only: cell c = i * H + h aims at visible key (start + c) mod |visible(i)| -- a few launches reach every key"""
    n = vis.shape[0]
    plan = Plan(n, H)
    for i in range(n):
        visible = np.flatnonzero(vis[i])
        for h in range(H):
            plan.kind[i][h], plan.keys[i][h], plan.scores[i][h] = "needle", (int(visible[(start + i * H + h) % len(visible)]),), (NEEDLE,)
    plan.negate = []
    return plan


def apply_negations(v, plan):
    for kvh, a, b in plan.negate:
        v[kvh, b] = -v[kvh, a]
    return v


def query_for(keys_rows, scores):
    """q in the span of the planted (rounded) K rows with q . k_j * SCALE = scores[j]"""
    G = keys_rows @ keys_rows.T
    c = torch.linalg.solve(G, torch.tensor(scores, dtype=torch.float64, device=keys_rows.device) / SCALE)
    return c @ keys_rows


def plant_queries(plan, k, H, n_pad=None):
    """float64 q [n_pad, H, D] from the plan over K rows k [Hkv, K, D] (already rounded to the dtype); rows >= n are zero.
    Cells with the same number of planted keys are solved as one batch."""
    n = len(plan.kind)
    Hkv = k.shape[0]
    q = torch.zeros((n_pad or n, H, D), dtype=torch.float64, device=k.device)
    by_m = {}
    for i in range(n):
        for h in range(H):
            by_m.setdefault(len(plan.keys[i][h]), []).append((i, h))
    for m, cells in by_m.items():
        ii = torch.tensor([c[0] for c in cells], device=k.device)
        hh = torch.tensor([c[1] for c in cells], device=k.device)
        keys = torch.tensor([plan.keys[i][h] for i, h in cells], device=k.device)                          # [N, m]
        sc = torch.tensor([plan.scores[i][h] for i, h in cells], dtype=torch.float64, device=k.device)     # [N, m]
        rows = k[(hh // (H // Hkv))[:, None], keys]                                                          # [N, m, D]
        c = torch.linalg.solve(rows @ rows.transpose(1, 2), sc / SCALE)
        q[ii, hh] = (c[:, None, :] @ rows)[:, 0]
    return q


# ---- float64 reference --------------------------------------------------------------------------------------------------------------------
def attend_head(q, k, v, vis, split_of=None, unit_weight=None):
    """softmax(q k^T * SCALE, masked by vis) v for one head, float64.  q [n, D], k / v [K, D], vis [n, K] bool tensor.
    split_of [K] + unit_weight [n, S] bool: the merge of per-split partials with the rescale factor of the flagged splits replaced by 1
    (the fault a merge without its exp2(m_s - M) makes); rows without a flag are exact."""
    s = (q @ k.T) * SCALE
    s = s.masked_fill(~vis, float("-inf"))
    out = torch.softmax(s, dim=-1) @ v
    if unit_weight is None or not bool(unit_weight.any()):
        return out
    unit_weight = unit_weight.to(s.device)
    rows = torch.nonzero(unit_weight.any(1)).flatten()
    S = unit_weight.shape[1]
    sr = s[rows]
    num = torch.zeros((len(rows), k.shape[1]), dtype=s.dtype, device=s.device)
    den = torch.zeros(len(rows), dtype=s.dtype, device=s.device)
    parts = []
    for sp in range(S):
        sel = torch.as_tensor(split_of == sp, device=s.device)
        ss = sr.masked_fill(~sel[None, :], float("-inf"))
        m = ss.max(1).values
        ok = torch.isfinite(m)
        p = torch.where(ok[:, None], torch.exp(ss - torch.where(ok, m, 0.0)[:, None]), 0.0)
        parts.append((m, ok, p.sum(1), p @ v))
    M = torch.stack([m for m, _, _, _ in parts]).max(0).values
    for sp, (m, ok, l_, o_) in enumerate(parts):
        w = torch.where(unit_weight[rows, sp], torch.ones_like(m), torch.exp(torch.where(ok, m - M, -1e300)))
        w = torch.where(ok, w, 0.0)
        num += w[:, None] * o_
        den += w * l_
    out = out.clone()
    out[rows] = num / den[:, None]
    return out


def reference(q, k, v, vis):
    """float64 [n, H, D]: q [n(_pad), H, D], k / v [Hkv, >= K, D], vis [n, K] (numpy bool); head by head"""
    n, K = vis.shape
    H, Hkv = q.shape[1], k.shape[0]
    dev = k.device
    vt = torch.as_tensor(vis, device=dev)
    out = torch.empty((n, H, D), dtype=torch.float64, device=dev)
    for h in range(H):
        kvh = h // (H // Hkv)
        out[:, h] = attend_head(q[:n, h].to(dev), k[kvh, :K], v[kvh, :K], vt)
    return out


def faulted(q, k, v, vis, plan, split_of=None):
    """the reference under the fault each planted cell targets: needle -> its key dropped; anti -> the masked key's bit flipped;
    two -> b's split merged with weight 1 (where a and b lie in different splits; else b dropped); spread -> every split merged with
    weight 1 (where the row's keys span several splits; else the needle dropped)"""
    n, K = vis.shape
    H, Hkv = q.shape[1], k.shape[0]
    dev = k.device
    out = torch.empty((n, H, D), dtype=torch.float64, device=dev)
    for h in range(H):
        kvh = h // (H // Hkv)
        vf = vis.copy()
        unit = np.zeros((n, SPLITS + 1), dtype=bool)
        for i in range(n):
            kind, keys = plan.kind[i][h], plan.keys[i][h]
            if kind == "needle":
                vf[i, keys[0]] = False
            elif kind == "anti":
                vf[i, keys[1]] = True
            elif kind == "two":
                if split_of is not None and split_of[keys[0]] != split_of[keys[1]]:
                    unit[i, split_of[keys[1]]] = True
                else:
                    vf[i, keys[1]] = False
            elif kind == "spread":
                if split_of is not None and len(set(split_of[np.flatnonzero(vis[i])].tolist())) > 1:
                    unit[i, :] = True
                else:
                    vf[i, keys[0]] = False
        out[:, h] = attend_head(q[:n, h].to(dev), k[kvh, :K], v[kvh, :K], torch.as_tensor(vf, device=dev),
                                split_of, torch.as_tensor(unit) if unit.any() else None)
    return out


def row_errors(got, want, dtype):
    """per (row, head): |got - want|_inf / (tol * max(|want_row|_inf, FLOOR))  -- > 1 fails"""
    bar = TOL[dtype] * torch.clamp(want.abs().amax(-1), min=FLOOR)
    return (got.double() - want).abs().amax(-1) / bar


def nearest_keys(out, v, H, n_keys):
    """[n, H]: the key whose V row is closest (L2) to each output row (v [Hkv, >= n_keys, D])"""
    Hkv = v.shape[0]
    res = torch.empty(out.shape[:2], dtype=torch.long)
    for h in range(H):
        kvh = h // (H // Hkv)
        res[:, h] = torch.cdist(out[:, h].double(), v[kvh, :n_keys].double()).argmin(-1).cpu()
    return res


def self_check(plan, want, wrong, dtype, factor=50.0):
    """every planted cell's targeted fault must move the output by more than `factor` times the tolerance"""
    r = torch.nan_to_num(row_errors(wrong, want, dtype).cpu(), nan=float("inf"))     # a row left with no key at all: NaN, certainly seen
    weak =[(i, h, plan.kind[i][h], round(float(r[i, h]), 1)) for i, h in plan.cells() if not r[i, h] > factor]
    assert not weak, f"planted cells whose fault the tolerance would not see (row, head, kind, x tol): {weak[:8]}"


def failures(got, want, plan, dtype, v, label=""):
    """messages for every (row, head) beyond the bar, and for every needle row whose output is not nearest the intended key's V row"""
    got = got.double().to(want.device)
    msgs = []
    if not torch.isfinite(got).all():
        bad = torch.nonzero(~torch.isfinite(got).all(-1))[:8].tolist()
        msgs.append(f"{label}: non-finite output at (row, head) {bad}")
    r = torch.nan_to_num(row_errors(got, want, dtype), nan=float("inf")).cpu().tolist()
    n, H = len(r), len(r[0])
    near = nearest_keys(torch.nan_to_num(got), v, H, v.shape[1]).tolist()
    for i in range(n):
        for h in range(H):
            kind, keys = plan.kind[i][h], plan.keys[i][h]
            named = kind in ("needle", "anti", "spread") and near[i][h] != keys[0]
            if r[i][h] > 1 or named:
                msgs.append(f"{label}: row {i}, head {h} ({kind}, keys {[int(x) for x in keys]}): error {r[i][h]:.2f} x tol, "
                            f"attended key {near[i][h]}, expected {int(keys[0])}")
    return msgs
