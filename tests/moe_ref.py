"""Float64 restatement of the sparse MLP block of Qwen3-MoE (HF Qwen3MoeSparseMoeBlock) as the kernels state it (include/samd_hip.h,
samd_moe_route / samd_moe_gate_up_silu / samd_moe_down_combine):

  * router logits are the unrounded sums (float64 here, fp32 on the device) -- NOT rounded to the model dtype as HF's low-precision F.linear
    does, which manufactures exact ties;
  * the softmax runs in fp32 on those logits (HF: softmax(..., dtype=torch.float), whatever the module's dtype);
  * top-k by value, ties to the lower expert index; selected probabilities renormalised in fp32 when norm_topk_prob;
  * the weights are rounded once to the model dtype;
  * per (row, slot): down_e(silu(gate_e(x)) * up_e(x)), then out[row] = sum_j w[row, j] * y[row, j] in slot order j = 0 .. k - 1.

Test infrastructure only (CPU or GPU tensors)."""
import torch


def router_logits(h, router):
    return h.double() @ router.double().T


def route(h, router, k, norm_topk, dtype):
    """-> (logits float64 [R, E], idx int64 [R, k] in descending order of value, w [R, k] float64 holding values of `dtype`)"""
    logits = router_logits(h, router)
    probs = torch.softmax(logits.float(), dim=-1)
    idx = torch.argsort(-logits, dim=-1, stable=True)[:, :k]             # stable: equal values keep ascending expert order
    p = probs.gather(1, idx)
    if norm_topk:
        p = p / p.sum(dim=-1, keepdim=True)
    return logits, idx, p.to(dtype).double()


def experts(h, gate_up, down, idx, w, n=None):
    """the experts and the slot-order combine in float64: h [R, H], gate_up [E, 2 I, H], down [E, H, I], idx / w [R, k]; rows >= n are zero"""
    R, k = idx.shape
    n = R if n is None else n
    out = torch.zeros((R, h.shape[1]), dtype=torch.float64, device=h.device)
    x, gu, dn = h.double(), gate_up.double(), down.double()
    for r in range(n):
        for j in range(k):
            e = int(idx[r, j])
            if e < 0:
                continue
            g, u = (gu[e] @ x[r]).chunk(2)
            y = dn[e] @ (torch.nn.functional.silu(g) * u)
            out[r] = out[r] + w[r, j].double() * y
    return out


def experts_grouped(h, gate_up, down, idx, w, n=None):
    """the same sums, expert by expert (one matrix product per active expert): for shapes where the per-row loop is too slow"""
    R, k = idx.shape
    n = R if n is None else n
    y = torch.zeros((R, k, h.shape[1]), dtype=torch.float64, device=h.device)
    x = h.double()
    for e in idx[:n][idx[:n] >= 0].unique().tolist():
        rows, slots = torch.nonzero(idx[:n] == e, as_tuple=True)
        g, u = (x[rows] @ gate_up[e].double().T).chunk(2, dim=-1)
        y[rows, slots] = (torch.nn.functional.silu(g) * u) @ down[e].double().T
    out = torch.zeros((R, h.shape[1]), dtype=torch.float64, device=h.device)
    for j in range(k):
        out[:n] = out[:n] + w[:n, j:j + 1].double() * y[:n, j]
    return out


def block(h, router, gate_up, down, k, norm_topk, dtype):
    logits, idx, w = route(h, router, k, norm_topk, dtype)
    return experts(h, gate_up, down, idx, w), logits, idx, w


def accumulation_bound(h, router, unit_roundoff=2.0 ** -24):
    """gamma_K * sum_i |x_i| |w_i| per (row, expert): the classical bound on an fp32 dot product of K terms, whatever the summation order"""
    K = h.shape[1]
    gamma = K * unit_roundoff / (1 - K * unit_roundoff)
    return gamma * (h.double().abs() @ router.double().abs().T)


def decided_rows(h, router, k):
    """rows whose k-th / (k + 1)-th logit gap exceeds the fp32 accumulation bound of that row (the largest over its experts)"""
    logits = router_logits(h, router)
    srt = torch.sort(logits, dim=-1, descending=True).values
    bound = accumulation_bound(h, router).max(dim=-1).values
    if k >= logits.shape[1]:
        return torch.ones(logits.shape[0], dtype=torch.bool, device=h.device), bound
    return (srt[:, k - 1] - srt[:, k]) > bound, bound


def orthogonal_router(E, H, g, device, norm=2.0):
    """a router [E, H] (E <= H) with orthogonal rows of the given norm: a planted direction then moves its own logit only, so the spacing of
    the planted amplitudes is the spacing of the logits (random rows would add cross terms as large as the spacing)"""
    q, _ = torch.linalg.qr(torch.randn((H, E), generator=g, device=device, dtype=torch.float32))
    return q.T.contiguous() * norm


def planted_rows(router, R, k, g, noise=0.02, exclude=()):
    """router inputs whose logits have k + 2 spaced leaders: h = sum_j a_j * unit(router[e_j]) + noise, the amplitudes 0.5 apart (times the
    router rows' norm: far above the fp32 accumulation bound), so that the reference alone decides nearly every row.  g: a generator on
    the router's device; exclude: experts that are never planted."""
    E, H = router.shape
    pool = torch.tensor([e for e in range(E) if e not in exclude], device=router.device)
    dev = router.device
    unit = router.float() / router.float().norm(dim=-1, keepdim=True)
    h = torch.randn((R, H), generator=g, device=dev) * noise
    m = min(k + 2, len(pool))
    for r in range(R):
        es = pool[torch.randperm(len(pool), generator=g, device=dev)[:m]]
        amp = 2.0 + 0.5 * torch.arange(m, 0, -1, device=dev).float() + 0.1 * torch.rand(m, generator=g, device=dev)
        h[r] += (amp[:, None] * unit[es]).sum(0)
    return h


def ordered_rows(h, router, k):
    """decided rows whose every gap INSIDE the selection exceeds the bound too: there the slot order is fixed as well"""
    decided, bound = decided_rows(h, router, k)
    if k < 2:
        return decided
    srt = torch.sort(router_logits(h, router), dim=-1, descending=True).values
    return decided & ((srt[:, :k - 1] - srt[:, 1:k]) > bound[:, None]).all(dim=-1)
