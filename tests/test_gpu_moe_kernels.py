"""The mixture-of-experts kernels (include/samd_hip.h: samd_moe_route, samd_moe_gate_up_silu, samd_moe_down_combine) against the float64
restatement tests/moe_ref.py on the same inputs.

Router: a row is DECIDED when the float64 gap between its k-th and (k + 1)-th logit exceeds the fp32 accumulation bound
gamma_K * sum |x_i| |w_i| of that row (the largest over the row's experts); the bound comes from the
inputs, never from the kernel.  On a decided row the indices equal the reference's slot by slot and every weight is within 1 ulp of the
model dtype.  The inputs are planted (tests/moe_ref.py: a router with orthogonal rows; a row is a mix of k + 2 router directions with
amplitudes 0.5 apart, plus noise) so that the reference alone leaves at most 2 % of the rows undecided AND no decided row with two selected logits closer
than the bound (asserted here, and on CPU in tests/test_moe_cpu.py); on an undecided row the selection may differ only among experts
inside the bound.  Two router rows are bitwise equal: that exact tie must go to the lower expert.

Expert GEMMs: pinned routing, error against float64 compared with the error HF's own Qwen3MoeExperts.forward makes in the model dtype on the
same GPU (ours <= 1.5 x that + 0.02 x max|out|, the margin of test_gpu_qwen.py)."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import samd_hip
from samd_hip import moe as MOE
import moe_ref as M

DT = {torch.float16: samd_hip.F16, torch.bfloat16: samd_hip.BF16}


def buffers(RP, H, I, E, k, dtype):
    return MOE.MoeBuffers(RP, H, I, E, k, dtype, DT[dtype], "cuda")


def d_int(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


planted_rows = M.planted_rows


def ulp(x, dtype):
    bits = 10 if dtype == torch.float16 else 7
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - bits)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("norm_topk", [True, False])
@pytest.mark.parametrize("E,k,H,RP,n", [(128, 8, 2048, 64, 64), (128, 8, 2048, 48, 37), (8, 2, 512, 16, 9), (64, 4, 1024, 32, 32), (256, 8, 768, 16, 1)])
def test_router_matches_the_reference(dtype, norm_topk, E, k, H, RP, n):
    g = torch.Generator(device="cuda").manual_seed(E + k + n)
    router = M.orthogonal_router(E, H, g, "cuda").to(dtype)
    tie = n >= 50                                                 # (one row in 64: within the 2 % of undecided rows)
    if tie:
        router[5] = router[3]                                     # an exact tie whenever both lead
    h = planted_rows(router, RP, k, g, exclude=(3, 5) if tie else ())     # (the twins lead in row 2 only)
    if tie:                                                       # row 2: expert 3 (and its twin 5) exactly at the k-th place
        unit = router.float() / router.float().norm(dim=-1, keepdim=True)
        others = [e for e in range(E) if e not in (3, 5)][:k - 1]
        h[2] = torch.randn(H, generator=g, device="cuda") * 0.02 + 3.0 * unit[3] + sum((6.0 + i) * unit[e] for i, e in enumerate(others))
    h = h.to(dtype)
    h_poison = h.clone()
    h_poison[n:] = float("nan")
    b = buffers(RP, H, 256, E, k, dtype)
    b.topk_idx.fill_(12345), b.topk_w.fill_(float("nan")), b.ws.fill_(0xFF)
    b.route(h_poison, router, d_int(n), norm_topk)
    torch.cuda.synchronize()
    logits, idx, w = M.route(h[:n], router, k, norm_topk, dtype)
    decided, bound = M.decided_rows(h[:n], router, k)
    srt = torch.sort(logits, dim=-1, descending=True).values
    ordered = M.ordered_rows(h[:n], router, k)
    und = int((~decided).sum())
    print(f"E={E} k={k} H={H} n={n} {dtype}: undecided rows {und}, rows with an undecided order {int((~ordered).sum())}, "
          f"median k-th gap {float((srt[:, k - 1] - srt[:, min(k, E - 1)]).median()):.4f}, max bound {float(bound.max()):.2e}")
    assert und <= 0.02 * n, und
    # the planted leaders are spaced far above the bound: a decided row's slot order is decided too, so indices are compared as they are
    assert torch.equal(ordered, decided), "the planted inputs must leave no decided row with an undecided order"
    got_i, got_w = b.topk_idx[:n].long(), b.topk_w[:n].double()
    # rows past n: no index, no weight
    assert bool((b.topk_idx[n:] == -1).all()) and bool((b.topk_w[n:] == 0).all())
    assert bool(((got_i >= 0) & (got_i < E)).all())
    assert torch.equal(got_i[decided], idx[decided]), "indices, slot by slot, on every decided row"
    # weights slot by slot, 1 ulp of the model dtype
    err = (got_w - w).abs()[decided]
    assert bool((err <= ulp(w[decided], dtype).double() * 1.0001).all()), float(err.max())
    # undecided rows: the selection differs only among experts inside the bound
    for r in torch.nonzero(~decided).flatten().tolist():
        a, c = set(got_i[r].tolist()), set(idx[r].tolist())
        for e in a ^ c:
            assert srt[r, k] - bound[r] <= logits[r, e] <= srt[r, k - 1] + bound[r], (r, e)
    if tie:                                                       # the exact tie of row 2 goes to the lower expert
        assert 3 in got_i[2].tolist() and 5 not in got_i[2].tolist(), got_i[2].tolist()
    # the lists: every (row, slot) of a row < n once, under its expert, ascending; nothing else
    n_active, active, counts, lists = b.routing_state()
    flat = b.topk_idx.flatten().tolist()
    assert active == sorted(set(flat[:n * k])) and n_active <= min(E, RP * k)
    for e, c, lst in zip(active, counts, lists):
        assert lst == [p for p in range(n * k) if flat[p] == e] and c == len(lst)


def hf_experts(E, H, I, gate_up, down, dtype):
    from transformers import Qwen3MoeConfig
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts
    cfg = Qwen3MoeConfig(hidden_size=H, moe_intermediate_size=I, num_experts=E)
    with torch.device("meta"):
        ex = Qwen3MoeExperts(cfg)
    ex.gate_up_proj = torch.nn.Parameter(gate_up.to(dtype), requires_grad=False)
    ex.down_proj = torch.nn.Parameter(down.to(dtype), requires_grad=False)
    return ex


def pinned(case, R, E, k, g):
    if case == "one_expert_all_rows":                             # expert 3 takes every row (slot 0); the other slots are spread
        idx = torch.stack([torch.full((R,), 3)] + [(4 + (torch.arange(R) + 5 * j) % (E - 4)) for j in range(1, k)], dim=1)
    elif case == "all_distinct":                                  # R * k = E active experts: the grid's upper bound itself
        idx = torch.arange(R * k).reshape(R, k) % E
    else:
        idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(R)])
    return idx.to(device="cuda", dtype=torch.int32)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case,E,k,H,I,RP,n", [
    ("one_expert_all_rows", 16, 2, 512, 256, 64, 64),
    ("all_distinct", 128, 2, 512, 256, 64, 64),
    ("all_distinct", 128, 8, 2048, 768, 16, 16),
    ("random", 128, 8, 2048, 768, 64, 64),
    ("random", 128, 8, 2048, 768, 16, 1),
    ("random", 8, 2, 1024, 1792, 48, 41),
    ("random", 32, 4, 512, 512, 32, 20),
])
def test_expert_gemms_with_pinned_routing(dtype, case, E, k, H, I, RP, n):
    """the expert launches against HF's own experts at workload statistics (randn inputs): error <= 1.5 x HF's + 0.02 x max|out|.  That bar
    says how the kernels compare with HF, not that they are exact: what every launch must store, bit for bit, is held by
    tests/test_gpu_moe_exact.py"""
    gc = torch.Generator().manual_seed(E * k + n)
    g = torch.Generator(device="cuda").manual_seed(E * k + n)
    gate_up = (torch.randn((E, 2 * I, H), generator=g, device="cuda") * 0.05).to(dtype)
    down = (torch.randn((E, H, I), generator=g, device="cuda") * 0.05).to(dtype)
    h = torch.randn((RP, H), generator=g, device="cuda").to(dtype)
    h[n:] = float("nan")
    idx = pinned(case, RP, E, k, gc)
    w = torch.rand((RP, k), generator=g, device="cuda") + 0.1
    w = (w / w.sum(-1, keepdim=True)).to(dtype)
    pgu, pd = MOE.pack_experts(gate_up, down)
    b = buffers(RP, H, I, E, k, dtype)
    b.topk_idx.copy_(idx), b.topk_w.copy_(w)
    b.act.fill_(float("nan")), b.ws.fill_(0xFF), b.out.fill_(float("nan"))
    b.lists(d_int(n))
    out = b.experts(h, pgu, pd, d_int(n))
    torch.cuda.synchronize()
    n_active = b.routing_state()[0]
    assert n_active == len(set(idx[:n].flatten().tolist()))
    want = M.experts_grouped(h[:n], gate_up, down, idx[:n].long(), w[:n])
    with torch.no_grad():
        hf = hf_experts(E, H, I, gate_up, down, dtype)(h[:n], idx[:n].long(), w[:n]).double()
    e_ours, e_hf, scale = (out[:n].double() - want).abs().max().item(), (hf - want).abs().max().item(), want.abs().max().item()
    print(f"{case} E={E} k={k} H={H} I={I} rows {n}/{RP} {dtype}: active {n_active}, ours {e_ours:.5f}, HF {dtype} {e_hf:.5f}, max|out| {scale:.3f}")
    assert bool(torch.isfinite(out[:n]).all()) and bool((out[n:] == 0).all())
    assert e_ours <= 1.5 * e_hf + 0.02 * scale, (e_ours, e_hf, scale)


def test_entries_the_lists_leave_out_add_nothing():
    """externally decided routing through samd_moe_lists: an index outside [0, E) and a repetition of an expert within a row are ignored by
    the lists and by the combine alike -- the output is that of the same routing with those slots empty, whatever y held before"""
    E, k, H, I, RP, n, dtype = 16, 4, 512, 256, 16, 12, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(3)
    gate_up = (torch.randn((E, 2 * I, H), generator=g, device="cuda") * 0.05).to(dtype)
    down = (torch.randn((E, H, I), generator=g, device="cuda") * 0.05).to(dtype)
    h = torch.randn((RP, H), generator=g, device="cuda").to(dtype)
    pgu, pd = MOE.pack_experts(gate_up, down)
    clean = pinned("random", RP, E, k, torch.Generator().manual_seed(3))
    dirty = clean.clone()
    dirty[0, 2], dirty[3, 1], dirty[5, 3], dirty[7, 0] = E + 3, dirty[3, 0], 4096, -7
    clean[0, 2] = clean[3, 1] = clean[5, 3] = clean[7, 0] = -1
    w = torch.full((RP, k), 0.25, dtype=dtype, device="cuda")
    outs = []
    for idx in (clean, dirty):
        b = buffers(RP, H, I, E, k, dtype)
        b.topk_idx.copy_(idx), b.topk_w.copy_(w)
        b.act.fill_(float("nan")), b.ws.fill_(0xFF)
        b.lists(d_int(n))
        outs.append(b.experts(h, pgu, pd, d_int(n)).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[1]).all()) and torch.equal(outs[0], outs[1])
    want = M.experts_grouped(h[:n], gate_up, down, clean[:n].long(), w[:n])
    assert (outs[1][:n].double() - want).abs().max().item() <= 0.03 * want.abs().max().item()


def run_block(h_rows, RP, router, pgu, pd, E, k, H, I, dtype, poison=False):
    n = h_rows.shape[0]
    h = torch.zeros((RP, H), dtype=dtype, device="cuda")
    h[:n] = h_rows
    b = buffers(RP, H, I, E, k, dtype)
    if poison:
        h[n:] = float("nan")
        b.act.fill_(float("nan")), b.ws.fill_(0xFF), b.out.fill_(float("nan")), b.topk_w.fill_(float("nan")), b.topk_idx.fill_(777)
    b.route(h, router, d_int(n), True)
    out = b.experts(h, pgu, pd, d_int(n)).clone()
    torch.cuda.synchronize()
    return out, b


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,k,H,I", [(32, 4, 512, 256), (128, 8, 2048, 768)])
def test_a_rows_output_does_not_depend_on_its_company(dtype, E, k, H, I):
    g = torch.Generator(device="cuda").manual_seed(7)
    router = (torch.randn((E, H), generator=g, device="cuda") * 0.05).to(dtype)
    gate_up = (torch.randn((E, 2 * I, H), generator=g, device="cuda") * 0.05).to(dtype)
    down = (torch.randn((E, H, I), generator=g, device="cuda") * 0.05).to(dtype)
    pgu, pd = MOE.pack_experts(gate_up, down)
    rows = torch.randn((64, H), generator=g, device="cuda").to(dtype)
    rows[1:] = rows[1:] * 0.5 + rows[0] * 0.5                    # the others lean towards the same experts: shared tiles
    args = (router, pgu, pd, E, k, H, I, dtype)
    alone = run_block(rows[:1], 16, *args)[0][0]
    assert bool(alone.abs().max() > 0)
    assert torch.equal(run_block(rows[:8], 16, *args)[0][0], alone), "with 7 others"
    assert torch.equal(run_block(rows[:64], 64, *args)[0][0], alone), "with 63 others"
    assert torch.equal(run_block(rows[:33], 48, *args)[0][0], alone), "with 32 others (48-row tile)"
    moved = torch.cat([rows[1:6], rows[:1], rows[6:8]])
    assert torch.equal(run_block(moved, 16, *args)[0][5], alone), "at position 5 of 8"
    moved = torch.cat([rows[1:41], rows[:1], rows[41:64]])
    assert torch.equal(run_block(moved, 64, *args)[0][40], alone), "at position 40 of 64"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("RP,n", [(16, 5), (64, 50)])
def test_poisoned_padding_and_workspaces_leave_no_trace(dtype, RP, n):
    E, k, H, I = 64, 4, 1024, 512
    g = torch.Generator(device="cuda").manual_seed(n)
    router = (torch.randn((E, H), generator=g, device="cuda") * 0.05).to(dtype)
    gate_up = (torch.randn((E, 2 * I, H), generator=g, device="cuda") * 0.05).to(dtype)
    down = (torch.randn((E, H, I), generator=g, device="cuda") * 0.05).to(dtype)
    pgu, pd = MOE.pack_experts(gate_up, down)
    rows = torch.randn((n, H), generator=g, device="cuda").to(dtype)
    clean, b0 = run_block(rows, RP, router, pgu, pd, E, k, H, I, dtype)
    dirty, b1 = run_block(rows, RP, router, pgu, pd, E, k, H, I, dtype, poison=True)
    assert bool(torch.isfinite(dirty).all()) and torch.equal(dirty, clean) and bool((dirty[n:] == 0).all())
    assert torch.equal(b0.topk_idx, b1.topk_idx) and torch.equal(b0.topk_w, b1.topk_w)
    assert b0.routing_state() == b1.routing_state()


def test_unsupported_shapes_raise():
    for kw in (dict(hidden=500), dict(moe_inter=300), dict(n_experts=257), dict(top_k=9), dict(n_experts=4, top_k=8)):
        a = dict(hidden=512, moe_inter=256, n_experts=8, top_k=2)
        a.update(kw)
        with pytest.raises(samd_hip.SamdError):
            MOE.check_shape(**a)
    b = buffers(16, 512, 256, 8, 2, torch.float16)
    b.rows_pad = 24
    with pytest.raises(samd_hip.SamdError, match="rows 16/32/48/64"):
        b.lists(d_int(1))
