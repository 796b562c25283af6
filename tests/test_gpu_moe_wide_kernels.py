"""The wide mixture-of-experts calls (include/samd_hip.h: samd_moe_wide_route, _lists, _gate_up_silu, _down_combine) on their own: many rows
in one launch, an expert's list served in several 64-row tiles.

  lists, tile table    against the plain Python restatement samd_hip.moe.wide_lists_reference, by equality, the tile count included; the
                       routing part of the workspace byte for byte over two runs
  outputs              every real row torch.equal to what the EXISTING <= 64-row calls (MoeBuffers(64, ...): samd_moe_lists + the two expert
                       launches of the format) return for the same rows with the same topk_idx / topk_w, 64-row slice by slice -- for the
                       model dtype, mxfp4, int4g128 and fp8b128 experts
  torch reference      tests/moe_ref.py in float64 at the bar tests/test_gpu_moe_kernels.py sets for pinned routing: ours <= 1.5 x the error
                       of HF's own experts in the model dtype + 0.02 x max|out|
  exact integers       the planted inputs of tests/moe_planting.py (its 64-row "counts" routing and its draws, stacked three times with
                       another draw per block: counts 3 .. 189, up to three tiles per expert) against its float64 references, bit for bit
  row independence     a row's bits at rows = 65, inside rows = 192, and at another position

Planted routing: E = 8, k = 2, rows = 160 with the per-expert counts [0, 1, 63, 64, 65, 127, 0, 0] -- an expert with nothing, one entry,
one short of a tile, exactly a tile, one over, one short of two tiles -- asserted on the host before anything runs; the same with
*d_n = 100 < rows, a row that repeats an expert and rows with out-of-range indices; E = 128, k = 8, rows = 192 routed by samd_moe_wide_route
on random states (its indices and weights must equal samd_moe_route's, slice by slice)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import moe as MOE
import moe_ref as M

DT = {torch.float16: samd_hip.F16, torch.bfloat16: samd_hip.BF16}
H, I, T = 256, 256, 64
FORMATS = [None, "mxfp4", "int4g128", "fp8b128"]
COUNTS = [0, 1, 63, 64, 65, 127, 0, 0]
NAN = float("nan")


def d_int(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def planted_idx():
    """[160, 2] int32: every row two distinct experts, expert e in COUNTS[e] rows; the larger experts first, each to the least loaded rows;
    the slots ascending on even rows and descending on odd ones"""
    rows, k = sum(COUNTS) // 2, 2
    idx, load = np.full((rows, k), -1, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    for e in sorted(range(len(COUNTS)), key=lambda i: -COUNTS[i]):
        take = np.argsort(load, kind="stable")[:COUNTS[e]]
        assert COUNTS[e] == 0 or load[take].max() < k
        idx[take, load[take]] = e
        load[take] += 1
    idx = np.sort(idx, axis=1)
    idx[1::2] = idx[1::2, ::-1]
    assert rows == 160 and bool((idx >= 0).all()) and bool((idx[:, 0] != idx[:, 1]).all())
    assert np.bincount(idx.reshape(-1), minlength=len(COUNTS)).tolist() == COUNTS
    return torch.from_numpy(idx.astype(np.int32))


def dirty_idx():
    """the planted routing with a repeated expert (row 3), an index >= E (row 7), a negative one (row 9) and one far outside (row 98)"""
    idx = planted_idx()
    idx[3, 1] = idx[3, 0]
    idx[7, 1], idx[9, 0], idx[98, 0] = 8, -7, 4096
    return idx


@functools.lru_cache(maxsize=None)
def weights(E, dtype):
    g = torch.Generator(device="cuda").manual_seed(100 + E)
    gate_up = (torch.randn((E, 2 * I, H), generator=g, device="cuda") * 0.05).to(dtype)
    down = (torch.randn((E, H, I), generator=g, device="cuda") * 0.05).to(dtype)
    return gate_up, down


@functools.lru_cache(maxsize=None)
def packed(E, dtype, fmt):
    gate_up, down = weights(E, dtype)
    if fmt is None:
        return MOE.pack_experts(gate_up, down)
    if fmt == "mxfp4":
        return MOE.pack_experts_mxfp4(*MOE.quantize_experts(gate_up, down, dtype))
    if fmt == "int4g128":
        return MOE.pack_experts_int4(*MOE.quantize_experts_int4(gate_up, down, dtype), dtype)
    return MOE.pack_experts_fp8(*MOE.quantize_experts_fp8(gate_up, down))


def states(rows, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((MOE.wide_rows_pad(rows), H), generator=g, device="cuda").to(dtype)


def mix_weights(rows_pad, k, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.rand((rows_pad, k), generator=g, device="cuda") + 0.1
    return (w / w.sum(-1, keepdim=True)).to(dtype)


def wide_buffers(rows, E, k, dtype, poison=True):
    b = MOE.MoeWideBuffers(rows, H, I, E, k, dtype, DT[dtype], "cuda")
    if poison:
        b.act.fill_(NAN), b.out.fill_(NAN), b.ws.fill_(0xFF)
        y_off = samd_hip.lib().samd_moe_wide_workspace_layout(7, rows, k)
        b.ws[y_off:].view(dtype).fill_(NAN)
    return b


def run_wide(h, idx, w, n, E, dtype, fmt, rows=None):
    rows = idx.shape[0] if rows is None else rows
    k = idx.shape[1]
    b = wide_buffers(rows, E, k, dtype)
    b.topk_idx[:idx.shape[0]].copy_(idx), b.topk_w[:idx.shape[0]].copy_(w[:idx.shape[0]])
    b.lists(d_int(n))
    out = b.experts(h, *packed(E, dtype, fmt), d_int(n), fmt)
    torch.cuda.synchronize()
    return out, b


def run_narrow(h, idx, w, n, E, dtype, fmt):
    """the existing <= 64-row calls, 64-row slice by slice, on the same rows: the yardstick"""
    k, outs = idx.shape[1], []
    for r0 in range(0, idx.shape[0], T):
        m = min(T, idx.shape[0] - r0)
        b = MOE.MoeBuffers(T, H, I, E, k, dtype, DT[dtype], "cuda")
        b.topk_idx[:m].copy_(idx[r0:r0 + m]), b.topk_w[:m].copy_(w[r0:r0 + m])
        d_n = d_int(max(0, min(m, n - r0)))
        b.lists(d_n)
        hs = torch.zeros((T, H), dtype=dtype, device="cuda")
        hs[:m] = h[r0:r0 + m]
        outs.append(b.experts(hs, *packed(E, dtype, fmt), d_n, fmt)[:m].clone())
    torch.cuda.synchronize()
    return torch.cat(outs)


def check_lists(b, idx, n, E):
    k = idx.shape[1]
    got, want = b.routing_state(), MOE.wide_lists_reference(idx, n, E)
    assert got["n_tiles"] == len(want["tiles"]) and got["n_active"] == len(want["active"]), (got["n_tiles"], got["n_active"])
    for key in ("active", "counts", "offsets", "entries", "tiles"):
        assert got[key] == want[key], key
    assert got["n_tiles"] <= MOE.wide_tile_bound(b.rows, E, k)
    return want


CASES = {"planted": (planted_idx, 160), "dirty_n100": (dirty_idx, 100)}


@pytest.mark.parametrize("case", list(CASES))
def test_lists_and_tile_table_equal_the_python_reference(case):
    make, n = CASES[case]
    idx = make()
    E, k, rows = 8, 2, idx.shape[0]
    want = MOE.wide_lists_reference(idx, n, E)
    if case == "planted":
        assert [want["counts"][want["active"].index(e)] if e in want["active"] else 0 for e in range(E)] == COUNTS
        assert [t[2] for t in want["tiles"]] == [1, 63, 64, 64, 1, 64, 63]
    else:
        p_out = [3 * k + 1, 7 * k + 1, 9 * k, 98 * k]
        assert not set(p_out) & set(want["entries"]) and max(want["entries"]) < n * k and len(want["entries"]) == n * k - len(p_out)
    images = []
    for _ in range(2):
        b = wide_buffers(rows, E, k, torch.bfloat16)
        b.topk_idx[:rows].copy_(idx.cuda())
        b.lists(d_int(n))
        torch.cuda.synchronize()
        check_lists(b, idx, n, E)
        images.append(b.routing_bytes())
    assert torch.equal(images[0], images[1]), "the routing part of the workspace over two runs"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", list(CASES))
def test_rows_equal_the_64_row_calls_under_planted_routing(case, fmt, dtype):
    make, n = CASES[case]
    idx = make().cuda()
    E, k, rows = 8, 2, idx.shape[0]
    h, w = states(rows, dtype, 1), mix_weights(MOE.wide_rows_pad(rows), k, dtype, 2)
    h[n:] = NAN
    out, b = run_wide(h, idx, w, n, E, dtype, fmt)
    check_lists(b, idx.cpu(), n, E)
    ref = run_narrow(h[:rows], idx, w, n, E, dtype, fmt)
    assert bool(torch.isfinite(out).all()) and bool(out[:n].abs().max() > 0)
    assert torch.equal(out[:rows], ref), f"{case} {fmt} {dtype}: a row differs from the <= 64-row calls"
    assert bool((out[n:] == 0).all()), "rows >= *d_n are zero"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_many_experts_routed_by_the_wide_router(dtype):
    E, k, rows, n = 128, 8, 192, 192
    g = torch.Generator(device="cuda").manual_seed(11)
    router = (torch.randn((E, H), generator=g, device="cuda") * 0.05).to(dtype)
    h = states(rows, dtype, 5)
    b = wide_buffers(rows, E, k, dtype)
    b.topk_idx.fill_(12345), b.topk_w.fill_(NAN)
    b.route(h, router, d_int(n), True)
    b.lists(d_int(n))
    torch.cuda.synchronize()
    for r0 in range(0, rows, T):                                  # the router is samd_moe_route's kernel: the same indices and weights
        nb = MOE.MoeBuffers(T, H, I, E, k, dtype, DT[dtype], "cuda")
        nb.route(h[r0:r0 + T].contiguous(), router, d_int(T), True)
        assert torch.equal(nb.topk_idx, b.topk_idx[r0:r0 + T]) and torch.equal(nb.topk_w, b.topk_w[r0:r0 + T])
    idx, w = b.topk_idx.clone(), b.topk_w.clone()
    want = check_lists(b, idx.cpu(), n, E)
    assert len(want["active"]) > 64 and max(want["counts"]) > 1
    for fmt in FORMATS:
        out = b.experts(h, *packed(E, dtype, fmt), d_int(n), fmt).clone()
        torch.cuda.synchronize()
        assert torch.equal(out, run_narrow(h, idx, w, n, E, dtype, fmt)), f"{fmt} {dtype}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", ["planted", "many_experts"])
def test_against_the_float64_reference_at_the_bar_of_the_64_row_kernels(case, dtype):
    """tests/test_gpu_moe_kernels.py::test_expert_gemms_with_pinned_routing's bar: error <= 1.5 x HF's own experts' + 0.02 x max|out|"""
    pytest.importorskip("transformers")
    from test_gpu_moe_kernels import hf_experts
    if case == "planted":
        E, idx = 8, planted_idx().cuda()
    else:
        E, gc = 128, torch.Generator().manual_seed(4)
        idx = torch.stack([torch.randperm(E, generator=gc)[:8] for _ in range(192)]).to(device="cuda", dtype=torch.int32)
    rows, k = idx.shape
    gate_up, down = weights(E, dtype)
    h, w = states(rows, dtype, 3), mix_weights(rows, k, dtype, 4)
    out = run_wide(h, idx, w, rows, E, dtype, None)[0][:rows]
    h, w = h[:rows], w[:rows]
    want = M.experts_grouped(h, gate_up, down, idx.long(), w)
    with torch.no_grad():
        hf = hf_experts(E, H, I, gate_up, down, dtype)(h, idx.long(), w).double()
    e_ours, e_hf, scale = (out.double() - want).abs().max().item(), (hf - want).abs().max().item(), want.abs().max().item()
    print(f"{case} {dtype}: ours {e_ours:.5f}, HF {e_hf:.5f}, max|out| {scale:.3f}")
    assert e_ours <= 1.5 * e_hf + 0.02 * scale, (e_ours, e_hf, scale)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_rows_bits_do_not_depend_on_rows_or_position(fmt, dtype):
    """row 0's routing and state at rows = 65 as row 64 (every row's first expert is the same one: its 65th entry, a tile of its own),
    inside rows = 192 as row 100 (the second of three tiles) and as row 3, and as row 0 of 65 -- against the row alone in a 64-row call"""
    E, k = 8, 2
    g = torch.Generator().manual_seed(9)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(192)]).to(device="cuda", dtype=torch.int32)
    idx[:, 0] = idx[0, 0]                                         # a crowded expert: the row's own first one, in every row
    idx[:, 1] = torch.where(idx[:, 1] == idx[:, 0], (idx[:, 0] + 1) % E, idx[:, 1])
    h, w = states(192, dtype, 6), mix_weights(192, k, dtype, 7)

    def placed(rows, at):
        hh, ii, ww = h[:MOE.wide_rows_pad(rows)].clone(), idx[:rows].clone(), w[:MOE.wide_rows_pad(rows)].clone()
        hh[at], ii[at], ww[at] = h[0], idx[0], w[0]
        return run_wide(hh, ii, ww, rows, E, dtype, fmt)[0][at].clone()
    alone = run_narrow(h[:1], idx[:1], w[:1], 1, E, dtype, fmt)[0]
    assert bool(alone.abs().max() > 0)
    for rows, at in ((65, 64), (192, 100), (192, 3), (65, 0)):
        assert torch.equal(placed(rows, at), alone), (rows, at)


# ------------------------------------------------------------------------------------------------ exact integers (tests/moe_planting.py)
@pytest.mark.parametrize("form", [None, "mxfp4"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_exact_integer_case_over_three_stacked_blocks(dtype, form):
    """moe_planting's 64-row "counts" routing (expert counts 1, 15, 16, 17, 33, 47, 48, 63) and its planted draws, stacked three times with
    block b taking draw b (modulo the case's draws): 192 rows, counts 3 .. 189 (one to three tiles per expert, none a multiple of 64).  A row's planted sums depend on
    its own state and its experts' weights alone, so what the wide launches must store is the blocks' float64 references stacked: act for
    every list entry, y for every list entry, out for every row, bit for bit."""
    import moe_planting as P
    from samd_hip import _ptr as ptr, check, current_stream
    from test_gpu_gemm_exact import same
    from test_gpu_moe_exact import pack_model, pack_mxfp4
    L, R, B = samd_hip.lib(), P.routing("counts", 64), 3
    E, k, rows, dc, code = R.E, R.k, 64 * B, DT[dtype], MOE.WIDE_FORMAT_CODES[form]
    idx = torch.from_numpy(np.concatenate([R.idx] * B)).cuda()
    d_n = d_int(rows)
    named = torch.tensor([p + 64 * k * b for b in range(B) for p in R.named], device="cuda")

    def workspace(hidden):
        ws = torch.full((L.samd_moe_wide_workspace(rows, hidden, 256, E, k, dc),), 0xFF, dtype=torch.uint8, device="cuda")
        y = ws[L.samd_moe_wide_workspace_layout(7, rows, k):].view(dtype).view(rows * k, hidden)
        y.fill_(NAN)
        check(L.samd_moe_wide_lists(ptr(idx), ptr(d_n), rows, E, k, ptr(ws), current_stream()))
        return ws, y
    # gate|up: hidden = 3 chunks, moe_inter 256
    c = P.gate_up_case(dtype, R, 256, 3, form, check=False)
    draws = [c.draws[b % len(c.draws)] for b in range(B)]
    W = torch.cat((c.Wg, c.Wu), dim=1)
    Wp = pack_mxfp4(W, np.concatenate(c.exps, axis=1), dtype, P.gate_up_row_order(c.inter)) if form else pack_model(W.to(dtype).cuda(), 1)
    hd = torch.cat([h for h, _ in draws]).to(dtype).cuda()
    want = torch.cat([a for _, a in draws]).to(dtype)
    ws, _ = workspace(256)
    act = torch.full((rows * k, c.inter), NAN, dtype=dtype, device="cuda")
    check(L.samd_moe_wide_gate_up_silu(ptr(hd), ptr(Wp), ptr(ws), rows, c.K, c.inter, E, k, code, ptr(act), dc, current_stream()))
    torch.cuda.synchronize()
    same(act[named], want[named.cpu()], "act")
    # down + combine: moe_inter = 3 chunks, hidden 256, large sums
    c = P.down_case(dtype, R, 256, 3, "large", form, check=False)
    draws = [c.draws[b % len(c.draws)] for b in range(B)]
    Wp = pack_mxfp4(c.W, c.exps, dtype) if form else pack_model(c.W.to(dtype).cuda(), 0)
    act = torch.cat([a for a, _, _ in draws]).to(dtype).cuda()
    w = torch.cat([c.w] * B).to(dtype).cuda()
    ws, y = workspace(c.N)
    out = torch.full((rows, c.N), NAN, dtype=dtype, device="cuda")
    check(L.samd_moe_wide_down_combine(ptr(act), ptr(Wp), ptr(idx), ptr(w), ptr(d_n), ptr(ws), rows, c.N, c.K, E, k, code, ptr(out), dc, current_stream()))
    torch.cuda.synchronize()
    same(y[named], torch.cat([yy for _, yy, _ in draws]).to(dtype)[named.cpu()], "y")
    same(out, torch.cat([o for _, _, o in draws]).to(dtype), "out")
