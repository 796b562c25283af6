"""The INT4 expert kernels (include/samd_hip.h: samd_moe_gate_up_silu_i4, samd_moe_down_combine_i4) against the float64 restatement
tests/moe_ref.py on the DEQUANTISED weights -- W = rne_dtype((q - z) * s) is a value of the model dtype, so quantisation error is no part
of the comparison: the kernels must multiply by exactly those weights.

Pinned routing: the cases and dtypes of test_gpu_moe_mxfp4_kernels.py (1, 2, 3, 7 and 8-chunk streams, all four row tiles, one row, the grid
bound R * k = E) with the margin of that file: error <= 1.5 x the error HF's own Qwen3MoeExperts makes in the model dtype on the same
dequantised weights + 0.02 x max|out|.  Every group of 128 is multiplied by 2^s (s seeded in [-6, 2]) before quantising, so neighbouring
groups' scales differ by up to 2^8 and the zero points span at least 8 codes: a swapped group word or zero point is gross.
Exact layout probe: one-hot activations make the down kernel copy weight columns, compared with torch.equal.
Exact integers: codes and zero points arbitrary in 0..15, scales 2^e with two different e in the two groups of every chunk, alternating
along the rows, activations integers |a| <= 8, K = 256 x every stream length of moe_planting.exact_sweep (depth - 1 .. depth + 2 of
every row tile's pipeline, and 1 chunk: shorter than every depth; 3; 9: longer than the deepest ring),
all four row tiles, expert counts from moe_planting.COUNTS.  Every exact sum is a multiple of 2^emin below 2^24 * 2^emin, so fp32 holds it
in any order and what the launch must store is rne_dtype(exact sum), bit for bit.  Gate|up: the first 128 columns of h are 1 and the gate
rows' first group is (q - z) = 4 at scale 2^-2, a bias of 128 that keeps every gate sum above 20; there 1 + __expf(-g) is 1.0f whatever
__expf's last bits are, so silu(g) = g and act = rne(rne(gate) * rne(up)): moe_planting's silu planting carried over to codes with a zero
point (the bias takes one whole group instead of one column).  The exactness conditions are asserted on the CPU side in the test itself.
Row independence, poison and the error returns as for the MXFP4 kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import moe_planting as MP
import moe_ref as M
import samd_hip
from samd_hip import int4 as I4
from samd_hip import moe as MOE
from test_gpu_gemm_exact import same
from test_gpu_moe_exact import Block
from test_gpu_moe_kernels import buffers, d_int, hf_experts, pinned

NAN = float("nan")


def group_scaled(t, g, sigma=0.05):
    """t [E, N, K] (randn * sigma) with every group of 128 along K shifted by a mean uniform in [-3, 3] sigma (the zero points then range
    over all codes) and multiplied by 2^s, s uniform in [-6, 2]"""
    E, N, K = t.shape
    s = torch.randint(-6, 3, (E, N, K // 128), generator=g, device=t.device)
    mean = (torch.rand((E, N, K // 128), generator=g, device=t.device) * 6.0 - 3.0) * sigma
    return ((t.view(E, N, K // 128, 128) + mean[..., None]) * torch.exp2(s.float())[..., None]).view(E, N, K)


def quantised_experts(E, H, I, g, dtype):
    """-> (packed gate|up, packed down, dequantised gate|up, dequantised down (fp32, values of dtype))"""
    gate_up = group_scaled(torch.randn((E, 2 * I, H), generator=g, device="cuda") * 0.05, g).to(dtype)
    down = group_scaled(torch.randn((E, H, I), generator=g, device="cuda") * 0.05, g).to(dtype)
    gu, dn = MOE.quantize_experts_int4(gate_up, down, dtype)
    for q, z, s in (gu, dn):
        assert int(z.max()) - int(z.min()) >= 8, "the zero points must span at least 8 codes"
        assert float(s.float().max() / s.float().min()) >= 64.0, "the group scales must differ widely"
    p_gu, p_down = MOE.pack_experts_int4(gu, dn, dtype)
    assert p_gu.dtype == torch.uint8 and p_gu.numel() == E * 2 * I * H // 2 + E * 2 * I * H // 32
    assert p_down.dtype == torch.uint8 and p_down.numel() == E * H * I // 2 + E * H * I // 32
    w_gu, w_down = MOE.dequantize_experts_int4(*gu), MOE.dequantize_experts_int4(*dn)
    assert torch.equal(w_gu, w_gu.to(dtype).float()) and torch.equal(w_down, w_down.to(dtype).float())
    return p_gu, p_down, w_gu, w_down


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
def test_int4_expert_gemms_with_pinned_routing(dtype, case, E, k, H, I, RP, n):
    """the expert launches against HF's own experts at workload statistics (randn inputs): error <= 1.5 x HF's + 0.02 x max|out|"""
    gc = torch.Generator().manual_seed(E * k + n)
    g = torch.Generator(device="cuda").manual_seed(E * k + n)
    p_gu, p_down, w_gu, w_down = quantised_experts(E, H, I, g, dtype)
    h = torch.randn((RP, H), generator=g, device="cuda").to(dtype)
    h[n:] = NAN
    idx = pinned(case, RP, E, k, gc)
    w = torch.rand((RP, k), generator=g, device="cuda") + 0.1
    w = (w / w.sum(-1, keepdim=True)).to(dtype)
    b = buffers(RP, H, I, E, k, dtype)
    b.topk_idx.copy_(idx), b.topk_w.copy_(w)
    b.act.fill_(NAN), b.ws.fill_(0xFF), b.out.fill_(NAN)
    b.lists(d_int(n))
    out = b.experts(h, p_gu, p_down, d_int(n), expert_format="int4g128")
    torch.cuda.synchronize()
    n_active = b.routing_state()[0]
    assert n_active == len(set(idx[:n].flatten().tolist()))
    want = M.experts_grouped(h[:n], w_gu, w_down, idx[:n].long(), w[:n])
    with torch.no_grad():
        hf = hf_experts(E, H, I, w_gu, w_down, dtype)(h[:n], idx[:n].long(), w[:n]).double()
    e_ours, e_hf, scale = (out[:n].double() - want).abs().max().item(), (hf - want).abs().max().item(), want.abs().max().item()
    print(f"int4 {case} E={E} k={k} H={H} I={I} rows {n}/{RP} {dtype}: active {n_active}, ours {e_ours:.5f}, HF {dtype} {e_hf:.5f}, max|out| {scale:.3f}")
    assert bool(torch.isfinite(out[:n]).all()) and bool((out[n:] == 0).all())
    assert e_ours <= 1.5 * e_hf + 0.02 * scale, (e_ours, e_hf, scale)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("I", [256, 768])
def test_down_kernel_copies_weight_columns_exactly(dtype, I):
    """one-hot act rows: y[p] = column k_p of the row's expert, exactly.  The k positions cover both j halves of a chunk (the two groups),
    every g, the first and the last element of a unit (low nibble of byte 0, high nibble of byte 15) and their neighbours, in every chunk:
    the nibble order, the unit, the group word, the zero point and the tile arithmetic are pinned."""
    E, k, H, RP = 4, 1, 512, 16
    g = torch.Generator(device="cuda").manual_seed(I)
    _, p_down, _, w_down = quantised_experts(E, H, I, g, dtype)
    assert bool((w_down != 0).float().mean() > 0.8)
    n_chunks = I // 256
    idx = (torch.arange(RP, device="cuda", dtype=torch.int32) % E).reshape(RP, 1)
    y_off = 4 * samd_hip.lib().samd_moe_workspace_layout(4)
    y_off = (y_off + 255) // 256 * 256
    chunks_seen = set()
    for first, last in ((0, 31), (1, 30), (16, 15)):
        kpos = [256 * ((r + first) % n_chunks) + 128 * ((r >> 2) & 1) + 32 * (r & 3) + (first if r < 8 else last) for r in range(RP)]
        assert {(p % 256) // 128 for p in kpos} == {0, 1} and {(p % 128) // 32 for p in kpos} == {0, 1, 2, 3}
        chunks_seen |= {p // 256 for p in kpos}
        b = buffers(RP, H, I, E, k, dtype)
        b.topk_idx.copy_(idx), b.topk_w.fill_(1.0)
        b.ws.fill_(0xFF), b.out.fill_(NAN)
        b.lists(d_int(RP))
        b.act.zero_()
        b.act[torch.arange(RP, device="cuda"), torch.tensor(kpos, device="cuda")] = 1.0
        L, d_n = samd_hip.lib(), d_int(RP)
        samd_hip.check(L.samd_moe_down_combine_i4(b.act.data_ptr(), p_down.data_ptr(), b.topk_idx.data_ptr(), b.topk_w.data_ptr(), d_n.data_ptr(),
                                                  b.ws.data_ptr(), RP, H, I, E, k, b.out.data_ptr(), b.dt, samd_hip.current_stream()))
        torch.cuda.synchronize()
        y = b.ws[y_off:y_off + RP * k * H * 2].view(dtype).view(RP * k, H)
        for r in range(RP):
            want = w_down[r % E, :, kpos[r]]
            assert torch.equal(y[r].float(), want), (I, r, kpos[r], (y[r].float() != want).nonzero().flatten()[:8].tolist())
        assert torch.equal(b.out, y)                             # k = 1, weight 1: the combine passes the products through
    assert chunks_seen == set(range(n_chunks))


# ------------------------------------------------------------------------------------------------ exact integers
# every stream length around the pipeline depth of each row tile (moe_planting.chunk_sweep) and the lengths 1, 3, 9 (K = 256 / 768 / 2304)
EXACT = MP.exact_sweep("int4g128")
EXACT_IDS = [f"{K}-{rows_pad}" for K, rows_pad in EXACT]


def rne(x, dtype):
    """float64 -> dtype, one rounding: every x here is exact in fp32 (asserted), so the step through fp32 rounds nothing"""
    assert torch.equal(x.float().double(), x)
    return x.float().to(dtype)


def exact_weights(rng, E, N, K, exps, bias_rows=None):
    """codes and zero points uniform in 0..15, scales 2^exps[(row + group) % 2]: (q [E, N, K/2], z, e [E, N, K/128] int64, W float64).
    bias_rows: the rows whose first group is the gate bias: (q - z) = 4 at 2^-2 (z uniform in 0..11)"""
    codes = rng.integers(0, 16, (E, N, K))
    z = rng.integers(0, 16, (E, N, K // 128))
    e = np.asarray(exps)[(np.arange(N)[:, None] + np.arange(K // 128)[None, :]) % 2][None].repeat(E, 0)
    if bias_rows is not None:
        z[:, bias_rows, 0] = rng.integers(0, 12, (E, len(bias_rows)))
        codes[:, bias_rows, :128] = z[:, bias_rows, 0][..., None] + 4
        e[:, bias_rows, 0] = -2
    assert codes.min() >= 0 and codes.max() <= 15 and z.min() >= 0 and z.max() <= 15
    for c in range(K // 256):                                    # two different exponents in the two groups of every chunk
        assert bool((e[:, :, 2 * c] != e[:, :, 2 * c + 1]).all())
    W = (codes - z.repeat(128, axis=2)).astype(np.float64) * np.exp2(e.repeat(128, axis=2).astype(np.float64))
    q = I4.pack_nibbles(torch.from_numpy(codes.reshape(E * N, K).astype(np.uint8))).reshape(E, N, K // 2)
    return q, torch.from_numpy(z.astype(np.uint8)), torch.from_numpy(e), torch.from_numpy(W)


def triple(q, z, e, dtype):
    s = torch.exp2(e.double()).to(dtype)
    assert torch.equal(s.double(), torch.exp2(e.double()))
    return q.cuda(), z.cuda(), s.cuda()


def assert_exact_in_fp32(x, emin):
    """every sum is a multiple of 2^emin below 2^24 * 2^emin: fp32 holds it, and every partial sum, in any order"""
    u = x / 2.0 ** emin
    assert bool((u == u.round()).all()) and u.abs().max().item() < 2 ** 24


DOWN_EXPS = (-4, -2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,rows_pad", EXACT, ids=EXACT_IDS)
def test_down_stores_the_rounded_exact_sum_of_every_list_entry(K, rows_pad, dtype):
    R = MP.routing("counts", rows_pad)
    N = 256
    rng = np.random.default_rng(MP.seed_of(K, rows_pad, 41))
    q, z, e, W = exact_weights(rng, R.E, N, K, DOWN_EXPS)
    dummy = exact_weights(rng, R.E, 2 * K, N, DOWN_EXPS)         # (the gate|up side of the pack call, [E, 2 I, H]: not launched)
    _, p_down = MOE.pack_experts_int4(triple(*dummy[:3], dtype), triple(q, z, e, dtype), dtype)
    act = torch.full((R.rows_pad * R.k, K), NAN, dtype=torch.float64)
    act[R.named] = torch.from_numpy(rng.integers(-8, 9, (len(R.named), K))).double()
    y_exact = torch.full((R.rows_pad * R.k, N), NAN, dtype=torch.float64)
    bound = 0.0
    for ex, lst in R.lists.items():
        y_exact[lst] = act[lst] @ W[ex].t()                      # float64: integers x 2^-4 far below 2^53
        bound = max(bound, (act[lst].abs() @ W[ex].abs().t()).max().item())
    # the exactness conditions, from the inputs alone: every partial sum in any order is bounded by the sum of the magnitudes
    assert bound < 2 ** 24 * 2.0 ** min(DOWN_EXPS) and act[R.named].abs().max().item() <= 8
    assert_exact_in_fp32(y_exact[R.named], min(DOWN_EXPS))
    assert y_exact[R.named].abs().max().item() < torch.finfo(torch.float16).max        # finite in fp16 too
    want = rne(y_exact[R.named], dtype)
    assert bool((want.double() != y_exact[R.named]).float().mean() > 0.05), "the rounding to the model dtype must be visible"
    b = Block(R, N, dtype)
    L = samd_hip.lib()
    w = MP.combine_weights(R).to(dtype).cuda()
    out = torch.full((R.rows_pad, N), NAN, dtype=dtype, device="cuda")
    act_d = act.to(dtype).cuda()
    samd_hip.check(L.samd_moe_down_combine_i4(act_d.data_ptr(), p_down.data_ptr(), b.idx.data_ptr(), w.data_ptr(), b.d_n.data_ptr(),
                                              b.ws.data_ptr(), R.rows_pad, N, K, R.E, R.k, out.data_ptr(), b.dc, samd_hip.current_stream()))
    torch.cuda.synchronize()
    same(b.y[b.named], want, f"y K={K} rows {rows_pad}")
    assert bool(torch.isnan(b.y[b.unnamed]).all()), "rows of y that no list names"
    assert bool(torch.isfinite(out[:R.n]).all())


GATE_EXPS, UP_EXPS = (-7, -8), (-6, -7)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,rows_pad", EXACT, ids=EXACT_IDS)
def test_gate_up_stores_the_rounded_product_of_every_list_entry(K, rows_pad, dtype):
    R = MP.routing("counts", rows_pad)
    inter = 256                                                  # 4 tiles of 64 gate | 64 up columns
    rng = np.random.default_rng(MP.seed_of(K, rows_pad, 43))
    qg, zg, eg, Wg = exact_weights(rng, R.E, inter, K, GATE_EXPS, bias_rows=np.arange(inter))
    qu, zu, eu, Wu = exact_weights(rng, R.E, inter, K, UP_EXPS)
    fused = tuple(torch.cat((a, b), dim=1) for a, b in zip((qg, zg, eg), (qu, zu, eu)))       # HF's fused gate_up_proj rows: gate, then up
    dummy = exact_weights(rng, R.E, K, inter, DOWN_EXPS)
    p_gu, _ = MOE.pack_experts_int4(triple(*fused, dtype), triple(*dummy[:3], dtype), dtype)
    h = torch.full((R.rows_pad, K), NAN, dtype=torch.float64)
    h[:R.n] = torch.from_numpy(rng.integers(-8, 9, (R.n, K))).double()
    h[:R.n, :128] = 1.0                                          # the bias block: 128 x 4 x 2^-2 = 128 on every gate column
    rows = R.rows_pad * R.k
    gate, up = torch.full((rows, inter), NAN, dtype=torch.float64), torch.full((rows, inter), NAN, dtype=torch.float64)
    bound = 0.0
    for ex, lst in R.lists.items():
        a = h[[p // R.k for p in lst]]
        gate[lst], up[lst] = a @ Wg[ex].t(), a @ Wu[ex].t()
        bound = max(bound, (a.abs() @ Wg[ex].abs().t()).max().item(), (a.abs() @ Wu[ex].abs().t()).max().item())
    emin = min(GATE_EXPS + UP_EXPS)
    assert bound < 2 ** 24 * 2.0 ** emin
    assert_exact_in_fp32(gate[R.named], emin), assert_exact_in_fp32(up[R.named], emin)
    gr, ur = rne(gate[R.named], dtype), rne(up[R.named], dtype)
    # silu(g) = g: 1 + exp(-g) is 1.0f with a factor of > 10 to spare below half an ulp of 1, whatever __expf's last bits are
    assert gr.float().min().item() >= 20.0 and bool((torch.exp(-gr.float()) < 2.0 ** -25 / 10).all())
    assert bool(((1.0 + torch.exp(-gr.float())) == 1.0).all())
    prod = gr.double() * ur.double()                             # two values of the model dtype: exact in fp32
    assert prod.abs().max().item() < torch.finfo(torch.float16).max and bool((ur != 0).float().mean() > 0.9)
    want = rne(prod, dtype)
    b = Block(R, 256, dtype)
    act = torch.full((rows, inter), NAN, dtype=dtype, device="cuda")
    h_d = h.to(dtype).cuda()
    samd_hip.check(samd_hip.lib().samd_moe_gate_up_silu_i4(h_d.data_ptr(), p_gu.data_ptr(), b.ws.data_ptr(), R.rows_pad, K, inter, R.E, R.k,
                                                           act.data_ptr(), b.dc, samd_hip.current_stream()))
    torch.cuda.synchronize()
    same(act[b.named], want, f"act K={K} rows {rows_pad}")
    assert bool(torch.isnan(act[b.unnamed]).all()), "rows of act that no list names"


# ------------------------------------------------------------------------------------------------ rows, poison, errors
def run_block4(h_rows, RP, router, p_gu, p_down, E, k, H, I, dtype, poison=False):
    n = h_rows.shape[0]
    h = torch.zeros((RP, H), dtype=dtype, device="cuda")
    h[:n] = h_rows
    b = buffers(RP, H, I, E, k, dtype)
    if poison:
        h[n:] = NAN
        b.act.fill_(NAN), b.ws.fill_(0xFF), b.out.fill_(NAN), b.topk_w.fill_(NAN), b.topk_idx.fill_(777)
    b.route(h, router, d_int(n), True)
    out = b.experts(h, p_gu, p_down, d_int(n), expert_format="int4g128").clone()
    torch.cuda.synchronize()
    return out, b


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,k,H,I", [(32, 4, 512, 256), (128, 8, 2048, 768)])
def test_a_rows_output_does_not_depend_on_its_company_with_int4_experts(dtype, E, k, H, I):
    g = torch.Generator(device="cuda").manual_seed(7)
    router = (torch.randn((E, H), generator=g, device="cuda") * 0.05).to(dtype)
    p_gu, p_down, _, _ = quantised_experts(E, H, I, g, dtype)
    rows = torch.randn((64, H), generator=g, device="cuda").to(dtype)
    rows[1:] = rows[1:] * 0.5 + rows[0] * 0.5                    # the others lean towards the same experts: shared tiles
    args = (router, p_gu, p_down, E, k, H, I, dtype)
    alone = run_block4(rows[:1], 16, *args)[0][0]
    assert bool(alone.abs().max() > 0)
    moved = torch.cat([rows[1:41], rows[:1], rows[41:64]])
    assert torch.equal(run_block4(moved, 64, *args)[0][40], alone), "as row 40 of 64"
    assert torch.equal(run_block4(rows[:8], 16, *args)[0][0], alone), "with 7 others"
    assert torch.equal(run_block4(rows[:33], 48, *args)[0][0], alone), "with 32 others (48-row tile)"
    assert torch.equal(run_block4(rows[:20], 32, *args)[0][0], alone), "with 19 others (32-row tile)"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("RP,n", [(16, 5), (64, 50)])
def test_poisoned_padding_and_workspaces_leave_no_trace_with_int4_experts(dtype, RP, n):
    E, k, H, I = 64, 4, 1024, 512
    g = torch.Generator(device="cuda").manual_seed(n)
    router = (torch.randn((E, H), generator=g, device="cuda") * 0.05).to(dtype)
    p_gu, p_down, _, _ = quantised_experts(E, H, I, g, dtype)
    rows = torch.randn((n, H), generator=g, device="cuda").to(dtype)
    clean, b0 = run_block4(rows, RP, router, p_gu, p_down, E, k, H, I, dtype)
    dirty, b1 = run_block4(rows, RP, router, p_gu, p_down, E, k, H, I, dtype, poison=True)
    assert bool(torch.isfinite(dirty).all()) and torch.equal(dirty, clean) and bool((dirty[n:] == 0).all())
    assert bool(clean[:n].abs().max() > 0)
    assert b0.routing_state() == b1.routing_state()


def test_unsupported_shapes_null_pointers_and_wrong_buffers_return_the_error():
    E, k, H, I, RP, dtype = 8, 2, 512, 256, 16, torch.float16
    g = torch.Generator(device="cuda").manual_seed(1)
    p_gu, p_down, w_gu, w_down = quantised_experts(E, H, I, g, dtype)
    b = buffers(RP, H, I, E, k, dtype)
    h = torch.zeros((RP, H), dtype=dtype, device="cuda")
    b.lists(d_int(0))
    L, st, P = samd_hip.lib(), samd_hip.current_stream(), lambda t: t.data_ptr()
    n1 = d_int(1)

    def gate_up(rows_pad=RP, hidden=H, inter=I, experts=E, top_k=k, W=P(p_gu), act=P(b.act), dt=b.dt):
        return L.samd_moe_gate_up_silu_i4(P(h), W, P(b.ws), rows_pad, hidden, inter, experts, top_k, act, dt, st)

    def down(rows_pad=RP, hidden=H, inter=I, experts=E, top_k=k, W=P(p_down), out=P(b.out), dt=b.dt):
        return L.samd_moe_down_combine_i4(P(b.act), W, P(b.topk_idx), P(b.topk_w), P(n1), P(b.ws), rows_pad, hidden, inter, experts, top_k, out, dt, st)
    assert gate_up() == 0 and down() == 0
    for call in (gate_up, down):
        for kw in (dict(rows_pad=24), dict(hidden=500), dict(inter=300), dict(inter=128), dict(experts=257), dict(top_k=9), dict(experts=4, top_k=8),
                   dict(dt=samd_hip.F16 + 7), dict(W=None)):
            assert call(**kw) != 0, (call.__name__, kw)
            with pytest.raises(samd_hip.SamdError, match="rows 16/32/48/64"):
                samd_hip.check(call(**kw))
    assert gate_up(act=None) != 0 and down(out=None) != 0
    # the Python wrapper refuses a wrong byte count, swapped buffers and buffers of the other formats instead of streaming them
    with pytest.raises(samd_hip.SamdError, match="pack_experts_int4"):
        b.experts(h, p_gu[:-17408], p_down, n1, expert_format="int4g128")
    with pytest.raises(samd_hip.SamdError, match="pack_experts_int4"):
        b.experts(h, p_down, p_gu, n1, expert_format="int4g128")
    with pytest.raises(samd_hip.SamdError, match="pack_experts_int4"):
        b.experts(h, *MOE.pack_experts(w_gu.to(dtype), w_down.to(dtype)), n1, expert_format="int4g128")
    # MXFP4 buffers of the same shape have the same byte count (4.25 bits per weight both): only what pack_experts_int4 returned is taken
    p4 = MOE.pack_experts_mxfp4(*MOE.quantize_experts(w_gu.to(dtype), w_down.to(dtype), dtype))
    assert p4[0].numel() == p_gu.numel() and p4[1].numel() == p_down.numel()
    with pytest.raises(samd_hip.SamdError, match="pack_experts_int4 did not return"):
        b.experts(h, *p4, n1, expert_format="int4g128")
    with pytest.raises(samd_hip.SamdError, match="pack_experts_int4 did not return"):      # (the guard fails closed: a copy has lost the mark)
        b.experts(h, p_gu.clone(), p_down, n1, expert_format="int4g128")
    with pytest.raises(samd_hip.SamdError, match="expert_format"):
        b.experts(h, p_gu, p_down, n1)
    with pytest.raises(samd_hip.SamdError, match="expected one of"):
        b.experts(h, p_gu, p_down, n1, expert_format="fp8")
    torch.cuda.synchronize()
