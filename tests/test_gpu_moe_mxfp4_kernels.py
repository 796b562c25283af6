"""The MXFP4 expert kernels (include/samd_hip.h: samd_moe_gate_up_silu_f4, samd_moe_down_combine_f4) against the float64 restatement
tests/moe_ref.py on the DEQUANTISED weights -- W = fp4(q) * 2^(e8 - 127) is exact in the model dtype, so quantisation error is no part of the
comparison: the kernels must multiply by exactly those weights.

Pinned routing: the cases and dtypes of test_gpu_moe_kernels.py (1, 2, 3, 7 and 8-chunk streams, all four row tiles, one row, the grid bound
R * k = E) with the margin of that file: error <= 1.5 x the error HF's own Qwen3MoeExperts makes in the model dtype on the same dequantised
weights + 0.02 x max|out|.  Every MX block is multiplied by 2^s (s seeded in [-6, 2]) before quantising, so neighbouring blocks' scales differ
by up to 2^8 and a misplaced scale byte is gross.  Exact layout probe: one-hot activations make the down kernel copy weight columns, compared
with torch.equal.  Row independence, poison and the error returns as for the model-dtype kernels."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import samd_hip
from samd_hip import moe as MOE
from samd_hip import mxfp4 as MX
import moe_ref as M
from test_gpu_moe_kernels import buffers, d_int, hf_experts, pinned


def block_scaled(t, g):
    """t [E, N, K] with every MX block (32 along K) multiplied by 2^s, s uniform in [-6, 2]"""
    E, N, K = t.shape
    s = torch.randint(-6, 3, (E, N, K // 32), generator=g, device=t.device)
    return (t.view(E, N, K // 32, 32) * torch.exp2(s.float())[..., None]).view(E, N, K)


def quantised_experts(E, H, I, g, dtype):
    """-> (packed gate|up, packed down, dequantised gate|up, dequantised down (fp32, exact in dtype))"""
    gate_up = block_scaled(torch.randn((E, 2 * I, H), generator=g, device="cuda") * 0.05, g).to(dtype)
    down = block_scaled(torch.randn((E, H, I), generator=g, device="cuda") * 0.05, g).to(dtype)
    q_gu, e8_gu, q_down, e8_down = MOE.quantize_experts(gate_up, down, dtype)
    lo, hi = MX.EXPONENT_RANGE[dtype]
    for e8 in (e8_gu, e8_down):
        assert lo <= int(e8.min()) - 127 and int(e8.max()) - 127 <= hi
        assert int(e8.max()) - int(e8.min()) >= 6, "the block scales must differ widely"
    p_gu, p_down = MOE.pack_experts_mxfp4(q_gu, e8_gu, q_down, e8_down)
    assert p_gu.dtype == torch.uint8 and p_gu.numel() == E * 2 * I * H // 2 + E * 2 * I * H // 32
    assert p_down.dtype == torch.uint8 and p_down.numel() == E * H * I // 2 + E * H * I // 32
    w_gu, w_down = MOE.dequantize_experts(q_gu, e8_gu), MOE.dequantize_experts(q_down, e8_down)
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
def test_4bit_expert_gemms_with_pinned_routing(dtype, case, E, k, H, I, RP, n):
    """the expert launches against HF's own experts at workload statistics (randn inputs): error <= 1.5 x HF's + 0.02 x max|out|.  That bar
    says how the kernels compare with HF, not that they are exact: what every launch must store, bit for bit, is held by
    tests/test_gpu_moe_exact.py"""
    gc = torch.Generator().manual_seed(E * k + n)
    g = torch.Generator(device="cuda").manual_seed(E * k + n)
    p_gu, p_down, w_gu, w_down = quantised_experts(E, H, I, g, dtype)
    h = torch.randn((RP, H), generator=g, device="cuda").to(dtype)
    h[n:] = float("nan")
    idx = pinned(case, RP, E, k, gc)
    w = torch.rand((RP, k), generator=g, device="cuda") + 0.1
    w = (w / w.sum(-1, keepdim=True)).to(dtype)
    b = buffers(RP, H, I, E, k, dtype)
    b.topk_idx.copy_(idx), b.topk_w.copy_(w)
    b.act.fill_(float("nan")), b.ws.fill_(0xFF), b.out.fill_(float("nan"))
    b.lists(d_int(n))
    out = b.experts(h, p_gu, p_down, d_int(n), expert_format="mxfp4")
    torch.cuda.synchronize()
    n_active = b.routing_state()[0]
    assert n_active == len(set(idx[:n].flatten().tolist()))
    want = M.experts_grouped(h[:n], w_gu, w_down, idx[:n].long(), w[:n])
    with torch.no_grad():
        hf = hf_experts(E, H, I, w_gu, w_down, dtype)(h[:n], idx[:n].long(), w[:n]).double()
    e_ours, e_hf, scale = (out[:n].double() - want).abs().max().item(), (hf - want).abs().max().item(), want.abs().max().item()
    print(f"mxfp4 {case} E={E} k={k} H={H} I={I} rows {n}/{RP} {dtype}: active {n_active}, ours {e_ours:.5f}, HF {dtype} {e_hf:.5f}, max|out| {scale:.3f}")
    assert bool(torch.isfinite(out[:n]).all()) and bool((out[n:] == 0).all())
    assert e_ours <= 1.5 * e_hf + 0.02 * scale, (e_ours, e_hf, scale)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("I", [256, 768])
def test_down_kernel_copies_weight_columns_exactly(dtype, I):
    """one-hot act rows: y[p] = column k_p of the row's expert, exactly.  The k positions cover both j halves of a chunk, every g, the first
    and the last element of a unit (low nibble of byte 0, high nibble of byte 15) and their neighbours, in every chunk: the nibble order, the
    unit, the scale byte and the tile arithmetic are pinned."""
    E, k, H, RP = 4, 1, 512, 16
    g = torch.Generator(device="cuda").manual_seed(I)
    _, p_down, _, w_down = quantised_experts(E, H, I, g, dtype)
    assert bool((w_down != 0).float().mean() > 0.8)
    n_chunks = I // 256
    idx = (torch.arange(RP, device="cuda", dtype=torch.int32) % E).reshape(RP, 1)
    y_off = 4 * samd_hip.lib().samd_moe_workspace_layout(4)
    y_off = (y_off + 255) // 256 * 256
    for first, last in ((0, 31), (1, 30), (16, 15)):
        kpos = [256 * ((r + first) % n_chunks) + 128 * ((r >> 2) & 1) + 32 * (r & 3) + (first if r < 8 else last) for r in range(RP)]
        assert {(p % 256) // 128 for p in kpos} == {0, 1} and {(p % 128) // 32 for p in kpos} == {0, 1, 2, 3}
        b = buffers(RP, H, I, E, k, dtype)
        b.topk_idx.copy_(idx), b.topk_w.fill_(1.0)
        b.ws.fill_(0xFF), b.out.fill_(float("nan"))
        b.lists(d_int(RP))
        b.act.zero_()
        b.act[torch.arange(RP, device="cuda"), torch.tensor(kpos, device="cuda")] = 1.0
        L, d_n = samd_hip.lib(), d_int(RP)
        samd_hip.check(L.samd_moe_down_combine_f4(b.act.data_ptr(), p_down.data_ptr(), b.topk_idx.data_ptr(), b.topk_w.data_ptr(), d_n.data_ptr(),
                                                  b.ws.data_ptr(), RP, H, I, E, k, b.out.data_ptr(), b.dt, samd_hip.current_stream()))
        torch.cuda.synchronize()
        y = b.ws[y_off:y_off + RP * k * H * 2].view(dtype).view(RP * k, H)
        for r in range(RP):
            want = w_down[r % E, :, kpos[r]]
            assert torch.equal(y[r].float(), want), (I, r, kpos[r], (y[r].float() != want).nonzero().flatten()[:8].tolist())
        assert torch.equal(b.out, y)                             # k = 1, weight 1: the combine passes the products through


def run_block4(h_rows, RP, router, p_gu, p_down, E, k, H, I, dtype, poison=False):
    n = h_rows.shape[0]
    h = torch.zeros((RP, H), dtype=dtype, device="cuda")
    h[:n] = h_rows
    b = buffers(RP, H, I, E, k, dtype)
    if poison:
        h[n:] = float("nan")
        b.act.fill_(float("nan")), b.ws.fill_(0xFF), b.out.fill_(float("nan")), b.topk_w.fill_(float("nan")), b.topk_idx.fill_(777)
    b.route(h, router, d_int(n), True)
    out = b.experts(h, p_gu, p_down, d_int(n), expert_format="mxfp4").clone()
    torch.cuda.synchronize()
    return out, b


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,k,H,I", [(32, 4, 512, 256), (128, 8, 2048, 768)])
def test_a_rows_output_does_not_depend_on_its_company_with_4bit_experts(dtype, E, k, H, I):
    g = torch.Generator(device="cuda").manual_seed(7)
    router = (torch.randn((E, H), generator=g, device="cuda") * 0.05).to(dtype)
    p_gu, p_down, _, _ = quantised_experts(E, H, I, g, dtype)
    rows = torch.randn((64, H), generator=g, device="cuda").to(dtype)
    rows[1:] = rows[1:] * 0.5 + rows[0] * 0.5                    # the others lean towards the same experts: shared tiles
    args = (router, p_gu, p_down, E, k, H, I, dtype)
    alone = run_block4(rows[:1], 16, *args)[0][0]
    assert bool(alone.abs().max() > 0)
    assert torch.equal(run_block4(rows[:8], 16, *args)[0][0], alone), "with 7 others"
    assert torch.equal(run_block4(rows[:64], 64, *args)[0][0], alone), "with 63 others"
    assert torch.equal(run_block4(rows[:33], 48, *args)[0][0], alone), "with 32 others (48-row tile)"
    assert torch.equal(run_block4(rows[:20], 32, *args)[0][0], alone), "with 19 others (32-row tile)"
    moved = torch.cat([rows[1:6], rows[:1], rows[6:8]])
    assert torch.equal(run_block4(moved, 16, *args)[0][5], alone), "at position 5 of 8"
    moved = torch.cat([rows[1:41], rows[:1], rows[41:64]])
    assert torch.equal(run_block4(moved, 64, *args)[0][40], alone), "at position 40 of 64"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("RP,n", [(16, 5), (64, 50)])
def test_poisoned_padding_and_workspaces_leave_no_trace_with_4bit_experts(dtype, RP, n):
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
    p_gu, p_down, _, _ = quantised_experts(E, H, I, g, dtype)
    b = buffers(RP, H, I, E, k, dtype)
    h = torch.zeros((RP, H), dtype=dtype, device="cuda")
    b.lists(d_int(0))
    L, st, P = samd_hip.lib(), samd_hip.current_stream(), lambda t: t.data_ptr()
    n1 = d_int(1)

    def gate_up(rows_pad=RP, hidden=H, inter=I, experts=E, top_k=k, W=P(p_gu), act=P(b.act), dt=b.dt):
        return L.samd_moe_gate_up_silu_f4(P(h), W, P(b.ws), rows_pad, hidden, inter, experts, top_k, act, dt, st)

    def down(rows_pad=RP, hidden=H, inter=I, experts=E, top_k=k, W=P(p_down), out=P(b.out), dt=b.dt):
        return L.samd_moe_down_combine_f4(P(b.act), W, P(b.topk_idx), P(b.topk_w), P(n1), P(b.ws), rows_pad, hidden, inter, experts, top_k, out, dt, st)
    assert gate_up() == 0 and down() == 0
    for call in (gate_up, down):
        for kw in (dict(rows_pad=24), dict(hidden=500), dict(inter=300), dict(inter=128), dict(experts=257), dict(top_k=9), dict(experts=4, top_k=8),
                   dict(dt=samd_hip.F16 + 7), dict(W=None)):
            assert call(**kw) != 0, (call.__name__, kw)
            with pytest.raises(samd_hip.SamdError, match="rows 16/32/48/64"):
                samd_hip.check(call(**kw))
    assert gate_up(act=None) != 0 and down(out=None) != 0
    # the Python wrapper refuses buffers of the other format instead of streaming them
    with pytest.raises(samd_hip.SamdError, match="pack_experts_mxfp4"):
        b.experts(h, p_down, p_down, n1, expert_format="mxfp4")
    with pytest.raises(samd_hip.SamdError, match="expert_format"):
        b.experts(h, p_gu, p_down, n1)
    with pytest.raises(samd_hip.SamdError, match="expected one of"):
        b.experts(h, p_gu, p_down, n1, expert_format="fp8")
    torch.cuda.synchronize()
