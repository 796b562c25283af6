"""Exact-integer parity of the mixture-of-experts kernels (csrc/gemm_kernels.hip: k_moe_gate_up_silu, k_moe_down, k_moe4_gate_up_silu,
k_moe4_down, k_moe_combine) on inputs planted by tests/moe_planting.py: every exact sum is an integer below 2^24 and every product of the
combine a multiple of 1/4, so what a kernel must store is determined bit for bit.  Every comparison is an equality on the stored tensor
against the float64 reference (`same` of tests/test_gpu_gemm_exact.py: the first mismatch is in the message).  act, y and out start
NaN-filled, the routing part of the workspace at 0xFF; the lists are built by samd_moe_lists from the pinned routing and compared with the
Python lists first; every launch is driven on its own through the C ABI, so one stage's planting does not constrain the next.  The cases
are those tests/test_moe_planting_cpu.py builds with every named fault checked (one product dropped or doubled, a tile row reading the next
list entry, the neighbouring expert, the source row p instead of p / top_k, gate and up swapped, truncating casts, w[row][j + 1], y of row
p + 1, the combine in the model dtype, nibbles swapped, the neighbouring block's exponent, ...); here they are built without that check.

  launch                               inputs                                          compared (all by equality)
  samd_moe_gate_up_silu, _f4           silu planting per expert, moe_inter 256 / 512   act[p] = round(g * u) for every list entry; the rows of
                                       (4 / 8 tile columns), hidden = 256 chunks       act no list names stay NaN
  samd_moe_down_combine, _f4           small and large sums, hidden 256 / 512,         y[p] (read from the workspace) for every list entry, NaN
                                       moe_inter = 256 chunks; w from {1/4 .. 2}       elsewhere; out for rows < n, exact zeros for rows >= n
  chunks                               model dtype 1-7 at every row bucket (depth 2); MXFP4 1-10 at 16 rows (depth 8), 1-5 and 7 at 32 / 48
                                       / 64 rows (depths 3 / 2 / 3): streams shorter than, at and above every depth, odd counts through the
                                       per-block refill at 48 / 64 rows
  routings                             one expert in every row, one entry per expert (E = 8, and E = 128, k = 8: the grid bound), random
                                       with n < rows_pad, expert counts 1, 15, 16, 17, 33, 47, 48, 63; out-of-range and repeated slots
  row independence                     rows >= n of h and the unnamed rows of act are NaN in EVERY case (n < rows_pad in the random and
                                       one-entry routings); one row alone at 16 rows against the same row as row 40 of 64: act, y, out equal
  slot order                           w y = (+2^15, +2^-10, -2^15, +2^-11) rotated by the row, y made by the down launch itself; top_k 4, 8
  samd_moe_pack_experts                2-byte counter payload against the numpy restatement, gate_up 0 and 1

Recorded on an MI355X: 52 cases, 38 s (tests/test_gpu_gemm_exact.py: 63 cases, 20 s); the slowest case 2.9 s, most of it the float64
references on the host.  SiLU epilogue: as in the dense epilogue, the device's __expf and fp32 divide deliver silu(g) = g exactly for every
planted gate (g in [24, 64] bf16 / [24, 512] fp16; MXFP4 form [28, 68] / [226, 286]): act equals round(g * u) bit for bit in all four
kernels, no fallback to a 1-ulp bar was needed.
Scratch builds with one changed line each, against this file / the tolerance files test_gpu_moe_kernels.py + test_gpu_moe_mxfp4_kernels.py
(router tests left out): a truncating cast of y in moe_expert_gemm 12 failed / all 51 pass; k_moe_combine adding in the model dtype 24
failed / all pass; k_moe_combine running j downwards 8 failed (the slot-order cases) / all pass; srow of moe_expert_gemm reading list entry
r + 1 for i = 0 (16 tile rows) 20 failed / 13 of 51 fail as well (whole rows of another token: gross at any tolerance)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import moe_planting as M
import samd_hip
from samd_hip import _ptr as P, check, current_stream, torch_dtype_code
from test_gpu_gemm_exact import same

NAN = float("nan")


def d_int(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


class Block:
    """the device state of one routing: indices, n, and a workspace whose routing part starts at 0xFF and whose y part starts NaN"""

    def __init__(self, R, hidden, dtype):
        L = samd_hip.lib()
        self.R, self.hidden, self.dtype, self.dc = R, hidden, dtype, torch_dtype_code(dtype)
        self.idx = torch.from_numpy(R.idx).cuda()
        self.d_n = d_int(R.n)
        self.ws = torch.full((L.samd_moe_workspace(R.rows_pad, hidden, R.E, R.k, self.dc),), 0xFF, dtype=torch.uint8, device="cuda")
        y_off = 256 * -(-4 * L.samd_moe_workspace_layout(4) // 256)
        assert y_off + R.rows_pad * R.k * hidden * 2 == self.ws.numel()
        self.y = self.ws[y_off:].view(dtype).view(R.rows_pad * R.k, hidden)
        self.y.fill_(NAN)
        check(L.samd_moe_lists(P(self.idx), P(self.d_n), R.rows_pad, R.E, R.k, P(self.ws), current_stream()))
        torch.cuda.synchronize()
        active, count, lst, stride, words = (L.samd_moe_workspace_layout(f) for f in range(5))
        w = self.ws[:4 * words].view(torch.int32).cpu()
        n_active = int(w[0])
        got = {int(w[active + a]): w[lst + stride * a:lst + stride * a + int(w[count + a])].tolist() for a in range(n_active)}
        assert list(got.items()) == list(R.lists.items()), "the device lists against the header's rule"
        self.named = torch.tensor(R.named, device="cuda")
        self.unnamed = torch.tensor(sorted(set(range(R.rows_pad * R.k)) - set(R.named)), dtype=torch.long, device="cuda")


def pack_model(W, gate_up):
    E, N, K = W.shape
    out = torch.empty_like(W)
    check(samd_hip.lib().samd_moe_pack_experts(P(W), P(out), E, N, K, gate_up, current_stream()))
    return out


def pack_mxfp4(W, exps, dtype, order=None):
    """W float32 [E, N, K] with block exponents [E, N, K / 32] -> samd_gemm_pack_f4's buffer of the E experts as one matrix of E N rows"""
    E, N, K = W.shape
    q, e8 = M.encode(W.numpy(), exps, dtype)
    if order is not None:
        q, e8 = q[:, order], e8[:, order]
    q, e8 = torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.from_numpy(np.ascontiguousarray(e8)).cuda()
    out = torch.empty(E * N * K // 2 + E * N * K // 32, dtype=torch.uint8, device="cuda")
    check(samd_hip.lib().samd_gemm_pack_f4(P(q), P(e8), P(out), E * N, K, current_stream()))
    return out


def run_gate_up(c, what):
    """launch every draw of a gate|up case; returns the last act"""
    L, R, dtype = samd_hip.lib(), c.R, c.dtype
    b = Block(R, 256, dtype)                                       # (the gate|up launch reads the routing part only)
    W = torch.cat((c.Wg, c.Wu), dim=1)                             # HF's fused gate_up_proj [E][2 I][H]
    if c.form:
        Wp = pack_mxfp4(W, np.concatenate(c.exps, axis=1), dtype, M.gate_up_row_order(c.inter))
        fn = L.samd_moe_gate_up_silu_f4
    else:
        Wp, fn = pack_model(W.to(dtype).cuda(), 1), L.samd_moe_gate_up_silu
    for h, want in c.draws:
        hd = h.to(dtype).cuda()
        act = torch.full((R.rows_pad * R.k, c.inter), NAN, dtype=dtype, device="cuda")
        check(fn(P(hd), P(Wp), P(b.ws), R.rows_pad, c.K, c.inter, R.E, R.k, P(act), b.dc, current_stream()))
        torch.cuda.synchronize()
        same(act[b.named], want[R.named].to(dtype), "act " + what)
        assert bool(torch.isnan(act[b.unnamed]).all()), "rows of act that no list names " + what
    return act


def launch_down(c, b, act, w):
    L, R = samd_hip.lib(), c.R
    if not hasattr(c, "Wp"):
        c.Wp = pack_mxfp4(c.W, c.exps, c.dtype) if c.form else pack_model(c.W.to(c.dtype).cuda(), 0)
    fn = L.samd_moe_down_combine_f4 if c.form else L.samd_moe_down_combine
    out = torch.full((R.rows_pad, c.N), NAN, dtype=c.dtype, device="cuda")
    check(fn(P(act), P(c.Wp), P(b.idx), P(w), P(b.d_n), P(b.ws), R.rows_pad, c.N, c.K, R.E, R.k, P(out), b.dc, current_stream()))
    torch.cuda.synchronize()
    return out


def run_down(c, what):
    """launch every draw of a down case; returns the last (y, out)"""
    R, dtype = c.R, c.dtype
    b = Block(R, c.N, dtype)
    w = c.w.to(dtype).cuda()
    for act, y, want in c.draws:
        b.y.fill_(NAN)
        out = launch_down(c, b, act.to(dtype).cuda(), w)
        same(b.y[b.named], y[R.named].to(dtype), "y " + what)
        assert bool(torch.isnan(b.y[b.unnamed]).all()), "rows of y that no list names " + what
        same(out, want.to(dtype), "out " + what)                   # rows >= n: exact zeros
    return b.y.clone(), out


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("rows_pad", M.ROWS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_gate_up_stores_the_rounded_product_of_every_list_entry(dtype, rows_pad, form):
    for kind, inter, chunks in M.gate_up_sweep(form, rows_pad):
        c = M.gate_up_case(dtype, M.routing(kind, rows_pad), inter, chunks, form, check=False)
        run_gate_up(c, f"{kind} inter={inter} chunks={chunks}")


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("rows_pad", M.ROWS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_down_and_combine_store_the_exact_sums(dtype, rows_pad, form):
    for kind, hidden, chunks, regime in M.down_sweep(form, rows_pad):
        c = M.down_case(dtype, M.routing(kind, rows_pad), hidden, chunks, regime, form, check=False)
        run_down(c, f"{kind} hidden={hidden} chunks={chunks} {regime}")


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_excluded_slots_add_nothing_exactly(dtype, form):
    """an out-of-range index and a repeated expert: no list names them, their rows of act and y stay NaN, and out is the reference with
    those slots empty"""
    R = M.routing("excluded", 16)
    run_gate_up(M.gate_up_case(dtype, R, 256, 2, form, check=False), "excluded")
    for regime in ("small", "large"):
        run_down(M.down_case(dtype, R, 256, 2, regime, form, check=False), "excluded " + regime)


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_a_row_alone_stores_the_bits_it_stores_as_row_40_of_64(dtype, form):
    """expert 0 holds all 64 rows and the row's other experts are shared too; alone the same row is tile row 0 of a 16-row launch"""
    gu, gu1, dn, dn1 = M.independence_cases(dtype, form)
    k = gu.R.k
    mine = slice(40 * k, 41 * k)
    act64, act1 = run_gate_up(gu, "64 rows"), run_gate_up(gu1, "alone")
    assert torch.equal(act1[:k], act64[mine])
    (y64, out64), (y1, out1) = run_down(dn, "64 rows"), run_down(dn1, "alone")
    assert torch.equal(y1[:k], y64[mine]) and torch.equal(out1[0], out64[40])


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_combine_adds_the_slots_in_ascending_order_in_fp32(dtype, k, form):
    """ascending fp32 gives 2^-11 on the unrotated rows; descending and a pairwise tree give 0, an exact sum 2^-10 + 2^-11"""
    c = M.order_case(dtype, k, form)
    b = Block(c.R, c.N, dtype)
    out = launch_down(c, b, c.act.to(dtype).cuda(), c.w.to(dtype).cuda())
    same(b.y, c.y.to(dtype), "y made by the down launch")
    same(out, c.out.to(dtype), "out in slot order")


@pytest.mark.parametrize("gate_up", [0, 1])
@pytest.mark.parametrize("E,inter", [(1, 128), (3, 320)])
def test_pack_experts_is_the_documented_permutation(E, inter, gate_up):
    """gate_up: N = 2 moe_inter (N % 128 == 0 with the half boundary inside a 128-row tile at 320); otherwise N = 128 / 384 as it is"""
    N, K = (2 * inter, 512) if gate_up else (128 if inter == 128 else 384, 256 * (1 + inter // 128))
    W = torch.arange(E * N * K // 2, dtype=torch.int32).view(torch.int16).view(E, N, K)      # every 4-byte word its own value: no unit repeats
    out = pack_model(W.cuda(), gate_up)
    assert np.array_equal(out.cpu().numpy().reshape(-1), M.pack_experts(W.numpy(), gate_up))
