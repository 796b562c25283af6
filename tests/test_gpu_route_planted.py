"""k_moe_route behind samd_moe_route and samd_moe_wide_route on the planted integer logits of tests/route_planting.py: the logits are exact
in fp32 in any order, so the selection is decided on EVERY row, ties included -- indices are compared by equality slot by slot on every
row of every case, weights by equality wherever their float64 value is more than 64 fp32 ulps from a rounding boundary of the model dtype
(either neighbour inside that band; at most 5 % of a case's weights, asserted).  Rows >= n hold NaN and must read -1 / 0; outputs and
workspace are poisoned before every launch.  The lists that follow the router are compared with the ones built in Python from the
reference indices (wide entry: samd_hip.moe.wide_lists_reference), and a planted row keeps its index and weight bits at every rows_pad,
row position and through the wide entry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import moe as MOE
import route_planting as RP

DT = {torch.float16: samd_hip.F16, torch.bfloat16: samd_hip.BF16}
INTER = 256                                                   # the buffers' expert width: no expert GEMM is launched here
ids = lambda s: "E{}_k{}_H{}_rows{}_n{}".format(*s)          # noqa: E731


def d_int(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def poison(b):
    b.topk_idx.fill_(RP.POISON_IDX), b.topk_w.fill_(float("nan")), b.ws.fill_(0xFF)


def outputs(b):
    torch.cuda.synchronize()
    return b.topk_idx.cpu().numpy().astype(np.int64), b.topk_w.double().cpu().numpy()


def held(case, ref, idx, w, dtype, norm):
    """compare, print what was seen, hold the cap"""
    band, other = RP.compare(case, ref, idx, w, dtype)
    print(f"ROUTE {case.name} {str(dtype)[6:]} norm={int(norm)}: {ref.band.size} weights compared, {band} in the band, {other} of them stored as the other neighbour")
    assert band <= RP.BAND_CAP * ref.band.size, (band, ref.band.size)
    for r in range(case.n):                                   # the exact plateaus: by equality, whatever the band says
        if RP.exact_plateau(case, r, norm):
            assert bool((w[r] == (1.0 / case.k if norm else 1.0 / case.E)).all()), (r, case.kinds[r], w[r].tolist())


@pytest.mark.parametrize("dtype", RP.DTYPES, ids=("f16", "bf16"))
@pytest.mark.parametrize("norm_topk", [True, False], ids=("norm", "raw"))
@pytest.mark.parametrize("shape", RP.ROUTE_SHAPES + (RP.EMPTY_SHAPE,), ids=ids)
def test_route_planted(shape, norm_topk, dtype):
    case = RP.route_case(shape)
    h, router = RP.tensors(case, dtype, "cuda")
    b = MOE.MoeBuffers(case.rows, case.H, INTER, case.E, case.k, dtype, DT[dtype], "cuda")
    poison(b)
    b.route(h, router, d_int(case.n), norm_topk)
    idx, w = outputs(b)
    ref = RP.reference(case.target, case.k, norm_topk, dtype)
    held(case, ref, idx, w, dtype, norm_topk)
    # the lists: built in Python from the REFERENCE indices -- no row is undecided
    n_active, active, counts, lists = b.routing_state()
    want = RP.lists_reference(ref.idx, case.n, case.k)
    assert (n_active, active, counts) == want[:3] and lists == want[3], case.name
    assert active == sorted(active) and all(lst == sorted(lst) for lst in lists)
    if case.n == 0:
        assert n_active == 0 and bool((idx == -1).all()) and bool((w == 0).all())


@pytest.mark.parametrize("dtype", RP.DTYPES, ids=("f16", "bf16"))
@pytest.mark.parametrize("norm_topk", [True, False], ids=("norm", "raw"))
@pytest.mark.parametrize("shape", RP.WIDE_SHAPES, ids=ids)
def test_wide_route_planted(shape, norm_topk, dtype):
    case = RP.route_case(shape)
    rows_pad = MOE.wide_rows_pad(case.rows)
    h, router = RP.tensors(case, dtype, "cuda", rows_alloc=rows_pad)
    b = MOE.MoeWideBuffers(case.rows, case.H, INTER, case.E, case.k, dtype, DT[dtype], "cuda")
    poison(b)
    b.route(h, router, d_int(case.n), norm_topk)
    b.lists(d_int(case.n))
    idx, w = outputs(b)                                       # all rows_pad rows: the rows behind `rows` read -1 / 0 too
    ref = RP.reference(case.target, case.k, norm_topk, dtype)
    held(case, ref, idx, w, dtype, norm_topk)
    got = b.routing_state()
    full = np.full((rows_pad, case.k), -1, np.int64)
    full[:case.n] = ref.idx
    want = MOE.wide_lists_reference(full.tolist(), case.n, case.E)
    assert got["n_tiles"] == len(want["tiles"]) and got["n_active"] == len(want["active"])
    for key in ("active", "counts", "offsets", "entries", "tiles"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("dtype", RP.DTYPES, ids=("f16", "bf16"))
@pytest.mark.parametrize("norm_topk", [True, False], ids=("norm", "raw"))
def test_a_planted_row_keeps_its_bits_wherever_it_sits(norm_topk, dtype):
    """16 planted rows (two of every plant), cyclically shifted so that each sits at other positions of launches of 16, 32, 48 and 64
    rows and of a wide launch of 130: index and weight bits per planted row are the same everywhere, and right"""
    E, k, H = 128, 8, 512
    base = RP.build_case(E, k, H, 16, 16, 4242, kind_offset=1, name="independence")
    ref = RP.reference(base.target, k, norm_topk, dtype)
    h16, router = RP.tensors(base, dtype, "cuda")
    first = None
    for rows, shift, wide in ((16, 0, False), (32, 5, False), (48, 11, False), (64, 3, False), (130, 7, True)):
        src = (torch.arange(MOE.wide_rows_pad(rows) if wide else rows) + shift) % 16
        h = h16[src.cuda()].contiguous()
        b = (MOE.MoeWideBuffers if wide else MOE.MoeBuffers)(rows, H, INTER, E, k, dtype, DT[dtype], "cuda")
        poison(b)
        b.route(h, router, d_int(rows), norm_topk)
        torch.cuda.synchronize()
        idx, bits = b.topk_idx[:rows].cpu(), b.topk_w[:rows].view(torch.int16).cpu()
        if first is None:
            first = (idx.clone(), bits.clone())
            RP.compare(base, ref, idx.numpy(), b.topk_w[:rows].double().cpu().numpy(), dtype)
        assert torch.equal(idx, first[0][src[:rows]]) and torch.equal(bits, first[1][src[:rows]]), (rows, shift)
        assert bool((b.topk_idx[rows:] == -1).all()) and bool((b.topk_w[rows:] == 0).all())
