"""Every SiLU epilogue held by equality across the whole gate range of the model dtype, on inputs planted by tests/silu_planting.py: the
stored value must be round_T(round_T(silu(round_T(gate))) * round_T(up)) with silu evaluated as HF's fp32 act_fn does (the helper's float64
restatement; torch's own fp32 silu agrees with it on every gate off the margin, tests/test_silu_planting_cpu.py).  Off the margin of 32
fp32 ulps round a rounding boundary of T the comparison is equality of the stored values (+-0 equal, NaN positions must coincide); on a
near-tie gate (under 1 % of the gates) the launch must store one of the two adjacent values.  Outputs start NaN-filled.

  entry point                          inputs                                              launches per test
  samd_silu_mul, T input               all 2^16 gate patterns, inf and NaN included, 8     1
                                       rows rotated by one element (every gate in every
                                       lane of the 8-element vector)
  samd_silu_mul, fp32 partials         1 and 3 partials summing exactly to gates AND ups   1
                                       that are no T values; the finite sweep, inter 8192
  samd_gemm_pairs_silu, _skinny_silu   two-hot planting, K 2048, inter 1024; 64 rows: every 2 + 2 (and the two kernels against each other)
                                       finite gate; 16 / 32 / 48 rows: a strided quarter,
                                       another phase each; a sweep launch and a rounding
                                       launch (residues of 3/8 ulp on gates of the curve)
  samd_gemm_pairs_silu_norm            the same at rows 5, 8, 9, 16 with ssq, eps and the  1 + 2
                                       norm weight planted so that the scale is exactly 1
                                       (first: the identity region returns x bit for bit)
  samd_moe_gate_up_silu, _f4, _i4,     hidden 1024, moe_inter 512, 4 experts, top-k 2,     64 rows: 2 + 2 (a row's two experts read the
  _i8, _f8                             lists from samd_moe_lists; 64 rows; 16 rows with    same 512 gates); 16 rows: 1 + 1
                                       one expert empty and one holding a single pair
  samd_moe_wide_gate_up_silu           192 rows (lists of 130, 96, 96, 62 pairs), expert   1 + 1 per format
                                       formats 0, 1, 2, 3, 5

The weights are +-1 and 0, which every format holds exactly (silu_planting.checkpoint_forms asserts it through the dequantisers).  The
cases and their references are built once and shared by the formats.  Run with -s for the number of near-tie outputs on which the device
stored the neighbouring value (a measurement, not an assertion).

Recorded on an MI355X: 52 tests in 5.0 s, all equal; the neighbour was stored on 1 of 332 near-tie fp16 gates and 0 of 268 bf16 gates
(samd_silu_mul), on at most 8 of 1164 near-tie outputs of any GEMM launch; rsqrtf(1.0f) is exactly 1 (the identity precondition of the
norm-fold form held at all four row counts).  Scratch builds with one changed line each, this file / the 32 existing tests that reach the
epilogue: silu(gate) not rounded 52 failed / all pass; __expf rounded to T 52 failed / all pass; the gate sum not rounded at the three GEMM
sites 46 failed / all pass."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import moe_planting as MP
import silu_planting as S
import samd_hip
from samd_hip import _ptr as P, check, current_stream, torch_dtype_code
from samd_hip import moe as MOE
from test_gpu_gemm_exact import dev, interleave, packed
from test_gpu_moe_exact import Block, pack_model

NAN = float("nan")
IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}
dtypes = pytest.mark.parametrize("dtype", S.DTYPES, ids=list(IDS.values()))
formats = pytest.mark.parametrize("fmt", S.FORMATS, ids=[f or "model" for f in S.FORMATS])
GATE_UP = {None: "samd_moe_gate_up_silu", "mxfp4": "samd_moe_gate_up_silu_f4", "int4g128": "samd_moe_gate_up_silu_i4",
           "int8g128": "samd_moe_gate_up_silu_i8", "fp8b128": "samd_moe_gate_up_silu_f8"}


def held(got, ref, dtype, what, gate=None):
    """equality with ref.want; where the gate is near-tie, ref.alt is right as well.  Returns (outputs on which the neighbour was stored,
    near-tie outputs)"""
    want, alt = ref.want.to(dtype).to(got.device), ref.alt.to(dtype).to(got.device)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    eq = (got == want) | (torch.isnan(got) & torch.isnan(want))
    ok = eq | (got == alt)
    if not bool(ok.all()):
        bad = torch.nonzero(~ok)
        i = tuple(bad[0].tolist())
        g = (ref.g_T if gate is None else gate)[i].item()
        pytest.fail(f"{what}: {len(bad)} of {got.numel()} stored values differ; first at {i}: gate {g!r} up {ref.u_T[i].item()!r} "
                    f"got {got[i].item()!r}, want {want[i].item()!r} (near-tie: {bool(ref.near[i])})")
    n, near = int((~eq).sum()), int(ref.near.sum())
    print(f"{what} {IDS[dtype]}: the neighbour on {n} of {near} near-tie outputs ({got.numel()} outputs)")
    return ~eq, near


def nan_out(rows, inter, dtype):
    return torch.full((rows, inter), NAN, device="cuda", dtype=dtype)


# ---- samd_silu_mul --------------------------------------------------------------------------------------------------------------------------------
@dtypes
def test_silu_mul_over_every_bit_pattern(dtype):
    c = S.direct_case(dtype)
    gu = torch.cat((c.gate, c.up), dim=1).to(dtype).cuda().contiguous()
    out = nan_out(S.DIRECT_ROWS, S.DIRECT_INTER, dtype)
    check(samd_hip.lib().samd_silu_mul(P(gu), P(out), S.DIRECT_ROWS, S.DIRECT_INTER, torch_dtype_code(dtype), 0, 0, current_stream()))
    torch.cuda.synchronize()
    moved, _ = held(out, c.ref, dtype, "samd_silu_mul", c.gate)
    gates = torch.unique(S.bits_of(c.gate[moved.cpu()], dtype))
    print(f"samd_silu_mul {IDS[dtype]}: the neighbour on {len(gates)} of {int(S.curve(dtype).near.sum())} near-tie GATES")


@dtypes
@pytest.mark.parametrize("n_partials", S.PARTIALS_N)
def test_silu_mul_rounds_the_sums_of_its_partials(dtype, n_partials):
    c = S.partials_case(dtype, n_partials)
    rows, inter = S.PARTIALS_ROWS, S.PARTIALS_INTER
    parts = c.parts.float().cuda().contiguous()
    out = nan_out(rows, inter, dtype)
    check(samd_hip.lib().samd_silu_mul(P(parts), P(out), rows, inter, torch_dtype_code(dtype), n_partials, rows * 2 * inter, current_stream()))
    torch.cuda.synchronize()
    held(out, c.ref, dtype, f"samd_silu_mul {n_partials} partials")


# ---- the dense GEMM epilogues -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_weights(dtype, rows, plan=None):
    """the packed two-hot weights of a row count (the sweep and the rounding launch share them) and the two cases"""
    L = samd_hip.lib()
    cases = [S.dense_case(dtype, rows, rounding, plan) for rounding in (False, True)]
    c = cases[0]
    assert all(torch.equal(x.Wg, c.Wg) and torch.equal(x.Wu, c.Wu) for x in cases)
    wg, wu = dev(c.Wg, dtype), dev(c.Wu, dtype)
    inter, K = c.L.inter, c.L.K
    w16 = packed(L.samd_gemm_pack_groups, interleave(wg, wu, 16), 2 * inter, K)
    w64 = packed(L.samd_gemm_pack_weights, interleave(wg, wu, 64), 2 * inter, K)
    return cases, w16, w64


@dtypes
@pytest.mark.parametrize("rows", S.DENSE_ROWS)
def test_pairs_silu_and_skinny_silu(dtype, rows):
    L, dc = samd_hip.lib(), torch_dtype_code(dtype)
    cases, w16, w64 = dense_weights(dtype, rows)
    for c, kind in zip(cases, ("sweep", "rounding")):
        inter, K = c.L.inter, c.L.K
        A = dev(c.h, dtype)
        out, ref = nan_out(rows, inter, dtype), nan_out(rows, inter, dtype)
        check(L.samd_gemm_pairs_silu(P(A), P(w16), rows, inter, K, P(out), dc, current_stream()))
        check(L.samd_gemm_skinny_silu(P(A), P(w64), rows, 2 * inter, K, P(ref), dc, current_stream()))
        torch.cuda.synchronize()
        held(out, c.ref, dtype, f"samd_gemm_pairs_silu {rows} rows {kind}")
        held(ref, c.ref, dtype, f"samd_gemm_skinny_silu {rows} rows {kind}")
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), "the two kernels store the same bits"


@dtypes
@pytest.mark.parametrize("rows", S.NORM_ROWS)
def test_pairs_silu_norm_at_a_scale_of_exactly_one(dtype, rows):
    L, dc = samd_hip.lib(), torch_dtype_code(dtype)
    K, inter = S.DENSE_K, S.DENSE_INTER
    ssq = S.norm_ssq(K).cuda()
    gamma = torch.ones(K, device="cuda", dtype=dtype)

    def launch(h, Wg, Wu):
        x = torch.full((16, K), NAN, device="cuda", dtype=dtype)      # rows >= `rows` are not fetched
        x[:rows] = dev(h, dtype)
        w16 = packed(L.samd_gemm_pack_groups, interleave(dev(Wg, dtype), dev(Wu, dtype), 16), 2 * inter, K)
        out = nan_out(16, inter, dtype)
        check(L.samd_gemm_pairs_silu_norm(P(x), P(ssq), P(gamma), S.NORM_EPS, P(w16), rows, inter, K, P(out), dc, current_stream()))
        torch.cuda.synchronize()
        assert bool((out[rows:] == 0).all()), "rows >= rows_pad are those of a zero input"
        return out[:rows]
    # the precondition: rsqrtf(1.0f) is exactly 1 and the norm passes x through, so gates >= 24 with up = 1 come back bit for bit
    i = S.identity_case(dtype, rows)
    got = launch(i.h, i.Wg, i.Wu)
    assert torch.equal(got, i.want.to(dtype).cuda()), "the launch's own scale is not exactly 1: rsqrtf(1.0f) != 1 on this device?"
    for rounding, kind in ((False, "sweep"), (True, "rounding")):
        c = S.dense_case(dtype, rows, rounding, S.norm_plan(rows, dtype))
        held(launch(c.h, c.Wg, c.Wu), c.ref, dtype, f"samd_gemm_pairs_silu_norm {rows} rows {kind}")


# ---- the expert GEMM epilogues ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moe_cases(dtype, kind):
    W = S.moe_weights(dtype)
    return [(S.moe_case(dtype, kind, rounding, plan, W), f"{name} {i}") for rounding, name in ((False, "sweep"), (True, "rounding"))
            for i, plan in enumerate(S.moe_plans(kind))]


@functools.lru_cache(maxsize=None)
def moe_packed(dtype, fmt):
    """the fused gate|up tensor [E, 2 I, H] of the two-hot weights in the buffer the format's launches stream"""
    Lib = samd_hip.lib()
    L, Wg, Wu = S.moe_weights(dtype)
    W = torch.cat((Wg, Wu), dim=1)
    E, N, K = W.shape
    if fmt is None:
        return pack_model(W.to(dtype).cuda(), 1)
    f = S.checkpoint_forms(W)[fmt]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if fmt == "mxfp4":
        order = MP.gate_up_row_order(L.inter)
        q, e8 = t(f["q"][:, order]), t(f["e8"][:, order])
        out = torch.empty(E * N * K // 2 + E * N * K // 32, dtype=torch.uint8, device="cuda")
        check(Lib.samd_gemm_pack_f4(P(q), P(e8), P(out), E * N, K, current_stream()))
        return out
    I = L.inter
    if fmt == "fp8b128":                                           # (the down side of the pack call is not launched)
        down = (torch.zeros((E, K, I), dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn), torch.ones((E, K // 128, I // 128), device="cuda"))
        return MOE.pack_experts_fp8((t(f["q"]).view(torch.float8_e4m3fn), t(f["s"])), down)[0]
    four = fmt == "int4g128"
    down = (torch.zeros((E, K, I // 2 if four else I), dtype=torch.uint8, device="cuda"), torch.zeros((E, K, I // 128), dtype=torch.uint8, device="cuda"),
            torch.ones((E, K, I // 128), dtype=dtype, device="cuda"))
    gu = (t(f["q"]), t(f["z"]), t(f["s"]).to(dtype))
    return (MOE.pack_experts_int4 if four else MOE.pack_experts_int8)(gu, down, dtype)[0]


@dtypes
@formats
@pytest.mark.parametrize("kind", S.MOE_KINDS)
def test_moe_gate_up_silu(dtype, fmt, kind):
    Lib, dc = samd_hip.lib(), torch_dtype_code(dtype)
    Wp = moe_packed(dtype, fmt)
    fn = getattr(Lib, GATE_UP[fmt])
    b = None
    for c, name in moe_cases(dtype, kind):
        if b is None:                                              # one routing per kind: the lists are built once, by samd_moe_lists
            b = Block(MP.Routing(kind, S.MOE_E, S.MOE_K, c.rows, c.rows, c.idx), 256, dtype)
            assert b.R.lists == c.lists
        act = nan_out(c.rows * S.MOE_K, c.L.inter, dtype)
        check(fn(P(dev(c.h, dtype)), P(Wp), P(b.ws), c.rows, c.L.K, c.L.inter, S.MOE_E, S.MOE_K, P(act), dc, current_stream()))
        torch.cuda.synchronize()
        held(act, c.ref, dtype, f"{GATE_UP[fmt]} {kind} {name}")


@dtypes
@formats
def test_moe_wide_gate_up_silu(dtype, fmt):
    Lib, dc = samd_hip.lib(), torch_dtype_code(dtype)
    Wp = moe_packed(dtype, fmt)
    code = MOE.WIDE_FORMAT_CODES_SERVED[fmt]
    rows, E, k = S.WIDE_ROWS, S.MOE_E, S.MOE_K
    ws = None
    for c, name in moe_cases(dtype, "wide"):
        if ws is None:
            idx, d_n = torch.from_numpy(c.idx).cuda(), torch.tensor([rows], dtype=torch.int32, device="cuda")
            ws = torch.full((Lib.samd_moe_wide_workspace(rows, c.L.K, c.L.inter, E, k, dc),), 0xFF, dtype=torch.uint8, device="cuda")
            check(Lib.samd_moe_wide_lists(P(idx), P(d_n), rows, E, k, P(ws), current_stream()))
        act = nan_out(rows * k, c.L.inter, dtype)
        check(Lib.samd_moe_wide_gate_up_silu(P(dev(c.h, dtype)), P(Wp), P(ws), rows, c.L.K, c.L.inter, E, k, code, P(act), dc, current_stream()))
        torch.cuda.synchronize()
        held(act, c.ref, dtype, f"samd_moe_wide_gate_up_silu format {code} {name}")
