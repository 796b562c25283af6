"""tests/silu_planting.py on the CPU: every case tests/test_gpu_silu_curve.py launches is built here, which runs the helper's conditions from
the reference alone -- the near-tie share (<= 1 % of the finite nonzero gates), products exact in fp32, exact and inexact gate sums, the
rounding share of the residues (>= 1/4), sweep coverage, the weight formats' dequantised values -- and `self_check` for every named fault
a case can show (each changes >= 5 % of the outputs it touches and >= 100 of them).  Torch's own fp32 F.silu(g).to(T) must equal the
float64 reference on every gate off the margin, which ties the restatement to HF's evaluation; the Python dequantisers of the package
must agree with the ones restated in the helper.  Run with -s for the shares.

The faults are checked per GPU test, over its sweep and rounding launches together: that is the unit that fails.

Recorded here (fp16 / bf16): near-tie gates 332 of 63486 (0.52 %) / 268 of 65278 (0.41 %) of the finite nonzero gates, 330 / 266 of them
with a nonzero result; torch's fp32 silu stores the neighbour on 1 / 0 of them.  Faults on the 64-row dense launches, changed / touched:
silu_not_rounded 21.0 % / 22.1 %, exp_in_T 11.8 % / 12.1 %, exp_sign 99.7 % / 100 %, gate_up_swapped 97.3 % / 98.0 %,
last_cast_truncates 46.4 % / 44.9 %, other_activation 86.1 % / 88.4 %, gate_not_rounded (gates of the curve that carry a residue)
31.5 % / 40.4 %, no_overflow_zero and exp_of_plus_g_overflow 100 %, last_cast_saturates 100 % (fp16); partials input: up_not_rounded
24.9 % / 31.1 %.  An unrounded gate gives another s_T on 37.4 % / 43.4 % of the residue-carrying gates (bar: a quarter).  The lowest share
anywhere is exp_in_T at 7.7 % (fp16, 9 rows of the norm-fold form).  23 tests in 5 s."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import silu_planting as S

IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}
dtypes = pytest.mark.parametrize("dtype", S.DTYPES, ids=list(IDS.values()))


def show(label, dtype, checked):
    print(f"{label} {IDS[dtype]}: " + ", ".join(f"{f} {c}/{n} ({100.0 * c / n:.1f} %)" for f, (c, n) in checked.items()))


@dtypes
def test_near_tie_gates_are_under_one_percent(dtype):
    share, n, tot = S.near_tie_share(dtype)
    c = S.curve(dtype)
    live = torch.isfinite(c.gate) & (c.gate != 0)
    nonzero = live & (c.s_T != 0)
    print(f"{IDS[dtype]}: {n} near-tie gates of {tot} finite nonzero ({100 * share:.2f} %); of {int(nonzero.sum())} with a nonzero result "
          f"{int((c.near & nonzero).sum())}")
    assert share <= S.NEAR_TIE_CAP
    assert bool((c.alt[~c.near] == c.s_T[~c.near])[torch.isfinite(c.s_T[~c.near])].all())
    assert bool((c.alt != c.s_T)[c.near].all())


@dtypes
def test_the_reference_at_the_ends_of_the_range(dtype):
    g = torch.tensor([float("inf"), float("-inf"), float("nan"), -89.0, -88.5, -1e30, 0.0, -0.0, 100.0], dtype=torch.float64)
    s = S.silu_ref(g)
    assert s[0].item() == float("inf") and bool(torch.isnan(s[1:3]).all())
    assert s[3].item() == 0 and np.signbit(s[3].item()) and s[5].item() == 0 and np.signbit(s[5].item())
    assert -4e-37 < s[4].item() < -3e-37 and s[6].item() == 0 and s[8].item() == 100.0
    if dtype == torch.bfloat16:                                   # the float64 value that bf16 could hold, and fp32 does not produce
        assert S.rounded(g[3:4] / (1.0 + torch.exp(-g[3:4])), dtype).item() != 0


@dtypes
def test_torch_fp32_silu_agrees_off_the_margin(dtype):
    c = S.curve(dtype)
    g = c.gate.to(dtype)
    hf = torch.nn.functional.silu(g.float()).to(dtype).double()
    bad = S.differs(hf, c.s_T) & ~c.near
    assert not bool(bad.any()), (IDS[dtype], c.gate[bad][:8].tolist())
    either = ~S.differs(hf, c.s_T) | ~S.differs(hf, c.alt)
    assert bool(either.all())
    print(f"{IDS[dtype]}: torch's fp32 silu stores the neighbour on {int(S.differs(hf, c.s_T).sum())} near-tie gates")


@dtypes
def test_up_pool(dtype):
    pool = S.up_pool(dtype)
    m = S.MANT[dtype]
    mant = torch.frexp(pool)[0].abs() * 2 ** (m + 1)
    assert bool((mant[2:] % 2 == 1).all()) and pool[:2].tolist() == [1.0, -1.0]
    mid = pool[2:26].abs()
    assert mid.min().item() >= 2.0 ** -6 and mid.max().item() < 2.0 ** 6 and bool((pool[2::2] == -pool[3::2]).sum() == 0)
    assert (len(pool) == 38) == (dtype == torch.float16)


@dtypes
def test_direct_case(dtype):
    c = S.direct_case(dtype)
    assert bool(torch.isnan(c.ref.want[torch.isnan(c.gate)]).all())
    assert bool(torch.isnan(c.ref.want[c.gate == float("-inf")]).all())
    pos = c.ref.want[c.gate == float("inf")]
    assert bool(torch.isinf(pos).all()) and bool((pos.sign() == c.up[c.gate == float("inf")].sign()).all())
    if dtype == torch.float16:                                    # overflowing products and subnormal results are among the outputs
        fin = torch.isfinite(c.gate)
        assert int((torch.isinf(c.ref.want) & fin).sum()) > 1000
        sub = (c.ref.want != 0) & (c.ref.want.abs() < 2.0 ** -14)
        assert int(sub.sum()) > 1000 and int((sub & (c.ref.want != c.ref.s_T * c.ref.u_T)).sum()) > 100
    show("direct", dtype, S.self_check(c.gate, c.up, dtype, S.direct_faults(dtype)))


@dtypes
@pytest.mark.parametrize("n_partials", S.PARTIALS_N)
def test_partials_cases(dtype, n_partials):
    c = S.partials_case(dtype, n_partials)
    assert c.parts.shape == (n_partials, S.PARTIALS_ROWS, 2 * S.PARTIALS_INTER)
    assert len(torch.unique(S.bits_of(c.ref.g_T, dtype))) > 0.99 * int(torch.isfinite(S.sweep(dtype)).sum())
    print(f"partials {n_partials} {IDS[dtype]}: unrounded gates give another s_T on {100 * c.rounding_share:.1f} %")
    show(f"partials {n_partials}", dtype, S.check_launches([c], dtype, True))


@dtypes
def test_dense_cases(dtype):
    cases = {rows: [S.dense_case(dtype, rows, rounding) for rounding in (False, True)] for rows in S.DENSE_ROWS}
    assert S.covers_finite_sweep(cases[64][:1], dtype)
    quarter = [cases[r][0] for r in (16, 32, 48)] + [S.dense_case(dtype, 16, False, (0, 4))]      # phases 1, 2, 3 and the one left
    assert S.covers_finite_sweep(quarter, dtype)
    for rows, pair in cases.items():
        assert all(c.gate.shape == (rows, S.DENSE_INTER) for c in pair)
        show(f"dense {rows} rows", dtype, S.check_launches(pair, dtype))
    print(f"dense 64 rows {IDS[dtype]}: unrounded gates give another s_T on {100 * cases[64][1].rounding_share:.1f} %")


@dtypes
def test_two_hot_lands_wrong_rows_and_columns_on_other_values(dtype):
    """a neighbouring row of h, a neighbouring output column's weights and another draw's permutation each change most outputs"""
    c = S.dense_case(dtype, 64, False)
    other = S.dense_case(dtype, 64, False, seed=1)
    ref = c.ref
    for name, gate, up in (("row_xor1", c.gate[torch.arange(64) ^ 1], c.up[torch.arange(64) ^ 1]),
                           ("column_next", c.gate.roll(1, 1), c.up.roll(1, 1)),
                           ("other_permutation", c.h @ other.Wg.t(), c.h @ other.Wu.t())):
        wrong = S.Ref(gate, up, dtype)
        # (a fifth of the fp16 gates lie below -17, where every result is -0 or +0 whatever the row: those cannot differ)
        changed = (S.differs(wrong.want, ref.want) & S.differs(wrong.want, ref.alt)).double().mean().item()
        assert changed > 0.75, (name, changed)


@dtypes
def test_norm_cases(dtype):
    for rows in S.NORM_ROWS:
        S.identity_case(dtype, rows)
        pair = [S.dense_case(dtype, rows, rounding, S.norm_plan(rows, dtype)) for rounding in (False, True)]
        show(f"norm {rows} rows", dtype, S.check_launches(pair, dtype))
    ssq = S.norm_ssq(S.DENSE_K)
    assert float(ssq.sum(0)[0]) / S.DENSE_K + S.NORM_EPS == 1.0
    assert [round(S.norm_plan(r, torch.float16)[1], 1) for r in S.NORM_ROWS] == [12.4, 7.8, 6.9, 3.9]


@dtypes
def test_moe_cases(dtype):
    W = S.moe_weights(dtype)
    for kind in S.MOE_KINDS + ("wide",):
        cases = [S.moe_case(dtype, kind, rounding, plan, W) for rounding in (False, True) for plan in S.moe_plans(kind)]
        if kind != "rows16":
            assert S.covers_finite_sweep(cases[:len(cases) // 2], dtype), kind
        for c in cases:
            assert sorted(p for lst in c.lists.values() for p in lst) == list(range(c.rows * S.MOE_K))
        show(f"moe {kind}", dtype, S.check_launches(cases, dtype))
    c = S.moe_case(dtype, "rows64", False, (0, 1), W)               # another expert's weights land on other values
    e_of = {p: e for e, lst in c.lists.items() for p in lst}
    nb = torch.stack([c.h[p // S.MOE_K] @ c.Wg[(e_of[p] + 1) % S.MOE_E].t() for p in range(c.rows * S.MOE_K)])
    nbu = torch.stack([c.h[p // S.MOE_K] @ c.Wu[(e_of[p] + 1) % S.MOE_E].t() for p in range(c.rows * S.MOE_K)])
    assert S.differs(S.Ref(nb, nbu, dtype).want, c.ref.want).double().mean().item() > 0.9


def test_every_format_holds_the_planted_weights_exactly():
    L, Wg, Wu = S.moe_weights(torch.bfloat16)
    W = torch.cat((Wg, Wu), dim=1)
    forms = S.checkpoint_forms(W)                                  # (asserts its own dequantisers)
    assert set(forms) == set(S.FORMATS) - {None}
    for dtype in S.DTYPES:
        assert torch.equal(S.rounded(W, dtype), W)
    # ... and the package's dequantisers say the same
    from samd_hip import moe as MOE
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    f = forms["mxfp4"]
    assert torch.equal(MOE.dequantize_experts(t(f["q"]), t(f["e8"])).double(), W)
    for name, deq in (("int4g128", MOE.dequantize_experts_int4), ("int8g128", MOE.dequantize_experts_int8)):
        f = forms[name]
        for dtype in S.DTYPES:
            assert torch.equal(deq(t(f["q"]), t(f["z"]), t(f["s"]).to(dtype)).double(), W), (name, dtype)
    f = forms["fp8b128"]
    assert torch.equal(MOE.dequantize_experts_fp8(t(f["q"]).view(torch.float8_e4m3fn), t(f["s"])).double(), W)
