"""tests/norm_planting.py on the CPU: its float64 RMSNorm against transformers' LlamaRMSNorm, the [hidden / 16][16] layout, ulp_T on normals
and subnormals, and every plan's own self check (each planted fault would miss its bar by the margins the GPU tests rely on)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import norm_planting as P

DTYPES = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden,eps", [(4096, 1e-6), (5120, 1e-5), (1000, 1e-6), (256, 1e-5)])
def test_reference_matches_transformers_llama_rmsnorm(dtype, hidden, eps):
    """the float64 reference with HF's roundings against LlamaRMSNorm run in `dtype` on the CPU (fp32 arithmetic inside): every element
    within 2 ulp_T (a 1-ulp flip of h = (x * rs).to(T) where fp32 and float64 1 / rms straddle a rounding boundary becomes up to 2 ulp of
    w * h), and at most 0.1 % of them different -- on randn rows and on the planted ones"""
    modeling = pytest.importorskip("transformers.models.llama.modeling_llama")
    rng = np.random.default_rng(hidden)
    w = P.norm_weight(rng, hidden, dtype)
    norm = modeling.LlamaRMSNorm(hidden, eps=eps)
    with torch.no_grad():
        norm.weight.copy_(w.to(torch.float32))
    norm = norm.to(dtype)
    planted, _ = P.plant(rng, 16, hidden, dtype, eps, P.vector_windows(hidden, 512))
    for x in (P.rounded(torch.from_numpy(rng.standard_normal((64, hidden))), dtype), planted):
        with torch.no_grad():
            got = norm(x.to(dtype)).to(P.F64)
        want = P.rmsnorm(x, w, eps, dtype)
        assert bool(((got - want).abs() <= P.ulp_bar(want, dtype)).all())
        assert P.mismatch(got, want) <= 1e-3


def test_ssq_layout_round_trips():
    rng = np.random.default_rng(1)
    y = torch.from_numpy(rng.standard_normal((7, 320)))
    lay = P.ssq_layout(y)
    assert lay.shape == (20, 16) and lay.dtype == torch.float32
    assert bool(torch.isnan(lay[:, 7:]).all())
    assert float(lay[3, 5]) == pytest.approx(float((y[5, 48:64] ** 2).sum()), rel=1e-7)
    assert torch.allclose(P.ssq_rows(lay, 7), P.tile_ssq(y), rtol=1e-7, atol=0)
    assert torch.allclose(P.tile_ssq(y).sum(-1), (y * y).sum(-1))


@pytest.mark.parametrize("dtype,mant,emin", [(torch.float16, 10, -14), (torch.bfloat16, 7, -126)])
def test_ulp_on_normals_and_subnormals(dtype, mant, emin):
    vals = torch.tensor([1.0, 1.5, 2.0, -3.0, 1000.0, 2.0 ** emin, 2.0 ** (emin - 3), 0.0], dtype=P.F64)
    want = [2.0 ** -mant, 2.0 ** -mant, 2.0 ** (1 - mant), 2.0 ** (1 - mant), 2.0 ** (9 - mant)] + [2.0 ** (emin - mant)] * 3
    assert P.ulp(vals, dtype).tolist() == want
    # the spacing is the distance to the next representable value, subnormals included
    for v in vals.tolist()[:-1]:
        t = torch.tensor([abs(v)], dtype=dtype)
        nxt = torch.nextafter(t.float(), torch.tensor([float("inf")])).to(dtype)            # fp32 nextafter, rounded up to T
        step = float(t.to(P.F64) + P.ulp(t.to(P.F64), dtype)) - float(t.to(P.F64))
        assert float(P.rounded(torch.tensor([abs(v) + step]), dtype)) == abs(v) + step                # t + ulp is representable ...
        assert float(P.rounded(torch.tensor([abs(v) + step / 4]), dtype)) == abs(v)                  # ... and nothing nearer is
        assert float(nxt) >= abs(v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,hidden,eps", [(16, 4096, 1e-6), (7, 1000, 1e-5), (64, 8192, 1e-5), (16, 5120, 1e-6), (16, 256, 1e-5)])
def test_rmsnorm_plans_pass_their_self_check(dtype, rows, hidden, eps):
    rng = np.random.default_rng(rows + hidden)
    x, plan = P.plant(rng, rows, hidden, dtype, eps, P.vector_windows(hidden, min(1024, max(64, hidden // 8))))
    w = P.norm_weight(rng, hidden, dtype)
    want = P.rmsnorm(x, w, eps, dtype)
    mx, rd = P.rmsnorm_faults(x, w, eps, dtype, plan)
    done = P.self_check_max(plan, want, mx, P.ulp_bar(want, dtype))
    assert set(done) == set(P.MAX_FAULTS)
    P.self_check_fraction(want, rd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", [4096, 5120, 8192])
def test_fold_plans_pass_their_self_check(dtype, hidden):
    """the fold kernels' plans: seam tiles of norm_issue, the per-row bars of P.fold_miss on a gate|up-shaped output"""
    rng = np.random.default_rng(hidden)
    tiles = hidden // P.TILE
    x, plan = P.plant(rng, 16, hidden, dtype, 1e-5, [P.TILE * t for t in P.seam_tiles(tiles)])
    w = P.norm_weight(rng, hidden, dtype)
    inter = 64
    Wg = P.rounded(torch.from_numpy(rng.standard_normal((inter, hidden))) * hidden ** -0.5, dtype)
    Wu = P.rounded(torch.from_numpy(rng.standard_normal((inter, hidden))) * hidden ** -0.5, dtype)
    want = P.pairs_silu_norm(x, w, 1e-5, Wg, Wu, dtype)
    wrongs = {f: P.pairs_silu_norm(x, w, 1e-5, Wg, Wu, dtype, f, plan.hot) for f in P.MAX_FAULTS}
    assert set(P.self_check_max(plan, want, wrongs, lambda a, b: P.fold_miss(a, b, dtype), factor=P.ACT_MISS)) == set(P.MAX_FAULTS)


def test_seam_tiles_cover_every_round():
    assert P.seam_tiles(256) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255]
    assert P.seam_tiles(320)[-3:] == [287, 288, 319] and len(P.seam_tiles(512)) == 32


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_rounding_faults_are_visible(dtype):
    """the residual add from a rounded projection / from partials whose sum is rounded first: dropping that rounding changes >= 10 % of
    the elements at K = 4096-like magnitudes (the caps are 1 %)"""
    rng = np.random.default_rng(5)
    x, _ = P.plant(rng, 16, 1024, dtype, 1e-6)
    A = P.rounded(torch.from_numpy(rng.standard_normal((16, 512))), dtype)
    W = P.rounded(torch.from_numpy(rng.standard_normal((1024, 512))) * 512 ** -0.5, dtype)
    y, p = P.cs_residual(x, A, W, dtype)
    P.self_check_fraction(y, {"no_proj_round": P.cs_residual(x, A, W, dtype, "no_proj_round")[0]})
    parts = P.grid_values(rng, (9, 16, 1024), bound=0.5)
    P.self_check_fraction(P.add_partials(x, parts, dtype), {"no_proj_round": P.add_partials(x, parts, dtype, "no_proj_round")})
    # partials on the grid add up exactly in fp32: the float32 sum equals the float64 one
    assert torch.equal(parts.float().sum(0).double(), parts.sum(0))
