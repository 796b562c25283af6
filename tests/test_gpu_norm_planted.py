"""RMSNorm and residual-stream parity on PLANTED rows (tests/norm_planting.py): rows whose scales are orders of magnitude apart, rows with
95 % of their energy in one 16-column tile (at tile 0, the last tile, both sides of every 32-tile round of norm_issue), rows where eps
decides 1 / rms, Llama-2-style massive activations, zero rows and norm weights of +-[0.5, 4].  Every launch is compared DIRECTLY with a
float64 reference that rounds to the model dtype where HF does, and every case first proves that the faults its rows target would miss its
bars (max-error faults by >= 50x, rounding faults by >= 10x the mismatch cap).

  samd_rmsnorm / _warm            out: every element <= 2 ulp_T, <= 1 % of the elements different; x after a T delta add bit-exact, after
                                  1..11 fp32 partials (sums exact in fp32 by construction) bit-exact; the warm form bit-identical
  samd_embed_rows_ssq / _rope     rows bit-exact, every tile's sum of squares within 2e-6 relative, cs rows bit-exact at the clamped
                                  position, rows beyond `rows` / `rope_rows` untouched
  samd_gemm_cs_residual (_early)  y per element within cs_residual_bar (1 ulp_T(y) + 1 ulp_T(p + slack) + slack, slack = the depth-d fp32
                                  summation bound, norm_planting.accumulation_slack), <= 1 % of the elements different
  samd_gemm_qkv_rope_norm / _vt,  per (row, head) / per row: tol x max(|want_row|_inf, 0.25), tol 4e-3 fp16 / 3e-2 bf16; nothing but q rows
  samd_gemm_pairs_silu_norm       < n and cache rows [L, L + n) written; NaN sums of squares of rows >= rows_pad never reach the others;
                                  through an identity V projection the folded norm itself is held to the RMSNorm bars
  MLP chain                       samd_embed_rows_ssq -> 3 x (pairs_silu_norm -> cs_residual) -> samd_rmsnorm with _forward_rows_fold's
                                  row counts, against the float64 chain
  samd_sum_partials_bias          1..12 partials, bias or none: bit-exact (grid partials: one rounding)"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_planting as P
import samd_hip
from samd_hip import _ptr, check

DTYPES = [torch.float16, torch.bfloat16]
F64 = P.F64


def env(dtype):
    return samd_hip.lib(), samd_hip.current_stream(), samd_hip.torch_dtype_code(dtype)


def gpu(x, dtype):
    return torch.as_tensor(x).to(device="cuda", dtype=dtype).contiguous()


def rand_matrix(seed, rows, cols, scale, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn((rows, cols), generator=g, device="cuda") * scale).to(dtype)


def expect_ulp(got, want, dtype, label, ulps=P.ULP_BAR, cap=P.FRAC_CAP):
    g = got.to(F64)
    bad = ~((g - want).abs() <= ulps * P.ulp(want, dtype))
    assert not bool(bad.any()), f"{label}: {int(bad.sum())} elements beyond {ulps} ulp, first at {torch.nonzero(bad)[:6].tolist()}"
    f = P.mismatch(g, want)
    assert f <= cap, f"{label}: {f:.4f} of the elements differ from the reference (cap {cap})"


def expect_rows(got, want, dtype, label):
    """per (row, head) -- or per row for 2-D outputs -- tol x max(|want_row|_inf, FLOOR), and the same in the 2-norm (P.fold_miss)"""
    m = P.fold_miss(got.to(F64), want, dtype)
    bad = torch.nonzero(m > 1).flatten().tolist()
    assert not bad, f"{label}: rows {bad[:8]} beyond the bar ({[round(float(m[i]), 2) for i in bad[:8]]} x tol)"


def fold_bar(dtype):
    return lambda wrong, want: P.fold_miss(wrong, want, dtype)


def sub_plan(plan, n):
    return P.Plan(plan.kind[:n], plan.hot[:n], plan.eps)


# ---- samd_rmsnorm / samd_rmsnorm_warm ---------------------------------------------------------------------------------------------------
_WARM = {}


def warm_target():
    """a real packed projection for the warm-up workgroups to read (N 1024, K 4096, 2 splits)"""
    if "w" not in _WARM:
        L, st, _ = env(torch.float16)
        w = rand_matrix(7, 1024, 4096, 0.05, torch.float16)
        wp = torch.empty_like(w)
        check(L.samd_gemm_pack_weights(_ptr(w), _ptr(wp), 1024, 4096, st))
        _WARM["w"] = wp
        _WARM["s"] = samd_hip.Warm(wp.data_ptr(), 1024, 4096, 2, 64, 2, 0)
    return _WARM["s"]


def residual_input(rng, x, plan, mode, dtype):
    """x0 and the delta (T tensor or fp32 grid partials, scaled per row by a power of two so their sums stay exact) whose add gives rows
    that keep the plan's character: the delta is ~0.5 of the row's RMS (fp32 partials: their sum), zero for zero rows"""
    rows, hidden = x.shape
    rms = x.pow(2).mean(-1).sqrt()
    if mode == "delta":
        d = P.rounded(torch.from_numpy(rng.standard_normal((rows, hidden))) * 0.5 * rms[:, None], dtype)
        return d
    n = mode
    parts = P.grid_values(rng, (n, rows, hidden), bound=1.0)
    sc = torch.where(rms > 0, torch.exp2(torch.round(torch.log2(0.5 * rms.clamp(min=1e-30) / math.sqrt(n / 3)))), torch.zeros_like(rms))
    return parts * sc[None, :, None]


def rmsnorm_case(rng, rows, hidden, dtype, mode):
    """planted rows x0, the residual operand of `mode` (None, "delta" or a partial count) as the launch takes it, the rows after the add
    x1, the norm weight and the reference output -- after the plan's self checks"""
    eps = 1e-5 if hidden % 2048 else 1e-6
    threads = min(1024, max(64, ((hidden // 8 + 63) // 64) * 64))
    x0, plan = P.plant(rng, rows, hidden, dtype, eps, P.vector_windows(hidden, threads))
    w = P.norm_weight(rng, hidden, dtype)
    label = f"rows {rows} hidden {hidden} residual {mode}"
    if mode is None:
        x1, delta, n_part, stride = x0, None, 0, 0
    elif mode == "delta":
        dl = residual_input(rng, x0, plan, mode, dtype)
        x1, delta, n_part, stride = P.add_delta(x0, dl, dtype), dl.to(dtype), 0, 0
    else:
        parts = residual_input(rng, x0, plan, mode, dtype)
        x1 = P.add_partials(x0, parts, dtype)
        P.self_check_fraction(x1, {"no_proj_round": P.add_partials(x0, parts, dtype, "no_proj_round")}, label=label)
        stride = rows * hidden + 64                               # a stride longer than the tensor: the launch must use it
        delta = torch.full((mode, stride), float("nan"), dtype=torch.float32)
        delta[:, :rows * hidden] = parts.reshape(mode, -1).float()
        n_part = mode
    want = P.rmsnorm(x1, w, eps, dtype)
    mx, rd = P.rmsnorm_faults(x1, w, eps, dtype, plan)
    P.self_check_max(plan, want, mx, P.ulp_bar(want, dtype), label)
    P.self_check_fraction(want, rd, label=label)
    return x0, delta, n_part, stride, x1, w, eps, want, label


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", [256, 1000, 4096, 5120, 8192])
@pytest.mark.parametrize("rows", [1, 7, 16, 64])
def test_rmsnorm_planted(dtype, rows, hidden):
    L, st, dc = env(dtype)
    rng = np.random.default_rng(rows * 10007 + hidden)
    warm = warm_target()
    for mode in (None, "delta", 1, 2, 8, 9, 11):
        x0, delta, n_part, stride, x1, w, eps, want, label = rmsnorm_case(rng, rows, hidden, dtype, mode)
        d = None if delta is None else delta.cuda()
        wd = gpu(w, dtype)
        res = []
        for nxt in (None, warm):
            xd = gpu(x0, dtype)
            out = torch.full((rows, hidden), float("nan"), device="cuda", dtype=dtype)
            if nxt is None:
                check(L.samd_rmsnorm(_ptr(xd), _ptr(d), _ptr(wd), _ptr(out), rows, hidden, eps, dc, n_part, stride, st))
            else:
                check(L.samd_rmsnorm_warm(_ptr(xd), _ptr(d), _ptr(wd), _ptr(out), rows, hidden, eps, dc, n_part, stride, C.byref(nxt), st))
            torch.cuda.synchronize()
            res.append((xd, out))
        (xd, out), (xw, outw) = res
        assert torch.equal(xd.to(F64).cpu(), x1), f"{label}: x after the residual add differs from the reference"
        expect_ulp(out.cpu(), want, dtype, label)
        assert torch.equal(xw, xd) and torch.equal(outw, out), f"{label}: samd_rmsnorm_warm differs from samd_rmsnorm"


# ---- samd_embed_rows_ssq / samd_embed_rows_ssq_rope ---------------------------------------------------------------------------------------
def expect_ssq(ssq, y, rows, label):
    """every tile of rows < `rows` within 2e-6 relative of the float64 sum over the STORED rows y; the rest still NaN"""
    want = P.tile_ssq(y.to(F64))
    got = ssq[:, :rows].t().to(F64)
    err = (got - want).abs()
    assert bool((err <= 2e-6 * want).all()), f"{label}: sums of squares off by up to {float((err / want.clamp(min=1e-300)).max()):.2e} relative"
    assert bool(torch.isnan(ssq[:, rows:]).all()), f"{label}: sums of squares of rows >= {rows} written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", [4096, 5120, 8192])
def test_embed_rows_ssq_and_rope_rows(dtype, hidden):
    L, st, dc = env(dtype)
    rng = np.random.default_rng(hidden)
    vocab, max_pos = 40, 300
    table, _ = P.plant(rng, vocab, hidden, dtype, 1e-5, [P.TILE * t for t in P.seam_tiles(hidden // 16)],
                       kinds=[P.PATTERN[r % 8] for r in range(vocab)])
    tab = gpu(table, dtype)
    cos_t = torch.from_numpy(rng.uniform(-1, 1, (max_pos, 64))).float().cuda()
    sin_t = torch.from_numpy(rng.uniform(-1, 1, (max_pos, 64))).float().cuda()
    base = max_pos - 6
    rel = np.arange(64, dtype=np.int32)
    rel[3] = -base - 5                                           # position below 0: clamped to 0
    d_rel, d_base = gpu(rel, torch.int32), gpu([base], torch.int32)
    for rows in (16, 5):
        toks = rng.integers(0, vocab, rows).astype(np.int32)
        toks[0], toks[-1] = -3, vocab + 7                         # out-of-range tokens: clamped to 0 / vocab - 1
        want_x = table[np.clip(toks, 0, vocab - 1)]
        d_toks = gpu(toks, torch.int32)
        for R in ((None,) if rows == 5 else (1, 8, 9, 64)):
            x = torch.full((16, hidden), float("nan"), device="cuda", dtype=dtype)
            ssq = torch.full((hidden // 16, 16), float("nan"), device="cuda", dtype=torch.float32)
            label = f"rows {rows} rope rows {R}"
            if R is None:
                check(L.samd_embed_rows_ssq(_ptr(d_toks), _ptr(tab), _ptr(x), _ptr(ssq), rows, hidden, vocab, dc, st))
            else:
                cs = torch.full((64, 128), float("nan"), device="cuda")
                check(L.samd_embed_rows_ssq_rope(_ptr(d_toks), _ptr(tab), _ptr(x), _ptr(ssq), rows, hidden, vocab, dc, _ptr(d_rel), _ptr(d_base),
                                                 _ptr(cos_t), _ptr(sin_t), _ptr(cs), R, 128, max_pos, st))
            torch.cuda.synchronize()
            assert torch.equal(x[:rows].to(F64).cpu(), want_x) and bool(torch.isnan(x[rows:]).all()), label
            expect_ssq(ssq, x[:rows], rows, label)
            if R is not None:
                pos = np.clip(base + rel[:R].astype(np.int64), 0, max_pos - 1)
                want_cs = torch.cat((cos_t[pos], sin_t[pos]), dim=1)
                assert torch.equal(cs[:R], want_cs) and bool(torch.isnan(cs[R:]).all()), label


# ---- samd_gemm_cs_residual (+ _early) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K", [(4096, 4096), (5120, 4096), (4096, 11008), (5120, 13824), (4096, 14336)])
def test_cs_residual_planted(dtype, N, K):
    """y = (x + (A W^T).to(T)).to(T) and the sums of squares of the stored y, at rows_pad 8 and 16.  Bar per element:
    1 ulp_T(y) (the final rounding) + 1 ulp_T(|p| + slack) (the projection's rounding may flip) + slack, where slack = (K / 128 + 64)
    2^-24 sum_k |a_k w_k| bounds the fp32 summation error of a depth <= K / 128 + 64 summation; at most 1 % of the elements may differ."""
    L, st, dc = env(dtype)
    rng = np.random.default_rng(N + K)
    W = rand_matrix(N + K, N, K, K ** -0.5, dtype)
    Wg = torch.empty_like(W)
    check(L.samd_gemm_pack_groups(_ptr(W), _ptr(Wg), N, K, st))
    A = rand_matrix(K, 16, K, 1.0, dtype)
    x0, plan = P.plant(rng, 16, N, dtype, 1e-6)
    A64, W64, x64 = A.to(F64), W.to(F64), x0.cuda()
    want, p = P.cs_residual(x64, A64, W64, dtype)
    slack = P.accumulation_slack(A64, W64, K)
    bar = P.cs_residual_bar(want, p, slack, dtype)
    P.self_check_fraction(want, {"no_proj_round": P.cs_residual(x64, A64, W64, dtype, "no_proj_round")[0]}, label=f"N {N} K {K}")
    del W64
    early = None
    for rows_pad in (8, 16):
        a = A.clone()
        a[rows_pad:] = float("nan")                                # rows the launch must not read
        x = gpu(x0, dtype)
        ssq = torch.full((N // 16, 16), float("nan"), device="cuda", dtype=torch.float32)
        check(L.samd_gemm_cs_residual(_ptr(a), _ptr(Wg), rows_pad, N, K, _ptr(x), _ptr(ssq), dc, st))
        torch.cuda.synchronize()
        label = f"N {N} K {K} rows_pad {rows_pad}"
        y = x[:rows_pad].to(F64)
        err = (y - want[:rows_pad]).abs() / bar[:rows_pad]
        assert float(err.max()) <= 1, f"{label}: {int((err > 1).sum())} elements beyond the bar (worst {float(err.max()):.2f} x)"
        f = P.mismatch(y, want[:rows_pad])
        assert f <= P.FRAC_CAP, f"{label}: {f:.4f} of the elements differ"
        assert torch.equal(x[rows_pad:].to(F64).cpu(), x0[rows_pad:]), f"{label}: rows >= rows_pad of x written"
        expect_ssq(ssq, x[:rows_pad], rows_pad, label)
        if rows_pad == 8 and K == 4096:
            # the seam-experiment form, in stream order: its producer count is already complete, so it must give the same bits
            xe = gpu(x0, dtype)
            se = torch.full_like(ssq, float("nan"))
            counter = torch.ones(1, dtype=torch.int32, device="cuda")
            epoch = torch.zeros(N // 16, dtype=torch.int32, device="cuda")
            check(L.samd_gemm_cs_residual_early(_ptr(a), _ptr(Wg), N, K, _ptr(xe), _ptr(se), dc, _ptr(counter), _ptr(epoch), 1, st))
            torch.cuda.synchronize()
            early = (xe, se, epoch)
            assert torch.equal(xe, x) and torch.equal(se[:, :8], ssq[:, :8]) and bool(torch.isnan(se[:, 8:]).all()), label + " (early)"
            assert bool((epoch == 1).all()), label + " (early): epochs not advanced"
    assert early is not None or K != 4096


# ---- the norm-applying projections -------------------------------------------------------------------------------------------------------
FOLD_SHAPES = [(32, 32, 4096, 11008), (32, 8, 4096, 14336), (40, 40, 5120, 13824), (4, 2, 8192, 256)]
FOLD_CASES = [(8, 1), (8, 7), (8, 8), (16, 9), (16, 16)]


def fold_windows(hidden, case, per_case=6):
    """the seam tiles, dealt out over the cases so that together they plant every one of them (first columns)"""
    s = P.seam_tiles(hidden // P.TILE)
    return [P.TILE * s[(case * per_case + i) % len(s)] for i in range(per_case)]


def fold_input(rng, hidden, dtype, case, rows_pad):
    eps = 1e-5 if case % 2 else 1e-6
    x, plan = P.plant(rng, 16, hidden, dtype, eps, fold_windows(hidden, case))
    ssq = P.ssq_layout(x.cuda())
    if rows_pad == 8:
        ssq[:, 8:] = float("nan")                                  # never to reach rows < 8
    return x, plan, ssq, eps


def producer_ssq(L, st, dc, x, hidden):
    """x's sums of squares as samd_embed_rows_ssq writes them (x as a 16-row embedding table)"""
    xs = torch.empty((16, hidden), device="cuda", dtype=x.dtype)
    ssq = torch.full((hidden // 16, 16), float("nan"), device="cuda", dtype=torch.float32)
    toks = torch.arange(16, dtype=torch.int32, device="cuda")
    check(L.samd_embed_rows_ssq(_ptr(toks), _ptr(x), _ptr(xs), _ptr(ssq), 16, hidden, 16, dc, st))
    torch.cuda.synchronize()
    return ssq


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,Hkv,hidden,inter", FOLD_SHAPES)
def test_qkv_rope_norm_planted(dtype, H, Hkv, hidden, inter):
    L, st, dc = env(dtype)
    D, max_len = 128, 1024
    Lc = max_len - 16
    rng = np.random.default_rng(H * 1000 + hidden)
    nh = H + 2 * Hkv
    W = rand_matrix(hidden + H, nh * D, hidden, hidden ** -0.5, dtype)
    W64p = torch.empty_like(W)
    check(L.samd_gemm_pack_qkv64(_ptr(W), _ptr(W64p), nh, hidden, st))
    Wd = W.to(F64)
    ang = (Lc + torch.arange(16, dtype=F64))[:, None] * (1.0 / 10000.0 ** (torch.arange(0, D, 2, dtype=F64) / D))[None, :]
    cs = torch.zeros((64, D), device="cuda")                      # as the runner's buffer: one row per possible draft row
    cs[:16] = torch.cat((ang.cos(), ang.sin()), dim=1).float().cuda()
    d_L = gpu([Lc], torch.int32)
    cases = FOLD_CASES * (2 if hidden == 8192 else 1)
    for ci, (rows_pad, n) in enumerate(cases):
        x, plan, ssq, eps = fold_input(rng, hidden, dtype, ci, rows_pad)
        w = P.norm_weight(rng, hidden, dtype)
        xg, wg_, xd = gpu(x, dtype), gpu(w, dtype), x.cuda()
        ref = lambda fault=None: torch.cat(P.qkv_norm(xd, wg_.to(F64), eps, Wd, cs[:16].to(F64), H, Hkv, dtype, fault, plan.hot), dim=1)[:n]
        want = ref()
        label = f"H {H} Hkv {Hkv} hidden {hidden} rows_pad {rows_pad} n {n}"
        P.self_check_max(sub_plan(plan, n), want, {f: ref(f) for f in P.MAX_FAULTS}, fold_bar(dtype), label)
        d_n = gpu([n], torch.int32)
        outs = []
        for vt in (False, True):
            for src in ((ssq, producer_ssq(L, st, dc, xg, hidden)) if ci == len(cases) - 1 else (ssq,)):
                q = torch.full((16, H, D), float("nan"), device="cuda", dtype=dtype)
                kc = torch.full((Hkv, max_len, D), float("nan"), device="cuda", dtype=dtype)
                vc = torch.full((Hkv, D, max_len) if vt else (Hkv, max_len, D), float("nan"), device="cuda", dtype=dtype)
                fn = L.samd_gemm_qkv_rope_norm_vt if vt else L.samd_gemm_qkv_rope_norm
                check(fn(_ptr(xg), _ptr(src), _ptr(wg_), eps, _ptr(W64p), rows_pad, hidden, _ptr(cs), _ptr(d_L), _ptr(d_n), _ptr(q), _ptr(kc), _ptr(vc),
                         H, Hkv, D, max_len, dc, st))
                torch.cuda.synchronize()
                vrows = vc[:, :, Lc:Lc + n].permute(2, 0, 1) if vt else vc[:, Lc:Lc + n].transpose(0, 1)
                got = torch.cat((q[:n], kc[:, Lc:Lc + n].transpose(0, 1), vrows), dim=1)
                lab = f"{label}{' vt' if vt else ''}{' producer ssq' if src is not ssq else ''}"
                expect_rows(got, want, dtype, lab)
                assert bool(torch.isnan(q[n:]).all()) and bool(torch.isnan(kc[:, :Lc]).all()) and bool(torch.isnan(kc[:, Lc + n:]).all()), lab + ": stray writes"
                vout = torch.cat((vc[:, :, :Lc], vc[:, :, Lc + n:]), dim=2) if vt else torch.cat((vc[:, :Lc], vc[:, Lc + n:]), dim=1)
                assert bool(torch.isnan(vout).all()), lab + ": stray V writes"
                outs.append(got)
        assert torch.equal(outs[0], outs[len(outs) // 2]), f"{label}: the V^T form differs from the row-major one"


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_norm_seen_through_an_identity_projection(dtype):
    """the norm that samd_gemm_qkv_rope_norm(_vt) applies on the way into LDS, read back EXACTLY: the V rows of the weight are unit vectors
    (a permutation of the 4096 hidden columns for 32 KV heads), so every V output is one product a_c * 1 summed with zeros -- exact in fp32
    -- and the V cache holds a = (w * (x * rs).to(T)).to(T) itself.  Held to the RMSNorm bars (2 ulp_T, <= 1 % of the elements
    different): a dropped intermediate rounding (~26 % of the elements), a wrong divisor or a lost eps shows, which the per-row bars of
    the projections cannot resolve."""
    L, st, dc = env(dtype)
    H = Hkv = 32
    hidden, D, max_len = 4096, 128, 1024
    Lc = max_len - 16
    rng = np.random.default_rng(4096)
    perm = torch.from_numpy(rng.permutation(hidden))
    W = torch.zeros(((H + 2 * Hkv) * D, hidden), dtype=dtype)
    W[(H + Hkv) * D + torch.arange(hidden), perm] = 1.0           # V column j reads hidden column perm[j]
    W = W.cuda()
    Wp = torch.empty_like(W)
    check(L.samd_gemm_pack_qkv64(_ptr(W), _ptr(Wp), H + 2 * Hkv, hidden, st))
    cs = torch.zeros((64, D), device="cuda")
    d_L = gpu([Lc], torch.int32)
    for ci, (rows_pad, n) in enumerate([(16, 16), (8, 8)]):
        x, plan, ssq, eps = fold_input(rng, hidden, dtype, ci, rows_pad)
        w = P.norm_weight(rng, hidden, dtype)
        want = P.rmsnorm(x, w, eps, dtype)[:n]
        label = f"identity V rows_pad {rows_pad}"
        mx, rd = P.rmsnorm_faults(x, w, eps, dtype, plan)
        P.self_check_max(sub_plan(plan, n), want, {f: v[:n] for f, v in mx.items()}, P.ulp_bar(want, dtype), label)
        P.self_check_fraction(want, {f: v[:n] for f, v in rd.items()}, label=label)
        xg, wn, d_n = gpu(x, dtype), gpu(w, dtype), gpu([n], torch.int32)
        for vt in (False, True):
            q = torch.full((16, H, D), float("nan"), device="cuda", dtype=dtype)
            kc = torch.full((Hkv, max_len, D), float("nan"), device="cuda", dtype=dtype)
            vc = torch.full((Hkv, D, max_len) if vt else (Hkv, max_len, D), float("nan"), device="cuda", dtype=dtype)
            fn = L.samd_gemm_qkv_rope_norm_vt if vt else L.samd_gemm_qkv_rope_norm
            check(fn(_ptr(xg), _ptr(ssq), _ptr(wn), eps, _ptr(Wp), rows_pad, hidden, _ptr(cs), _ptr(d_L), _ptr(d_n), _ptr(q), _ptr(kc), _ptr(vc),
                     H, Hkv, D, max_len, dc, st))
            torch.cuda.synchronize()
            v = (vc[:, :, Lc:Lc + n].permute(2, 0, 1) if vt else vc[:, Lc:Lc + n].transpose(0, 1)).reshape(n, hidden).cpu()
            a = torch.empty_like(v)
            a[:, perm] = v
            expect_ulp(a, want, dtype, label + (" vt" if vt else ""))
            assert bool((q[:n] == 0).all()), label + ": q of zero weight rows"


def pack_pairs(L, st, wg, wu):
    inter, K = wg.shape
    w = torch.stack([wg.view(inter // 16, 16, K), wu.view(inter // 16, 16, K)], dim=1).reshape(2 * inter, K).contiguous()
    out = torch.empty_like(w)
    check(L.samd_gemm_pack_groups(_ptr(w), _ptr(out), 2 * inter, K, st))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,Hkv,hidden,inter", FOLD_SHAPES)
def test_pairs_silu_norm_planted(dtype, H, Hkv, hidden, inter):
    L, st, dc = env(dtype)
    rng = np.random.default_rng(inter + hidden)
    wg = rand_matrix(inter, inter, hidden, hidden ** -0.5, dtype)
    wu = rand_matrix(inter + 1, inter, hidden, hidden ** -0.5, dtype)
    Wp = pack_pairs(L, st, wg, wu)
    wg64, wu64 = wg.to(F64), wu.to(F64)
    cases = [(8, 0), (16, 1), (8, 2), (16, 3)] + ([(8, 4), (16, 5)] if hidden == 8192 else [])
    for rows_pad, ci in cases:
        x, plan, ssq, eps = fold_input(rng, hidden, dtype, ci, rows_pad)
        w = P.norm_weight(rng, hidden, dtype)
        xg, wn, xd = gpu(x, dtype), gpu(w, dtype), x.cuda()
        ref = lambda fault=None: P.pairs_silu_norm(xd, wn.to(F64), eps, wg64, wu64, dtype, fault, plan.hot)[:rows_pad]
        want = ref()
        label = f"hidden {hidden} inter {inter} rows_pad {rows_pad} case {ci}"
        P.self_check_max(sub_plan(plan, rows_pad), want, {f: ref(f) for f in P.MAX_FAULTS}, fold_bar(dtype), label, P.ACT_MISS)
        for src in ((ssq, producer_ssq(L, st, dc, xg, hidden)) if ci == 1 else (ssq,)):
            out = torch.full((16, inter), float("nan"), device="cuda", dtype=dtype)
            check(L.samd_gemm_pairs_silu_norm(_ptr(xg), _ptr(src), _ptr(wn), eps, _ptr(Wp), rows_pad, inter, hidden, _ptr(out), dc, st))
            torch.cuda.synchronize()
            expect_rows(out[:rows_pad], want, dtype, label)
            assert bool((out[rows_pad:] == 0).all()), f"{label}: rows >= rows_pad are not those of a zero input"


# ---- the MLP half of _forward_rows_fold, three layers deep ----------------------------------------------------------------------------------
CHAIN = dict(hidden=4096, inter=2048, eps=1e-5, layers=3)


def chain_ref(x, layers, w_final, eps, dtype, R, fault=None, hot=None):
    """float64 emulation of the chain over all 16 rows (rows are independent); a fault is applied in every folded norm"""
    for (ln, wg, wu, wd) in layers:
        act = P.pairs_silu_norm(x, ln, eps, wg, wu, dtype, fault, hot)
        x, _ = P.cs_residual(x, act, wd, dtype)
    return P.rmsnorm(x[:R], w_final, eps, dtype)


def chain_inputs(rng, dtype, device, matrix):
    """planted embedding rows (16 tokens), three layers' (ln2, W_gate, W_up, W_down) and the final norm weight"""
    hidden, inter, eps = CHAIN["hidden"], CHAIN["inter"], CHAIN["eps"]
    table, plan = P.plant(rng, 16, hidden, dtype, eps, [P.TILE * t for t in P.seam_tiles(hidden // 16)][::2])
    layers = []
    for li in range(CHAIN["layers"]):
        layers.append((P.norm_weight(rng, hidden, dtype).to(device), matrix(100 + li, inter, hidden, hidden ** -0.5),
                       matrix(200 + li, inter, hidden, hidden ** -0.5), matrix(300 + li, hidden, inter, inter ** -0.5)))
    return table.to(device), plan, layers, P.norm_weight(rng, hidden, dtype).to(device)


def chain_case(x0, plan, layers64, wf, dtype, R):
    """the reference rows < R and the self check: each max-error fault, applied in every layer's folded norm, still shows in them"""
    eps = CHAIN["eps"]
    want = chain_ref(x0, layers64, wf, eps, dtype, R)
    sub = sub_plan(plan, R)
    P.self_check_max(sub, want, {f: chain_ref(x0, layers64, wf, eps, dtype, R, f, plan.hot) for f in P.MAX_FAULTS}, fold_bar(dtype), f"chain R {R}", P.ACT_MISS)
    return want


@pytest.mark.parametrize("dtype", DTYPES)
def test_mlp_chain_of_the_norm_fold_forward(dtype):
    """samd_embed_rows_ssq -> 3 x (samd_gemm_pairs_silu_norm -> samd_gemm_cs_residual) -> samd_rmsnorm with the row counts of
    _forward_rows_fold (rows_cs = rows_a = 8 for R <= 8, else 16): the sums of squares are handed from launch to launch, and the 8-row
    forms leave rows 8..15 stale -- poisoned here with NaN, x and sums of squares alike.  Per-row bars of the fold kernels."""
    L, st, dc = env(dtype)
    hidden, inter, eps = CHAIN["hidden"], CHAIN["inter"], CHAIN["eps"]
    rng = np.random.default_rng(11)
    table, plan, layers, wf = chain_inputs(rng, dtype, "cuda", lambda seed, r, c, sc: rand_matrix(seed, r, c, sc, dtype))
    tab, wfd = table.to(dtype), wf.to(dtype)
    layers64, packed = [], []
    for ln, wg, wu, wd in layers:
        wdp = torch.empty_like(wd)
        check(L.samd_gemm_pack_groups(_ptr(wd), _ptr(wdp), hidden, inter, st))
        layers64.append((ln, wg.to(F64), wu.to(F64), wd.to(F64)))
        packed.append((ln.to(dtype), pack_pairs(L, st, wg, wu), wdp))
    toks = torch.arange(16, dtype=torch.int32, device="cuda")
    for R in (1, 7, 8, 9, 16):
        rows = 8 if R <= 8 else 16
        want = chain_case(table, plan, layers64, wf, dtype, R)
        x = torch.full((16, hidden), float("nan"), device="cuda", dtype=dtype)
        ssq = torch.full((hidden // 16, 16), float("nan"), device="cuda", dtype=torch.float32)
        act = torch.full((16, inter), float("nan"), device="cuda", dtype=dtype)
        out = torch.full((16, hidden), float("nan"), device="cuda", dtype=dtype)
        check(L.samd_embed_rows_ssq(_ptr(toks), _ptr(tab), _ptr(x), _ptr(ssq), 16, hidden, 16, dc, st))
        if rows == 8:
            x[8:] = float("nan")
            ssq[:, 8:] = float("nan")
        for ln, wgu, wdp in packed:
            check(L.samd_gemm_pairs_silu_norm(_ptr(x), _ptr(ssq), _ptr(ln), eps, _ptr(wgu), rows, inter, hidden, _ptr(act), dc, st))
            check(L.samd_gemm_cs_residual(_ptr(act), _ptr(wdp), rows, hidden, inter, _ptr(x), _ptr(ssq), dc, st))
        check(L.samd_rmsnorm(_ptr(x), None, _ptr(wfd), _ptr(out), R, hidden, eps, dc, 0, 0, st))
        torch.cuda.synchronize()
        expect_rows(out[:R], want, dtype, f"chain R {R}")
        assert bool(torch.isnan(out[R:]).all()), f"chain R {R}: rows >= R of the final norm written"


# ---- samd_sum_partials_bias ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,N", [(3, 1000), (8, 4099), (1, 37)])
def test_sum_partials_bias(dtype, rows, N):
    """(sum of fp32 partials + bias).to(T): the partials lie on a 2^-14 grid and the bias on a 2^-7 grid, so the fp32 sum is exact
    and the result has one correct rounding -- every element within 1 ulp_T of it (in fact equal), the output's tail untouched"""
    L, st, dc = env(dtype)
    rng = np.random.default_rng(rows * N)
    for n in range(1, 13):
        parts = P.grid_values(rng, (n, rows, N))
        stride = rows * N + 5
        buf = torch.full((n, stride), float("nan"), dtype=torch.float32)
        buf[:, :rows * N] = parts.reshape(n, -1).float()
        buf = buf.cuda()
        for with_bias in (False, True):
            bias = torch.from_numpy(np.round(rng.uniform(-2, 2, N) * 128) / 128) if with_bias else None
            want = P.sum_partials_bias(parts, bias, dtype)
            out = torch.full((rows * N + 64,), float("nan"), device="cuda", dtype=dtype)
            b = gpu(bias, dtype) if with_bias else None
            check(L.samd_sum_partials_bias(_ptr(buf), n, stride, _ptr(b), _ptr(out), rows, N, dc, st))
            torch.cuda.synchronize()
            label = f"rows {rows} N {N} partials {n} bias {with_bias}"
            expect_ulp(out[:rows * N].view(rows, N).cpu(), want, dtype, label, ulps=1, cap=1.0)
            assert torch.equal(out[:rows * N].view(rows, N).to(F64).cpu(), want), label
            assert bool(torch.isnan(out[rows * N:]).all()), f"{label}: written past rows x N"
