"""samd_rope_kv_write_epi (include/samd_hip.h): the q|k|v epilogue of Qwen2 / Qwen3 -- bias, per-head q / k RMSNorm -- in front of the RoPE and
the K / V write, bit for bit against its restatement (tests/qkv_epilogue_ref.py) on planted rows.

Planting: where a norm runs, every x is a multiple of 2^-6 below 1 (the partials and the bias too), so the fp32 sum of squares is exact in any
order and only rsqrtf is approximate: a (row, head) must equal the restatement at the correctly rounded rsqrt or one fp32 ulp either side, or
else meet the bar tests/norm_planting.py sets k_rmsnorm's rsqrtf (every element within 2 ulp_T, at most 1 % of the elements off); >= 90 % of
the heads equal the correctly rounded restatement.  Bias alone: random fp32 partials / products, which makes the single rounding of
sum + bias visible.  Outputs start as NaN: rows >= n, cache positions outside [L, L + n) and at or past max_len must stay NaN.
Covered: f16 / bf16; 0 / 1 / 3 / 9 partials; bias, norm, both; position tables and cs; row-major V and V^T; GQA 1 / 3 / 7; >= 128 rows
(k_rope_kv_wide_epi and k_v_rows_to_vt_bias with the tables and no partials); n < rows; L near max_len."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import QkvEpilogue, _ptr, check, current_stream, lib, torch_dtype_code
import norm_planting as NP
import qkv_epilogue_ref as R

# (H, Hkv, rows, n, L, max_len)
GEOM = {"gqa3": (6, 2, 16, 11, 37, 256), "gqa7_near_end": (7, 1, 64, 64, 200, 248), "gqa1_wide": (4, 4, 192, 150, 20, 512)}
EPS = 1e-6


def norm_w(g, dtype):
    return ((0.5 + 1.5 * torch.rand(128, generator=g)) * torch.where(torch.rand(128, generator=g) < 0.5, -1.0, 1.0)).to(dtype)


def make_inputs(seed, dtype, H, Hkv, rows, n_part, mode):
    g = torch.Generator().manual_seed(seed)
    cols = (H + 2 * Hkv) * 128
    bias = qn = kn = None
    if mode == "bias":
        bias = (torch.randn(cols, generator=g) * 0.7).to(dtype)
        qkv = torch.randn(rows, cols, generator=g).to(dtype)
        parts = torch.randn(n_part, rows, cols, generator=g) / max(n_part, 1) ** 0.5 if n_part else None
    else:
        xi = torch.randint(-60, 61, (rows, cols), generator=g)
        bi = torch.randint(-3, 4, (cols,), generator=g) if mode == "both" else torch.zeros(cols, dtype=torch.long)
        rest = xi - bi
        if mode == "both":
            bias = (bi.float() / 64).to(dtype)
        qkv = (rest.float() / 64).to(dtype)
        parts = None
        if n_part:
            pi = torch.randint(-8, 9, (n_part, rows, cols), generator=g)
            pi[-1] = rest - pi[:-1].sum(0)
            parts = pi.float() / 64
        qn, kn = norm_w(g, dtype), norm_w(g, dtype)
    return qkv, parts, bias, qn, kn


def run_epi(dtype, geom, n_part, mode, form, vt, seed=0):
    H, Hkv, rows, n, L, max_len = geom
    qkv, parts, bias, qn, kn = make_inputs(seed, dtype, H, Hkv, rows, n_part, mode)
    g = torch.Generator().manual_seed(seed + 1)
    max_pos = max_len + 16
    ang = torch.rand(max_pos, 64, generator=g, dtype=torch.float64) * 6.2831853
    cos_t, sin_t = ang.cos().float(), ang.sin().float()
    rel = torch.randint(0, 12, (rows,), generator=g, dtype=torch.int32)
    pos = (L + rel.long()).clamp(max=max_pos - 1)
    cos_r, sin_r = cos_t[pos], sin_t[pos]
    dev = lambda t: None if t is None else t.cuda().contiguous()
    nanT = lambda *s: torch.full(s, float("nan"), dtype=dtype, device="cuda")
    q_out, k_cache, v_cache = nanT(rows, H, 128), nanT(Hkv, max_len, 128), nanT(Hkv, max_len, 128)
    d_src = dev(parts) if n_part else dev(qkv)
    d_b, d_qn, d_kn = dev(bias), dev(qn), dev(kn)
    epi = QkvEpilogue(_ptr(d_b), _ptr(d_qn), _ptr(d_kn), EPS)
    d_cs = torch.cat([cos_r, sin_r], 1).cuda().contiguous() if form == "cs" else None
    d_cos, d_sin = (None, None) if form == "cs" else (cos_t.cuda(), sin_t.cuda())
    d_rel, d_L, d_n = rel.cuda(), torch.tensor([L], dtype=torch.int32, device="cuda"), torch.tensor([n], dtype=torch.int32, device="cuda")
    check(lib().samd_rope_kv_write_epi(_ptr(d_src), _ptr(d_rel), _ptr(d_L), _ptr(d_n), _ptr(d_cos), _ptr(d_sin), _ptr(d_cs), _ptr(q_out),
                                       _ptr(k_cache), _ptr(v_cache), vt, rows, H, Hkv, 128, max_len, max_pos, torch_dtype_code(dtype), n_part,
                                       rows * (H + 2 * Hkv) * 128, C.byref(epi), current_stream()))
    torch.cuda.synchronize()
    v_rows = v_cache.view(Hkv, 128, max_len).transpose(1, 2) if vt else v_cache
    return dict(q=q_out.float().cpu(), k=k_cache.float().cpu(), v=v_rows.float().cpu(), qkv=qkv, parts=parts, bias=bias, qn=qn, kn=kn,
                cos=cos_r, sin=sin_r)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("geom", list(GEOM))
@pytest.mark.parametrize("n_part", [0, 1, 3, 9])
@pytest.mark.parametrize("mode", ["bias", "norm", "both"])
@pytest.mark.parametrize("form,vt", [("tables", 0), ("tables", 1), ("cs", 0), ("cs", 1)])
def test_epilogue_bit_exact_on_planted_rows(dtype, geom, n_part, mode, form, vt):
    H, Hkv, rows, n, L, max_len = GEOM[geom]
    o = run_epi(dtype, GEOM[geom], n_part, mode, form, vt, seed=zlib.crc32(f"{geom} {n_part} {mode}".encode()) % 1000)
    live = [r for r in range(n) if L + r < max_len]
    shifts = (0,) if mode == "bias" else (0, -1, 1)
    refs = [R.restate(o["qkv"], o["parts"], o["bias"], o["qn"], o["kn"], EPS, o["cos"], o["sin"], H, Hkv, dtype, inv_ulps=u) for u in shifts]
    exact0, heads, off_elems = 0, 0, 0

    def head_ok(got, want_at):                      # want_at(ref) -> the head in that restatement
        nonlocal exact0, heads, off_elems
        hit = [torch.equal(got, want_at(ref)) for ref in refs]
        exact0 += hit[0]; heads += 1
        if any(hit):
            return True
        # rsqrtf's bar (tests/norm_planting.py, k_rmsnorm): every element within ULP_BAR ulp_T, few elements off
        want = want_at(refs[0])
        off_elems += int((got != want).sum())
        return mode != "bias" and bool(((got - want).abs().double() <= NP.ULP_BAR * NP.ulp(want, dtype)).all())
    for r in live:
        for h in range(H):
            assert head_ok(o["q"][r, h], lambda ref: ref[0][r, h]), ("q", r, h)
        for h in range(Hkv):
            assert head_ok(o["k"][h, L + r], lambda ref: ref[1][r, h]), ("k", r, h)
            assert torch.equal(o["v"][h, L + r], refs[0][2][r, h]), ("v", r, h)
    assert exact0 >= 0.9 * heads and off_elems <= NP.FRAC_CAP * heads * 128
    # untouched: rows >= n of q, cache positions outside the live rows
    assert torch.isnan(o["q"][n:]).all()
    written = torch.zeros(max_len, dtype=torch.bool)
    written[[L + r for r in live]] = True
    assert torch.isnan(o["k"][:, ~written]).all() and torch.isnan(o["v"][:, ~written]).all()
    if len(live) < n:
        assert L + n > max_len                                               # (the geometry near the end of the cache exercises the guard)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("geom", ["gqa3", "gqa1_wide"])
@pytest.mark.parametrize("n_part", [0, 3])
def test_null_epilogue_equals_the_existing_entry_points(dtype, geom, n_part):
    H, Hkv, rows, n, L, max_len = GEOM[geom]
    g = torch.Generator(device="cuda").manual_seed(7)
    cols = (H + 2 * Hkv) * 128
    src = torch.randn(n_part, rows, cols, generator=g, device="cuda") if n_part else torch.randn(rows, cols, generator=g, device="cuda").to(dtype)
    max_pos = max_len + 16
    cos_t, sin_t = torch.rand(max_pos, 64, generator=g, device="cuda"), torch.rand(max_pos, 64, generator=g, device="cuda")
    rel = torch.randint(0, 12, (rows,), generator=g, device="cuda", dtype=torch.int32)
    cs = torch.rand(rows, 128, generator=g, device="cuda")
    d_L, d_n = torch.tensor([L], dtype=torch.int32, device="cuda"), torch.tensor([n], dtype=torch.int32, device="cuda")
    dt, st, Lb, stride = torch_dtype_code(dtype), current_stream(), lib(), rows * cols
    empty = QkvEpilogue(None, None, None, EPS)
    for form in ("tables", "cs"):
        for vt in (0, 1):
            outs = []
            for which in ("old", "epi_null", "epi_empty"):
                q = torch.full((rows, H, 128), float("nan"), dtype=dtype, device="cuda")
                k, v = torch.full_like(q.new_empty(Hkv, max_len, 128), float("nan")), torch.full_like(q.new_empty(Hkv, max_len, 128), float("nan"))
                if which == "old":
                    if form == "tables":
                        check((Lb.samd_rope_kv_write_vt if vt else Lb.samd_rope_kv_write)(
                            _ptr(src), _ptr(rel), _ptr(d_L), _ptr(d_n), _ptr(cos_t), _ptr(sin_t), _ptr(q), _ptr(k), _ptr(v), rows, H, Hkv, 128,
                            max_len, max_pos, dt, n_part, stride, st))
                    else:
                        check((Lb.samd_rope_kv_write_cs_vt if vt else Lb.samd_rope_kv_write_cs)(
                            _ptr(src), _ptr(rel), _ptr(d_L), _ptr(d_n), _ptr(cs), _ptr(q), _ptr(k), _ptr(v), rows, H, Hkv, 128, max_len, dt,
                            n_part, stride, st))
                else:
                    tabs = (None, None, _ptr(cs)) if form == "cs" else (_ptr(cos_t), _ptr(sin_t), None)
                    check(Lb.samd_rope_kv_write_epi(_ptr(src), _ptr(rel), _ptr(d_L), _ptr(d_n), *tabs, _ptr(q), _ptr(k), _ptr(v), vt, rows, H, Hkv,
                                                    128, max_len, max_pos, dt, n_part, stride, None if which == "epi_null" else C.byref(empty), st))
                torch.cuda.synchronize()
                outs.append([t.view(torch.int16).clone() for t in (q, k, v)])
            for other in outs[1:]:
                assert all(torch.equal(a, b) for a, b in zip(outs[0], other)), (form, vt)


def test_epilogue_argument_checks():
    d = torch.zeros(16, dtype=torch.int32, device="cuda")
    x = torch.zeros(4096, dtype=torch.float16, device="cuda")
    w = torch.ones(128, dtype=torch.float16, device="cuda")
    Lb, st = lib(), current_stream()

    def call(epi, head_dim=128, dtype=0, cs=None, tabs=True):
        return Lb.samd_rope_kv_write_epi(_ptr(x), _ptr(d), _ptr(d), _ptr(d), _ptr(x) if tabs else None, _ptr(x) if tabs else None, _ptr(cs),
                                         _ptr(x), _ptr(x), _ptr(x), 0, 1, 1, 1, head_dim, 8, 8, dtype, 0, 0, C.byref(epi), st)
    assert call(QkvEpilogue(_ptr(w), _ptr(w), None, EPS)) != 0                    # q norm without k norm
    assert call(QkvEpilogue(_ptr(w), None, None, EPS), head_dim=64) != 0
    assert call(QkvEpilogue(_ptr(w), None, None, EPS), dtype=2) != 0              # fp32 model dtype
    assert call(QkvEpilogue(None, _ptr(w), _ptr(w), -1.0)) != 0
    assert call(QkvEpilogue(_ptr(w), None, None, EPS), cs=x) != 0                 # tables and cs together
    assert call(QkvEpilogue(_ptr(w), None, None, EPS), tabs=False) != 0           # neither
    torch.cuda.synchronize()
