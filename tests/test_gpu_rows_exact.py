"""Exact-row activation fetch in the <= 16-row verify projections (samd_gemm_cs_residual, samd_gemm_qkv_rope_norm[_vt],
samd_gemm_pairs_silu_norm with rows 5 and 9; LlamaRunner.forward_rows(rows_fetch=n); DecodeEngine._graphs_exact).  Everything here is a
bit-for-bit comparison against the bucket's own form (8 rows for 5, 16 for 9) on the same inputs: the rows a draft has go through the
same arithmetic in the same order, so torch.equal is the bound.  The rows the exact form must not fetch hold NaN -- a NaN row that reached
an MFMA would poison nothing (rows are independent), so the proof that they are not fetched INTO A SUM is that they are not written either:
result rows past the fetched ones keep a sentinel (complete-sum projection) or are exactly the rows of a zero input (gate|up)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from util import random_parents

DTYPES = [torch.float16, torch.bfloat16]
PAIRS = [(5, 8), (9, 16)]                         # (exact rows, the bucket form they are compared with)
SENTINEL = 7.0


def _env():
    return samd_hip.lib(), samd_hip.current_stream(), samd_hip._ptr


def _rnd(g, dtype, *shape, sc=1.0):
    return (torch.randn(shape, generator=g, device="cuda") * sc).to(dtype)


# K = 256: one chunk, waves 1-7 have none.  512: two.  2816: 11 chunks, unequal shares per wave (as 11008 has).
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,ref_rows", PAIRS)
@pytest.mark.parametrize("K", [256, 512, 2816])
def test_complete_sum_projection_fetches_and_writes_exactly_its_rows(dtype, rows, ref_rows, K):
    Lb, st, P = _env()
    dc = samd_hip.torch_dtype_code(dtype)
    N = 32
    g = torch.Generator(device="cuda").manual_seed(K + rows)
    A = _rnd(g, dtype, 16, K)
    A[rows:] = float("nan")
    W = _rnd(g, dtype, N, K, sc=K ** -0.5)
    Wp = torch.empty_like(W)
    samd_hip.check(Lb.samd_gemm_pack_groups(P(W), P(Wp), N, K, st))
    x0 = _rnd(g, dtype, 16, N)
    x0[rows:] = SENTINEL
    out = {}
    for r in (ref_rows, rows):
        x = x0.clone()
        ssq = torch.full((N // 16, 16), -1.0, device="cuda", dtype=torch.float32)
        samd_hip.check(Lb.samd_gemm_cs_residual(P(A), P(Wp), r, N, K, P(x), P(ssq), dc, st))
        out[r] = (x, ssq)
    torch.cuda.synchronize()
    (x, ssq), (xr, ssqr) = out[rows], out[ref_rows]
    assert torch.isfinite(x[:rows].float()).all() and not torch.equal(x[:rows], x0[:rows])
    assert torch.equal(x[:rows], xr[:rows]) and torch.equal(ssq[:, :rows], ssqr[:, :rows])
    assert bool((x[rows:] == SENTINEL).all()) and bool((ssq[:, rows:] == -1.0).all())


def _norm_inputs(g, dtype, K, rows):
    """residual stream x [16][K] with NaN in the rows the exact form must not fetch, the per-tile sums of squares of its real rows (NaN
    for the others as well), the norm weight"""
    x = _rnd(g, dtype, 16, K)
    ssq = x.float().view(16, K // 16, 16).pow(2).sum(-1).t().contiguous()
    x[rows:] = float("nan")
    ssq[:, rows:] = float("nan")
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(dtype)
    return x, ssq, gamma


# the smallest geometries of the norm-fold tests for these entry points (head_dim 128, K a multiple of 256, q|k|v width divisible by 48
# and 64): one chunk, two chunks, and five -- one more than the four the stream keeps in flight
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,ref_rows,n", [(5, 8, 5), (5, 8, 3), (9, 16, 9)])
@pytest.mark.parametrize("H,K", [(3, 256), (2, 512), (6, 1280)])
@pytest.mark.parametrize("vt", [False, True])
def test_qkv_projection_with_the_norm_folded_in(dtype, rows, ref_rows, n, H, K, vt):
    Lb, st, P = _env()
    dc = samd_hip.torch_dtype_code(dtype)
    D, max_len, L, eps = 128, 256, 100, 1e-6
    g = torch.Generator(device="cuda").manual_seed(H * K + rows + n)
    x, ssq, gamma = _norm_inputs(g, dtype, K, rows)
    W = _rnd(g, dtype, 3 * H * D, K, sc=K ** -0.5)
    W64 = torch.empty_like(W)
    samd_hip.check(Lb.samd_gemm_pack_qkv64(P(W), P(W64), 3 * H, K, st))
    cs = torch.rand((64, D), generator=g, device="cuda")
    d_L = torch.tensor([L], dtype=torch.int32, device="cuda")
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    launch = Lb.samd_gemm_qkv_rope_norm_vt if vt else Lb.samd_gemm_qkv_rope_norm
    out = {}
    for r in (ref_rows, rows):
        q = torch.full((16, H, D), SENTINEL, device="cuda", dtype=dtype)
        kc = torch.full((H, max_len, D), SENTINEL, device="cuda", dtype=dtype)
        vc = torch.full((H, D, max_len) if vt else (H, max_len, D), SENTINEL, device="cuda", dtype=dtype)
        samd_hip.check(launch(P(x), P(ssq), P(gamma), eps, P(W64), r, K, P(cs), P(d_L), P(d_n), P(q), P(kc), P(vc), H, H, D, max_len, dc, st))
        out[r] = (q, kc, vc)
    torch.cuda.synchronize()
    q, kc, vc = out[rows]
    v_rows = vc[:, :, L:L + n].transpose(1, 2) if vt else vc[:, L:L + n]
    for t in (q[:n], kc[:, L:L + n], v_rows):
        assert torch.isfinite(t.float()).all() and not bool((t == SENTINEL).all())
    # whole tensors: the draft's rows bit for bit, and neither form writes a row past the draft
    assert all(torch.equal(a, b) for a, b in zip(out[rows], out[ref_rows]))
    assert bool((q[n:] == SENTINEL).all()) and bool((kc[:, L + n:] == SENTINEL).all()) and bool((kc[:, :L] == SENTINEL).all())


def _pack_pairs(wg, wu):
    Lb, st, P = _env()
    inter, K = wg.shape
    w = torch.stack([wg.view(inter // 16, 16, K), wu.view(inter // 16, 16, K)], dim=1).reshape(2 * inter, K).contiguous()
    out = torch.empty_like(w)
    samd_hip.check(Lb.samd_gemm_pack_groups(P(w), P(out), 2 * inter, K, st))
    return out


# inter 48: three pairs in three workgroups (one pair each, six idle waves); 1024: 64 pairs; 256 CUs' worth of 2-3 pairs needs 11008 and is
# what the whole-forward tests of the suite run
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,ref_rows", PAIRS)
@pytest.mark.parametrize("K,inter", [(256, 48), (512, 256), (1280, 1024)])
def test_gate_up_projection_with_the_norm_folded_in(dtype, rows, ref_rows, K, inter):
    Lb, st, P = _env()
    dc = samd_hip.torch_dtype_code(dtype)
    g = torch.Generator(device="cuda").manual_seed(K + inter + rows)
    x, ssq, gamma = _norm_inputs(g, dtype, K, rows)
    Wp = _pack_pairs(_rnd(g, dtype, inter, K, sc=K ** -0.5), _rnd(g, dtype, inter, K, sc=K ** -0.5))
    out = {}
    for r in (ref_rows, rows):
        o = torch.full((16, inter), SENTINEL, device="cuda", dtype=dtype)
        samd_hip.check(Lb.samd_gemm_pairs_silu_norm(P(x), P(ssq), P(gamma), 1e-6, P(Wp), r, inter, K, P(o), dc, st))
        out[r] = o
    torch.cuda.synchronize()
    o = out[rows]
    assert torch.isfinite(o.float()).all() and o[:rows].float().abs().sum().item() > 0
    assert torch.equal(o[:rows], out[ref_rows][:rows])
    assert o[rows:].float().abs().sum().item() == 0                      # silu(0) * 0: the rows that are not fetched are zeros in LDS


def test_unsupported_row_counts_are_still_errors():
    Lb, st, P = _env()
    t = torch.zeros(16 * 256, device="cuda", dtype=torch.float16)
    f = torch.zeros(64, device="cuda", dtype=torch.float32)
    for r in (0, 4, 6, 7, 10, 13, 17, 32):
        assert Lb.samd_gemm_cs_residual(P(t), P(t), r, 16, 256, P(t), P(f), samd_hip.torch_dtype_code(torch.float16), st) != 0
        assert Lb.samd_gemm_pairs_silu_norm(P(t), P(f), P(t), 1e-6, P(t), r, 16, 256, P(t), samd_hip.torch_dtype_code(torch.float16), st) != 0


# ---- whole forward and engine: the smallest decoder that takes the norm-fold form (48 q|k|v heads of 128 = 128 tiles of 48 columns;
# gate|up rows a multiple of 128, down_proj's K a multiple of 256 with unequal shares per wave)
CFG = dict(hidden_size=2048, intermediate_size=768, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=16, vocab_size=512,
           max_position_embeddings=1024, rms_norm_eps=1e-6)
MAX_LEN = 512


@pytest.fixture(scope="module")
def runner():
    from samd_hip.llama import LlamaRunner
    from test_gpu_lm_shapes import hf_llama
    lm = hf_llama(CFG, seed=5)
    r = LlamaRunner.from_hf(lm, max_cache_len=MAX_LEN, dtype=torch.float16, share_weights=False)
    assert r.norm_fold and r.rows_exact(8) == (5,) and r.rows_exact(16) == (9,) and r.rows_exact(32) == ()
    return r


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).cuda()


@pytest.mark.parametrize("n", [5, 9])
def test_forward_rows_with_the_drafts_own_row_count(runner, n):
    rng = np.random.default_rng(n)
    V, P0 = CFG["vocab_size"], 40
    sess = samd_hip.Session(MAX_LEN + samd_hip.MAX_DRAFT)
    runner.prefill(sess, torch.tensor([rng.integers(3, V, P0).tolist()], device="cuda"))
    sess.set_draft(_dev(rng.integers(3, V, n)), _dev(random_parents(rng, n, "random")), n, type_=1)
    R = runner.bucket(n)
    kv0 = runner.kv.clone()
    b = runner.verify(sess, R)
    torch.cuda.synchronize()
    want = (b["logits"][:n].clone(), b["argmax"][:n].clone(), runner.kv.clone())
    runner.kv.copy_(kv0)
    b = runner.verify(sess, R, rows_fetch=n)
    torch.cuda.synchronize()
    assert torch.isfinite(want[0].float()).all() and not torch.equal(want[2], kv0)          # the draft's K/V rows were written ...
    assert torch.equal(b["logits"][:n], want[0]) and torch.equal(b["argmax"][:n], want[1])
    assert torch.equal(runner.kv, want[2])                                                  # ... and are the same bits, nothing else touched
    with pytest.raises(samd_hip.SamdError):
        runner.verify(sess, R, rows_fetch=n + 1)


def _scripted_run(runner, monkeypatch, exact):
    """a few decode steps on installed chain drafts of 5, 9, 7, 12, 5 and 9 nodes that follow the scripted continuation up to a planted
    miss; returns (token stream, replays per graph kind, sizes of the two graph tables after pre-capture and after the run, K/V cache)"""
    import samd_sam_only as SO
    from samd_hip.engine import ScriptedAcceptance
    monkeypatch.setenv("SAMD_ROWS_EXACT", "1" if exact else "0")
    V, P0 = CFG["vocab_size"], 48
    rng = np.random.default_rng(7)
    target = rng.integers(3, V, MAX_LEN).tolist()
    sa = ScriptedAcceptance(runner, V, MAX_LEN)
    sa.set_target(target)
    cfg = SO.SamdConfig(max_predicts=16, alpha=4.0, K=8, len_bias=0)
    model = SO.SamdModel(cfg, sa, SO.DraftModel(cfg, device="cuda"), 2, torch.float16, "cuda")
    model.set_cache(SO.SamdGenerationConfig(max_new_tokens=64, max_cache_len=MAX_LEN))
    eng = model.engine
    eng._capture(8)
    eng._capture(16)
    sizes = [(len(eng._graphs), len(eng._graphs_exact))]
    replays = {"bucket": 0, "exact": 0}

    def counted(g, kind):
        inner = g.replay

        def replay():
            replays[kind] += 1
            inner()
        g.replay = replay
    for g in eng._graphs.values():
        counted(g, "bucket")
    for g in eng._graphs_exact.values():
        counted(g, "exact")
    eng.start(torch.tensor([target[:P0]], device="cuda"))
    pos, stream = P0, []
    for n, miss in ((5, 3), (9, 9), (7, 2), (12, 6), (5, 5), (9, 1)):
        toks = target[pos:pos + n]
        if miss < n:
            toks[miss] = 3 + (toks[miss] - 2) % (V - 3)                  # another token than the continuation's: the chain is accepted up to here
        eng.session.set_draft(_dev(toks), _dev(random_parents(rng, n, "chain")), n, type_=1)
        rep = eng.step(n)
        assert not rep.error and len(rep.tokens) == min(miss, n)
        stream += list(rep.tokens)
        pos += len(rep.tokens)
    torch.cuda.synchronize()
    sizes.append((len(eng._graphs), len(eng._graphs_exact)))
    assert stream == target[P0:pos]
    return stream, replays, sizes, runner.kv.clone()


def test_engine_replays_the_exact_graphs_for_5_and_9_node_drafts(runner, monkeypatch):
    stream, replays, sizes, kv = _scripted_run(runner, monkeypatch, exact=True)
    assert replays == {"exact": 4, "bucket": 2}                          # 5, 9, 5, 9 | 7, 12
    assert sizes == [(2, 2), (2, 2)]                                     # nothing is captured after the pre-capture
    stream0, replays0, sizes0, kv0 = _scripted_run(runner, monkeypatch, exact=False)
    assert replays0 == {"exact": 0, "bucket": 6} and sizes0 == [(2, 0), (2, 0)]
    assert stream == stream0 and torch.equal(kv, kv0)
