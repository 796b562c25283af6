"""The kernels that turn logits into tokens on PLANTED inputs (tests/select_planting.py): samd_argmax_rows, the four top-8 implementations
(k_topk8_rows and k_topk8_part + k_topk8_merge behind samd_recycle_update; k_e2_rowstats and k_e2_rowstats_part + _merge behind
samd_e2_rowstats), samd_e2_select / samd_e2_finish and samd_posterior_sampled / _nodes.  Every output starts poisoned (-1 / NaN), every index
is compared by equality with np.lexsort((index, -value)) on the float64 values; only top_logp and row_lse have a bar (2e-4 absolute, the one
of tests/test_gpu_eagle_kernels.py, against float64)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code

import select_planting as P
from test_gpu_eagle_kernels import make_state

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
IDS = ["f16", "bf16", "f32"]
DEAD = 2                                  # rows behind a device-side row count, full of the largest value


def _cuda(x):
    return x.cuda() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- 3.1 arg-max ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", range(5), ids=["v1", "v7", "v8", "v1003", "two-passes-and-tail"])
def test_argmax_rows_planted(dtype, which):
    """every tie pair (same vector / next pass / two lanes / two waves with the lower index in the higher wave / body and tail / both in the
    tail / first and last), -0.0 before +0.0, all -inf, -inf but one, finite only in the tail: rows at an aligned stride and at an odd one
    (rows 1, 2, .. unaligned: all tail), padding columns and two dead rows behind a device-side row count full of a larger value"""
    es = P.ESIZE[dtype]
    vocab = P.ARGMAX_VOCABS(es)[which]
    n = 0
    for stride in P.strides(vocab, es):
        for batch in P.batches("argmax", es, vocab, stride, rows=8 - DEAD):
            x = _cuda(P.assemble(batch, stride, dtype, dead_rows=DEAD))
            want = [int(c.expect[0]) for c in batch]
            live = len(batch)
            for d_rows, rows in ((None, live), (_cuda(np.array([live], np.int32)), live + DEAD)):
                out = torch.full((live + DEAD,), -1, dtype=torch.int32, device="cuda")
                check(lib().samd_argmax_rows(_ptr(x), torch_dtype_code(dtype), rows, vocab, stride, _ptr(d_rows), _ptr(out), current_stream()))
                got = out.cpu().tolist()
                assert got[:live] == want, [(c.name, g, w) for c, g, w in zip(batch, got, want) if g != w]
                assert got[live:] == [-1] * DEAD
            n += live
    assert n >= 2


# ---- 3.2 top-8 ----------------------------------------------------------------------------------------------------------------------------------
def _top8_batches(kernels, es, vocab, rows):
    """(stride, batch) over both strides and over the cases of every map in `kernels`: a planted row is a valid input for any kernel, and the
    expectation does not depend on the map, so both forms of a pair run the plants of both and must give the same indices"""
    for stride in P.strides(vocab, es):
        for kernel in kernels:
            for batch in P.batches(kernel, es, vocab, stride, rows=rows):
                yield stride, batch


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("vocab", P.TOP8_VOCABS)
def test_recycle_update_planted(dtype, vocab):
    """samd_recycle_update: fp32 runs k_topk8_rows, f16 / bf16 the split form k_topk8_part + k_topk8_merge; read back through
    samd_recycle_export with distinct tokens per row.  Two more rows behind the device-side count d_n hold the largest value everywhere:
    their tokens must stay absent.  Both forms run the plants of both maps against the same expectation, so they agree with each other."""
    es = P.ESIZE[dtype]
    off = np.zeros(2, np.int32); ch = np.zeros(1, np.int32)
    h = C.c_void_p()
    check(lib().samd_recycle_create(vocab, _ptr(off), _ptr(ch), 1, C.byref(h)))
    try:
        for stride, batch in _top8_batches(("segment", "rows256"), es, vocab, 8 - DEAD):
            live = len(batch)
            x = _cuda(P.assemble(batch, stride, dtype, dead_rows=DEAD))
            tokens = _cuda(np.arange(live + DEAD, dtype=np.int32)[::-1].copy())          # row r writes table row (live + DEAD - 1 - r)
            d_n = _cuda(np.array([live], np.int32))
            # forget the previous batch: a table row is valid only where `present` says so, and present is cleared by re-creating below
            check(lib().samd_recycle_update(h, _ptr(tokens), _ptr(x), torch_dtype_code(dtype), live + DEAD, _ptr(d_n), vocab, stride, current_stream()))
            table = np.full((vocab, 8), -1, np.int32); present = np.full(vocab, 255, np.uint8)
            check(lib().samd_recycle_export(h, _ptr(table), _ptr(present), current_stream()))
            toks = tokens.cpu().numpy()
            for r, c in enumerate(batch):
                assert present[toks[r]] == 1 and table[toks[r]].tolist() == c.expect.tolist(), (c.name, stride, table[toks[r]].tolist(), c.expect.tolist())
            for r in range(live, live + DEAD):
                assert present[toks[r]] == 0, "a row behind d_n was written"
            assert int(present.sum()) == live
            lib().samd_recycle_free(h)
            h = C.c_void_p()
            check(lib().samd_recycle_create(vocab, _ptr(off), _ptr(ch), 1, C.byref(h)))
    finally:
        lib().samd_recycle_free(h)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("vocab", P.TOP8_VOCABS)
def test_rowstats_planted(dtype, vocab):
    """samd_e2_rowstats without a workspace (k_e2_rowstats) and, in f16 / bf16, with one (k_e2_rowstats_part + _merge), on the plants of both
    maps: top_idx by equality, top_logp and row_lse against float64 at 2e-4 (the planted rows' plain fp32 evaluation is within 1e-5 of float64,
    tests/test_select_planting_cpu.py, so the bar is left for summation order and __expf), and the two forms equal on the indices.
    Largest errors recorded on an MI355X, the same for f16, bf16 and fp32 at every vocabulary (8: 4.787e-07 for row_lse):
    |top_logp - float64| = 1.429e-06, |row_lse - float64| = 5.005e-07."""
    es = P.ESIZE[dtype]
    nbytes = lib().samd_e2_rowstats_workspace(vocab)
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    forms = [False] + ([True] if dtype != torch.float32 else [])
    worst_p = worst_l = 0.0
    for stride, batch in _top8_batches(("segment", "rowstats"), es, vocab, 8):
        rows = len(batch)
        x = _cuda(P.assemble(batch, stride, dtype))
        got_idx = {}
        for split in forms:
            t, st = make_state()
            t["top_idx"].fill_(-1); t["top_logp"].fill_(float("nan")); t["row_lse"].fill_(float("nan"))
            check(lib().samd_e2_rowstats(_ptr(x), torch_dtype_code(dtype), rows, vocab, stride, C.byref(st), _ptr(ws) if split else None, nbytes if split else 0,
                                         current_stream()))
            idx = t["top_idx"].view(8, 8).cpu().numpy()
            logp = t["top_logp"].view(8, 8).cpu().numpy().astype(np.float64)
            lse = t["row_lse"].cpu().numpy().astype(np.float64)
            assert (idx[rows:] == -1).all() and np.isnan(lse[rows:]).all()
            for r, c in enumerate(batch):
                assert idx[r].tolist() == c.expect.tolist(), (c.name, "split" if split else "one-workgroup", stride, idx[r].tolist(), c.expect.tolist())
                want = c.row[c.expect] - c.lse
                fin = np.isfinite(want)
                assert np.array_equal(logp[r][~fin], want[~fin]), (c.name, logp[r], want)          # -inf stays -inf
                worst_p = max(worst_p, float(np.abs(logp[r][fin] - want[fin]).max()))
                worst_l = max(worst_l, abs(float(lse[r]) - c.lse))
                assert np.abs(logp[r][fin] - want[fin]).max() < P.LSE_BAR and abs(float(lse[r]) - c.lse) < P.LSE_BAR, (c.name, split, logp[r], want, lse[r], c.lse)
            got_idx[split] = idx[:rows].copy()
        if len(forms) == 2:
            assert np.array_equal(got_idx[False], got_idx[True])
    print(f"rowstats planted {dtype} vocab {vocab}: largest |top_logp - float64| = {worst_p:.3e}, largest |row_lse - float64| = {worst_l:.3e}")


# ---- 3.3 select / finish ------------------------------------------------------------------------------------------------------------------------
H, VOCAB = 64, 50


def _write_state(t, S):
    for k, v in S.items():
        t[k][:len(v)].copy_(torch.from_numpy(v))


def _assert_state(t, S, what):
    for k, v in S.items():
        got = t[k][:len(v)].cpu().numpy()
        assert np.array_equal(got, v, equal_nan=v.dtype.kind == "f"), (what, k, got, v)


def _poisoned_state(depth, keep):
    t, st = make_state(depth, keep)
    for k, v in t.items():
        v.fill_(float("nan") if v.dtype == torch.float32 else -1)
    return t, st


def _run_select(t, st, S, level, top_logp, top_idx, dtype, embed, hidden, advance_L, L0):
    t["top_logp"].copy_(torch.from_numpy(np.asarray(top_logp, np.float32).reshape(64)))
    t["top_idx"].copy_(torch.from_numpy(np.asarray(top_idx, np.int32).reshape(64)))
    fc_in = torch.full((8, 2 * H), -1, dtype=torch.int16, device="cuda")
    relpos = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    d_L, d_Lw, d_n = (_cuda(np.array([v], np.int32)) for v in (L0, -1, -1))
    check(lib().samd_e2_select(C.byref(st), level, _ptr(hidden), _ptr(embed), H, VOCAB, _ptr(fc_in), _ptr(relpos), _ptr(d_L), _ptr(d_Lw), _ptr(d_n), advance_L,
                               torch_dtype_code(dtype), current_stream()))
    ids, src = P.e2_select(S, level, top_logp, top_idx)
    _assert_state(t, S, ("level", level))
    want_fc = torch.cat((embed.cpu()[torch.from_numpy(P.e2_clamped(ids, VOCAB))], hidden.cpu()[torch.from_numpy(src.astype(np.int64))]), dim=1)
    assert torch.equal(fc_in.cpu(), want_fc), ("fc_in", level)
    assert relpos.cpu().tolist() == [level + 1] * 8
    assert (d_L.item(), d_Lw.item(), d_n.item()) == (L0 + advance_L, L0 + advance_L + 8 * (level + 1), 8)
    assert np.array_equal(t["top_logp"].cpu().numpy(), np.asarray(top_logp, np.float32).reshape(64))           # inputs untouched
    return L0 + advance_L


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_e2_select_and_finish_planted(dtype):
    """states in quarters written straight into the arrays: single levels (all 8 from one row, one from each row, a four-way tie across
    rows at the 8th place, tie-free, tokens outside the vocabulary) and a chain of levels -1, 0, 1, 2 + finish at keep values that cut
    inside a group of tied candidates, that leave a kept node without its parent (it hangs off the root), and that keep everything.  After
    every level the whole state -- rec_*, both halves of scores, cs_index, ids, row_src, mask_rows, parents_list, all_scores, all_tokens --,
    the 8 rows of fc_in bit for bit, relpos, d_L, d_Lw and d_n are compared by equality; embed and hidden hold a 2-byte counter."""
    embed = torch.arange(VOCAB * H, dtype=torch.int16, device="cuda").view(VOCAB, H)
    hidden = (torch.arange(8 * H, dtype=torch.int16, device="cuda") + 20000).view(8, H)
    for case in P.e2_level_cases(VOCAB):
        t, st = _poisoned_state(3, 8)
        S, _ = P.e2_level_state(case)
        _write_state(t, S)
        _run_select(t, st, S, 1, case.top_logp, case.top_idx, dtype, embed, hidden, 0, 40)
    levels = P.e2_chain(vocab=VOCAB)
    keeps = P.e2_chain_keeps(levels)
    n = keeps[-1]
    t, st = _poisoned_state(3, n)
    S = P.e2_new_state(3, n)
    L = 100
    for level, lp, ti in levels:
        L = _run_select(t, st, S, level, lp, ti, dtype, embed, hidden, 5 if level < 0 else 0, L)
    assert L == 105
    sample = _cuda(np.array([7], np.int64))
    for keep in keeps:
        for k in ("rec_final_vals", "rec_final_idx"):
            t[k].fill_(float("nan") if t[k].dtype == torch.float32 else -1)
            S[k][:] = np.nan if S[k].dtype.kind == "f" else -1
        tokens = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda")
        parents = torch.full((n + 2,), -9, dtype=torch.int32, device="cuda")
        check(lib().samd_e2_finish(C.byref(st), 3, keep, _ptr(sample), _ptr(tokens), _ptr(parents), current_stream()))
        want_t, want_p = P.e2_finish(S, 3, keep, 7)
        assert tokens.cpu().tolist() == want_t.tolist() + [-1] * (n + 1 - keep), keep
        assert parents.cpu().tolist() == want_p.tolist() + [-9] * (n + 1 - keep), keep
        _assert_state(t, S, ("finish", keep))


# ---- 3.4 sampling -------------------------------------------------------------------------------------------------------------------------------
def _run_sampled(probs, cand, uniforms, dtype, rowmap, n_rows):
    V = probs.shape[1]
    C_, D = cand.shape
    d_probs = _cuda(torch.from_numpy(np.ascontiguousarray(probs)).to(dtype))
    d_cand = _cuda(np.ascontiguousarray(cand, dtype=np.int64))
    d_u = _cuda(np.asarray(list(uniforms) + [0.25], np.float64))            # (one spare so that the array is never empty; n_uniforms bounds it)
    work = torch.full((V,), float("nan"), dtype=dtype, device="cuda")
    out = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    if rowmap is None:
        check(lib().samd_posterior_sampled(_ptr(d_probs), torch_dtype_code(dtype), _ptr(d_cand), C_, D, V, _ptr(d_u), len(uniforms), _ptr(work), _ptr(out),
                                           current_stream()))
    else:
        d_map = _cuda(np.ascontiguousarray(rowmap, dtype=np.int32))
        check(lib().samd_posterior_sampled_nodes(_ptr(d_probs), torch_dtype_code(dtype), _ptr(d_map), n_rows, _ptr(d_cand), C_, D, V, _ptr(d_u), len(uniforms),
                                                 _ptr(work), _ptr(out), current_stream()))
    return out.cpu().tolist(), work.cpu()


PAIR_P = (0.5, 2.0 ** -9)


def decision_table(dtype):
    """for every planted kind of uniform at p = 1/2 and 2^-9, and 0.0 against 0: (kind, p, r, CPU torch, device torch, kernel) where the two
    torch columns evaluate the reference's expression `r <= acp` on a 0-dim tensor of dtype T and the kernel column is the accept length of a
    one-candidate walk"""
    rows = []
    for p in PAIR_P + (0.0,):
        for kind in (P.UNIFORM_KINDS if p else ("zero",)):
            r = P.uniform_for(kind, p, dtype)
            probs = np.zeros((1, 8)); probs[0, 3] = p; probs[0, 5] = 0.25
            out, _ = _run_sampled(probs, np.array([[1, 3]]), [r], dtype, None, 0)
            assert out[2] == 1 and out[4] == 0
            rows.append((kind, p, r, P.torch_accepts(r, p, dtype, "cpu"), P.torch_accepts(r, p, dtype, "cuda"), out[1] == 2))
    return rows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sampling_decisions_follow_torch_on_the_device(dtype):
    """The reference decides with `r <= acp`: a Python float against a 0-dim DEVICE tensor of the logits' dtype.  This test evaluates that
    expression itself on the device for the planted (r, p) pairs, prints it next to CPU torch, and asserts that the kernel's decision equals
    the device's on every pair.

    Recorded on an MI355X (CPU torch | device torch | kernel; A = accept, R = reject).  Device and CPU torch agree on every pair, so nothing
    had to be decided between them; had they differed, the kernel would follow the device, which is what the reference computes on.
    Both round the host scalar through fp32 into T (twice for the 2-byte types): the double just above the fp16 / bf16 tie still accepts.

        kind       r at p = 1/2 (f16 / bf16 / f32)                                  f16      bf16     f32
        p          0.5                                                               A A A    A A A    A A A
        above      0.5000000000000001                                                A A A    A A A    A A A
        tie        0.500244140625 / 0.501953125 / 0.5000000298023224                 A A A    A A A    A A A
        ulp        0.50048828125 / 0.50390625 / 0.5000000596046448                   R R R    R R R    R R R
        below      0.49999999999999994                                               A A A    A A A    A A A
        tie_above  0.5002441406250001 / 0.5019531250000001 / 0.5000000298023225      A A A    A A A    R R R
        zero       0.0 against p = 0.0                                               A A A    A A A    A A A

    and the same seven rows, with the same decisions, at p = 2^-9 (tie 0.0019540786743164062 / 0.00196075439453125 / 0.001953125116415322).
    A comparison of Python floats gives R for above, tie and tie_above."""
    rows = decision_table(dtype)
    print(f"\n{dtype}: kind, p, r -> CPU torch, device torch, kernel")
    for kind, p, r, cpu, dev, ker in rows:
        print(f"  {kind:10s} p={p!r:12} r={r!r:24} {'accept' if cpu else 'reject':7s} {'accept' if dev else 'reject':7s} {'accept' if ker else 'reject'}")
    assert all(ker == dev for _, _, _, _, dev, ker in rows), [r for r in rows if r[4] != r[5]]


@pytest.mark.parametrize("entry", ["cells", "nodes"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [5, 1025, 3001])
def test_posterior_sampled_planted(dtype, V, entry):
    """every planted chain, table and uniform through samd_posterior_sampled (one probability row per cell) and samd_posterior_sampled_nodes
    (one per node; the last node written as -1 and as an entry >= n_rows): out[0..4] and, where the residual flag is set, the whole work
    vector by equality -- with all the uniforms the walk needs, with one fewer (status 1, everything decided before it reported) and with
    none.  The expectation performs the reference's `r <= acp` and its renormalisation with torch on device tensors of dtype T."""
    nodes_entry = entry == "nodes"
    for c in P.sampling_cases(V):
        probs, rowmap, n_rows = P.sampling_inputs(c, nodes_entry)
        full = P.sampling_expect(c, dtype, nodes_entry, device="cuda")
        for n_u in (len(c.script), len(c.script) - 1, 0):
            want = full if n_u == len(c.script) else P.sampling_expect(c, dtype, nodes_entry, n_uniforms=n_u, device="cuda")
            out, work = _run_sampled(probs, c.cand, full["all_uniforms"][:n_u], dtype, rowmap, n_rows)
            assert out == want["out"], (c.name, n_u, out, want["out"])
            assert want["out"][4] == (1 if n_u < len(c.script) else 0)
            if want["out"][3]:
                assert torch.equal(work, want["work"].cpu()), (c.name, n_u)
