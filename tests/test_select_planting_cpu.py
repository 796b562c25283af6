"""tests/select_planting.py on the CPU: every planted row places what its name says under the restated element maps, every planted value is
exact in bf16 / fp16 / fp32, every named fault changes the expectation of every case that names it (and every case is named), the log-sum-exp
condition holds, the EAGLE-2 restatement agrees with torch.topk where there are no ties, the sampling chains are exact with torch's own ops,
and samd_sam_only.posterior._sampled takes the planted decisions."""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import select_planting as P

FULL = {"argmax": [(2, 2 * 1024 * 8 + 5), (4, 2 * 1024 * 4 + 5)], "rows256": [(4, P.TOP8_VOCABS[2]), (4, P.TOP8_VOCABS[3])],
        "rowstats": [(2, P.TOP8_VOCABS[2]), (4, P.TOP8_VOCABS[3])], "segment": [(2, P.TOP8_VOCABS[3])]}
SHAPES = ([("argmax", es, v) for es in (2, 4) for v in P.ARGMAX_VOCABS(es)] + [("rows256", 4, v) for v in P.TOP8_VOCABS]
          + [(k, 2, v) for k in ("rowstats", "segment") for v in P.TOP8_VOCABS] + [("rowstats", 4, v) for v in P.TOP8_VOCABS])


def test_maps_partition_the_row():
    """every element has one owner, a thread meets its elements in ascending index, no thread of a segment holds more than 16, and the
    maps agree with the kernels' loops written out for a few elements"""
    for kernel, es, v in SHAPES:
        for aligned in (True, False):
            L = P.Layout(kernel, es, v, aligned)
            owner = np.stack((L.key, L.slot), 1)
            assert len(np.unique(owner, axis=0)) == v, (kernel, es, v, aligned)
            order = np.lexsort((L.slot, L.key))
            same = np.diff(L.key[order]) == 0
            assert (np.diff(order)[same] > 0).all()
            if kernel == "segment":
                assert L.slot.max() < 16 and np.unique(L.key, return_counts=True)[1].max() <= 16
    # k_argmax_rows, fp16, vocab 16389: vector 1025 = elements 8200..8207 -> thread 1, second pass; the tail 16384.. -> threads 0..4
    L = P.Layout("argmax", 2, 16389, True)
    assert (L.thread[8200], L.slot[8200], L.vec[8207], L.tail[8207]) == (1, 8, 1025, False)
    assert L.thread[16384:].tolist() == [0, 1, 2, 3, 4] and L.tail[16384:].all() and L.slot[16384] == 16 and not L.tail[16383]
    assert P.Layout("argmax", 2, 16389, False).tail.all() and P.Layout("argmax", 2, 16389, False).thread[1025] == 1
    # e2_load_segment, bf16: e0 = seg0 + (u * 256 + tid) * 8 -> element 4096 + (1 * 256 + 3) * 8 + 5 is thread 3, slot 8 + 5 of segment 1
    L = P.Layout("segment", 2, 3 * 4096, True)
    i = 4096 + (256 + 3) * 8 + 5
    assert (L.seg[i], L.thread[i], L.slot[i]) == (1, 3, 13)
    L = P.Layout("segment", 2, 3 * 4096, False)                 # g = seg0 + q * 256 + tid
    assert (L.seg[i], L.thread[i], L.slot[i]) == (1, (i - 4096) % 256, (i - 4096) // 256)
    L = P.Layout("segment", 4, 4096, True)                      # fp32: four units of 256 x 4
    assert (L.thread[1024 + 4 * 7 + 2], L.slot[1024 + 4 * 7 + 2]) == (7, 6)
    assert P.merge_place(33, 0) == (8, 1) and P.merge_place(1, 0) == (8, 0) and P.merge_place(31, 7) == (255, 0)


@pytest.mark.parametrize("kernel", ["argmax", "rows256", "rowstats", "segment"])
def test_planted_rows_place_what_they_name_and_are_exposed(kernel):
    """claims (checked in the builders against Layout.describe), exact values, expectation = np.lexsort, every named fault changes it"""
    seen_faults, n_cases = set(), 0
    for k, es, v in SHAPES:
        if k != kernel:
            continue
        for aligned in (True, False):
            L = P.Layout(k, es, v, aligned)
            cases = P.cases_for(k, es, v, aligned)
            assert len({c.name for c in cases}) == len(cases)
            for c in cases:
                n_cases += 1
                finite = c.row[np.isfinite(c.row)]
                assert P.exact_in_all(finite) and (len(finite) == 0 or np.abs(finite).max() < P.PAD_VALUE)
                n = len(c.expect)
                want = np.lexsort((np.arange(v), -c.row))[:n]
                assert np.array_equal(c.expect, want), c.name
                desc = L.describe(c.planted)
                assert all(desc[key] == val for key, val in c.claim.items()), (c.name, c.claim, desc)
                padded = np.concatenate((c.row, np.full(5, P.PAD_VALUE)))
                for f in c.must:
                    assert f in P.APPLIES[k]
                    if f == "lse_counts_inf":
                        assert np.isnan(P.lse_faulted(c.row, f)) and not np.isnan(c.lse)
                    else:
                        assert not np.array_equal(P.faulted(c.row, L, f, n=n, padded=padded), c.expect), (c.name, f)
                assert c.must or v == 1, c.name              # a row of one element has one possible answer
                seen_faults |= set(c.must)
    assert seen_faults == set(P.APPLIES[kernel]) and n_cases > 20
    for es, v in FULL[kernel]:
        have = {c.name for c in P.cases_for(kernel, es, v, True)}
        cannot = ({"merge_two_slots"} if v < 33 * P.SEG else set()) | ({"tie_both_tail"} if v % (16 // es) < 2 else set())      # (a tail of one element)
        assert set(P.REQUIRED[kernel]) - have <= cannot, (kernel, es, v, set(P.REQUIRED[kernel]) - have)
        have = {c.name for c in P.cases_for(kernel, es, v, False)}
        assert set(P.REQUIRED[kernel]) - have <= set(P.NO_VECTORS), (kernel, es, v)


def test_named_plants_sit_where_the_issue_puts_them():
    """the plants the kernels' special paths need, spelled out at the shapes the GPU test runs"""
    cs = {c.name: c for c in P.cases_for("segment", 2, P.TOP8_VOCABS[3], True)}
    L = P.Layout("segment", 2, P.TOP8_VOCABS[3], True)
    assert L.describe(cs["one_thread_8"].planted)["per_thread"] == (8,) and "no_rescan" in cs["one_thread_8"].must
    assert L.describe(cs["lanes_3_2_3"].planted)["per_thread"] == (3, 3, 2) and "no_rescan" in cs["lanes_3_2_3"].must
    assert len(cs["one_thread_9_equal"].planted) == 9 and cs["one_thread_9_equal"].planted[8] not in cs["one_thread_9_equal"].expect
    m = cs["merge_two_slots"]
    assert {1, 33} <= set(L.seg[list(m.planted)].tolist()) and "merge_256" in m.must and m.expect[-1] == 33 * P.SEG + 1
    a, b = cs["tie_two_waves_inverted"].planted
    assert a < b and L.wave[a] > L.wave[b] and "tie_by_slot" in cs["tie_two_waves_inverted"].must
    assert len(set(L.seg[list(cs["twelve_equal"].planted)].tolist())) == 4 and len(cs["twelve_equal"].planted) == 12
    assert "seg_edge" in cs["one_per_segment"].must and 4095 in cs["one_per_segment"].planted
    t = cs["tie_body_tail"].planted
    assert not L.tail[t[0]] and L.tail[t[1]] and t[1] == (P.TOP8_VOCABS[3] // 8) * 8
    z = cs["neg_zero_first"]
    assert np.signbit(z.row[z.planted[0]]) and not np.signbit(z.row[z.planted[1]]) and z.expect[0] == z.planted[0] and (np.delete(z.row, z.planted) < 0).all()
    cs = {c.name: c for c in P.cases_for("rowstats", 2, P.TOP8_VOCABS[2], True)}
    assert "list7" in cs["one_thread_8"].must and "list7" in cs["one_thread_9_equal"].must and "drop_tail" in cs["finite_only_in_tail"].must
    un = {c.name: c for c in P.cases_for("segment", 2, P.TOP8_VOCABS[2], False)}
    assert len(un["finite_only_in_tail"].planted) == 9 and np.isfinite(un["finite_only_in_tail"].row).sum() == 9
    am = {c.name: c for c in P.cases_for("argmax", 2, 7, True)}
    assert am["all_neg_inf"].expect.tolist() == [0] and am["tie_first_last"].expect.tolist() == [0]


def test_log_sum_exp_condition():
    """plain sequential fp32 is within 1e-5 of float64 on every planted row with a finite element: the GPU bar of 2e-4 is left for summation
    order and __expf; the planted values are known in closed form"""
    worst = 0.0
    for k, es, v in SHAPES:
        if k == "argmax":
            continue
        for c in P.cases_for(k, es, v, True):
            err = abs(P.lse32_sequential(c.row) - c.lse)
            worst = max(worst, err)
            assert err <= P.LSE_FP32_BAR, (c.name, v, err)
            if c.name == "neg_inf_but_one":
                assert c.lse == -3.0
            if c.name.startswith("lse_max"):
                assert 20.0 <= c.lse < 20.0 + 1e-9
    assert worst < P.LSE_FP32_BAR < P.LSE_BAR / 10


def test_batches_hold_every_case_at_the_alignment_it_was_built_for():
    for kernel, es, v in [("segment", 2, 4099), ("rowstats", 4, 12287), ("argmax", 2, 1003)]:
        al, un = P.strides(v, es)
        assert al > v and (al * es) % 16 == 0 and un > v and (un * es) % 16 != 0
        got = [c.name for b in P.batches(kernel, es, v, al) for c in b]
        assert got == [c.name for c in P.cases_for(kernel, es, v, True)]
        unal = P.cases_for(kernel, es, v, False)
        placed = []
        for b in P.batches(kernel, es, v, un):
            assert len(b) <= 8
            for r, c in enumerate(b):
                pool = P.cases_for(kernel, es, v, P.row_aligned(r, un, es))
                assert any(c is q for q in pool)
                if not P.row_aligned(r, un, es):
                    placed.append(c.name)
        assert placed == [c.name for c in unal]
        x = P.assemble(P.batches(kernel, es, v, un)[0], un, torch.float32, dead_rows=2)
        assert float(x[0, v:].min()) == P.PAD_VALUE and float(x[-1].min()) == P.PAD_VALUE and x.shape[1] == un


# ---- EAGLE-2 --------------------------------------------------------------------------------------------------------------------------------
def test_e2_levels_are_exact_and_exposed():
    cases = {c.name: c for c in P.e2_level_cases()}
    assert set(cases) == {"all_from_one_row", "one_from_each_row", "four_way_tie_at_8th", "tie_free", "tokens_out_of_range"}
    for c in cases.values():
        assert c.must, c.name
        cu64 = c.top_logp.astype(np.float64) + c.scores.astype(np.float64)[:, None]
        assert np.array_equal((c.top_logp + c.scores[:, None]).astype(np.float64), cu64)        # exact in fp32
        _, S = P.e2_level_state(c)
        sel = S["cs_index"]
        if c.name == "all_from_one_row":
            assert (sel // 8 == 5).all() and sel.tolist() == [40, 41, 42, 43, 44, 45, 46, 47]
        if c.name == "one_from_each_row":
            assert sorted((sel // 8).tolist()) == list(range(8)) and "select_tie_reversed" in c.must
        if c.name == "four_way_tie_at_8th":
            flat = cu64.reshape(64)
            tied = np.nonzero(flat == flat[sel[7]])[0]
            assert len(tied) == 4 and sel[6:].tolist() == tied[:2].tolist() and len(set((tied // 8).tolist())) == 4
        if c.name == "tie_free":
            assert len(np.unique(cu64)) == 64
            top = torch.topk(torch.from_numpy(cu64.reshape(64)), 8)
            assert top.indices.tolist() == sel.tolist() and top.values.tolist() == S["scores"][0:8].astype(np.float64).tolist()
            assert c.must == ("scores_not_added",)
        if c.name == "tokens_out_of_range":
            assert (S["ids"] >= 50).any() and (S["ids"] < 0).any()
            assert P.e2_clamped(S["ids"], 50).min() == 0 and P.e2_clamped(S["ids"], 50).max() == 49


def test_e2_chain_and_finish():
    """the chain's restatement against the reference's own lines written with torch (topk on a tie-free chain), the keep values, the fault"""
    levels = P.e2_chain()
    tie_cut, orphan, n = P.e2_chain_keeps(levels)
    S = P.e2_new_state(3, n)
    for level, lp, t in levels:
        P.e2_select(S, level, lp, t)
    assert not np.isnan(S["all_scores"]).any() and (S["parents_list"] >= 0).all()
    sc = S["all_scores"].astype(np.float64)
    ranked = np.lexsort((np.arange(n), -sc))
    assert sc[ranked[tie_cut - 1]] == sc[ranked[tie_cut]]                                  # the cut is inside a group of equal scores
    tok, par = P.e2_finish(S, 3, orphan, 7)
    _, par_f = P.e2_finish(S, 3, orphan, 7, "finish_no_unkept_rule")
    kept = np.sort(ranked[:orphan])
    bad = [t for t in range(orphan) if S["parents_list"][kept[t] // 8] != 0 and S["parents_list"][kept[t] // 8] - 1 not in kept]
    assert bad and all(par[1 + t] == 0 for t in bad) and not np.array_equal(par, par_f)
    tok, par = P.e2_finish(S, 3, n, 7)
    assert par[0] == -1 and all(0 <= par[i] < i for i in range(1, n + 1)) and tok[0] == 7
    assert np.array_equal(np.sort(S["rec_final_idx"]), np.arange(n))
    # a tie-free chain, level by level, against the reference's lines in torch (eagle2_model.py:872-913)
    rng = np.random.default_rng(2)
    S = P.e2_new_state(2, 30)
    lp0 = -0.25 * np.sort(rng.permutation(16)[:8]).astype(np.float32); t0 = rng.integers(0, 50, (8, 8))
    top = np.zeros((8, 8), np.float32); top[0] = lp0
    P.e2_select(S, -1, top, t0)
    scores, cs = torch.from_numpy(lp0.copy()), torch.arange(8)
    scores_list, parents_list, toks = [scores[None]], [torch.zeros(1, dtype=torch.long)], [torch.from_numpy(t0[:1])]
    for i in range(2):
        cu = -0.25 * np.sort(rng.permutation(64).reshape(8, 8), axis=1) - 16.0 * (i + 1)
        lp = (cu - scores.numpy()[:, None]).astype(np.float32)
        t = rng.integers(0, 50, (8, 8))
        P.e2_select(S, i, lp, t)
        parents_list.append(cs + 1 + 64 * max(0, i - 1) + (8 if i > 0 else 0))
        cu_t = torch.from_numpy(lp) + scores[:, None]
        tk = torch.topk(cu_t.view(-1), 8)
        cs, scores = tk.indices, tk.values
        scores_list.append(cu_t); toks.append(torch.from_numpy(t))
        assert S["cs_index"].tolist() == cs.tolist() and S["row_src"].tolist() == (cs // 8).tolist()
        assert S["ids"].tolist() == torch.from_numpy(t).view(-1)[cs].tolist()
    flat = torch.cat([s.reshape(-1) for s in scores_list])
    idx = torch.sort(torch.topk(flat, 30).indices).values
    dp = torch.cat(parents_list)[idx // 8]
    mi = torch.searchsorted(idx, dp - 1, right=False); mi[dp == 0] = -1; mi = mi + 1
    tok, par = P.e2_finish(S, 2, 30, 9)
    assert par[1:].tolist() == mi.tolist() and tok[1:].tolist() == torch.cat([x.reshape(-1) for x in toks])[idx].tolist()
    assert S["parents_list"].tolist() == torch.cat(parents_list).tolist()


# ---- sampling -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("V", [5, 1025, 3001])
def test_sampling_chains_are_exact_with_torch(dtype, V):
    """rejecting the masses in descending order leaves powers of two at every step, in T, with torch's own sum and division"""
    toks = P.chain_tokens(V)
    assert len(toks) == 5 and toks[0] == 0 and toks[-1] == V - 1 and (V < 2048 or {1023, 1024, 2047} <= set(toks))
    w = torch.from_numpy(P.chain_probs(V, (0, 1, 2, 3, 4))).to(dtype)
    assert float(w.double().sum()) == 1.0
    for k in range(4):
        assert float(w[toks[k]]) == 0.5
        w[toks[k]] = 0
        w = w / w.sum()
        assert float(w.double().sum()) == 1.0 and set(w.double().tolist()) <= {0.0, 1.0, 0.5, 0.25, 0.125}
    assert float(w[toks[4]]) == 1.0
    if V > 600:
        w = torch.from_numpy(P.small_masses_probs(V, 0)).to(dtype)
        w[0] = 0
        w = w / w.sum()
        assert int((w == 2.0 ** -9).sum()) == 512 and float(w.double().sum()) == 1.0


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_planted_uniforms_straddle_the_rounding_of_the_scalar(dtype):
    """torch's rule on this CPU for every kind of planted uniform at p = 1/2 and p = 2^-9 (even mantissas: the tie rounds to p), against a
    comparison in double"""
    for p in (0.5, 2.0 ** -9):
        got = {k: P.torch_accepts(P.uniform_for(k, p, dtype), p, dtype) for k in P.UNIFORM_KINDS}
        dbl = {k: P.uniform_for(k, p, dtype) <= p for k in P.UNIFORM_KINDS}
        assert dbl == dict(p=True, above=False, tie=False, ulp=False, below=True, tie_above=False)
        assert got == dict(p=True, above=True, tie=True, ulp=False, below=True, tie_above=dtype != torch.float32), (p, got)
    assert P.torch_accepts(0.0, 0.0, dtype)
    r = P.uniform_for("ulp", 0.5, dtype)
    assert float(torch.tensor(r, dtype=dtype)) == r > 0.5


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("V", [5, 1025, 3001])
def test_sampling_cases_do_what_they_name_and_are_exposed(dtype, V):
    cases = {c.name: c for c in P.sampling_cases(V)}
    kinds = set()
    for c in cases.values():
        assert P.exact_in_all(c.probs) and c.cellnode.shape == c.cand.shape and np.allclose(c.probs.sum(1), 1.0, atol=0)
        kinds |= set(c.script)
        for nodes_entry in (False, True):
            want = P.sampling_expect(c, dtype, nodes_entry)
            assert want["out"][4] == 0 and want["out"][2] == len(c.script)
            changing = set()
            for f in P.SAMPLING_FAULTS:
                got = P.sampling_expect(c, dtype, nodes_entry, fault=f)
                same = got["out"] == want["out"] and (want["work"] is None or (got["work"] is not None and torch.equal(got["work"], want["work"])))
                if not same:
                    changing.add(f)
            need = set(c.must) - (set() if nodes_entry else {"rowmap_neg_row0"})
            assert need <= changing, (c.name, nodes_entry, need - changing)
            # one uniform fewer: status 1, the decisions before it stand; none: nothing accepted
            short = P.sampling_expect(c, dtype, nodes_entry, n_uniforms=len(c.script) - 1)
            assert short["out"][4] == 1 and short["out"][2] == len(c.script) - 1 and short["pairs"] == want["pairs"][:-1]
            none = P.sampling_expect(c, dtype, nodes_entry, n_uniforms=0)
            assert none["out"] == [0, 1, 0, 0, 1]
    assert kinds >= set(P.UNIFORM_KINDS) and ("zero" in kinds or V == 5)
    w = P.sampling_expect(cases["reject_reject_accept"], dtype, False)
    assert [ok for _, _, ok in w["pairs"]] == [False, False, True, True] and w["out"] == [3, 3, 4, 0, 0]
    assert [p for _, p, _ in w["pairs"]] == [0.5, 0.5, 0.5, 0.5]
    assert P.sampling_expect(cases["accept_to_full_depth"], dtype, False)["out"] == [0, 5, 4, 0, 0]
    e = P.sampling_expect(cases["every_row_rejected"], dtype, True)
    assert e["out"] == [0, 1, 4, 1, 0] and float(e["work"][P.chain_tokens(V)[4]]) == 1.0 and float(e["work"].double().sum()) == 1.0
    rm = P.sampling_inputs(cases["last_node_cells"], True)[1]
    assert (rm == -1).any() and (rm >= 3).any()
    if V > 5:
        z = P.sampling_expect(cases["zero_against_zero"], dtype, False)
        assert z["pairs"][0] == (0.0, 0.0, True)


class _Cfg:
    greedy = False

    @staticmethod
    def logits_processor(_, x):
        return x


@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("V", [5, 1025])
def test_posterior_sampled_takes_the_planted_decisions(dtype, V, monkeypatch):
    """samd_sam_only.posterior._sampled on CPU tensors: the same decisions as the reference's `r <= acp` on a tensor of dtype T, for every
    planted kind of uniform -- the double just above p and the tie accept where a comparison of Python floats rejects.  _sampled takes
    logits: they are log(p) in T, whose softmax gives the planted masses back only up to a rounding in the 2-byte types, so the uniforms
    are made by the walk from the probabilities that torch.softmax returns (the same op on the same tensor), by the cases' scripts."""
    posterior = pytest.importorskip("samd_sam_only.posterior")
    teeth = 0
    for c in P.sampling_cases(V):
        probs = torch.from_numpy(c.probs[c.cellnode.reshape(-1)])
        C, D = c.cand.shape
        logits = torch.log(probs).clamp(min=-60.0).to(dtype).reshape(C, D, V)
        back = torch.softmax(logits, dim=-1).reshape(C * D, V).double().numpy()
        want = P.sample_walk(back, c.cand, None, dtype, script=c.script + ("p",) * 8)
        assert want["out"][4] == 0
        teeth += P.sample_walk(back, c.cand, want["uniforms"] + [0.999] * 8, dtype, fault="double_compare")["out"][:2] != want["out"][:2]
        stream = iter(want["uniforms"] + [0.999] * 4)
        monkeypatch.setattr(random, "random", lambda: next(stream))
        best, n_acc, sample_p = posterior._sampled(logits, torch.from_numpy(c.cand), _Cfg)
        assert [int(best), int(n_acc)] == want["out"][:2], (c.name, dtype)
        assert next(stream) == 0.999 and len(want["uniforms"]) == want["out"][2]              # the host stream stands where the reference's would
        if want["out"][3]:
            assert torch.equal(sample_p.reshape(-1), want["work"])
    assert teeth >= 2
