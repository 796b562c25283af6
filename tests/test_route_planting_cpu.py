"""The planted router cases of tests/route_planting.py, on the CPU: the logits are exact, every plant selects what its name says, the
either-neighbour band stays under its cap in every case and dtype (from the reference alone), every pair kind of the tie plant occurs, the
lane-by-lane model of k_moe_route equals the reference, every named fault changes an index or a weight that is compared by equality, and
HF's router (fp32 module) agrees with the restatement on the rows without ties."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import route_planting as RP

SHAPES = RP.ROUTE_SHAPES + RP.WIDE_SHAPES + (RP.EMPTY_SHAPE,)
CONFIGS = [(dt, norm) for dt in RP.DTYPES for norm in (True, False)]
ids = lambda s: "E{}_k{}_H{}_rows{}_n{}".format(*s)          # noqa: E731


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_logits_are_exact_and_plants_select_what_they_say(shape):
    c = RP.route_case(shape)
    RP.check_case(c)                                          # h @ W.T == target, sum |h| |W| < 2^24, the casts lose nothing
    E, k = c.E, c.k
    fine = c.H >= 2 * E
    assert c.P == (RP.COARSE if fine else 1)
    # what the fp32 kernel adds, unit by unit: integers, so any order of the same terms gives the same sum
    ref = RP.reference(c.target, k, True, torch.float16)
    for r in range(c.n):
        t, kind, got = c.target[r], c.kinds[r], ref.idx[r].tolist()
        want = sorted(range(E), key=lambda e: (-int(t[e]), e))[:k]
        assert got == want, (r, kind)
        assert len(set(got)) == k
        top = np.nonzero(t == t.max())[0]
        if kind == "plateau_all":
            assert len(top) == E and got == list(range(k))
        elif kind == "plateau_k":
            assert len(top) == k and got == top.tolist()
        elif kind == "tie_above":
            assert len(top) == min(k + 3, E) and got == top[:k].tolist()
        elif kind == "ramp":
            assert got in (list(range(E - 1, E - 1 - k, -1)), list(range(k)))
        elif kind == "all_negative":
            assert t.max() < -5
        elif kind == "resolution":
            srt = sorted(range(E), key=lambda e: (-int(t[e]), e))
            hi, lo = (srt[k - 1], srt[k]) if k < E else (srt[k - 2], srt[k - 1])
            assert t[hi] == t[lo] + 1 and lo < hi and t[lo] >= RP.BIG_LOGIT          # the LOWER expert holds the smaller logit ...
            for dt in RP.DTYPES:                                                  # ... and the dtype sees a tie
                assert float(torch.tensor(float(t[hi])).to(dt)) == float(torch.tensor(float(t[lo])).to(dt)) == float(t[lo])
        elif kind == "tie_kth":
            pk, a, b, decisive = c.pairs[r]
            tied = np.nonzero(t == t[a])[0]
            assert t[a] == t[b] and 2 <= len(tied) <= 6
            above = int((t > t[a]).sum())
            if k < E:
                assert above < k < above + len(tied), "the cut runs through the tie"
                assert got[above:] == tied[:k - above].tolist()
            if decisive:
                assert tied.tolist() == [a, b] and a in got and b not in got
    if c.n >= 16 and fine and E >= 2:
        assert {"spaced", "tie_kth", "tie_above", "plateau_k", "ramp", "all_negative", "resolution"} <= set(c.kinds)
    if c.n >= 16 and not fine:
        assert "resolution" not in c.kinds                       # (H = E: no column for the low bits; said in the helper)


def test_every_plant_and_every_pair_kind_occurs():
    cases = RP.all_cases()
    assert {k for c in cases for k in c.kinds} == set(RP.KINDS)
    decisive = {p[0] for c in cases for p in c.pairs if p is not None and p[3]}
    assert decisive == set(RP.PAIR_KINDS), set(RP.PAIR_KINDS) - decisive
    placed = {}
    for c in cases:
        for p in c.pairs:
            if p is not None:
                placed.setdefault(p[0], []).append((RP.expert_place(p[1]), RP.expert_place(p[2]), p[1], p[2], c.E))
    for kind, lst in placed.items():
        for (la, sa, wa, ra), (lb, sb, wb, rb), a, b, E in lst:
            if kind.startswith("same_lane"):
                assert la == lb and sb - sa == int(kind.split("_")[-1]) // 64
            elif kind.startswith("neighbour"):
                assert lb == la + 1 and sa == sb and a % 2 == (kind == "neighbour_odd")
            elif kind == "lanes_31_32":
                assert (la, lb) == (31, 32)
            elif kind == "lanes_0_63":
                assert {la, lb} == {0, 63}
            elif kind == "waves_rounds":
                assert wa != wb and ra != rb
            else:
                assert (a, b) == (0, E - 1)
    # both parities of the neighbouring lanes, both forms of lanes 0 | 63 (expert 63 | 64 puts the LOWER expert into the higher lane)
    assert {(p[1], p[2]) for c in cases for p in c.pairs if p is not None and p[0] == "lanes_0_63"} == {(0, 63), (63, 64)}


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_band_cap_holds_from_the_reference_alone(shape):
    c = RP.route_case(shape)
    for dt, norm in CONFIGS:
        ref = RP.reference(c.target, c.k, norm, dt)
        share = RP.band_share(ref)
        print(f"{c.name} {str(dt)[6:]} norm={int(norm)}: {int(ref.band.sum())} of {ref.band.size} weights in the band ({100 * share:.2f} %)")
        assert share <= RP.BAND_CAP, (c.name, dt, norm, share)
        assert bool((ref.p[:, :-1] >= ref.p[:, 1:]).all()) and bool((ref.p >= 2.0 ** -126).all())       # descending; normal fp32 numbers
        if norm:
            assert np.allclose(ref.p.sum(axis=1), 1.0, rtol=0, atol=1e-15)
        # rounding: numpy's half-even grid against torch's cast, wherever a double rounding through fp32 cannot matter
        tw = torch.from_numpy(ref.p).to(dt).double().numpy()
        assert np.array_equal(tw[~ref.band], ref.w[~ref.band])
        lo, hi = RP.neighbours(ref.p, dt)
        assert bool(((tw == lo) | (tw == hi)).all())
        for r in range(c.n):
            if RP.exact_plateau(c, r, norm):                  # the exact rows: a dtype value, never in the band
                want = 1.0 / c.k if norm else 1.0 / c.E
                assert bool((ref.p[r] == want).all()) and bool((ref.w[r] == want).all()) and not ref.band[r].any(), (r, c.kinds[r])


def test_margin_and_band_geometry():
    assert RP.MARGIN_ULPS == 64
    for dt, mant in ((torch.float16, 10), (torch.bfloat16, 7)):
        u = 2.0 ** (-2 - mant)                                # the dtype's spacing in [1/4, 1/2)
        mid = 0.25 + 5 * u + u / 2
        f32 = 2.0 ** (-2 - 23)
        p = np.array([mid, mid + 64 * f32, mid - 64 * f32, mid + 65 * f32, mid - 65 * f32, 0.25 + 5 * u, 0.25])
        assert RP.in_band(p, dt).tolist() == [True, True, True, False, False, False, False]
        assert RP.round_to(p, dt).tolist() == [0.25 + 6 * u, 0.25 + 6 * u, 0.25 + 5 * u, 0.25 + 6 * u, 0.25 + 5 * u, 0.25 + 5 * u, 0.25]
    assert RP.round_to(np.array([2.0 ** -26, 2.0 ** -25, 3 * 2.0 ** -25]), torch.float16).tolist() == [0.0, 0.0, 2.0 ** -23]       # fp16 subnormals, half-even


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_model_without_a_fault_is_the_reference(shape):
    c = RP.route_case(shape)
    for dt, norm in CONFIGS:
        ref = RP.reference(c.target, c.k, norm, dt)
        idx, w = RP.model_route(c, norm, dt)
        assert np.array_equal(idx[:c.n], ref.idx) and np.array_equal(w[:c.n], ref.w)
        assert bool((idx[c.n:] == -1).all()) and bool((w[c.n:] == 0).all())
        assert RP.compare(c, ref, idx, w, dt) == (int(ref.band.sum()), 0)
    n_active, active, counts, lists = RP.lists_reference(ref.idx, c.n, c.k)
    assert active == sorted(set(ref.idx.reshape(-1).tolist())) and n_active == len(active) and sum(counts) == c.n * c.k
    flat = ref.idx.reshape(-1).tolist()
    for e, cnt, lst in zip(active, counts, lists):
        assert lst == [p for p in range(c.n * c.k) if flat[p] == e] and cnt == len(lst)
        assert cnt <= 64 or c.rows > 64                       # (the <= 64-row call's lists hold 64 entries per expert)


def test_every_named_fault_is_caught():
    """a fault counts as caught by a (case, dtype, norm_topk) when it changes an index (or leaves a row >= n unwritten), or a weight that
    the reference compares by equality on a row whose indices it left alone; weights in the band never count"""
    caught = {f: [] for f in RP.FAULTS}
    by_kind = {f: set() for f in RP.FAULTS}
    for c in RP.all_cases():
        for dt, norm in CONFIGS:
            ref = RP.reference(c.target, c.k, norm, dt)
            for f in RP.FAULTS:
                idx, w = RP.model_route(c, norm, dt, f)
                rows_i = (idx[:c.n] != ref.idx).any(axis=1)
                rows_w = ((w[:c.n] != ref.w) & ~ref.band).any(axis=1) & ~rows_i
                tail = bool((idx[c.n:] != -1).any())
                if rows_i.any() or rows_w.any() or tail:
                    caught[f].append((c.name, str(dt)[6:], norm))
                    by_kind[f] |= {c.kinds[r] for r in np.nonzero(rows_i | rows_w)[0]}
                    with pytest.raises(AssertionError):       # ... and the comparison the GPU test makes refuses it
                        RP.compare(c, ref, idx, w, dt)
    for f in RP.FAULTS:
        print(f"{f}: caught by {len(caught[f])} (case, dtype, norm) combinations; plants {sorted(by_kind[f])}")
    assert all(caught[f] for f in RP.FAULTS), [f for f in RP.FAULTS if not caught[f]]
    # the plants that exist for a fault do catch it
    assert "tie_kth" in by_kind["tie_to_higher"] and "tie_kth" in by_kind["lane_slot_order"] and "tie_kth" in by_kind["shuffle_tie_keeps_own"]
    assert "plateau_all" in by_kind["tie_to_higher"] and "tie_above" in by_kind["tie_to_higher"]
    assert "ramp" in by_kind["no_removal_upper_slots"]
    assert "all_negative" in by_kind["pad_zero"] and "all_negative" in by_kind["last_group_dropped"]
    assert by_kind["logits_in_dtype"] == {"resolution"}
    assert {c for c, _, n in caught["renorm_always"]} and all(not n for _, _, n in caught["renorm_always"])
    assert all(n for _, _, n in caught["renorm_never"]) and all(n for _, _, n in caught["weights_rounded_twice"])
    assert all(c.n < c.rows for c in RP.all_cases() if any(c.name == x[0] for x in caught["rows_past_n_kept"]))


def test_decisive_pairs_split_the_tie_faults():
    """which decisive pair catches which tie fault, from the model: a same-lane pair is the lane scan's business, a pair in two lanes the
    tree's; keeps-own shows only where the HIGHER expert reaches lane 0 first (lane 32 before lane 31, an even lane before an odd one)"""
    seen = {f: set() for f in ("tie_to_higher", "lane_slot_order", "shuffle_tie_keeps_own")}
    for c in RP.all_cases():
        ref = RP.reference(c.target, c.k, True, torch.float16)
        for f in seen:
            idx, _ = RP.model_select(RP.model_logits(c, torch.float16), c.k, f) if c.n else (ref.idx, None)
            for r in range(c.n):
                p = c.pairs[r]
                if p is not None and p[3] and idx[r].tolist() != ref.idx[r].tolist():
                    seen[f].add(p[0] if p[0] != "lanes_0_63" else f"lanes_0_63{(p[1], p[2])}")
    every = set(RP.PAIR_KINDS) - {"lanes_0_63"} | {"lanes_0_63(0, 63)", "lanes_0_63(63, 64)"}
    assert seen["tie_to_higher"] == every
    assert seen["lane_slot_order"] == {"same_lane_64", "same_lane_128", "same_lane_192"}
    assert seen["shuffle_tie_keeps_own"] >= {"lanes_31_32", "neighbour_odd", "lanes_0_63(63, 64)"}
    assert not seen["shuffle_tie_keeps_own"] & {"same_lane_64", "same_lane_128", "same_lane_192", "neighbour_even", "lanes_0_63(0, 63)"}


def test_hf_router_agrees_on_rows_without_ties():
    """the restatement itself: transformers' Qwen3MoeTopKRouter as an fp32 module on the exact inputs (torch.softmax in fp32, torch.topk,
    HF's renormalisation) gives the reference's indices on every row without ties, and its weights, rounded to the dtype, under the same
    either-neighbour rule"""
    pytest.importorskip("transformers")
    from transformers import Qwen3MoeConfig
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeTopKRouter
    rows = 0
    for c in RP.all_cases():
        keep = [r for r in range(c.n) if c.kinds[r] in ("spaced", "ramp", "all_negative", "resolution")]
        keep = [r for r in keep if len(set(np.sort(c.target[r])[::-1][:min(c.k + 1, c.E)].tolist())) == min(c.k + 1, c.E)]
        if not keep:
            continue
        for norm in (True, False):
            gate = Qwen3MoeTopKRouter(Qwen3MoeConfig(hidden_size=c.H, num_experts=c.E, num_experts_per_tok=c.k, norm_topk_prob=norm))
            gate.weight = torch.nn.Parameter(torch.from_numpy(c.W).float(), requires_grad=False)
            with torch.no_grad():
                logits, w, idx = gate(torch.from_numpy(c.h[keep]).float())
            assert np.array_equal(logits.double().numpy(), c.target[keep].astype(np.float64))
            for dt in RP.DTYPES:
                ref = RP.reference(c.target[keep], c.k, norm, dt)
                assert np.array_equal(idx.numpy(), ref.idx), c.name
                got = w.to(dt).double().numpy()
                lo, hi = RP.neighbours(ref.p, dt)
                assert bool(np.where(ref.band, (got == lo) | (got == hi), got == ref.w).all()), (c.name, dt, norm)
        rows += len(keep)
    assert rows >= 300
