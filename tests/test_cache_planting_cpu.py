"""CPU proof of tests/cache_planting.py: the workloads meet the plan, the simulated loop is the oracle's, the float64 reference is
self-consistent, and every named fault lies far outside the bar -- from the references alone, no product code involved.

Measured here on the `base` workload's committed text (232 tokens, KV heads 2), per tensor: e_twin 0.0009 - 0.0022 in fp16 and 0.007 -
0.019 in bf16, so the bars are 0.0023 - 0.0043 and 0.018 - 0.037; the faults give e from 1.2 (a rejected node's row left in place) to 2.4
(every later row one row late) on the tensors they touch: 300 - 1000 bars in fp16, 35 - 130 in bf16.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import cache_planting as P
from oracle import sam_oracle as O

DTYPES = [torch.float16, torch.bfloat16]
SEPARATION = {torch.float16: 100.0, torch.bfloat16: 10.0}


@pytest.fixture(scope="module")
def sims():
    return {name: P.simulate(P.build_workload(name)) for name in P.WORKLOADS}


@pytest.fixture(scope="module")
def base(sims):
    """(fp32 module, master, committed text, records, reference cache) of the base workload"""
    lm32 = P.tiny_llama(kv_heads=2, seed=1)
    master = P.as_master(lm32)
    w, recs = P.build_workload("base"), sims["base"]
    text = w["target"][:recs[-1]["L1"]]
    return lm32, master, text, recs, P.reference_cache(master, text)


@pytest.mark.parametrize("name", list(P.WORKLOADS))
def test_workload_meets_the_plan(name, sims):
    w, recs = P.build_workload(name), sims[name]
    P.assert_plan(name, recs)
    assert 60 <= len(w["prompt"]) <= 130 and recs[-1]["L1"] < w["max_cache_len"]
    assert all(r["L"] + r["n"] <= w["max_cache_len"] for r in recs), "no draft row is written behind the cache"
    assert name == "end" or 25 <= len(recs) <= 45
    print(name, [(r["type"], r["n"], r["a"]) for r in recs])


@pytest.mark.parametrize("name", list(P.WORKLOADS))
def test_simulation_is_the_oracle_draft_model_step_by_step(name, sims):
    """a second DraftModel driven by hand along the committed text reproduces every record's draft, and every record's accept is the longest
    root path of the draft that the target continues"""
    w, recs = P.build_workload(name), sims[name]
    target = w["target"]
    d = O.DraftModel(w["max_predicts"], w["alpha"], w["K"], w["len_bias"], sam_static=O.StaticSAM.build(w["docs"], w["eos"]))
    d.reset()
    d.update(w["prompt"])
    L = len(w["prompt"])
    for r in recs:
        assert r["L"] == L
        ty, toks, anc = d.lookup_raw(target[L])
        assert (ty, toks, anc) == (r["type"], r["tokens"], r["anc"])
        assert r["n"] == len(toks) <= w["max_predicts"] and toks[0] == target[L]
        follows = [i for i in range(r["n"]) if all(toks[j] == target[L + r["depth"][j]] for j in _path(anc, i))]
        assert r["a"] == 1 + max(r["depth"][i] for i in follows)
        assert r["kv_index"][0] == 0 and all(anc[k] == r["kv_index"][j] for j, k in enumerate(r["kv_index"][1:]))
        assert r["accepted"] == target[L:L + r["a"]] and r["L1"] == L + r["a"]
        d.update(r["accepted"])
        L += r["a"]


def _path(anc, i):
    out = []
    while i != -1:
        out.append(i)
        i = anc[i]
    return out


def test_reference_is_self_consistent(base):
    lm32, master, text, recs, want = base
    assert want.shape == (2, 2, 2, len(text), 128) and want.dtype == torch.float64
    for m in (1, 97, len(text) - 1):
        assert (P.reference_cache(master, text[:m]) - want[:, :, :, :m]).abs().max().item() < 1e-12
    # a draft's rows along its accepted path are the committed text's rows: the invariant itself, on the reference
    r = next(r for r in recs if P.moved(r) and r["a"] >= 3)
    rows = P.draft_rows(master, text, r)
    assert (rows[:, :, :, r["kv_index"]] - want[:, :, :, r["L"]:r["L1"]]).abs().max().item() < 1e-12
    # ... and the master's rotary angles are float64: against HF's own fp32 angles the K rows move, the V rows of layer 0 do not
    plain = P.reference_cache(lm32.double(), text)
    assert 0 < (plain[:, 0] - want[:, 0]).abs().max().item() < 1e-3 and torch.equal(plain[0, 1], want[0, 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_every_named_fault_lies_far_outside_the_bar(dtype, base):
    lm32, master, text, recs, want = base
    e_twin = P.cache_error(P.reference_cache(P.low_precision_twin(lm32, dtype), text), want)
    bar = P.bar(e_twin, dtype)
    print(f"{dtype}: e_twin {e_twin.flatten().tolist()}, bar {bar.flatten().tolist()}")
    assert bool((e_twin > 0).all()) and bool((e_twin < (0.004 if dtype == torch.float16 else 0.04)).all())
    assert bool((P.cache_error(want, want) == 0).all())
    for fault in P.FAULTS:
        e = P.cache_error(P.apply_fault(fault, want, master, text, recs), want)
        ratio = e / bar
        print(f"  {fault}: e {e.flatten().tolist()} = {ratio.flatten().tolist()} bars")
        need = SEPARATION[dtype]
        assert bool((ratio >= need).any()), (fault, ratio)
        if fault in P.ON_EVERY_TENSOR:
            assert bool((ratio >= need).all()), (fault, ratio)


def test_a_nan_in_a_committed_row_is_an_error_of_the_metric(base):
    want = base[4]
    got = want.clone()
    got[1, 1, 0, 5, 7] = float("nan")
    e = P.cache_error(got, want)
    assert bool(torch.isnan(e[1, 1])) and not bool(e[1, 1] <= 1e9)
