"""The planting of tests/dyn_planting.py checked on the CPU: what tests/test_gpu_dyn_planted.py relies on.

  * every case's condition holds on the model (run lengths, rounds, the wrap past slot H - 1, state / edge / clone counts, clone degree);
  * RefDynSAM (the model of the table layout) gives oracle.sam_oracle.DynSAM's export on every case, whole and midway;
  * every named fault changes a compared output (the table image, the export or a lookup result) in at least one case, and every case
    catches at least one fault -- printed as a table (pytest -s).  This is the proof that the GPU file bites: no defective kernel is
    ever built or run."""
import os

import numpy as np
import pytest

import dyn_planting as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_restated_from_the_sources():
    """the constants this module restates are the ones the kernel and the session use"""
    dev = open(os.path.join(ROOT, "sam-decoding_amd", "csrc", "sam_device.h")).read()
    ker = open(os.path.join(ROOT, "sam-decoding_amd", "csrc", "sam_kernels.hip")).read()
    assert "k *= 0x9E3779B97F4A7C15ull;" in dev and "return (uint32_t)(k >> 29);" in dev
    assert "((uint64_t)(uint32_t)state << 32) | (uint32_t)tok" in dev
    assert "#define WAVE 64" in dev and "h = (h + WAVE) & D.hmask;" in dev
    assert "uint32_t H = 1024; while (H < (uint32_t)max_tokens * 8u) H <<= 1;" in ker
    assert "D.cap_states = 2 * max_tokens + 2;" in ker and "D.cap_text = max_tokens + 2;" in ker
    assert [P.table_size(n) for n in (1, 128, 129, 256, 257, 520)] == [1024, 1024, 2048, 2048, 4096, 8192]
    assert P.dyn_hash(0) == 0 and P.dyn_hash(1) == (0x9E3779B97F4A7C15 >> 29) & 0xFFFFFFFF
    assert P.dyn_key(3, P.TOK_MAX) == (3 << 32) | 0x7FFFFFFF


def test_export_table_is_declared_and_bound():
    import samd_hip
    hdr = open(os.path.join(ROOT, "include", "samd_hip.h")).read()
    assert "int samd_session_export_table(samd_session_t *s, int64_t out_info[2], uint64_t *h_key, int32_t *h_dst, int32_t *h_next," in hdr
    res, args = samd_hip._PROTOS["samd_session_export_table"]
    assert len(args) == 8 and hasattr(samd_hip.Session, "export_table")


def test_cluster_tokens():
    for mt, window in ((128, 24), (256, 24), (128, 8)):
        H = P.table_size(mt)
        toks = P.cluster_tokens(mt, mt - 8, window)
        assert len(set(toks)) == mt - 8 and all(0 <= t <= P.TOK_MAX for t in toks)
        assert all(P.home(0, t, H) >= H - window for t in toks)
    cand = P.candidates()
    assert [next(cand), next(cand), next(cand)] == [0, P.TOK_MAX, 1]


@pytest.mark.parametrize("name", list(P.CASES))
def test_conditions_hold_on_the_model(name):
    fig = P.conditions(name)
    print(name, fig)
    m = P.model(name)
    P.image_invariants(m.image(), m.n_edges)


@pytest.mark.parametrize("name", list(P.CASES))
def test_model_equals_oracle(name):
    case = P.CASES[name]
    cuts = {len(case.text)} | {P.midway(name, c) for c in case.chunkings} - {None}
    for upto in sorted(cuts):
        upto = None if upto == len(case.text) else upto
        assert P.same_export(P.model(name, upto).export(), P.oracle_export(P.oracle(name, upto))), upto
    # the chunking changes nothing
    want = P.model(name)
    for c, chunks in case.chunkings.items():
        if c != "per_token":
            m = P.build(case, chunks=chunks)
            assert P.same_export(m.export(), want.export()) and P.same_image(m.image(), want.image()), c
    if name in P.CLUSTERS:
        ora = P.oracle(name)
        q = P.lookups(name)
        assert P.lookup_results(want, q) == [ora.transfer_state(s, l, t) for s, l, t in q]
        deep = P.deep_keys(name)
        assert q[:len(deep)] == [(s, want.length[s], t) for s, t, _, _ in deep]
        assert P.lookup_results(want, q[:len(deep)]) == [(d, want.length[s] + 1) for s, _, d, _ in deep]
        n_abs = len(P.absent_probes(name))
        assert P.lookup_results(want, q[len(deep):len(deep) + n_abs]) == [(0, 0)] * n_abs


def _outputs(name, faults):
    """what the GPU file compares, from a (faulty) model; None when the model ran away"""
    try:
        m = P.build(P.CASES[name], faults)
        out = dict(image=m.image(), export=m.export())
        if name in P.CLUSTERS:
            out["lookups"] = P.lookup_results(m, P.lookups(name))
        if name.startswith("long_climb"):
            s = P.model(name)
            out["lookups"] = [m.transfer_state(s.last, s.length[s.last], P.C_)]
        return out
    except (P.Runaway, IndexError, KeyError):
        return None


def test_every_fault_is_caught_and_every_case_catches_one():
    caught = {}
    for name in P.CASES:
        want = _outputs(name, ())
        assert want is not None
        for f in P.FAULTS:
            got = _outputs(name, (f,))
            caught[name, f] = (got is None or not P.same_image(got["image"], want["image"]) or not P.same_export(got["export"], want["export"])
                               or got.get("lookups") != want.get("lookups"))
    w = max(len(n) for n in P.CASES)
    print("\n" + " " * w + "  " + " ".join("%d" % i for i in range(len(P.FAULTS))))
    for name in P.CASES:
        print(name.ljust(w) + "  " + " ".join("x" if caught[name, f] else "." for f in P.FAULTS))
    for i, f in enumerate(P.FAULTS):
        print("%d = %s: %s" % (i, f, ", ".join(n for n in P.CASES if caught[n, f])))
    for f in P.FAULTS:
        assert any(caught[n, f] for n in P.CASES), f
    for n in P.CASES:
        assert any(caught[n, f] for f in P.FAULTS), n
    # the probe faults are the clusters' to catch, the deepcopy faults the hub's
    for f in P.FAULTS[:4]:
        assert all(caught[n, f] for n in P.CLUSTERS), f
    assert caught["hub_clone", "clone_first_64_edges"] and caught["hub_clone", "clone_reversed_order"]
    assert caught["thue_morse", "repoint_one_hop"]


def test_invariants_see_what_the_chain_walk_cannot():
    """a duplicated key, an orphaned slot and a stale key leave Session.export() unchanged; the image check fails on each"""
    m = P.model("cluster128")
    img = m.image()
    free = int(np.flatnonzero(img["key"] == np.uint64(P.EMPTY))[0])
    occ = int(np.flatnonzero(img["key"] != np.uint64(P.EMPTY))[0])
    for key in (img["key"][occ], np.uint64(P.dyn_key(999, 5))):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in img.items()}
        bad["key"][free] = key
        assert not P.same_image(bad, img)
        with pytest.raises(AssertionError):
            P.image_invariants(bad, m.n_edges)
