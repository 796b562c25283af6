"""The dynamic suffix automaton on planted inputs (tests/dyn_planting.py): hash clusters that wrap the table end and are probed
in rounds 1 to 4, the strings with the most states / edges at exactly max_tokens tokens, a clone of a 71-edge state, climbs of n
suffix links -- fed per token, in launches of 63 / 64 / 65 / 1, whole, and with a device-side count.

Two equalities after every case: Session.export() == the oracle's export, and Session.export_table() == the table image of the model
(key of every slot, dst / next of every occupied slot, head / tail of every state), plus the image's own invariants.  The second ties
the planting to the real layout: if the hash, the sizing rule or the probe order changes, it fails at "device table != model" instead
of silently planting nothing.  tests/test_dyn_planting_cpu.py shows on the CPU which named fault each case catches.

Everything is integer work; every comparison is an equality.  Measured on an MI355X: 59 tests in 3.6 s, the slowest (drafts from
all 254 states of edges_max128) 0.5 s."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import Params
from oracle import sam_oracle as O
import dyn_planting as P

E_CAPACITY = -2


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64), dtype=torch.int32).cuda()


def check_structure(sess, ref, ora):
    """the two equalities + the invariants of the image"""
    got, want = sess.export(), P.oracle_export(ora)
    assert got["error"] == 0
    for k in P.EXPORT_KEYS:                                                      # edges in dict order
        assert np.array_equal(got[k], want[k]), k
    assert (got["cur_index"], got["cur_length"]) == want["cursor"]
    assert (got["last"], got["max_length"]) == (want["last"], want["max_length"])
    img, model = sess.export_table(), ref.image()
    assert (img["H"], img["n_states"]) == (model["H"], model["n_states"])
    diff = np.flatnonzero(img["key"] != model["key"])
    assert diff.size == 0, "device table != model: first at slot %d of %d slots" % (diff[0], diff.size)
    occ = model["key"] != np.uint64(P.EMPTY)
    for k in ("dst", "next"):
        assert np.array_equal(img[k][occ], model[k][occ]), "device table != model: " + k
    for k in ("head", "tail"):
        assert np.array_equal(img[k], model[k]), "device table != model: " + k
    assert got["n_edges"] == ref.n_edges
    P.image_invariants(img, got["n_edges"])


def feed(sess, name, chunks, midway=None):
    """the case's text in the launches of `chunks`; the structure is checked once more where `midway` tokens are in"""
    text, fed = P.CASES[name].text, 0
    for a, b, dn in chunks:
        if dn is None:
            sess.add_tokens(dev(text[a:b]))
        else:
            sess.add_tokens(dev(text[a:b]), n=b - a, d_n=dev([dn]))
        fed += (b - a) if dn is None else dn
        if fed == midway:
            check_structure(sess, P.model(name, midway), P.oracle(name, midway))
    assert fed == len(text)


CASE_CHUNKINGS = [(n, c) for n in P.CASES for c in P.CASES[n].chunkings]


@pytest.mark.parametrize("name,chunking", CASE_CHUNKINGS, ids=["%s-%s" % nc for nc in CASE_CHUNKINGS])
def test_structure(name, chunking):
    P.conditions(name)
    case = P.CASES[name]
    sess = samd_hip.Session(case.max_tokens)
    mid = P.midway(name, chunking) if name in P.CLUSTERS else None
    assert name not in P.CLUSTERS or chunking == "whole" or mid is not None
    feed(sess, name, case.chunkings[chunking], mid)
    check_structure(sess, P.model(name), P.oracle(name))


def walk_all(sess, queries):
    """one lookup (commit=False) per (state, length, token); one tensor, one synchronisation"""
    out = torch.full((len(queries), 2), -9, dtype=torch.int32, device="cuda")
    toks = dev([t for _, _, t in queries])
    for i, (s, l, _) in enumerate(queries):
        sess.set_cursors(s, l, 0, 0)
        sess.dyn_walk(toks[i:i + 1], 1, commit=False, d_out=out[i])
    return [tuple(r) for r in out.cpu().tolist()]


@pytest.mark.parametrize("name", P.CLUSTERS)
def test_cluster_lookups(name):
    case, ref, ora = P.CASES[name], P.model(name), P.oracle(name)
    sess = samd_hip.Session(case.max_tokens)
    feed(sess, name, case.chunkings["whole"])
    deep, absent, q = P.deep_keys(name), P.absent_probes(name), P.lookups(name)
    assert len(deep) >= 40 and len(absent) >= 64
    want = [(d, ref.length[s] + 1) for s, _, d, _ in deep] + [(0, 0)] * len(absent)
    want += [ora.transfer_state(s, l, t) for s, l, t in q[len(want):]]
    assert len(want) == len(q)
    got = walk_all(sess, q)
    bad = [(i, q[i], got[i], want[i]) for i in range(len(q)) if got[i] != want[i]]
    assert not bad, bad[:5]
    # lookups write nothing
    sess.set_cursors(*ora.cursor(), 0, 0)
    check_structure(sess, ref, ora)


def cursor(sess):
    e = sess.export(with_edges=False)
    return e["cur_index"], e["cur_length"]


def test_long_climb():
    n = 128
    sess = samd_hip.Session(n)
    out = torch.full((2,), -9, dtype=torch.int32, device="cuda")
    # a^n: a cursor of length n meets a token that is absent everywhere -> n link hops to (0, 0)
    feed(sess, "long_climb", P.CASES["long_climb"].chunkings["whole"])
    check_structure(sess, P.model("long_climb"), P.oracle("long_climb"))
    for commit in (False, True):
        sess.set_cursors(n, n, 0, 0)
        sess.dyn_walk(dev([P.C_]), 1, commit=commit, d_out=out)
        assert out.cpu().tolist() == [0, 0]
        assert cursor(sess) == ((0, 0) if commit else (n, n))
    # b a^(n-1): b is present at the root only -> the climb from the deepest state ends in the root's edge
    sess.reset()
    feed(sess, "long_climb_root", P.CASES["long_climb_root"].chunkings["whole"])
    ref = P.model("long_climb_root")
    check_structure(sess, ref, P.oracle("long_climb_root"))
    assert P.oracle("long_climb_root").transfer_state(ref.last, n, P.C_) == (1, 1)
    for commit in (False, True):
        sess.set_cursors(ref.last, n, 0, 0)
        sess.dyn_walk(dev([P.C_]), 1, commit=commit, d_out=out)
        assert out.cpu().tolist() == [1, 1]
        assert cursor(sess) == ((1, 1) if commit else (ref.last, n))


def test_reset_leaves_no_stale_key():
    sess = samd_hip.Session(128)
    feed(sess, "cluster128", P.CASES["cluster128"].chunkings["whole"])
    sess.reset()
    img = sess.export_table()
    assert img["n_states"] == 1 and (img["key"] == np.uint64(P.EMPTY)).all() and img["head"].tolist() == [-1] and img["tail"].tolist() == [-1]
    feed(sess, "thue_morse128", P.CASES["thue_morse128"].chunkings["63_64_65_1"])
    check_structure(sess, P.model("thue_morse128"), P.oracle("thue_morse128"))         # the model of a FRESH session


def test_commit_path():
    """the tail of cluster128 enters through accept + commit: sequence drafts of at most 64 tokens, all accepted"""
    name, first = "cluster128", 60
    text = P.CASES[name].text
    sess = samd_hip.Session(128)
    sess.add_tokens(dev(text[:first]))
    pos = first
    for k in (64, len(text) - first - 64):
        toks = list(text[pos:pos + k])
        sess.set_draft(dev(toks), dev([i - 1 for i in range(k)]), k, type_=0)
        sess.accept(dev(toks[1:] + [0]))                 # node i's arg-max is node i + 1's token: everything is accepted
        sess.commit(None)
        v = sess.read_verdict()
        assert v.accept == k and list(v.tokens[:k]) == toks
        pos += k
    assert pos == len(text)
    check_structure(sess, P.model(name), P.oracle(name))


# ---------------------------------------------------------------------------------------------------------------------------------
# drafts from every state
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seq_buffers(n):
    """gen_buffers of the chain 0 <- 1 <- ... <- n-1: position, mask words (low, high), the one retrieve row"""
    b = O.gen_buffers([i - 1 for i in range(n)])
    m = b["tree_attn_mask"][0, 0].astype(np.uint64)
    lo = (m[:, :64] << np.arange(min(n, 64), dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    hi = (m[:, 64:] << np.arange(max(n - 64, 0), dtype=np.uint64)).sum(axis=1, dtype=np.uint64) if n > 64 else np.zeros(n, np.uint64)
    return b["tree_position_ids"][0].astype(np.int32), lo, hi, b["tree_retrieve_indices"].astype(np.int32)


def check_draft(d, tokens, what):
    n = len(tokens)
    pos, lo, hi, ret = seq_buffers(n)
    arr = lambda x: np.ctypeslib.as_array(x)
    assert (d.type, d.n, d.n_leaves, d.max_depth) == (0, n, ret.shape[0], ret.shape[1]), what
    assert arr(d.tokens)[:n].tolist() == list(tokens), what
    assert np.array_equal(arr(d.parent)[:n], np.arange(n) - 1), what
    assert np.array_equal(arr(d.position)[:n], pos), what
    assert np.array_equal(arr(d.mask)[:n], lo) and np.array_equal(arr(d.mask_hi)[:n], hi), what
    assert not arr(d.mask)[n:].any() and not arr(d.mask_hi)[n:].any(), what                 # padded rows attend nothing
    assert np.array_equal(arr(d.retrieve)[:ret.size].reshape(ret.shape), ret), what


def matches(max_predicts, alpha):
    """match lengths on both sides of the max_predicts clamp of n = min(max_predicts, 1 + int(match * alpha)), and one so long that
    end + n passes the end of any text here"""
    at = next(m for m in range(1000) if 1 + int(m * alpha) >= max_predicts)
    return (max(at - 1, 0), at, at + 3, 100000)


@pytest.mark.parametrize("name", ["edges_max128", "thue_morse128", "hub_clone"])
def test_drafts_from_every_state(name):
    case, ref, ora = P.CASES[name], P.model(name), P.oracle(name)
    sess = samd_hip.Session(case.max_tokens)
    feed(sess, name, case.chunkings["whole"])
    L, n_text = O.lib(), len(case.text) + 1
    buf = np.empty(130, np.int32)
    bufp = buf.ctypes.data_as(O.i32p)
    past_end = 0
    for s in range(ref.n_states):
        start = 77 + s
        # DynSAM.gen_draft: every max_predicts at every state; alpha and the match length rotate with the state
        for j, mp in enumerate((1, 40, 64, 65, 128)):
            alpha = (0.7, 4.0)[(s + j) & 1]
            ms = matches(mp, alpha)
            match = ms[(s // 2 + j) % len(ms)]
            m = L.osam_gen_draft_seq(ora._h, s, match, start, mp, float(alpha), bufp)
            past_end += ref.minend[s] + min(mp, 1 + int(match * alpha)) > n_text
            sess.draft_seq(Params(variant=0, max_predicts=mp, alpha=alpha, K=8, len_bias=0), s, match, start)
            check_draft(sess.read_draft(), buf[:m].tolist(), (name, "seq", s, mp, alpha, match))
        # the full variant's gen_draft: to_anc climb, fixed length, zero padded
        for npred in (1, 40, 65, 128):
            L.osam_gen_draft_fixed(ora._h, s, start, npred, 1, bufp)
            sess.draft_fixed(None, Params(variant=1, max_predicts=64, alpha=4.0, K=8, len_bias=5, n_predicts=npred, len_threshold=5), 0, s, start)
            check_draft(sess.read_draft(), buf[:npred].tolist(), (name, "fixed", s, npred))
    assert past_end >= ref.n_states                      # drafts cut by the end of the text are not rare here
    check_structure(sess, ref, ora)                      # drafting writes nothing into the automaton


def test_capacity_then_reset():
    name = "states_max128"
    case = P.CASES[name]
    sess = samd_hip.Session(case.max_tokens)
    feed(sess, name, case.chunkings["whole"])            # exactly max_tokens tokens fit ...
    check_structure(sess, P.model(name), P.oracle(name))
    sess.add_tokens(dev([P.B] * 3))                      # ... max_tokens + 3 do not
    assert sess.export(with_edges=False)["error"] == E_CAPACITY
    over = P.build(case)                                 # reported, not corrupted: the model refuses the same launch and keeps its table
    over.add_tokens([P.B] * 3)
    assert over.error == E_CAPACITY and P.same_image(sess.export_table(), over.image())
    sess.reset()
    feed(sess, name, case.chunkings["63_64_65_1"])
    check_structure(sess, P.model(name), P.oracle(name))
