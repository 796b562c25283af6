"""The static automaton's derived walk tables on planted corpora (tests/static_planting.py; tests/test_static_planting_cpu.py shows on the
CPU that every plant exists, that the model's lookup is the oracle's transfer_state, and which named fault each case catches).

For every corpus, in the three handle states (edge blocks + hot words + bigram table; SAMD_EDGE_BLOCKS=0: the edge table; both switched off: the
nodes and their spill blocks) and at 2 / 4 / 64 slots per entry:
  * export_tables() equals the model -- chain words, root entries, child bitmap, hot words and edge blocks slot for slot; the bigram and edge
    tables, whose slots racing threads claim, through check_open_table (every key once, inside the run that starts at its home, payload equal,
    nothing else, the displaced bit exactly where a key homed there lives elsewhere).  A changed hash, sizing rule or fill order fails HERE with
    "device table != model" instead of silently planting nothing;
  * every stream through walk (trace), lookup_batch (visited states), walk_streams and Session.static_walk gives the oracle's (index, length)
    after every token, its committed cursors and its visited-state count -- in one launch, and as a second launch from the cursors the first
    one committed (the probed state is then met by index);
  * all handle states and sizes agree bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
import static_planting as P
from test_gpu_sam import check_stream_major_walk, dev
from util import walk_visited

ENV = {"blocks": None, "edge": ("0", "1"), "plain": ("0", "0")}


def upload(c, mode, monkeypatch):
    if ENV[mode]:
        monkeypatch.setenv("SAMD_EDGE_BLOCKS", ENV[mode][0])
        monkeypatch.setenv("SAMD_EDGE_TABLE", ENV[mode][1])
    else:
        monkeypatch.delenv("SAMD_EDGE_BLOCKS", raising=False)
        monkeypatch.delenv("SAMD_EDGE_TABLE", raising=False)
    return samd_hip.StaticAutomaton.build(c.docs, P.EOS, 0).upload()


def same(got, want, what):
    assert got is not None, "device table != model: the handle has no " + what
    got, want = np.asarray(got), np.asarray(want, dtype=np.uint32)
    assert got.shape == want.shape, "device table != model: %s has %s slots, the model %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)) if got.size else []
    assert not len(bad), "device table != model: %s slot %d: %s, model %s" % (what, bad[0], [hex(int(v)) for v in np.atleast_1d(got[bad[0]])],
                                                                          [hex(int(v)) for v in np.atleast_1d(want[bad[0]])])


def check_tables(prod, c, mode, per):
    """-> per plant the longest run of occupied slots (start, length, wraps past the last slot) and the longest probe distance of a key, all
    read from the device's export"""
    T, info, dev_t = c.tables(mode, per), prod.derived_info(), prod.export_tables()
    assert prod.info()["vocab"] == c.vocab and prod.info()["n_states"] == c.img.n
    assert info["bigram_slots"] == T["bigram_slots"], "device table != model: bigram slots %d, model %d" % (info["bigram_slots"], T["bigram_slots"])
    for k in ("chain", "root16", "rc_bits"):
        same(dev_t[k], T[k], k)
    fig = dict(bigram_probe=P.check_open_table(dev_t["bigram"], T["bigram_rows"], T["bigram_homes"], T["bigram_dword"], "bigram table"),
               bigram_run=P.longest_run(dev_t["bigram"][:, 0] != P.U32))
    if mode == "blocks":
        assert info["edge_block_slots"] == len(T["blocks"]) and info["edge_table_slots"] == 0 and dev_t["edge_table"] is None
        same(dev_t["hot"], T["hot"], "hot words")
        same(dev_t["blocks"], T["blocks"], "edge blocks")
        hubs = c.notes.get("hubs") or ({"hub": c.notes["hub"]} if "hub" in c.notes else {"top%d" % L: i for L, (i, _) in c.notes.get("tops", {}).items()})
        fig.update({k: P.longest_run(P.block_of(dict(T, blocks=dev_t["blocks"]), s)[1]) for k, s in hubs.items()})
    else:
        assert info["edge_block_slots"] == 0 and dev_t["hot"] is None and dev_t["blocks"] is None
        if mode == "edge":
            assert info["edge_table_slots"] == T["edge_slots"]
            fig["edge_probe"] = P.check_open_table(dev_t["edge_table"], T["edge_rows"], T["edge_homes"], None, "edge table")
            fig["edge_run"] = P.longest_run(dev_t["edge_table"][:, 0] != P.U32)
        else:
            assert info["edge_table_slots"] == 0 and dev_t["edge_table"] is None
    return fig


def check_spill_image(prod, c):
    """the spill blocks of the image are the model's (the derivation kernels enumerate them; spill_search probes them)"""
    nodes, _, spill, _ = prod.host_image()
    nodes, spill = nodes.view(np.int32).reshape(-1, 16), spill.view(np.int32).reshape(-1, 2)
    for s, (head, tab) in c.img.spill.items():
        if s == 0:
            continue
        off = int(nodes[s, 14])
        assert spill[off:off + len(head) + len(tab)].tolist() == [list(e) for e in head + tab], "image != model: spill block of state %d" % s
    assert [int(nodes[s, 14]) for s in range(c.img.n) if s not in c.img.spill] == [-1] * (c.img.n - len(c.img.spill))


def walks(prod, name):
    """every launch of the case through walk / lookup_batch / walk_streams / Session.static_walk against the oracle -> the traces"""
    L, want, S = P.launches(name), P.expected(name), P.streams(name)
    export = P.case(name).oracle.export()
    out, carried = {}, None
    for k in ("one", "first", "second"):
        toks, start = L[k]
        if k == "second":
            start = carried
        T, B = toks.shape
        w_trace, w_cur, w_visited = want[k]
        d_toks, cur = dev(toks), dev(start)
        trace = torch.full((T, B, 2), -7, dtype=torch.int32, device="cuda")
        prod.walk(cur, d_toks, commit=True, trace=trace)
        got = trace.cpu().numpy()
        bad = np.argwhere((got != w_trace).any(axis=2))
        assert not len(bad), (k, S[bad[0][1]][0], S[bad[0][1]][1], "token", int(bad[0][0]), got[:, bad[0][1]].tolist(), w_trace[:, bad[0][1]].tolist())
        assert np.array_equal(cur.cpu().numpy(), w_cur), k
        res = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
        visited = torch.zeros(1, dtype=torch.int64, device="cuda")
        before = dev(start)
        prod.lookup_batch(before, d_toks, res, visited=visited)
        assert np.array_equal(res.cpu().numpy(), w_cur) and np.array_equal(before.cpu().numpy(), start), k
        assert int(visited.item()) == w_visited, (k, int(visited.item()), w_visited)
        if not start.any():
            assert w_visited == walk_visited(export, toks)
        check_stream_major_walk(prod, toks, w_trace, dev(w_cur), w_visited, start=dev(start) if start.any() else None)
        if k == "first":
            carried = w_cur.copy()
            for b, s in enumerate(S):
                if s[2] == 0:
                    carried[b] = s[3]
        sess = samd_hip.Session(64)                          # the product's own path: one cursor, single-wave st_transfer_tokens
        outs = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
        d_bt = dev(np.ascontiguousarray(toks.T))
        for b in range(B):
            sess.set_cursors(0, 0, int(start[b, 0]), int(start[b, 1]))
            sess.static_walk(prod, d_bt[b], T, commit=True, d_out=outs[b])
        assert np.array_equal(outs.cpu().numpy(), w_cur), ("session", k)
        out[k] = got
    return out


@pytest.mark.parametrize("name", P.CASES)
def test_planted_tables_and_walks(name, monkeypatch):
    c = P.case(name)
    P.conditions(name)
    first, figures = None, {}
    for mode in P.MODES:
        prod = upload(c, mode, monkeypatch)
        if mode == "blocks":
            check_spill_image(prod, c)
        for per in (4, 2, 64):
            prod.set_bigram_slots(0 if per == 4 else per)
            figures[mode, per] = check_tables(prod, c, mode, per)
            got = walks(prod, name)
            if first is None:
                first = got
            assert all(np.array_equal(got[k], first[k]) for k in first), (mode, per)
    for k, v in figures.items():
        print(name, "%s/%d" % k, v)


def test_export_tables_rejects_a_table_the_handle_lacks(monkeypatch):
    import ctypes as C
    c = P.case("edge_v32767")
    prod = upload(c, "plain", monkeypatch)
    buf = np.zeros((4, 4), np.uint32)
    args = [None] * 7
    for k in (3, 4, 5):                                      # edge table, hot words, edge blocks
        a = list(args); a[k] = buf.ctypes.data_as(C.c_void_p)
        assert samd_hip.lib().samd_static_export_tables(prod._h, *a) == samd_hip.lib().samd_static_export_tables(None, *args) != 0
    assert samd_hip.lib().samd_static_export_tables(prod._h, *args) == 0
    t = prod.export_tables()
    assert t["edge_table"] is None and t["hot"] is None and t["blocks"] is None and t["bigram"].shape == (1024, 4)
