"""Planted inputs for the dynamic suffix automaton (csrc/sam_device.h dyn_find / dyn_insert / dyn_transfer / dyn_add_state /
dyn_add_tokens): a model of its hash table, the reference automaton on top of that model, and named faults (numpy + the oracle only;
no product import).  Everything is integer work and every comparison an equality.

  layout       restated from the kernel: key = state << 32 | tok, dyn_hash(key) = low 32 bits of (key * 0x9E3779B97F4A7C15) >> 29,
               H = table_size(max_tokens) = max(1024, pow2 >= 8 * max_tokens) slots, home = hash & (H - 1).  One probe ROUND looks at
               64 consecutive slots (wrapping with & (H - 1)); a hit anywhere in the round wins, else the first empty slot of the
               round ends the probe, else the next round starts 64 slots on; H / 64 rounds at the most.  Every state keeps its edges
               in dict (insertion) order as a chain head -> hnext -> ... -> tail of slots.
  DynTable     that table: find / insert with the probe above, and for every key the round in which it was placed.
  RefDynSAM    the reference's add_state / transfer_state / add_tokens (samd_sam_only/sam/dyn_sam.py) in plain Python with
               next[state][tok] = DynTable.find, the capacity rules of the kernel included.  It yields the table IMAGE slot by slot
               (what Session.export_table() must equal) and the export of tests/test_gpu_sam.py's check_dyn.  It is a model of the
               layout, not a second oracle: tests/test_dyn_planting_cpu.py holds it against oracle.sam_oracle.DynSAM on every case.
  clusters     cluster_tokens(max_tokens, n, window): n distinct token ids (candidates 0, 2^31 - 1, then 1 .. 152063 ascending; never
               negative) whose ROOT edge (0, tok) has its home in the last `window` slots of the table.  A text of all-distinct cluster
               tokens piles the root's edges into one run of occupied slots that wraps past slot H - 1: keys are placed and found in
               rounds 1, 2, ..., which a random stream never does at a load of 3/8.  The tail of repeats is searched so that clones
               copy and re-point such keys.
  cases        CASES: name -> Case(max_tokens, text, chunkings); `conditions(case)` asserts on the model what the case is for.
  faults       FAULTS: each a flag of DynTable / RefDynSAM.  A faulty model always terminates: its loops are capped and running into
               the cap raises Runaway, which counts as a changed output.  Nothing here is ever built into a kernel."""
import functools

import numpy as np

from oracle import sam_oracle as O

WAVE = 64
MASK64 = (1 << 64) - 1
EMPTY = MASK64                     # SAMD_HEMPTY
E_CAPACITY = -2                    # SAMD_E_CAPACITY
VOCAB = 152064                     # cluster candidates stay below a real vocabulary's size
TOK_MAX = 2 ** 31 - 1

FAULTS = ("first_round_only", "no_wrap", "slot_skipped_between_rounds", "hit_from_round0_base", "clone_first_64_edges",
          "clone_reversed_order", "repoint_one_hop", "clone_minend_of_cur", "text_first_64_only")
STALE_TEXT = -7                    # what text_first_64_only leaves where it stored nothing (no token is negative)


class Runaway(Exception):
    """a faulty model ran into a loop cap (on the device: a hang)"""


def dyn_key(state, tok):
    return ((state & 0xFFFFFFFF) << 32) | (tok & 0xFFFFFFFF)


def dyn_hash(key):
    return (((key * 0x9E3779B97F4A7C15) & MASK64) >> 29) & 0xFFFFFFFF


def table_size(max_tokens):
    H = 1024
    while H < max_tokens * 8:
        H <<= 1
    return H


def home(state, tok, H):
    return dyn_hash(dyn_key(state, tok)) & (H - 1)


class DynTable:
    """the open-addressed transition table with the kernel's probe.  find -> (slot | -1, first empty slot | -1, round)."""

    def __init__(self, H, faults=()):
        self.H, self.faults = H, frozenset(faults)
        self.key = [EMPTY] * H
        self.dst = [0] * H
        self.nxt = [0] * H
        self.head, self.tail = {}, {}
        self.placed_round = {}                     # key -> round of the probe that found its slot free

    def find(self, state, tok):
        f, mask, key = self.faults, self.H - 1, dyn_key(state, tok)
        h0 = h = dyn_hash(key) & mask
        rounds = 1 if "first_round_only" in f else self.H // WAVE
        for r in range(rounds):
            hit = empty = -1
            for bit in range(WAVE):
                raw = h + bit
                k = EMPTY if ("no_wrap" in f and raw > mask) else self.key[raw & mask]
                if k == key and hit < 0:
                    hit = bit
                if k == EMPTY and empty < 0:
                    empty = bit
            if hit >= 0:
                return ((h0 if "hit_from_round0_base" in f else h) + hit) & mask, -1, r
            if empty >= 0:
                return -1, (h + empty) & mask, r
            h = (h + (65 if "slot_skipped_between_rounds" in f else WAVE)) & mask
        return -1, -1, rounds

    def insert(self, slot, state, tok, dst, rnd):
        key = dyn_key(state, tok)
        self.key[slot], self.dst[slot], self.nxt[slot] = key, dst, -1
        t = self.tail.get(state, -1)
        if t < 0:
            self.head[state] = slot
        else:
            self.nxt[t] = slot
        self.tail[state] = slot
        self.placed_round.setdefault(key, rnd)

    def chain(self, state):
        """the slots of a state's dict order; capped (a faulty table can close a cycle)"""
        out, e = [], self.head.get(state, -1)
        while e >= 0:
            out.append(e)
            if len(out) > self.H:
                raise Runaway("edge chain of state %d" % state)
            e = self.nxt[e]
        return out

    def longest_run(self):
        """(start, length) of the longest run of occupied slots, wrapping past slot H - 1"""
        H, occ = self.H, [k != EMPTY for k in self.key]
        if all(occ):
            return 0, H
        z = occ.index(False)
        best, s, n = (0, 0), None, 0
        for i in range(1, H + 1):
            j = (z + i) % H
            if occ[j]:
                if n == 0:
                    s = j
                n += 1
                if n > best[1]:
                    best = (s, n)
            else:
                n = 0
        return best


class RefDynSAM:
    """DynSAM (dyn_sam.py:37-114) on a DynTable, with the kernel's capacity rules (samd_session_create, dyn_add_state)."""

    def __init__(self, max_tokens, faults=()):
        self.max_tokens, self.faults = max_tokens, frozenset(faults)
        self.cap_states, self.cap_text = 2 * max_tokens + 2, max_tokens + 2
        self.reset()

    def reset(self):
        self.table = DynTable(table_size(self.max_tokens), self.faults)
        self.link, self.length, self.minend = [-1], [0], [0]
        self.n_edges, self.last, self.max_length, self.error = 0, 0, 0, 0
        self.cur = (0, 0)
        self.text = [-1]
        self.clones = []                 # (cloned state, its degree) per clone
        self.insert_chain = []           # per token: the number of states it was inserted on
        self.cloned_keys, self.repointed_keys, self.repoint_hops = [], [], []
        self.hops = 0                    # suffix links climbed by the last transfer_state
        self._budget = 0

    def _tick(self):
        self._budget += 1
        if self._budget > 64 * (self.cap_states + self.table.H):
            raise Runaway("loop cap")

    @property
    def n_states(self):
        return len(self.link)

    def _full(self):
        return (self.n_edges + 8) * 2 > self.table.H - 1

    def _new_state(self, link, length, minend):
        self.link.append(link); self.length.append(length); self.minend.append(minend)
        return len(self.link) - 1

    def transfer_state(self, index, length, tok):
        T, hopped, self.hops = self.table, False, 0
        while True:
            self._tick()
            if hopped:
                length = self.length[index]
            e, _, _ = T.find(index, tok)
            if e >= 0 or index == 0:
                break
            index, hopped = self.link[index], True
            self.hops += 1
        return (T.dst[e], length + 1) if e >= 0 else (0, 0)

    def add_state(self, tok):
        T, f = self.table, self.faults
        if self.n_states + 2 > self.cap_states or self._full():
            self.error = E_CAPACITY
            return
        self.max_length += 1
        cur = self._new_state(-1, self.max_length, self.max_length)
        p, e, chain = self.last, -1, 0
        while p != -1:
            self._tick()
            e, fs, r = T.find(p, tok)
            if e >= 0:
                break
            if fs < 0 or self._full():
                self.error = E_CAPACITY
                return
            T.insert(fs, p, tok, cur, r); self.n_edges += 1; chain += 1
            p = self.link[p]
        self.insert_chain.append(chain)
        if p == -1:
            self.link[cur] = 0
        else:
            q = T.dst[e]
            if self.length[p] + 1 == self.length[q]:
                self.link[cur] = q
            else:
                clone = self._new_state(self.link[q], self.length[p] + 1, self.minend[cur if "clone_minend_of_cur" in f else q])
                edges = T.chain(q)
                self.clones.append((q, len(edges)))
                if "clone_first_64_edges" in f:
                    edges = edges[:WAVE]
                if "clone_reversed_order" in f:
                    edges = edges[::-1]
                for qe in edges:
                    self._tick()
                    t, d = T.key[qe] & 0xFFFFFFFF, T.dst[qe]
                    _, fs, r = T.find(clone, t)
                    if self._full() or fs < 0:
                        self.error = E_CAPACITY
                        return
                    T.insert(fs, clone, t, d, r); self.n_edges += 1
                    self.cloned_keys.append(dyn_key(clone, t))
                hops = 0
                while p != -1:
                    self._tick()
                    pe, _, _ = T.find(p, tok)
                    if pe < 0 or T.dst[pe] != q:
                        break
                    T.dst[pe] = clone
                    self.repointed_keys.append(dyn_key(p, tok))
                    hops += 1
                    if "repoint_one_hop" in f:
                        break
                    p = self.link[p]
                self.repoint_hops.append(hops)
                self.link[q] = clone; self.link[cur] = clone
        self.last = cur

    def add_tokens(self, toks):
        toks = [int(t) for t in toks]
        n = len(toks)
        if len(self.text) + n > self.cap_text:
            self.error, n = E_CAPACITY, 0
        for t in toks[:n]:
            if self.error:
                break
            self.cur = self.transfer_state(self.cur[0], self.cur[1], t)
            self.add_state(t)
        if self.error == 0:
            keep = WAVE if "text_first_64_only" in self.faults else n
            self.text += toks[:keep] + [STALE_TEXT] * (n - min(keep, n))

    # ---- what is compared ----
    def export(self):
        T, ns = self.table, self.n_states
        deg, et, ed = [], [], []
        for s in range(ns):
            ch = T.chain(s)
            deg.append(len(ch)); et += [T.key[e] & 0xFFFFFFFF for e in ch]; ed += [T.dst[e] for e in ch]
        i32 = lambda a: np.asarray(a, dtype=np.int64).astype(np.int32)
        return dict(link=i32(self.link), length=i32(self.length), aux=i32(self.minend), deg=i32(deg), edge_tok=i32(et),
                    edge_dst=i32(ed), text=i32(self.text), cursor=tuple(self.cur), last=self.last, max_length=self.max_length,
                    error=self.error)

    def image(self):
        T, ns = self.table, self.n_states
        return dict(H=T.H, n_states=ns, key=np.asarray(T.key, dtype=np.uint64), dst=np.asarray(T.dst, dtype=np.int32),
                    next=np.asarray(T.nxt, dtype=np.int32), head=np.asarray([T.head.get(s, -1) for s in range(ns)], dtype=np.int32),
                    tail=np.asarray([T.tail.get(s, -1) for s in range(ns)], dtype=np.int32))


def oracle_export(ora):
    out = ora.export()
    out.update(cursor=ora.cursor(), last=ora.last, max_length=ora.max_length, error=0)
    return out


EXPORT_KEYS = ("link", "length", "aux", "deg", "edge_tok", "edge_dst", "text")


def same_export(a, b):
    return all(np.array_equal(a[k], b[k]) for k in EXPORT_KEYS) and all(a[k] == b[k] for k in ("cursor", "last", "max_length", "error"))


def same_image(a, b):
    """key of every slot, dst / next of every occupied slot, head / tail of every state"""
    if a["H"] != b["H"] or a["n_states"] != b["n_states"] or not np.array_equal(a["key"], b["key"]):
        return False
    occ = a["key"] != np.uint64(EMPTY)
    return (np.array_equal(a["dst"][occ], b["dst"][occ]) and np.array_equal(a["next"][occ], b["next"][occ])
            and np.array_equal(a["head"], b["head"]) and np.array_equal(a["tail"], b["tail"]))


def image_invariants(img, n_edges):
    """from the image alone: every occupied slot lies on exactly one chain, no key occurs twice, the occupied count is n_edges,
    every chain ends in its state's tail and holds that state's keys only"""
    key, nxt, H = img["key"], img["next"], img["H"]
    occ = np.flatnonzero(key != np.uint64(EMPTY))
    assert len(occ) == n_edges, (len(occ), n_edges)
    assert len(np.unique(key[occ])) == len(occ), "a key occurs twice"
    seen = np.zeros(H, dtype=np.int32)
    for s in range(img["n_states"]):
        e, last, steps = int(img["head"][s]), -1, 0
        while e >= 0:
            assert 0 <= e < H and key[e] != np.uint64(EMPTY) and int(key[e]) >> 32 == s, (s, e)
            seen[e] += 1
            last, e, steps = e, int(nxt[e]), steps + 1
            assert steps <= H, "a chain does not end"
        assert int(img["tail"][s]) == last, s
    assert np.array_equal(np.flatnonzero(seen == 1), occ) and seen.max(initial=0) <= 1, "orphaned or shared slot"


# ---------------------------------------------------------------------------------------------------------------------------------
# clusters
# ---------------------------------------------------------------------------------------------------------------------------------
def candidates():
    yield 0
    yield TOK_MAX
    yield from range(1, VOCAB)


@functools.lru_cache(maxsize=None)
def cluster_tokens(max_tokens, n, window):
    H = table_size(max_tokens)
    out = []
    for t in candidates():
        if home(0, t, H) >= H - window:
            out.append(t)
            if len(out) == n:
                return tuple(out)
    raise AssertionError("not enough cluster tokens")


@functools.lru_cache(maxsize=None)
def cluster_text(max_tokens, window=24):
    """all-distinct cluster tokens (max_tokens - 8), then 8 repeats: each repeat t_k that does not continue the previous one clones the
    state of t_0 .. t_k's one-token suffix (copying its edge on t_k+1) and re-points the root's edge on t_k.  The repeats are chosen,
    on the model, among the tokens whose root edge was placed in round >= 1, preferring those whose cloned edge probes into round >= 1."""
    base = list(cluster_tokens(max_tokens, max_tokens - 8, window))
    m = RefDynSAM(max_tokens)
    m.add_tokens(base)
    deep = [k for k in range(len(base) - 1) if m.table.placed_round[dyn_key(0, base[k])] >= 1]
    assert len(deep) >= 8
    text, prev, used = list(base), len(base) - 1, set()
    for _ in range(8):
        clone = m.n_states + 1                                 # add_state takes cur first, then the clone
        ok = [k for k in deep if k != prev + 1 and k not in used]
        good = [k for k in ok if m.table.find(clone, base[k + 1])[2] >= 1]
        k = (good or ok)[0]
        used.add(k); prev = k
        text.append(base[k]); m.add_tokens([base[k]])
    return tuple(text)


@functools.lru_cache(maxsize=None)
def absent_probes(name, count=64):
    """tokens NOT in the text whose root key has its home in the first 8 slots of the longest run and whose probe finds its empty
    slot in round >= 2 -> [(tok, round)]"""
    m = model(name)
    T, H = m.table, m.table.H
    start, _ = T.longest_run()
    text, out = set(CASES[name].text), []
    for t in candidates():
        if t in text or (home(0, t, H) - start) % H >= 8:
            continue
        e, fs, r = T.find(0, t)
        assert e < 0 and fs >= 0
        if r >= 2:
            out.append((t, r))
            if len(out) == count:
                break
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
A, B, C_ = 0, TOK_MAX, 151643          # the extremal strings use the smallest and the largest token id the header defines


def thue_morse(n):
    return [(A, B)[bin(i).count("1") & 1] for i in range(n)]


def fibonacci(n):
    a, b = [A], [A, B]
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def hub_text():
    z, x, w = 5, 6, 7
    t = [z, x]
    for i in range(70):
        t += [1000 + i, z, x]
    return t + [w, x]


def chunkings(n, per_token=False):
    """name -> list of (tokens handed to the launch, device-side count or None) as slices of the text"""
    out = {"whole": [(0, n, None)]}
    cuts, pos, sizes = [], 0, (63, 64, 65, 1)
    while pos < n:
        k = min(sizes[len(cuts) % 4], n - pos)
        cuts.append((pos, pos + k, None)); pos += k
    out["63_64_65_1"] = cuts
    cut = max(1, (2 * n) // 3)
    out["d_n"] = [(0, n, cut), (cut, n, n - cut)]              # the launch is handed more tokens than the device-side count takes
    if per_token:
        out["per_token"] = [(i, i + 1, None) for i in range(n)]
    return out


class Case:
    def __init__(self, max_tokens, text, per_token=False):
        self.max_tokens, self.text = max_tokens, tuple(int(t) for t in text)
        self.chunkings = chunkings(len(self.text), per_token)


def _cases():
    c = {}
    for mt in (128, 256):
        c["cluster%d" % mt] = Case(mt, cluster_text(mt), per_token=(mt == 128))
    for n in (128, 129, 520):
        c["states_max%d" % n] = Case(n, [A] + [B] * (n - 1), per_token=(n == 128))
        c["edges_max%d" % n] = Case(n, [A] + [B] * (n - 2) + [C_], per_token=(n == 128))
    c["run_then_run"] = Case(128, [A] * 64 + [B] * 64, per_token=True)
    c["thue_morse"] = Case(520, thue_morse(520))
    c["thue_morse128"] = Case(128, thue_morse(128))            # what follows the reset of a cluster session; a draft case
    c["fibonacci"] = Case(520, fibonacci(520))
    c["hub_clone"] = Case(214, hub_text())
    c["long_climb"] = Case(128, [B] * 128, per_token=True)
    # no token is present at the root only in a^n: the second walk of long_climb runs on b a^(n-1) after a reset
    c["long_climb_root"] = Case(128, [C_] + [B] * 127)
    return c


CASES = _cases()
CLUSTERS = ("cluster128", "cluster256")


def build(case, faults=(), chunks=None, upto=None):
    """the model after the case's text (or its first `upto` tokens), fed in the chunks given (default: one launch)"""
    m = RefDynSAM(case.max_tokens, faults)
    text = list(case.text if upto is None else case.text[:upto])
    for a, b, dn in (chunks or [(0, len(text), None)]):
        m.add_tokens(text[a:b] if dn is None else text[a:a + dn])
    return m


@functools.lru_cache(maxsize=None)
def model(name, upto=None):
    return build(CASES[name], upto=upto)


@functools.lru_cache(maxsize=None)
def oracle(name, upto=None):
    """the oracle's automaton after the case's text (or its first `upto` tokens): built once, shared, never fed again"""
    ora = O.DynSAM()
    ora.add_tokens(list(CASES[name].text[:upto]))
    return ora


def midway(name, chunking):
    """number of tokens after the first launch boundary at or past half of the text (None: the chunking has none inside the text)"""
    n, pos = len(CASES[name].text), 0
    for a, b, dn in CASES[name].chunkings[chunking]:
        pos += (b - a) if dn is None else dn
        if 2 * pos >= n and pos < n:
            return pos
    return None


def deep_keys(name):
    """[(state, tok, dst, round)] of every key placed in round >= 1"""
    m = model(name)
    T = m.table
    return [(k >> 32, k & 0xFFFFFFFF, T.dst[T.find(k >> 32, k & 0xFFFFFFFF)[0]], r) for k, r in T.placed_round.items() if r >= 1]


def lookups(name):
    """[(state, length, tok)] asked of a cluster case: every deep key from its state, the planted absent keys from the root, and
    from the deepest state (last) every tenth text token and the absent ones"""
    m = model(name)
    q = [(s, m.length[s], t) for s, t, _, _ in deep_keys(name)]
    q += [(0, 0, t) for t, _ in absent_probes(name)]
    q += [(m.last, m.length[m.last], t) for t in CASES[name].text[::10]]
    q += [(m.last, m.length[m.last], t) for t, _ in absent_probes(name)[:8]]
    return q


def lookup_results(m, queries):
    return [m.transfer_state(s, l, t) for s, l, t in queries]


def conditions(name):
    """what the case is for, asserted on the model; -> a dict of the figures"""
    case, m = CASES[name], model(name)
    T, n = m.table, len(case.text)
    assert m.error == 0 and len(m.text) == n + 1 and n <= case.max_tokens
    fig = dict(n=n, states=m.n_states, edges=m.n_edges, clones=len(m.clones), insert_chain=max(m.insert_chain),
               clone_degree=max([d for _, d in m.clones], default=0), repoint_hops=max(m.repoint_hops, default=0))
    if name in CLUSTERS:
        start, run = T.longest_run()
        rounds = [r for r in T.placed_round.values()]
        fig.update(run=run, run_start=start, by_round=[rounds.count(r) for r in range(max(rounds) + 1)])
        assert run >= case.max_tokens, run
        assert (T.H - 1 - start) % T.H < run and (0 - start) % T.H < run, "the run does not wrap the table end"
        assert sum(1 for r in rounds if r >= 1) >= 40
        if name == "cluster256":
            assert sum(1 for r in rounds if r >= 3) >= 10
        assert len(set(case.text[:case.max_tokens - 8])) == case.max_tokens - 8
        assert len(m.clones) >= 3
        assert any(T.placed_round[k] >= 1 for k in m.cloned_keys), "no cloned edge in round >= 1"
        assert any(T.placed_round[k] >= 1 for k in m.repointed_keys), "no re-pointed edge in round >= 1"
        ab = absent_probes(name)
        assert len(ab) >= 64 and all(r >= 2 for _, r in ab)
        fig.update(absent=len(ab))
    elif name.startswith("states_max"):
        assert n == case.max_tokens and m.n_states == 2 * n - 1
    elif name.startswith("edges_max"):
        assert n == case.max_tokens and m.n_edges == 3 * n - 4 and m.insert_chain[-1] == n - 1
    elif name == "run_then_run":
        assert len(m.clones) == 63 and max(m.insert_chain) == 65
    elif name == "hub_clone":
        assert len(m.clones) == 1 and m.clones[0][1] >= 65
    elif name == "long_climb":
        absent = C_
        assert n == case.max_tokens and m.n_states == n + 1 and m.length[n] == n
        assert m.transfer_state(n, n, absent) == (0, 0) and m.hops == n
    elif name == "long_climb_root":
        assert n == case.max_tokens and m.length[m.last] == n
        assert [s for s in range(m.n_states) if T.find(s, C_)[0] >= 0] == [0]           # present at the root only
        assert m.transfer_state(m.last, n, C_) == (1, 1) and m.hops >= n - 2
    return fig
