"""Planted inputs for the STATIC automaton's derived walk tables (csrc/samd_common.h StaticDev; csrc/sam_kernels.hip k_build_chain / k_bg_fill /
k_bg_displaced / k_eh_fill / k_eb_size / k_eb_ref / k_eb_fill; csrc/sam_device.h spill_search / edge_find / block_find / fail_of_slot /
fail_of_hot / st_transfer_chain_impl / st_transfer_blocks_impl): the hashes and layouts restated, a model of the derivation, a model of the
lookups that runs on table images (the model's or the device's), token searches that plant probe runs, and named faults.  numpy + the oracle
only; no product import.  Everything is integer work and every comparison an equality.

  layout     samd_common.h:53-57 samd_spill_slots, :60 samd_chain_w, :62-66 samd_bigram_hash, :68-72 samd_edge_hash, :73-75 samd_spill_hash,
             :88-92 samd_eb_base / _mask / _hash / _tok_bits, :77-87 the kinds and bits; sam_kernels.hip:696-700 alloc_table (1024 floor, pow2 >=
             per x entries), :575 k_eb_size (pow2 >= max(4, per x deg) for s >= 1, deg >= 2, link != 0), :588 k_eb_ref (first slot / 4 | log2 << 27
             over the exclusive prefix sum in state order), :595-603 eb_fail, :611-649 k_eb_fill, :461-503 k_bg_fill, :509-517 k_bg_displaced,
             :541-563 k_eh_fill, :86-107 k_build_chain; sam_build.cpp:186-224 layout (ranks, spill block), :141-153 finalize_runs.
  Image      the oracle's export as the node image: rank order (stable, successor count descending -- KIND_COUNT), SINGLE / RUN flags, the
             spill blocks.  std::partial_sort leaves the ranks >= 8 in an unspecified order, so every planted state of degree > 8 has its
             edges in rank order already (conditions() asserts it): no implementation permutes a sorted row.
  tables     expected_tables(export, vocab, per, mode): chain words, root16, rc_bits, hot words and blocks slot for slot; the bigram and edge
             tables as (rows, homes) for check_open_table, plus one legal image of each (keys claimed in thread order) for the lookup model.
  Walker     st_transfer_blocks_impl / st_transfer_chain_impl in plain Python over table images -> (index, length, visited) and the probe count.
  FAULTS     flags of the builder model and of the Walker.  A faulty model always terminates (Runaway = a changed output).  Nothing here is
             ever built into a kernel."""
import functools

import numpy as np

from oracle import sam_oracle as O

U32 = 0xFFFFFFFF
INLINE, HEAD = 5, 3                                   # SAMD_INLINE_EDGES, SAMD_SPILL_HEAD
SINGLE, RUN, LEN_MASK = 0x40000000, 0x20000000, 0x1FFFFFFF
FK_ROOT, FK_ROOTCHILD, FK_HUB, FK_STATE = 0, 1, 2, 3
EB_IDX_MASK, EB_HUB, EB_KIND_SHIFT, EB_ROOTCHILD = 0x07FFFFFF, 0x08000000, 28, 0x40000000
EB_DISPLACED, BG_DISPLACED = 0x80000000, 0x20000000
EOS, PAD = 2, 1                                       # PAD: an id no corpus holds (a stream's front padding: the cursor stays at the root)
MODES = ("blocks", "edge", "plain")                   # default; SAMD_EDGE_BLOCKS=0; SAMD_EDGE_BLOCKS=0 SAMD_EDGE_TABLE=0

BUILDER_FAULTS = ("bit_on_previous_slot", "bit_dropped_on_overwrite", "spill_head_skipped", "spill_last_slot_skipped", "header_len_le")
LOOKUP_FAULTS = ("probe_no_wrap", "probe_one_round", "bit_of_current_slot", "bit_ignored", "w8_no_guard", "bigram_ignores_a", "len_ok_ignored",
                 "stale_header", "lb_escape_not_taken")
FAULTS = BUILDER_FAULTS + LOOKUP_FAULTS


class Runaway(Exception):
    """a faulty model ran into a loop cap (on the device: a hang)"""


# ---------------------------------------------------------------------------------------------------------------------------------
# hashes and sizes (python ints, or numpy uint64 arrays: every product is masked to 32 bits)
# ---------------------------------------------------------------------------------------------------------------------------------
def _u(x):
    return np.asarray(x).astype(np.uint64) if isinstance(x, np.ndarray) else int(x) & U32


def _m(x):
    return x & (np.uint64(U32) if isinstance(x, np.ndarray) else U32)


def _mul(a, k):
    return _m(_u(a) * (np.uint64(k) if isinstance(a, np.ndarray) else k))


def _sh(h, n):
    return h >> (np.uint64(n) if isinstance(h, np.ndarray) else n)


def bigram_hash(a, b):
    h = _m(_mul(a, 0x9E3779B1) + _mul(b, 0x85EBCA77))
    h = h ^ _sh(h, 15); h = _mul(h, 0x2C1B3C6D)
    return h ^ _sh(h, 13)


def edge_hash(state, tok):
    h = _mul(state, 0x85EBCA77) ^ _m(_mul(tok, 0x9E3779B1) + (np.uint64(0x7F4A7C15) if isinstance(tok, np.ndarray) else 0x7F4A7C15))
    h = h ^ _sh(h, 16); h = _mul(h, 0x2C1B3C6D)
    return h ^ _sh(h, 15)


def spill_hash(tok, slots):
    return _sh(_mul(tok, 0x9E3779B1), 7) & (np.uint64(slots - 1) if isinstance(tok, np.ndarray) else slots - 1)


def eb_hash(tok):
    h = _mul(tok, 0x9E3779B1)
    return h ^ _sh(h, 15)


def spill_slots(deg):
    need, m = 2 * (deg - INLINE), 4
    while m < need:
        m <<= 1
    return m


def chain_w(vocab):
    return 8 if vocab <= 32767 else 4


def eb_tok_bits(vocab):
    b = 8
    while b < 31 and (1 << b) - 1 < vocab:
        b += 1
    return b


def table_slots(entries, per):
    slots = 1024
    while slots < per * entries:
        slots <<= 1
    return slots


def block_slots(deg, per):
    m = 4
    while m < per * deg:
        m <<= 1
    return m


def eb_base(ref):
    return (ref & EB_IDX_MASK) << 2


def eb_mask(ref):
    return (1 << (ref >> 27)) - 1


def tokens_homed(hashfn, mask, slots, vocab, exclude=(), lo=3):
    """ids in lo .. vocab - 1, ascending, whose home hashfn(id) & mask is one of `slots`"""
    ids = np.arange(lo, vocab, dtype=np.int64)
    h = (hashfn(ids) & np.uint64(mask)).astype(np.int64)
    keep = np.isin(h, np.asarray(list(slots), dtype=np.int64)) & ~np.isin(ids, np.asarray(list(exclude) or [-1], dtype=np.int64))
    return [int(t) for t in ids[keep]]


# ---------------------------------------------------------------------------------------------------------------------------------
# the node image from the oracle's export
# ---------------------------------------------------------------------------------------------------------------------------------
class Image:
    def __init__(self, export):
        self.link, self.length, self.aux, self.deg = (export[k].tolist() for k in ("link", "length", "aux", "deg"))
        et, ed = export["edge_tok"].tolist(), export["edge_dst"].tolist()
        self.n = n = len(self.link)
        self.edges, k = [], 0
        for d in self.deg:
            self.edges.append(list(zip(et[k:k + d], ed[k:k + d]))); k += d
        aux = self.aux
        self.rank = [sorted(e, key=lambda td: -aux[td[1]]) for e in self.edges]        # stable: ties in dict order (sam_build.cpp:203-205)
        self.next = [dict(e) for e in self.edges]
        self.vocab = max(t for t, _ in self.edges[0]) + 1
        self.root_next = self.next[0]
        self.rctok = {d: t for t, d in self.edges[0]}
        self.single = [d <= 1 for d in self.deg]
        self.e0 = [r[0] if r else (-1, -1) for r in self.rank]
        run = [0] * (n + 1)
        for i in range(n - 1, -1, -1):
            run[i] = min(8, run[i + 1] + 1) if self.e0[i][0] >= 0 and self.e0[i][1] == i + 1 else 0
        self.run = [self.e0[i][0] >= 0 and run[self.e0[i][1]] >= 2 for i in range(n)]
        self.spill = {}                                                                  # state -> (head[3], slots[m]) of (tok, dst)
        for s in range(n):
            d = self.deg[s]
            if d > INLINE:
                m, r = spill_slots(d), self.rank[s]
                head = [r[INLINE + j] if INLINE + j < d else (-1, -1) for j in range(HEAD)]
                tab = [(-1, -1)] * m
                for t, dst in r[INLINE:]:
                    h = spill_hash(t, m)
                    while tab[h][0] != -1:
                        h = (h + 1) & (m - 1)
                    tab[h] = (t, dst)
                self.spill[s] = (head, tab)

    def flags(self, s):
        return (SINGLE if self.single[s] else 0) | (RUN if self.run[s] else 0)

    def spill_region(self):
        """the image's spill region as sam_build.cpp lays it out: int32 [n_spill, 2]"""
        out = []
        for s in sorted(self.spill):
            out += self.spill[s][0] + self.spill[s][1]
        return np.asarray(out, dtype=np.int32).reshape(-1, 2)

    def enum_edges(self, s, faults=()):
        """the order in which every derivation kernel meets the edges of s: inline ranks, spill head, spill slots"""
        out = list(self.rank[s][:INLINE])
        if s in self.spill:
            head, tab = self.spill[s]
            if "spill_head_skipped" not in faults:
                out += head
            out += tab[:-1] if "spill_last_slot_skipped" in faults else tab
        return [(t, d) for t, d in out if t >= 0 and d >= 0]

    def sorted_beyond_topk(self, s):
        return self.rank[s] == self.edges[s] or self.deg[s] <= 8


def ref_transfer(img, idx, length, tok):
    """transfer_state (static_sam.py:98-107) on the export -> (index, length, visited states)"""
    visited = 1
    while idx != 0 and tok not in img.next[idx]:
        idx = img.link[idx]; length = img.length[idx]; visited += 1
    if tok in img.next[idx]:
        return img.next[idx][tok], length + 1, visited
    return 0, 0, visited


# ---------------------------------------------------------------------------------------------------------------------------------
# the derivation
# ---------------------------------------------------------------------------------------------------------------------------------
def chain_words(img):
    W = chain_w(img.vocab)
    LOW = 0x7FFF if W == 8 else 0x7FFFFFFF
    out = np.zeros((img.n, 4), np.uint32)
    for s in range(img.n):
        tokw, alive = [], True
        for j in range(W):
            e = LOW | (LOW + 1)
            if alive and s + j < img.n:
                t, d = img.e0[s + j]
                if 0 <= t < LOW and d == s + j + 1:
                    p = img.link[s + j]
                    flagged = img.single[s + j] and p > 0 and img.link[p] == 0
                    e = t | (0 if flagged else LOW + 1)
                else:
                    alive = False
            else:
                alive = False
            tokw.append(e)
        out[s] = [tokw[2 * k] | (tokw[2 * k + 1] << 16) for k in range(4)] if W == 8 else tokw
    return out


def open_fill(rows, homes, slots, displaced_word=None, faults=()):
    """one legal image of an open-addressing table: rows claimed in the order given; then k_bg_displaced's bit"""
    tab = np.full((slots, 4), U32, np.uint32)
    pos = []
    for row, h in zip(rows, homes):
        while tab[h, 0] != U32:
            h = (h + 1) & (slots - 1)
        tab[h] = row; pos.append(h)
    if displaced_word is not None:
        for p, h in zip(pos, homes):
            if p != h:
                tab[((p - 1) & (slots - 1)) if "bit_on_previous_slot" in faults else h, displaced_word] |= BG_DISPLACED
    return tab


def expected_tables(export, vocab, per, mode="blocks", faults=()):
    img = export if isinstance(export, Image) else Image(export)
    assert img.vocab == vocab, (img.vocab, vocab)
    W, n, f = chain_w(vocab), img.n, frozenset(faults)
    chain = chain_words(img)
    out = dict(img=img, W=W, vocab=vocab, per=per, mode=mode, chain=chain, tok_bits=eb_tok_bits(vocab))
    # ---- blocks + hot words -------------------------------------------------------------------------------------------------------
    bref = [0] * n
    if mode == "blocks":
        off = 0
        for s in range(1, n):
            if img.deg[s] >= 2 and img.link[s] != 0:
                m = block_slots(img.deg[s], per)
                bref[s] = (off >> 2) | ((m.bit_length() - 1) << 27); off += m
        tok_bits = out["tok_bits"]
        tmask, lmax_slot = (1 << tok_bits) - 1, (1 << (32 - tok_bits)) - 1

        def eb_fail(s, lmax):
            p = img.link[s]
            if p <= 0:
                return FK_ROOT, 0, 0
            if img.link[p] == 0:
                return FK_ROOTCHILD, img.rctok[p], 0
            L = img.length[p]
            if bref[p] and (L <= lmax if "header_len_le" in f else L < lmax):
                return FK_HUB, bref[p], L
            return FK_STATE, p, min(L, lmax)

        hot, blocks = np.zeros((n, 4), np.uint32), np.zeros((off, 4), np.uint32)
        hot[0] = (0, 0, U32, U32)
        for s in range(1, n):
            kind, ref, ln = eb_fail(s, EB_IDX_MASK)
            x = img.rctok.get(s, -1) & U32 if kind == FK_ROOT else (ref if img.single[s] else bref[s])
            hot[s] = (x, (ln if img.single[s] else 0) | (kind << 27) | img.flags(s), img.e0[s][0] & U32, img.e0[s][1] & U32)
            if not bref[s]:
                continue
            kind, ref, ln = eb_fail(s, lmax_slot)
            base, bmask = eb_base(bref[s]), eb_mask(bref[s])
            blk = blocks[base:base + bmask + 1]
            blk[:] = (tmask | (ln << tok_bits), kind << EB_KIND_SHIFT, U32, ref)
            for t, d in img.enum_edges(s, f):
                if t >= tmask:
                    continue
                home = p = eb_hash(t) & bmask
                for probes in range(bmask + 1):
                    cur = int(blk[p, 0]) & tmask
                    if cur == t:
                        break
                    if cur == tmask:
                        y = (d & EB_IDX_MASK) | (kind << EB_KIND_SHIFT) | (EB_HUB if bref[d] else 0) | (EB_ROOTCHILD if d > 0 and img.link[d] == 0 else 0)
                        if "bit_dropped_on_overwrite" not in f:
                            y |= int(blk[p, 1]) & EB_DISPLACED
                        blk[p] = (t | (ln << tok_bits), y, bref[d] if bref[d] else int(chain[d, 0]), ref)
                        if probes:
                            blk[((p - 1) & bmask) if "bit_on_previous_slot" in f else home, 1] |= EB_DISPLACED
                        break
                    p = (p + 1) & bmask
        out.update(hot=hot, blocks=blocks)
    out["bref"] = bref
    # ---- bigram table, root16, rc_bits --------------------------------------------------------------------------------------------
    root16 = np.zeros((vocab, 4), np.uint32); root16[:, 0] = U32
    rc_bits = np.zeros((vocab + 31) // 32, np.uint32)
    rows, homes, pairs = [], [], 0
    with_hub = mode == "edge"
    for a in sorted(img.root_next):
        c = img.root_next[a]
        root16[a] = (c, 0, 0, img.length[c])
        rc_bits[a >> 5] |= np.uint32(1 << (a & 31))
        pairs += img.deg[c]
    bslots = table_slots(pairs, per)
    for a in sorted(img.root_next):
        c = img.root_next[a]
        lb, seen = min(img.length[c] - 1, 3), set()
        for t, d in img.enum_edges(c, f):
            if t in seen:
                continue
            seen.add(t)
            cx, cy = (int(chain[d, 0]), int(chain[d, 1])) if d > 0 else (U32, U32)
            hub = 0x80000000 if (with_hub and d > 0 and not img.single[d]) else 0
            if mode == "blocks":
                hub = 0x80000000 if d > 0 and bref[d] else 0
                if hub:
                    cx = bref[d]
                if d > 0 and img.link[d] == 0:
                    hub |= EB_ROOTCHILD
            rows.append((a | (t << 15) | (lb << 30), d | hub, cx, cy) if W == 8 else (a | ((lb & 1) << 31), t | ((lb >> 1) << 31), d | hub, cx))
            homes.append(bigram_hash(a, t) & (bslots - 1))
    dword = (1 if W == 8 else 2) if mode == "blocks" else None
    out.update(root16=root16, rc_bits=rc_bits, bigram_slots=bslots, bigram_rows=rows, bigram_homes=homes, bigram_pairs=pairs, bigram_dword=dword,
               bigram=open_fill(rows, homes, bslots, dword, f))
    # ---- edge table ---------------------------------------------------------------------------------------------------------------
    if mode == "edge":
        rows, homes = [], []
        total = sum(img.deg[s] for s in range(1, n) if img.deg[s] >= 2)
        eslots = table_slots(total, per)
        for s in range(1, n):
            if img.deg[s] < 2:
                continue
            seen = set()
            for t, d in img.enum_edges(s, f):
                if t in seen:
                    continue
                seen.add(t)
                rows.append((s, t, d | (0 if img.single[d] else 0x80000000), int(chain[d, 0])))
                homes.append(edge_hash(s, t) & (eslots - 1))
        out.update(edge_slots=eslots, edge_rows=rows, edge_homes=homes, edge_table=open_fill(rows, homes, eslots))
    return out


def check_open_table(image, rows, homes, displaced_word=None, what="table"):
    """an open-addressing table filled by racing threads (k_bg_fill / k_eh_fill): every key exactly once, inside the contiguous non-empty run
    that starts at its home, payload words equal, no other non-empty slot, the displaced bit (word `displaced_word`; None: never set) on a
    slot if and only if some key homed there is stored elsewhere.  Raises AssertionError('device table != model: ...')."""
    image = np.asarray(image, dtype=np.uint32)
    slots = len(image)
    clean, occupied = image.copy(), image[:, 0] != U32
    assert (image[~occupied] == U32).all(), "device table != model: %s: an empty slot that is not all-ones" % what
    bit = np.zeros(slots, bool)
    if displaced_word is not None:
        bit = occupied & ((image[:, displaced_word] & np.uint32(BG_DISPLACED)) != 0)
        clean[occupied, displaced_word] &= np.uint32(~BG_DISPLACED & U32)
    occ = np.flatnonzero(clean[:, 0] != U32)
    assert len(occ) == len(rows), "device table != model: %s holds %d entries, the model %d" % (what, len(occ), len(rows))
    where = {tuple(int(v) for v in clean[p]): int(p) for p in occ}
    assert len(where) == len(occ), "device table != model: %s holds a duplicated entry" % what
    nonempty = clean[:, 0] != U32
    want_bit = np.zeros(slots, bool)
    longest = 0
    for row, h in zip(rows, homes):
        key = tuple(int(v) & U32 for v in row)
        assert key in where, "device table != model: %s lacks the entry %r (or its payload differs)" % (what, key)
        p = where[key]
        dist = (p - h) & (slots - 1)
        assert all(nonempty[(h + k) & (slots - 1)] for k in range(dist + 1)), "device table != model: %s entry %r outside its probe run" % (what, key)
        longest = max(longest, dist + 1)
        if p != h:
            want_bit[h] = True
    if displaced_word is not None:       # (without blocks the bit's place belongs to the payload, which the rows above pin word for word)
        assert np.array_equal(bit, want_bit), "device table != model: %s displaced bits at %s, model %s" % (what, np.flatnonzero(bit), np.flatnonzero(want_bit))
    return longest


def runs(occupied):
    """[(start, length)] of the maximal runs of occupied slots, wrapping"""
    occ, n = list(map(bool, occupied)), len(occupied)
    if all(occ):
        return [(0, n)]
    if not any(occ):
        return []
    z, out, s, k = occ.index(False), [], None, 0
    for i in range(1, n + 1):
        j = (z + i) % n
        if occ[j]:
            if k == 0:
                s = j
            k += 1
        elif k:
            out.append((s, k)); k = 0
    return out


def longest_run(occupied):
    """(start, length, wraps) of the longest run"""
    r = max(runs(occupied), key=lambda sl: sl[1], default=(0, 0))
    return r[0], r[1], r[0] + r[1] > len(occupied)


# ---------------------------------------------------------------------------------------------------------------------------------
# the lookups, on table images
# ---------------------------------------------------------------------------------------------------------------------------------
class Cursor:
    def __init__(self, idx=0, length=0):
        self.idx, self.len, self.ent, self.used, self.hub, self.ptok = idx, length, None, 0, 0, -1


class Walker:
    """st_transfer_chain (sam_device.h:167-172) over the tables `T` (expected_tables' dict, or the device's export put in its place)"""

    def __init__(self, T, faults=()):
        self.T, self.f, self.img = T, frozenset(faults), T["img"]
        self.W, self.vocab, self.mode = T["W"], T["vocab"], T["mode"]
        self.LOW = 0x7FFF if self.W == 8 else 0x7FFFFFFF
        self.bmask = T["bigram_slots"] - 1
        self.probes = 0

    # ---- chain words ----
    def _entries(self, words, count, used):
        if self.W == 8:
            e = [(int(words[k // 2]) >> (16 * (k & 1))) & 0xFFFF for k in range(count)]
        else:
            e = [int(words[k]) for k in range(count)]
        return e + [self.LOW | (self.LOW + 1)] * (self.W - count), used

    def _load(self, c, s):
        c.ent, c.used = self._entries(self.T["chain"][s], self.W, 0); c.hub = 0

    def _half(self, c, lo, hi):
        c.ent, c.used = self._entries((lo, hi), self.W // 2, self.W // 2); c.hub = 0

    def _first(self, c, x):
        c.ent, c.used = self._entries((x,), 1, self.W - 1); c.hub = 0

    def _from_edge(self, c, x):
        if self.W == 8:
            c.ent, c.used = self._entries((x,), 2, self.W - 2); c.hub = 0
        else:
            self._first(c, x)

    def resolve(self, idx):
        return int(self.T["root16"][-2 - idx, 0]) if idx <= -2 else idx

    def _from_root(self, c, tok):
        bits = self.T["rc_bits"]
        if tok < self.vocab and (int(bits[tok >> 5]) >> (tok & 31)) & 1:
            c.idx, c.len = -2 - tok, 1
        else:
            c.idx, c.len = 0, 0

    # ---- probes ----
    def _bigram(self, c, a, tok, set_len, conclusive):
        """the bigram lambdas (sam_device.h:227-249, :423-448) -> extra visited states"""
        B, W, f, mask = self.T["bigram"], self.W, self.f, self.bmask
        h = bigram_hash(a, tok) & mask
        hit, e = False, None
        for probes in range(mask + 1):
            e = [int(v) for v in B[h]]; self.probes += 1
            if W == 8:
                if "bigram_ignores_a" in f:
                    hit = ((e[0] >> 15) & 0x7FFF) == (tok & 0x7FFF) and e[0] != U32 and tok < 0x8000
                else:
                    hit = (e[0] & 0x3FFFFFFF) == ((a | (tok << 15)) & U32) and ("w8_no_guard" in f or tok < 0x8000)
            else:
                hit = ("bigram_ignores_a" in f or (e[0] & 0x7FFFFFFF) == a) and (e[1] & 0x7FFFFFFF) == tok and e[0] != U32
            if hit or e[0] == U32:
                break
            if conclusive and "bit_ignored" not in f:
                dw = e[1] if W == 8 else e[2]
                if (probes == 0 or "bit_of_current_slot" in f) and not dw & BG_DISPLACED:
                    break
            if "probe_one_round" in f or ("probe_no_wrap" in f and h == mask):
                break
            h = (h + 1) & mask
        if hit:
            if set_len:
                lb = e[0] >> 30 if W == 8 else (e[0] >> 31) | ((e[1] >> 31) << 1)
                c.len = lb + 1 if (lb < 3 or "lb_escape_not_taken" in f) else int(self.T["root16"][a, 3])
            c.len += 1
            d, extra = (e[1], e[2]) if W == 8 else (e[2], e[3])
            if self.mode == "blocks":
                if d & EB_ROOTCHILD:
                    c.idx = -2 - tok
                    return 0
                c.idx = d & EB_IDX_MASK
                if d & 0x80000000:
                    c.hub = extra
                    return 0
            else:
                c.idx = d & 0x7FFFFFFF
            if W == 8:
                self._half(c, e[2], e[3])
            else:
                self._first(c, e[3])
            if self.mode != "blocks":
                c.hub = d >> 31
            return 0
        self._from_root(c, tok)
        return 1

    def _block_find(self, ref, tok):
        """block_find (sam_device.h:363-374) -> (hit, the slot that ended the probe)"""
        Bk, f = self.T["blocks"], self.f
        tmask, base, bmask = (1 << self.T["tok_bits"]) - 1, eb_base(ref), eb_mask(ref)
        p = eb_hash(tok) & bmask
        e = [int(v) for v in Bk[base + p]]; self.probes += 1
        for probes in range(bmask + 1):
            t = e[0] & tmask
            if tok < tmask and t == tok:
                return True, e
            if t == tmask:
                return False, e
            if "bit_ignored" not in f and (probes == 0 or "bit_of_current_slot" in f) and not e[1] & EB_DISPLACED:
                return False, e
            if "probe_one_round" in f or ("probe_no_wrap" in f and p == bmask):
                return False, e
            p = (p + 1) & bmask
            e = [int(v) for v in Bk[base + p]]; self.probes += 1
        return False, e

    def _fail_of_slot(self, e):
        lmax = (1 << (32 - self.T["tok_bits"])) - 1
        ln = e[0] >> self.T["tok_bits"]
        return ((e[1] >> EB_KIND_SHIFT) & 3, e[3], ln, ln != lmax or "len_ok_ignored" in self.f)

    @staticmethod
    def _fail_of_hot(h):
        return ((h[1] >> 27) & 3, h[0], h[1] & EB_IDX_MASK, True)

    def _edge_find(self, state, tok):
        E, mask = self.T["edge_table"], self.T["edge_slots"] - 1
        h = edge_hash(state, tok) & mask
        for probes in range(mask + 1):
            e = [int(v) for v in E[h]]; self.probes += 1
            if e[0] == state and e[1] == tok:
                return e
            if e[0] == U32 or "probe_one_round" in self.f or ("probe_no_wrap" in self.f and h == mask):
                return None
            h = (h + 1) & mask
        return None

    def _spill_search(self, s, tok):
        head, tab = self.img.spill[s]
        m = len(tab)
        h = spill_hash(tok, m)
        for probes in range(m):
            t, d = tab[h]; self.probes += 1
            if t == tok:
                return d
            if t == -1 or "probe_one_round" in self.f or ("probe_no_wrap" in self.f and h == m - 1):
                return -1
            h = (h + 1) & (m - 1)
        return -1

    # ---- one transition ----
    def step(self, c, tok):
        v = self._step_blocks(c, tok) if self.mode == "blocks" else self._step_chain(c, tok)
        c.ptok = tok
        return v

    def _register(self, c, tok):
        """the register path shared by both (sam_device.h:185-205, :383-401) -> handled?"""
        LOW = self.LOW
        ent = c.ent[0] if c.ent else LOW | (LOW + 1)
        is_tok = (ent & LOW) != LOW
        if is_tok and (ent & LOW) == tok:
            c.idx += 1; c.len += 1; c.hub = 0
            c.ent = c.ent[1:] + [LOW | (LOW + 1)]
            c.used += 1
            if c.used == self.W:
                self._load(c, c.idx)
            return True, is_tok, ent
        return False, is_tok, ent

    def _step_blocks(self, c, tok):
        T, img = self.T, self.img
        if tok < 0:
            c.idx, c.len, c.ent, c.hub = 0, 0, None, 0
            return 1
        done, is_tok, ent = self._register(c, tok)
        if done:
            return 1
        climbing = is_tok and not ent & (self.LOW + 1) and c.ptok >= 0
        my_ref = c.hub if c.idx > 0 else 0
        c.ent, c.used, c.hub = None, 0, 0
        visited = 1 if climbing else 0
        probing = climbing or c.idx <= -2
        if not probing and c.idx == 0:
            self._from_root(c, tok)
            return 1

        def land_e0(d, run):
            c.idx = d; c.len += 1
            if run:
                self._load(c, d)

        def follow_block(e):
            c.len += 1
            if e[1] & EB_ROOTCHILD:
                c.idx = -2 - tok
                return
            c.idx = e[1] & EB_IDX_MASK
            if e[1] & EB_HUB:
                c.hub = e[2]
            else:
                self._from_edge(c, e[2])

        if probing:
            a0 = c.ptok if climbing else -2 - c.idx
            return visited + 1 + self._bigram(c, a0, tok, climbing, True)
        visited += 1
        last_ref = 0
        if my_ref:
            hit, e = self._block_find(my_ref, tok)
            if hit:
                follow_block(e)
                return visited
            f = self._fail_of_slot(e); last_ref = my_ref
        else:
            h = [int(x) for x in T["hot"][c.idx]]
            f = self._fail_of_hot(h)
            if h[2] == tok & U32 and h[2] != U32:
                land_e0(h[3], bool(h[1] & RUN))
                return visited
            if not h[1] & SINGLE:
                if f[0] == FK_ROOT:
                    return visited + self._bigram(c, h[0], tok, False, True)
                hit, e = self._block_find(h[0], tok)
                if hit:
                    follow_block(e)
                    return visited
                f = self._fail_of_slot(e); last_ref = h[0]
        for _ in range(4 * img.n + 8):
            visited += 1
            kind, ref, ln, len_ok = f
            if kind == FK_ROOT:
                c.len = 0; self._from_root(c, tok)
                return visited
            if kind == FK_ROOTCHILD:
                return visited + self._bigram(c, ref, tok, True, True)
            c.len = ln
            if kind == FK_HUB:
                hit, e = self._block_find(ref, tok)
                if hit:
                    follow_block(e)
                    return visited
                if "stale_header" in self.f and last_ref:
                    e = [int(x) for x in T["blocks"][eb_base(last_ref) + (eb_hash(tok) & eb_mask(last_ref))]]
                f = self._fail_of_slot(e); last_ref = ref
                continue
            h = [int(x) for x in T["hot"][ref]]
            if not len_ok:
                c.len = img.length[ref]
            if h[2] == tok & U32 and h[2] != U32:
                land_e0(h[3], bool(h[1] & RUN))
                return visited
            if h[1] & SINGLE:
                f = self._fail_of_hot(h)
            else:
                hit, e = self._block_find(h[0], tok)
                if hit:
                    follow_block(e)
                    return visited
                f = self._fail_of_slot(e); last_ref = h[0]
        raise Runaway("climb")

    def _node_edge(self, s, tok):
        """the node beyond word 0 (sam_device.h:320-329): inline ranks 1 .. 4, then the spill table"""
        for t, d in self.img.rank[s][1:INLINE]:
            if t == tok:
                return d
        if self.img.deg[s] > INLINE:
            return self._spill_search(s, tok)
        return -1

    def _step_chain(self, c, tok):
        img, have_edges = self.img, self.mode == "edge"
        if tok < 0:
            c.idx, c.len, c.ent, c.hub = 0, 0, None, 0
            return 1
        done, is_tok, ent = self._register(c, tok)
        if done:
            return 1
        climbing = is_tok and not ent & (self.LOW + 1) and c.ptok >= 0
        at_hub = bool(c.hub) and have_edges and c.idx > 0
        c.ent, c.used, c.hub = None, 0, 0
        visited = 1 if climbing else 0
        probing = climbing or c.idx <= -2
        if not probing and c.idx == 0:
            self._from_root(c, tok)
            return 1
        if probing:
            a = c.ptok if climbing else -2 - c.idx
            extra = self._bigram(c, a, tok, climbing, False)
            return visited + 1 + extra

        def follow(e):
            c.idx = e[2] & 0x7FFFFFFF; c.len += 1
            self._from_edge(c, e[3]); c.hub = e[2] >> 31

        def rank0(s):
            c.idx = img.e0[s][1]; c.len += 1
            if img.run[s]:
                self._load(c, c.idx)

        hopped = False
        first = True
        for _ in range(4 * img.n + 8):
            visited += 1
            s = c.idx
            if s == 0:
                if hopped:
                    c.len = 0
                self._from_root(c, tok)
                return visited
            if hopped:
                c.len = img.length[s]
            if have_edges and first and at_hub:
                e = self._edge_find(s, tok)
                if e:
                    follow(e)
                    return visited
            else:
                if img.e0[s][0] == tok and not (have_edges and hopped and not img.single[s]):      # (a hop's branching state: the table alone)
                    rank0(s)
                    return visited
                if not img.single[s]:
                    if have_edges:
                        e = self._edge_find(s, tok)
                        if e:
                            follow(e)
                            return visited
                    else:
                        d = self._node_edge(s, tok)
                        if d >= 0:
                            c.idx = d; c.len += 1
                            if d > 0:
                                self._load(c, d)
                            return visited
            first = False
            c.idx = img.link[s]; hopped = True
        raise Runaway("climb")

    def run(self, tokens, start=(0, 0)):
        """-> [(index, length)] after every token, visited states in all"""
        c, out, visited = Cursor(*start), [], 0
        for t in tokens:
            visited += self.step(c, int(t))
            out.append((self.resolve(c.idx), c.len))
        return out, visited


def oracle_run(img, tokens, start=(0, 0)):
    idx, ln, out, visited = start[0], start[1], [], 0
    for t in tokens:
        if t < 0:
            idx, ln, v = 0, 0, 1
        else:
            idx, ln, v = ref_transfer(img, idx, ln, int(t))
        visited += v
        out.append((idx, ln))
    return out, visited


# ---------------------------------------------------------------------------------------------------------------------------------
# planted corpora
# ---------------------------------------------------------------------------------------------------------------------------------
class Ids:
    """fresh token ids: ascending from `lo`, never one that is reserved or already handed out"""

    def __init__(self, vocab, lo):
        self.vocab, self.next, self.used = vocab, lo, {EOS, PAD, vocab - 1}

    def reserve(self, toks):
        self.used.update(int(t) for t in toks)
        return [int(t) for t in toks]

    def fresh(self):
        while self.next in self.used:
            self.next += 1
        assert self.next < self.vocab - 1
        self.used.add(self.next)
        return self.next

    def take(self, pool, n):
        out = [t for t in pool if t not in self.used][:n]
        assert len(out) == n, "the pool is too small"
        return self.reserve(out)


class Case:
    """docs (every document starts with a token of its own, so that no two documents share a left context and the state of a planted
    string has a deeper single-edge state above it), the targets [(name, kind, state-landing prefix or start cursor, probes)]"""

    def __init__(self, name, vocab, per=4):
        self.name, self.vocab, self.per = name, vocab, per
        self.ids = Ids(vocab, 40 if vocab <= 32767 else 33000)
        self.docs, self.targets, self.notes = [[vocab - 1]], [], {}

    def doc(self, *toks):
        h = self.ids.fresh()
        self.docs.append([h] + [int(t) for t in toks])
        return h

    @functools.cached_property
    def oracle(self):
        return O.StaticSAM.build(self.docs, EOS)

    @functools.cached_property
    def img(self):
        return Image(self.oracle.export())

    def tables(self, mode="blocks", per=None, faults=()):
        return _tables(self, mode, per or self.per, tuple(sorted(faults)))

    def state_of(self, prefix):
        return oracle_run(self.img, prefix)[0][-1]


@functools.lru_cache(maxsize=64)
def _tables(case, mode, per, faults):
    return expected_tables(case.img, case.vocab, per, mode, faults)


def block_classes(T, s, used, want=2):
    """probe tokens of hub s by what its block does with them -> dict class -> [tok]"""
    img, ref, tmask = T["img"], T["bref"][s], (1 << T["tok_bits"]) - 1
    base, bmask = eb_base(ref), eb_mask(ref)
    blk = T["blocks"][base:base + bmask + 1]
    occ = (blk[:, 0] & np.uint32(tmask)) != tmask
    disp = (blk[:, 1] & np.uint32(EB_DISPLACED)) != 0
    ids = np.asarray([t for t in range(3, min(T["vocab"], tmask, 32767)) if t not in used], dtype=np.int64)
    home = (eb_hash(ids) & np.uint64(bmask)).astype(np.int64)
    out = dict(present=[t for t, _ in img.rank[s]], absent_empty=[int(t) for t in ids[~occ[home]][:want]],
               absent_conclusive=[int(t) for t in ids[occ[home] & ~disp[home]][:want]], absent_in_run=[int(t) for t in ids[occ[home] & disp[home]][:want]])
    p0 = out["present"][0]
    out["out_of_range"] = [T["vocab"], T["vocab"] + 5, tmask, p0 + tmask + 1, p0 + (1 << 27)]
    return out


def bigram_classes(T, a, used, want=2):
    img, B, mask = T["img"], T["bigram"], T["bigram_slots"] - 1
    occ = B[:, 0] != U32
    disp = (B[:, T["bigram_dword"]] & np.uint32(BG_DISPLACED)) != 0 if T["bigram_dword"] is not None else np.zeros(len(B), bool)
    c = img.root_next[a]
    out = dict(present=[t for t, _ in img.rank[c]], absent_empty=[], absent_conclusive=[], absent_in_run=[])
    for t in range(3, min(T["vocab"], 32767)):
        if t in used:
            continue
        h = bigram_hash(a, t) & mask
        k = "absent_empty" if not occ[h] else ("absent_in_run" if disp[h] else "absent_conclusive")
        if len(out[k]) < want:
            out[k].append(t)
    p0 = out["present"][0]
    out["out_of_range"] = [T["vocab"], T["vocab"] + 5, p0 + (1 << 27)]
    return out


def _probes(classes):
    seen, out = set(), []
    for k in ("present", "absent_empty", "absent_conclusive", "absent_in_run", "out_of_range", "alias"):
        for t in classes.get(k, []):
            if t not in seen:
                seen.add(t); out.append(t)
    return out


LAST64 = lambda vocab: tokens_homed(eb_hash, 63, [63], vocab)


def case_hubs(vocab):
    """hub clusters of every kind below the root children (module docstring of tests/test_static_planting_cpu.py)"""
    c = Case("hubs_v%d" % vocab, vocab)
    ids, last = c.ids, LAST64(vocab)
    f = ids.fresh
    # A: degree 16, every edge homed in the last slot of its 64-slot block (4 slots per entry): one run of 16 that wraps to slot 14
    x, y, w, q = f(), f(), f(), f()
    TA = ids.take(last, 16)
    hA = [c.doc(x, y, t) for t in TA]
    c.doc(w, y, q)
    # B: degree 32: at 2 slots per entry half of its 64-slot block is one run
    x2, y2, w2, q2 = f(), f(), f(), f()
    TB = ids.take(last, 32)
    hB = [c.doc(x2, y2, t) for t in TB]
    c.doc(w2, y2, q2)
    # C: homes 61 (4 keys), 62 (3), 63 (3): the home slot of the keys homed in 62 and 63 holds a displaced key homed in 61
    x3, y3, w3, q3 = f(), f(), f(), f()
    TC = ids.take(tokens_homed(eb_hash, 63, [61], vocab), 4) + ids.take(tokens_homed(eb_hash, 63, [62], vocab), 3) + ids.take(last, 3)
    hC = [c.doc(x3, y3, t) for t in TC]
    c.doc(w3, y3, q3)
    # a chain of three hubs: [a b c d] -> [b c d] -> [c d] -> root child [d]; e1 .. e5 all homed in the last slot of blocks of 8 and 16 slots
    a, b, cc, d, z1, z2, z3 = (f() for _ in range(7))
    e = ids.take(last, 5)
    g = [c.doc(a, b, cc, d, e[0]), c.doc(a, b, cc, d, e[1]), c.doc(z3, b, cc, d, e[2]), c.doc(z2, cc, d, e[3]), c.doc(z1, d, e[4])]
    # single states whose fail header is a plain state: [i g h] -> [g h] (one edge) -> root child [h]
    i_, j_, g_, h_, k_, k2 = (f() for _ in range(6))
    s1 = c.doc(i_, g_, h_, k_); c.doc(j_, g_, h_, k_); c.doc(h_, k2)
    # a hub whose link is a root child of length 5 (lb = 3: the match length comes from root16)
    o, p, qq, r, z, v1, v2 = (f() for _ in range(7))
    s = ids.take(last, 3)
    l1 = c.doc(v1, o, p, qq, r, z, s[0]); c.doc(v1, o, p, qq, r, z, s[1]); l3 = c.doc(v2, o, p, qq, r, z, s[2])
    used = set(ids.used)
    T = c.tables()
    H = c.state_of
    hubs = dict(A=H([x, y])[0], B=H([x2, y2])[0], C=H([x3, y3])[0], G1=H([a, b, cc, d])[0], G2=H([b, cc, d])[0], G3=H([cc, d])[0], L=H([v1, o, p, qq, r, z])[0])
    c.notes.update(hubs=hubs, TA=TA, TB=TB, TC=TC, e=e, lb_child=z, chain3=(hubs["G1"], hubs["G2"], hubs["G3"]), state_kind=(H([s1, i_, g_, h_])[0], H([g_, h_])[0]))
    cls = {k: block_classes(T, s_, used) for k, s_ in hubs.items()}
    c.notes["classes"] = cls
    for name, pre, deeper in (("A", [x, y], [hA[0], x, y]), ("B", [x2, y2], [hB[3], x2, y2]), ("C", [x3, y3], [hC[5], x3, y3])):
        c.targets += [(name + ".cursor", pre, _probes(cls[name])), (name + ".climb", deeper, _probes(cls[name]))]
    for name, child, flagged in (("A", y, [w, y]), ("B", y2, [w2, y2]), ("C", y3, [w3, y3])):
        bc = bigram_classes(T, child, used)
        c.targets += [(name + ".child", [child], _probes(bc)), (name + ".flagged", flagged, _probes(bc)[:12])]
    three = e + cls["G1"]["absent_empty"] + cls["G2"]["absent_in_run"] + cls["G3"]["absent_conclusive"] + cls["G1"]["out_of_range"]
    c.targets += [("G1.cursor", [a, b, cc, d], three), ("G1.climb", [g[0], a, b, cc, d], three), ("G2.cursor", [b, cc, d], three), ("G2.climb", [g[2], z3, b, cc, d], three),
                  ("G3.cursor", [cc, d], three), ("d.child", [d], three)]
    c.targets += [("state.climb", [s1, i_, g_, h_], [k_, k2, e[0], vocab]), ("state.mid", [g_, h_], [k_, k2, e[0]])]
    c.targets += [("L.cursor", [v1, o, p, qq, r, z], s + [e[0], vocab]), ("L.climb", [l1, v1, o, p, qq, r, z], s + [e[0]]), ("L.flagged", [l3, v2, o, p, qq, r, z], s + [e[0]]),
                  ("L.child", [z], s + [e[0]])]
    return c


def case_bigram(vocab):
    """one root child a = 17 with 24 successors homed in the last four slots of the 1024-slot bigram table: one wrapping run"""
    c = Case("bigram_v%d" % vocab, vocab)
    a = 17
    c.ids.reserve([a])
    hb = lambda t: bigram_hash(a, t)
    pool = tokens_homed(hb, 1023, [1020, 1021, 1022, 1023], min(vocab, 32767))
    alias = []
    if vocab <= 32767:                                   # W = 8: b + 0x8000 and b + 0x20000 shift to b's key; their home must lie inside the run before b
        for off in (0x8000, 0x20000):
            alias.append(next(t for t in pool if t not in alias and ((bigram_hash(a, t + off) & 1023) >= 1020 or (bigram_hash(a, t + off) & 1023) < 16)))
        c.ids.reserve(alias)
    B = c.ids.take(pool, 24 - len(alias)) + alias
    hs = [c.doc(a, t) for t in B]
    # a pair (a2, b*) of ANOTHER root child stored inside the run, b* no successor of a and homed under a at the run's start: a hit test that
    # forgets a finds it
    bstar = c.ids.take(pool, 1)[0]
    a2 = next(t for t in range(c.ids.next, vocab) if t not in c.ids.used and ((bigram_hash(t, bstar) & 1023) >= 1022 or (bigram_hash(t, bstar) & 1023) < 8))
    c.ids.reserve([a2]); c.doc(a2, bstar)
    used = set(c.ids.used)
    T = c.tables()
    bc = bigram_classes(T, a, used)
    if alias:
        bc["alias"] = [alias[0] + 0x8000, alias[1] + 0x20000]
    bc["absent_in_run"] = [bstar] + bc["absent_in_run"]
    c.notes.update(a=a, B=B, alias=alias, classes=bc, foreign=(a2, bstar))
    c.targets += [("a.child", [a], _probes(bc)), ("a.flagged", [hs[2], a], _probes(bc))]
    return c


def case_spill(vocab):
    """a hub of degree 22 (and the root child below it, degree 23) whose successors are all homed in the last of their 64 spill slots"""
    c = Case("spill_v%d" % vocab, vocab)
    f = c.ids.fresh
    x, y, w, q = f(), f(), f(), f()
    sh = lambda t: spill_hash(t, 64)
    pool = tokens_homed(sh, 63, [63], min(vocab, 60000))
    # ranks 0 .. 4 live in the node; ranks 5, 6, 7 (which the spill HEAD repeats) are homed in slots 60, 61, 62, so that the last slot holds a key
    # that only the table names; everything else is homed in the last slot: one run 60 .. 63, 0 .. 12
    TS = c.ids.take(pool, 5) + [c.ids.take(tokens_homed(sh, 63, [k], min(vocab, 60000)), 1)[0] for k in (60, 61, 62)] + c.ids.take(pool, 14)
    hs = [c.doc(x, y, t) for t in TS]
    c.doc(w, y, q)
    used = set(c.ids.used)
    T = c.tables()
    s = c.state_of([x, y])[0]
    cls = block_classes(T, s, used)
    cls["absent_in_run"] = cls["absent_in_run"] + [t for t in pool if t not in used][:3]           # spill home 63: probes to the end of the spill run
    c.notes.update(hub=s, TS=TS, classes=cls, child=y)
    c.targets += [("S.cursor", [x, y], _probes(cls)), ("S.climb", [hs[1], x, y], _probes(cls)), ("S.child", [y], _probes(cls)), ("S.flagged", [w, y], _probes(cls)[:12])]
    return c


def case_edge(vocab):
    """the edge table (SAMD_EDGE_BLOCKS=0) keys by (state, token): a hub of degree 12 homed in the table's last four slots.  Built once with
    provisional ids to learn the hub's index, then with the ids picked for that index (the automaton's shape depends on the equality pattern
    of the tokens only)."""
    def build(toks):
        c = Case("edge_v%d" % vocab, vocab)
        f = c.ids.fresh
        x, y, w, q = f(), f(), f(), f()
        T_ = c.ids.reserve(toks) if toks else [f() for _ in range(12)]
        hs = [c.doc(x, y, t) for t in T_]
        c.doc(w, y, q)
        return c, (x, y, w, q), hs, T_
    c0, (x, y, _, _), _, _ = build(None)
    s = c0.state_of([x, y])[0]
    taken = set(c0.ids.used)
    pool = [t for t in tokens_homed(lambda t: edge_hash(np.uint64(s) + np.zeros_like(t), t), 1023, [1020, 1021, 1022, 1023], min(vocab, 60000)) if t not in taken]
    c, (x, y, w, q), hs, TE = build(pool[:12])
    assert c.state_of([x, y])[0] == s, "the hub's index moved"
    used = set(c.ids.used)
    spare = [t for t in pool[12:] if t not in used][:3]
    c.notes.update(hub=s, TE=TE, in_run=spare)
    probes = TE + spare + [t for t in range(3, 40) if t not in used][:3] + [vocab, vocab + 5]
    c.targets += [("E.cursor", [x, y], probes), ("E.climb", [hs[1], x, y], probes), ("E.child", [y], probes)]
    return c


WIDTH_VOCAB = (1 << 22) + 1                                # tok_bits 23: a 9-bit length field, lmax = 511


def case_width():
    """hubs whose suffix link is a hub of length 510 (fits the slot's length field), 511 (the escape value itself) and 600 (beyond)"""
    c = Case("width", WIDTH_VOCAB)
    f = c.ids.fresh
    r = f()
    A, B, C = f(), f(), f()
    d = [f() for _ in range(6)]
    h = [c.doc(A, *([r] * 510), d[0]), c.doc(A, *([r] * 510), d[1]), c.doc(B, *([r] * 511), d[2]), c.doc(B, *([r] * 511), d[3]),
         c.doc(C, *([r] * 601), d[4]), c.doc(C, *([r] * 601), d[5])]
    # (r^601 occurs below C only, so it shares the state of C r^601, whose link is r^600: three edges -- r, d[4], d[5])
    tops = {L: c.state_of([t] + [r] * n) for L, t, n in ((510, A, 510), (511, B, 511), (600, C, 601))}
    c.notes.update(r=r, tops=tops, d=d)
    absent = c.ids.fresh()
    for L, (idx, ln) in tops.items():
        c.targets.append(("W%d" % L, (idx, ln), d + [r, absent, WIDTH_VOCAB, (1 << 23) - 1]))
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, v = name.partition("_v")
    return case_width() if name == "width" else dict(hubs=case_hubs, bigram=case_bigram, spill=case_spill, edge=case_edge)[kind](int(v))


CASES = tuple("%s_v%d" % (k, v) for k in ("hubs", "bigram", "spill", "edge") for v in (32767, 70000)) + ("width",)


# ---------------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def streams(name):
    """[(target, tokens, split, start cursor)]: the landing, the probe, then the hub's first token again (a climb from wherever the probe
    ended).  split = where the second launch begins (the probe: its cursor is then met by index)."""
    c, out = case(name), []
    for tname, landing, probes in c.targets:
        for t in probes:
            if isinstance(landing, tuple):
                out.append((tname, [t, probes[0]], 0, landing))
            else:
                out.append((tname, list(landing) + [t, probes[0]], len(landing), (0, 0)))
    return out


def launches(name):
    """the token matrices of the launches, time-major, padded with PAD (the cursor falls to the root and stays):
    one = everything from the start cursors; first = the landings (padded in FRONT, from the root); second = from the cursors `first` left
    (streams that start on a cursor keep it) -> dict name -> (tokens [T, B] int32, start cursors [B, 2] int32)"""
    S = streams(name)
    B = len(S)
    T1, T0, T2 = max(len(s[1]) for s in S), max(max(s[2] for s in S), 1), max(len(s[1]) - s[2] for s in S)
    one, first, second = (np.full((T, B), PAD, np.int32) for T in (T1, T0, T2))
    start = np.zeros((B, 2), np.int32)
    for b, (_, toks, split, st) in enumerate(S):
        one[:len(toks), b] = toks
        if split:
            first[T0 - split:, b] = toks[:split]
        second[:len(toks) - split, b] = toks[split:]
        start[b] = st
    return dict(one=(one, start), first=(first, np.zeros((B, 2), np.int32)), second=(second, None))


def run_launch(step_run, toks, start):
    """-> trace [T, B, 2], final cursors [B, 2], visited"""
    T, B = toks.shape
    trace, cur, visited = np.zeros((T, B, 2), np.int32), np.zeros((B, 2), np.int32), 0
    for b in range(B):
        out, v = step_run([int(t) for t in toks[:, b]], (int(start[b, 0]), int(start[b, 1])))
        trace[:, b] = out; cur[b] = out[-1]; visited += v
    return trace, cur, visited


def run_all(name, step_run):
    """the three launches through step_run(tokens, start) -> dict launch -> (trace, cursors, visited)"""
    L, S = launches(name), streams(name)
    out = {"one": run_launch(step_run, *L["one"]), "first": run_launch(step_run, *L["first"])}
    carried = out["first"][1].copy()
    for b, s in enumerate(S):
        if s[2] == 0:
            carried[b] = s[3]
    out["second"] = run_launch(step_run, L["second"][0], carried)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    img = case(name).img
    return run_all(name, lambda toks, start: oracle_run(img, toks, start))


def same_runs(a, b):
    return all(np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]) and a[k][2] == b[k][2] for k in a)


def model_runs(name, mode="blocks", per=None, faults=()):
    """-> (run_all's dict, probes in all); a Runaway is reported as None"""
    c = case(name)
    bf = [f for f in faults if f in BUILDER_FAULTS]
    w = Walker(c.tables(mode, per, bf), faults)
    try:
        return run_all(name, w.run), w.probes
    except Runaway:
        return None, w.probes


# ---------------------------------------------------------------------------------------------------------------------------------
# what every case is for, asserted on the model
# ---------------------------------------------------------------------------------------------------------------------------------
def block_of(T, s):
    ref, tmask = T["bref"][s], (1 << T["tok_bits"]) - 1
    blk = T["blocks"][eb_base(ref):eb_base(ref) + eb_mask(ref) + 1]
    return blk, (blk[:, 0] & np.uint32(tmask)) != tmask, tmask


def foreign_home(T, s):
    """present keys of hub s whose home slot holds another key"""
    blk, occ, tmask = block_of(T, s)
    return [int(x) & tmask for p, x in enumerate(blk[:, 0]) if occ[p] and int(blk[eb_hash(int(x) & tmask) & (len(blk) - 1), 0]) & tmask != int(x) & tmask]


def conditions(name):
    c = case(name)
    img, T, fig = c.img, c.tables(), dict(states=c.img.n, streams=len(streams(name)))
    assert all(img.sorted_beyond_topk(s) for s in range(1, img.n)), "a state of degree > 8 whose edges are not in rank order"
    if name.startswith("hubs"):
        hubs = c.notes["hubs"]
        blk, occ, _ = block_of(T, hubs["A"])
        assert len(blk) == 64 and longest_run(occ) == (63, 16, True)
        T2 = c.tables(per=2)
        blk, occ, _ = block_of(T2, hubs["B"])
        assert len(blk) == 64 and longest_run(occ) == (63, 32, True)
        blk, occ, _ = block_of(T, hubs["C"])
        assert len(blk) == 64 and longest_run(occ) == (61, 10, True) and len(foreign_home(T, hubs["C"])) >= 6
        assert int(blk[62, 1]) & EB_DISPLACED and int(blk[63, 1]) & EB_DISPLACED and not int(blk[0, 1]) & EB_DISPLACED
        kinds = lambda s: (int(T["blocks"][eb_base(T["bref"][s]), 1]) >> EB_KIND_SHIFT) & 3
        g1, g2, g3 = c.notes["chain3"]
        assert [kinds(s) for s in (hubs["A"], g1, g2, g3, hubs["L"])] == [FK_ROOTCHILD, FK_HUB, FK_HUB, FK_ROOTCHILD, FK_ROOTCHILD]
        assert img.link[g1] == g2 and img.link[g2] == g3 and [len(block_of(T, s)[0]) for s in (g1, g2, g3)] == [8, 16, 16]
        s_top, s_mid = c.notes["state_kind"]
        assert (int(T["hot"][s_top, 1]) >> 27) & 3 == FK_STATE and int(T["hot"][s_top, 0]) == s_mid and (int(T["hot"][s_mid, 1]) >> 27) & 3 == FK_ROOTCHILD
        assert img.length[img.root_next[c.notes["lb_child"]]] == 5
        for k, cl in c.notes["classes"].items():
            assert cl["absent_empty"] and cl["absent_in_run"] and cl["absent_conclusive"], k
        fig.update(runA=16, runB=32, runC=10, foreign=len(foreign_home(T, hubs["C"])))
    elif name.startswith("bigram"):
        assert T["bigram_slots"] == 1024 and T["bigram_pairs"] * 4 <= 1024
        occ = T["bigram"][:, 0] != U32
        start, n, wraps = longest_run(occ)
        assert n >= 24 and wraps and start >= 1020, (start, n, wraps)
        cl = c.notes["classes"]
        assert cl["absent_empty"] and cl["absent_in_run"] and cl["absent_conclusive"]
        if c.notes["alias"]:
            B, a = T["bigram"], c.notes["a"]
            for b, off in zip(c.notes["alias"], (0x8000, 0x20000)):
                pos = next(p for p in range(1024) if int(B[p, 0]) & 0x3FFFFFFF == a | (b << 15))
                ah = bigram_hash(a, b + off) & 1023
                assert (ah - start) % 1024 < (pos - start) % 1024 < n, "the alias's home is not inside the run before the key"
        fig.update(run=n, run_start=start)
    elif name.startswith("spill"):
        s = c.notes["hub"]
        head, tab = img.spill[s]
        assert img.deg[s] == 22 and len(tab) == 64 and longest_run([t != -1 for t, _ in tab]) == (60, 17, True)
        assert tab[63][0] not in [t for t, _ in head]
        assert len(img.spill[img.root_next[c.notes["child"]]][1]) == 64
        cl, used = c.notes["classes"], {t for d in c.docs for t in d}
        assert cl["absent_empty"] and cl["absent_conclusive"] and len(cl["absent_in_run"]) >= 5           # the block's classes + three spill ids
        spare = cl["absent_in_run"][-3:]
        assert all(spill_hash(t, 64) == 63 and t not in used for t in spare) and any(spill_hash(t, 64) not in range(60, 64) and tab[spill_hash(t, 64)][0] == -1
                                                                                      for t in cl["absent_empty"] + cl["absent_conclusive"])
        fig.update(run=17)
    elif name.startswith("edge"):
        Te = c.tables("edge")
        assert Te["edge_slots"] == 1024
        start, n, wraps = longest_run(Te["edge_table"][:, 0] != U32)
        assert n >= 12 and wraps and start >= 1020
        spare, s_, used = c.notes["in_run"], c.notes["hub"], {t for d in c.docs for t in d}
        assert len(spare) == 3 and all(edge_hash(s_, t) & 1023 >= 1020 and t not in used for t in spare)          # absent, homed inside the run
        empty = [t for t in c.targets[0][2] if t not in used and t < c.vocab and Te["edge_table"][edge_hash(s_, t) & 1023, 0] == U32]
        assert empty, "no absent id homed in an empty slot of the edge table"
        fig.update(run=n, run_start=start)
    elif name == "width":
        assert T["tok_bits"] == 23
        want = {510: (FK_HUB, 510), 511: (FK_STATE, 511), 600: (FK_STATE, 511)}
        for L, (idx, ln) in c.notes["tops"].items():
            assert ln == L + (2 if L == 600 else 1) and img.length[img.link[idx]] == L and T["bref"][idx] and T["bref"][img.link[idx]]
            x, y = int(T["blocks"][eb_base(T["bref"][idx]), 0]), int(T["blocks"][eb_base(T["bref"][idx]), 1])
            assert ((y >> EB_KIND_SHIFT) & 3, x >> 23) == want[L], (L, (y >> EB_KIND_SHIFT) & 3, x >> 23)
    return fig


TABLE_KEYS = ("chain", "root16", "rc_bits", "hot", "blocks", "bigram", "edge_table")


def fault_marks(name, fault, modes=MODES):
    """what the fault changes in this case: 'T' a table of the model, 'S' a stream (index, length, cursor or visited count), 'P' the probe
    count alone -> a string, empty when the case does not notice"""
    c, marks = case(name), set()
    for mode in modes:
        clean, bad = c.tables(mode), c.tables(mode, faults=[fault] if fault in BUILDER_FAULTS else [])
        if any(k in clean and not np.array_equal(clean[k], bad[k]) for k in TABLE_KEYS):
            marks.add("T")
        got, probes = model_runs(name, mode, faults=(fault,))
        if got is None or not same_runs(got, expected(name)):
            marks.add("S")
        elif probes != _clean_probes(name, mode):
            marks.add("P")
    return "".join(sorted(marks))


@functools.lru_cache(maxsize=None)
def _clean_probes(name, mode):
    return model_runs(name, mode)[1]


# k_eb_fill's `y |= blk[p].y & SAMD_EB_DISPLACED` keeps a bit that an EMPTY slot carries when a key moves in.  No empty slot ever carries one: the
# bit is set on the home slot of a key that found that slot occupied, and slots are never vacated.  The line is a guard that cannot fire, and the
# fault that removes it changes nothing -- which tests/test_static_planting_cpu.py asserts instead of demanding a case for it.
UNREACHABLE = ("bit_dropped_on_overwrite",)


def fault_matrix(names=CASES, faults=FAULTS):
    return {n: {f: fault_marks(n, f) for f in faults} for n in names}


def format_matrix(M):
    faults = list(next(iter(M.values())))
    lines = ["%-16s" % "case" + " ".join("%2d" % i for i in range(len(faults)))]
    lines += ["%-16s" % n + " ".join("%2s" % (row[f] or ".")[:2] for f in faults) for n, row in M.items()]
    return "\n".join(lines + ["%2d = %s" % (i, f) for i, f in enumerate(faults)])
