"""The planting of tests/static_planting.py checked on the CPU: what tests/test_gpu_static_planted.py relies on.

  * the hashes, sizing rules and bit layouts the module restates are the ones in the sources, and its token searches find what the issue's
    table says (ids whose home is the last slot of a 64 / 256 / 1024-slot block, ids homed under a = 17 at the end of the bigram table);
  * every plant exists in the model's tables: run lengths, the wrap past the last slot, present keys whose home slot holds a foreign
    displaced key, conclusive-miss and run-to-the-end ids, the three header-width hubs on HUB / STATE / STATE;
  * the model's lookup (a port of st_transfer_blocks_impl / st_transfer_chain_impl onto the model's tables) gives the oracle's
    transfer_state -- (index, length) after every token, the committed cursors and the visited-state count -- on every stream, in all three
    handle states and at 2 / 4 / 64 slots per entry;
  * every named fault changes a table ('T'), a stream ('S') or the probe count ('P') in at least one case, and every case catches at least
    one fault -- printed as a matrix (pytest -s).  This is the proof that the GPU file bites: no defective kernel is ever built or run."""
import os

import numpy as np
import pytest

import static_planting as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sam-decoding_amd", "csrc")


def test_layout_restated_from_the_sources():
    com, ker, dev = (open(os.path.join(SRC, f)).read() for f in ("samd_common.h", "sam_kernels.hip", "sam_device.h"))
    for line in ("uint32_t h = (uint32_t)a * 0x9E3779B1u + (uint32_t)b * 0x85EBCA77u;", "h ^= h >> 15; h *= 0x2C1B3C6Du;", "return h ^ (h >> 13);",
                 "uint32_t h = (uint32_t)state * 0x85EBCA77u ^ ((uint32_t)tok * 0x9E3779B1u + 0x7F4A7C15u);", "h ^= h >> 16; h *= 0x2C1B3C6Du;",
                 "return (((uint32_t)tok * 0x9E3779B1u) >> 7) & (slots - 1);", "uint32_t h = (uint32_t)tok * 0x9E3779B1u; return h ^ (h >> 15);",
                 "uint32_t need = 2u * (uint32_t)(deg - SAMD_INLINE_EDGES), m = 4;", "return vocab <= 32767 ? 8 : 4;",
                 "int b = 8; while (b < 31 && ((int64_t)1 << b) - 1 < vocab) b++; return b;", "#define SAMD_EB_DISPLACED 0x80000000u",
                 "#define SAMD_BG_DISPLACED 0x20000000u", "#define SAMD_EB_IDX_MASK 0x07FFFFFFu", "#define SAMD_EB_HUB 0x08000000u",
                 "#define SAMD_EB_KIND_SHIFT 28", "#define SAMD_EB_ROOTCHILD 0x40000000u", "#define SAMD_INLINE_EDGES 5", "#define SAMD_SPILL_HEAD 3",
                 "enum { SAMD_FK_ROOT = 0, SAMD_FK_ROOTCHILD = 1, SAMD_FK_HUB = 2, SAMD_FK_STATE = 3 };",
                 "return (ref & SAMD_EB_IDX_MASK) << 2;", "return (1u << (ref >> 27)) - 1u;"):
        assert line in com, line
    for line in ("long long slots = 1024;", "while (slots < per * (long long)entries) slots <<= 1;",
                 "if (s >= 1 && nd.deg >= 2 && nd.link != 0) { m = 4; while (m < (unsigned long long)per * (unsigned)nd.deg) m <<= 1; }",
                 "off_to_ref[s] = m ? ((off_to_ref[s] >> 2) | ((uint32_t)(31 - __clz(m)) << 27)) : 0u;",
                 "if (bref[p] && L < lmax) { kind = SAMD_FK_HUB; ref = bref[p]; len = L; return; }",
                 "if (probes) blk[samd_eb_hash(t) & bmask].y |= SAMD_EB_DISPLACED;",
                 "if (h != p) atomicOr(reinterpret_cast<unsigned *>(table + h) + (W == 8 ? 1 : 2), SAMD_BG_DISPLACED);",
                 "const unsigned key = (unsigned)tok | ((unsigned)t << 15) | (lb << 30);"):
        assert line in ker, line
    for line in ("if (probes == 0 && !(e.y & SAMD_EB_DISPLACED)) return false;", "if (probes == 0 && !((W == 8 ? e.y : e.z) & SAMD_BG_DISPLACED)) break;",
                 "hit = (e.x & 0x3FFFFFFFu) == ((unsigned)a | ((unsigned)tok << 15)) && tok < 0x8000;", "len = lb < 3 ? (int)lb + 1 : (int)S.root16[a].w;",
                 "if (!f.len_ok) len = S.nodes[p_idx].length & SAMD_LEN_MASK;"):
        assert line in dev, line
    assert [P.spill_slots(d) for d in (6, 7, 8, 22, 37, 38)] == [4, 4, 8, 64, 64, 128]
    assert [P.eb_tok_bits(v) for v in (1, 255, 256, 32767, 32768, 70000, (1 << 22) - 1, 1 << 22, (1 << 22) + 1)] == [8, 8, 9, 15, 16, 17, 22, 23, 23]
    assert [P.table_slots(e, 4) for e in (0, 256, 257)] == [1024, 1024, 2048] and [P.block_slots(d, 4) for d in (2, 3, 16, 17)] == [8, 16, 64, 128]
    assert P.block_slots(32, 2) == 64 and P.block_slots(2, 2) == 4
    # scalar and vector forms agree; spot values worked by hand from the definitions
    ids = np.arange(3, 2000, dtype=np.int64)
    for fn in (P.eb_hash, lambda t: P.bigram_hash(17, t), lambda t: P.spill_hash(t, 64), lambda t: P.edge_hash(9 + 0 * t, t)):
        assert [int(v) for v in fn(ids)[:50]] == [int(fn(int(t))) for t in ids[:50]]
    assert P.eb_hash(1) == 0x9E3779B1 ^ (0x9E3779B1 >> 15) and P.spill_hash(1, 64) == (0x9E3779B1 >> 7) & 63


def test_export_tables_is_declared_and_bound():
    import samd_hip
    hdr = open(os.path.join(ROOT, "include", "samd_hip.h")).read()
    assert "int samd_static_export_tables(const samd_static_t *sam, uint32_t *h_bigram, uint32_t *h_root16, uint32_t *h_rc_bits, uint32_t *h_edge_table," in hdr
    res, args = samd_hip._PROTOS["samd_static_export_tables"]
    assert len(args) == 8 and hasattr(samd_hip.StaticAutomaton, "export_tables")


@pytest.mark.parametrize("vocab,want", [(32767, (515, 126, 32, 30, 142)), (70000, (1093, 269, 69, 63, 273))])
def test_token_search_finds_what_the_plants_need(vocab, want):
    got = tuple(len(P.tokens_homed(P.eb_hash, m, [m], vocab)) for m in (63, 255, 1023))
    got += (len(P.tokens_homed(lambda b: P.bigram_hash(17, b), 1023, [1023], vocab)), len(P.tokens_homed(lambda b: P.bigram_hash(17, b), 1023, range(1020, 1024), vocab)))
    assert got == want
    toks = P.tokens_homed(P.eb_hash, 63, [63], vocab, exclude=[P.tokens_homed(P.eb_hash, 63, [63], vocab)[0]])
    assert len(toks) == want[0] - 1 and all(P.eb_hash(t) & 63 == 63 and 3 <= t < vocab for t in toks) and toks == sorted(toks)


@pytest.mark.parametrize("name", P.CASES)
def test_plants_exist_in_the_model(name):
    print(name, P.conditions(name))
    c = P.case(name)
    assert max(max(d) for d in c.docs) == c.vocab - 1 and P.PAD not in {t for d in c.docs for t in d}
    assert max(len(s[1]) for s in P.streams(name)) <= 32 and len(P.streams(name)) <= 500


@pytest.mark.parametrize("name", P.CASES)
def test_model_tables_pass_their_own_check(name):
    c = P.case(name)
    for mode in ("blocks", "edge"):
        T = c.tables(mode)
        longest = P.check_open_table(T["bigram"], T["bigram_rows"], T["bigram_homes"], T["bigram_dword"], "bigram table")
        assert longest >= 1
        if mode == "edge":
            P.check_open_table(T["edge_table"], T["edge_rows"], T["edge_homes"], None, "edge table")
    # the keys of different threads claimed in another order are as legal
    T = c.tables("blocks")
    order = np.random.default_rng(1).permutation(len(T["bigram_rows"]))
    other = P.open_fill([T["bigram_rows"][i] for i in order], [T["bigram_homes"][i] for i in order], T["bigram_slots"], T["bigram_dword"])
    P.check_open_table(other, T["bigram_rows"], T["bigram_homes"], T["bigram_dword"])
    # and damage is seen: a duplicated key, a key outside its run, a payload word, a displaced bit too many / too few
    occ = np.flatnonzero(T["bigram"][:, 0] != P.U32)
    empty = int(np.flatnonzero(T["bigram"][:, 0] == P.U32)[len(occ) + 7])
    for damage in ("duplicate", "stray", "payload", "bit_set", "bit_clear"):
        bad = T["bigram"].copy()
        marked = [p for p in occ if bad[p, T["bigram_dword"]] & P.BG_DISPLACED]
        if damage == "duplicate":
            bad[empty] = bad[occ[0]]
        elif damage == "stray":
            bad[empty] = bad[occ[0]]; bad[occ[0]] = P.U32
        elif damage == "payload":
            bad[occ[0], 3] ^= 1
        elif damage == "bit_set":
            bad[[p for p in occ if p not in marked][0], T["bigram_dword"]] |= P.BG_DISPLACED
        elif marked:
            bad[marked[0], T["bigram_dword"]] &= ~np.uint32(P.BG_DISPLACED)
        else:
            continue
        with pytest.raises(AssertionError, match="device table != model"):
            P.check_open_table(bad, T["bigram_rows"], T["bigram_homes"], T["bigram_dword"])


@pytest.mark.parametrize("name", P.CASES)
def test_model_lookup_equals_oracle(name):
    want = P.expected(name)
    for mode, per in [(m, None) for m in P.MODES] + [("blocks", 2), ("blocks", 64), ("edge", 2)]:
        got, probes = P.model_runs(name, mode, per)
        assert got is not None and P.same_runs(got, want), (mode, per)
    assert want["one"][2] >= want["one"][0].shape[0] * want["one"][0].shape[1]


def test_every_fault_is_caught_and_every_plant_is_needed():
    M = P.fault_matrix()
    print("\n" + P.format_matrix(M))
    for f in P.FAULTS:
        hits = [n for n in P.CASES if M[n][f]]
        if f in P.UNREACHABLE:
            assert not hits, "the guard fires after all: give it a case (%s)" % hits
        else:
            assert hits, "no case notices the fault " + f
    for n in P.CASES:
        assert any(M[n].values()), "no fault needs the case " + n
    # the faults a plant is FOR
    assert all("S" in M[n]["probe_no_wrap"] and "S" in M[n]["probe_one_round"] and "P" in M[n]["bit_ignored"] for n in P.CASES)
    assert "S" in M["bigram_v32767"]["w8_no_guard"] and all("S" in M[n]["bigram_ignores_a"] for n in ("bigram_v32767", "bigram_v70000"))
    assert "T" in M["width"]["header_len_le"] and "S" in M["width"]["len_ok_ignored"]
    assert all("S" in M[n]["stale_header"] and "S" in M[n]["lb_escape_not_taken"] and "T" in M[n]["bit_on_previous_slot"] for n in ("hubs_v32767", "hubs_v70000"))
    assert all("T" in M[n]["spill_last_slot_skipped"] and "S" in M[n]["spill_last_slot_skipped"] for n in ("spill_v32767", "spill_v70000"))
    assert all("T" in M[n]["spill_head_skipped"] for n in ("hubs_v32767", "hubs_v70000"))
