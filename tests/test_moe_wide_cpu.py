"""The wide mixture-of-experts calls without a GPU: workspace and layout arithmetic, the SAMD_E_INVALID cases and their messages (every one is
raised before any device work, so the library answers without a device), the tile bound against the Python restatement of the lists over
random routings, SAMD_MOE_PREFILL_ROWS, and the compiled k_wmoe* kernels inside libsamd_hip.so."""
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import SamdError
from samd_hip import moe as MOE
from test_codeobject_cpu import READELF, SO, gfx950_code_objects

E_INVALID = -1
F16, BF16 = samd_hip.F16, samd_hip.BF16
# word offsets of the routing part (include/samd_hip.h): n_tiles, n_active, 16 words in all; three tables of 256; 768 tile records of 3 words
ACTIVE, COUNT, OFFSET, TILE, TILE_INTS, ENTRY, MAX_ROWS, MAX_TILES = 16, 272, 528, 784, 3, 784 + 3 * 768, 4096, 768


def layout(field, rows, k):
    return samd_hip.lib().samd_moe_wide_workspace_layout(field, rows, k)


def last_error():
    return samd_hip.lib().samd_last_error().decode()


@pytest.mark.parametrize("rows,k,hidden", [(1, 1, 256), (64, 2, 256), (65, 2, 512), (160, 2, 256), (300, 8, 2048), (4096, 8, 2048)])
def test_workspace_and_layout_arithmetic(rows, k, hidden):
    L = samd_hip.lib()
    rp = -(-rows // 64) * 64
    assert MOE.wide_rows_pad(rows) == rp
    assert [layout(f, rows, k) for f in range(6)] == [ACTIVE, COUNT, OFFSET, TILE, TILE_INTS, ENTRY]
    assert (layout(8, rows, k), layout(9, rows, k), layout(10, rows, k)) == (MAX_ROWS, MAX_TILES, -1)
    words = ENTRY + rp * k
    y_off = -(-4 * words // 256) * 256
    assert layout(6, rows, k) == words and layout(7, rows, k) == y_off
    for dt in (F16, BF16):
        assert L.samd_moe_wide_workspace(rows, hidden, 256, 8, k, dt) == y_off + rp * k * hidden * 2
    # the table holds the bound of the largest launch, and the bound of this one
    assert MOE.wide_tile_bound(rows, 256, k) <= MAX_TILES == 256 + MAX_ROWS * 8 // 64
    assert MOE.wide_tile_bound(rows, 8, k) == min(8, rp * k) + rp * k // 64


def test_the_narrow_workspace_is_untouched():
    L = samd_hip.lib()
    assert [L.samd_moe_workspace_layout(f) for f in range(6)] == [16, 272, 528, 64, 528 + 256 * 64, -1]
    assert L.samd_moe_workspace(64, 512, 8, 2, F16) == -(-4 * (528 + 256 * 64) // 256) * 256 + 64 * 2 * 512 * 2


def _calls(rows=64, hidden=256, inter=256, E=8, k=2, fmt=0, dt=F16, p=1):
    """every wide entry point with the given scalars; p: a non-null dummy for every pointer (never dereferenced: the checks come first)"""
    L = samd_hip.lib()
    P = lambda: p or None
    return {
        "samd_moe_wide_workspace": (lambda: L.samd_moe_wide_workspace(rows, hidden, inter, E, k, dt)) if fmt == 0 and p else None,
        "samd_moe_wide_route": (lambda: L.samd_moe_wide_route(P(), P(), P(), rows, hidden, E, k, 1, P(), P(), dt, None)) if fmt == 0 and inter == 256 else None,
        "samd_moe_wide_lists": (lambda: L.samd_moe_wide_lists(P(), P(), rows, E, k, P(), None)) if fmt == 0 and inter == 256 and hidden == 256 and dt == F16 else None,
        "samd_moe_wide_gate_up_silu": lambda: L.samd_moe_wide_gate_up_silu(P(), P(), P(), rows, hidden, inter, E, k, fmt, P(), dt, None),
        "samd_moe_wide_down_combine": lambda: L.samd_moe_wide_down_combine(P(), P(), P(), P(), P(), P(), rows, hidden, inter, E, k, fmt, P(), dt, None),
    }


@pytest.mark.parametrize("kw,text", [
    (dict(rows=0), "rows 0 outside 1 .. 4096"),
    (dict(rows=-5), "rows -5 outside 1 .. 4096"),
    (dict(rows=4097), "rows 4097 outside 1 .. 4096"),
    (dict(fmt=4), "unknown expert_format 4"),
    (dict(fmt=-1), "unknown expert_format -1"),
    (dict(hidden=300), "unsupported shape"),
    (dict(inter=128), "unsupported shape"),
    (dict(E=257), "unsupported shape"),
    (dict(E=0), "unsupported shape"),
    (dict(k=9, E=16), "unsupported shape"),
    (dict(k=4, E=2), "unsupported shape"),
    (dict(dt=2), "unsupported shape"),
    (dict(fmt=3, hidden=16640), "unsupported shape"),
    (dict(p=0), "null pointer"),
])
def test_invalid_arguments_are_refused_with_their_message_before_any_device_work(kw, text):
    ran = 0
    for name, call in _calls(**kw).items():
        if call is None:                                          # the call does not take the argument under test
            continue
        assert call() == E_INVALID, (name, kw)
        msg = last_error()
        assert msg.startswith(name + ": ") and text in msg, (name, msg)
        ran += 1
    assert ran >= 2


def test_rows_come_first_then_the_format_then_the_shape_then_the_pointers():
    L = samd_hip.lib()
    assert L.samd_moe_wide_gate_up_silu(None, None, None, 0, 300, 256, 8, 2, 9, None, F16, None) == E_INVALID and "rows 0" in last_error()
    assert L.samd_moe_wide_gate_up_silu(None, None, None, 64, 300, 256, 8, 2, 9, None, F16, None) == E_INVALID and "expert_format 9" in last_error()
    assert L.samd_moe_wide_gate_up_silu(None, None, None, 64, 300, 256, 8, 2, 1, None, F16, None) == E_INVALID and "unsupported shape" in last_error()
    assert L.samd_moe_wide_gate_up_silu(None, None, None, 64, 256, 256, 8, 2, 1, None, F16, None) == E_INVALID and "null pointer" in last_error()
    assert MOE.WIDE_FORMAT_CODES == {None: 0, "mxfp4": 1, "int4g128": 2, "fp8b128": 3} and set(MOE.WIDE_FORMAT_CODES) == set(MOE.EXPERT_FORMATS_KNOWN)


def test_wide_buffers_refuse_bad_rows_without_a_device():
    with pytest.raises(SamdError, match="rows 5000 outside"):
        MOE.MoeWideBuffers(5000, 256, 256, 8, 2, torch.float16, F16, "cpu")
    with pytest.raises(SamdError, match="unsupported shape"):
        MOE.MoeWideBuffers(64, 256, 300, 8, 2, torch.float16, F16, "cpu")


def brute_lists(idx, n, E):
    """the rule, entry by entry: {expert: [p, ...]}"""
    per = {}
    for p in range(min(n, idx.shape[0]) * idx.shape[1]):
        r, j = divmod(p, idx.shape[1])
        e = int(idx[r, j])
        if 0 <= e < E and e not in idx[r, :j].tolist():
            per.setdefault(e, []).append(p)
    return per


def test_the_reference_lists_and_their_tile_count_stay_inside_the_grid_bound():
    rng = np.random.default_rng(0)
    for trial in range(300):
        E, k = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        k = min(k, E)
        rows = int(rng.integers(1, 200))
        n = int(rng.integers(0, rows + 1))
        kind = trial % 4
        if kind == 0:                                             # distinct experts per row
            idx = np.stack([rng.permutation(E)[:k] for _ in range(rows)])
        elif kind == 1:                                           # skewed: most rows on few experts, repetitions allowed
            idx = np.minimum(rng.geometric(0.4, (rows, k)) - 1, E - 1)
        elif kind == 2:                                           # anything, out-of-range values included
            idx = rng.integers(-2, E + 3, (rows, k))
        else:                                                     # every row the same experts: the longest lists
            idx = np.tile(np.arange(k), (rows, 1))
        ref = MOE.wide_lists_reference(torch.from_numpy(idx), n, E)
        per = brute_lists(idx, n, E)
        assert ref["active"] == sorted(per) and ref["counts"] == [len(per[e]) for e in ref["active"]]
        assert ref["entries"] == [p for e in ref["active"] for p in per[e]]
        assert ref["offsets"] == [int(x) for x in np.cumsum([0] + ref["counts"][:-1])][:len(ref["active"])]
        # the tiles: one expert's adjacent, 64 entries each but the last, covering the entries once and in order
        assert len(ref["tiles"]) == sum(-(-c // 64) for c in ref["counts"])
        assert [p for e, first, c in ref["tiles"] for p in ref["entries"][first:first + c]] == ref["entries"]
        assert all(1 <= c <= 64 and e == ref["active"][max(a for a, o in enumerate(ref["offsets"]) if o <= first)] for e, first, c in ref["tiles"])
        assert len(ref["tiles"]) <= MOE.wide_tile_bound(rows, E, k), (E, k, rows, n, len(ref["tiles"]))
        assert len(ref["entries"]) <= MOE.wide_rows_pad(rows) * k


def test_one_entry_over_a_tile_per_expert_takes_two_tiles_each():
    """E experts of 65 entries each: 2 E tiles, where entries / 64 alone (rounded down per expert) would promise E; the bound adds the E"""
    E, k, rows = 8, 8, 65
    ref = MOE.wide_lists_reference(np.tile(np.arange(k), (rows, 1)).tolist(), rows, E)
    assert len(ref["tiles"]) == 2 * E and MOE.wide_tile_bound(rows, E, k) == E + 128 * k // 64


@pytest.mark.parametrize("raw,want", [(None, 4096), ("", 4096), ("128", 128), ("4096", 4096), ("1024", 1024), (256, 256)])
def test_prefill_rows_are_parsed(monkeypatch, raw, want):
    monkeypatch.delenv(MOE.PREFILL_ROWS_ENV, raising=False)
    if isinstance(raw, str):
        monkeypatch.setenv(MOE.PREFILL_ROWS_ENV, raw)
        assert MOE.prefill_rows() == want
    else:
        assert MOE.prefill_rows(raw) == want


@pytest.mark.parametrize("raw", ["100", "64", "0", "-128", "4160", "8192", "12x", "1e3", "130"])
def test_prefill_rows_outside_the_range_are_rejected(monkeypatch, raw):
    monkeypatch.setenv(MOE.PREFILL_ROWS_ENV, raw)
    with pytest.raises(SamdError, match=MOE.PREFILL_ROWS_ENV):
        MOE.prefill_rows()


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_wide_kernels_are_in_the_library_and_use_no_scratch(tmp_path):
    """the 64-row tile of each of the four expert formats, gate|up and down, both dtypes, and the list builder; a kernel with hand-issued
    loads and counted waits must not spill; each keeps the registers and the static LDS of the 64-row kernel it restates"""
    kernels = {}
    for i, co in enumerate(gfx950_code_objects(open(SO, "rb").read())):
        path = tmp_path / f"co{i}.elf"
        path.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"), vgprs=get("vgpr_count"),
                                 static_lds=get("group_segment_fixed_size"))
    wide = {n: v for n, v in kernels.items() if "k_wmoe" in n}
    assert len(wide) == 17 and len([n for n in wide if "k_wmoe_lists" in n]) == 1, sorted(wide)
    assert not {n: v for n, v in wide.items() if v["scratch"] or v["vgpr_spills"]}
    twins = {"k_wmoe_gu": "k_moe_gate_up_silu", "k_wmoe_dn": "k_moe_down", "k_wmoe4_gu": "k_moe4_gate_up_silu", "k_wmoe4_dn": "k_moe4_down",
             "k_wmoe_i4_gu": "k_moe_i4_gate_up_silu", "k_wmoe_i4_dn": "k_moe_i4_down", "k_wmoe8_gu": "k_moe8_gate_up_silu", "k_wmoe8_dn": "k_moe8_down"}
    for new, old in twins.items():
        for tt in ("4GF16", "5GBF16"):
            a = [v for n, v in wide.items() if re.search(rf"\d+{new}I{tt}E", n)]
            b = [v for n, v in kernels.items() if re.search(rf"\d+{old}I{tt}Li4E", n)]
            assert len(a) == len(b) == 1, (new, old, tt)
            assert a[0]["static_lds"] == b[0]["static_lds"] and a[0]["vgprs"] <= b[0]["vgprs"] + 2, (new, a, b)
