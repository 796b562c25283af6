"""Static checks on the compiled INT8 kernels inside libsamd_hip.so (no GPU needed): the sibling of test_int4_codeobject_cpu.py.

k_gemm_skinny_i8 issues its code and group-data loads by hand and waits with counted `s_waitcnt vmcnt(N)`, so the compiler does not know
when a destination register holds its data.  Two things keep that safe, and both are read off the code object here:
  * no register copy (`v_mov`) touches a hand-issued load's destination in the prologue of any instantiation (first load to first barrier,
    where a short split's skipped loads would be merged with loaded values by copies);
  * no instantiation has a private segment: a spilled destination would be stored to scratch before its data has landed."""
import os
import re
import subprocess

import pytest

from test_codeobject_cpu import READELF, SO, gfx950_code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "k_gemm_skinny_i8"


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_no_register_copy_touches_an_in_flight_load_destination(tmp_path):
    blob = open(SO, "rb").read()
    found = 0
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        text = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
        for chunk in re.split(r"\n(?=[0-9a-f]+ <)", text):
            head = chunk.split("\n", 1)[0]
            if KERNEL not in head:
                continue
            found += 1
            body = [l.split("//")[0].strip() for l in chunk.split("\n")[1:]]
            dests, load_at, group_loads = set(), [], 0
            for i, l in enumerate(body):
                m = re.match(r"global_load_dwordx([42]) v\[(\d+):(\d+)\]", l)
                if m:
                    dests |= set(range(int(m.group(2)), int(m.group(3)) + 1))
                    if m.group(1) == "4":
                        load_at.append(i)
                    else:
                        group_loads += 1
            assert len(load_at) >= 8 and group_loads >= 2, head
            barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier") and i > load_at[0])
            bad = []
            for i in range(load_at[0], barrier):                         # the prologue: first hand-issued load to the first phase's barrier
                m = re.match(r"v_mov_b32_e32 v(\d+), (?:v(\d+))?", body[i])
                if m and (int(m.group(1)) in dests or (m.group(2) is not None and int(m.group(2)) in dests)):
                    bad.append(body[i])
            assert not bad, f"{head}: register copies of hand-issued load destinations: {bad[:8]}"
    assert found == 8, f"expected the 8 instantiations of {KERNEL} (2 dtypes x 4 row tiles), found {found}"


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_no_instantiation_uses_scratch(tmp_path):
    blob = open(SO, "rb").read()
    kernels = {}
    for k, co in enumerate(gfx950_code_objects(blob)):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split(".name:")[1:]:
            name = block.split()[0]
            if KERNEL not in name:
                continue
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"), vgprs=get("vgpr_count"))
    for name, v in sorted(kernels.items()):
        print(name, v)
    assert len(kernels) == 8, f"expected the 8 instantiations of {KERNEL}, found {sorted(kernels)}"
    bad = {n: v for n, v in kernels.items() if v["scratch"] or v["vgpr_spills"]}
    assert not bad, f"kernels with hand-issued loads must not spill: {bad}"
