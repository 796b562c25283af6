"""Static check on the compiled MXFP4 kernels inside libsamd_hip.so (no GPU needed).

k_gemm_skinny_f4 issues its weight and scale loads by hand and waits with counted `s_waitcnt vmcnt(N)`, so the compiler does not know when a
destination register holds its data.  A `v_mov` that reads such a register between the issue and the wait moves stale bits, and the landing
load then overwrites whatever the allocator has put there since -- met while this kernel was written: a short split's skipped prologue load
was merged with the loaded value by register copies, and the 64-row tile faulted.  The destinations are therefore in-out operands of one
value each; this test keeps it so: in the prologue of every instantiation (first hand-issued load to the first barrier, where the copies
appeared) no v_mov touches a load destination."""
import os
import re
import subprocess

import pytest

from test_codeobject_cpu import SO, gfx950_code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


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
            if "k_gemm_skinny_f4" not in head:
                continue
            found += 1
            body = [l.split("//")[0].strip() for l in chunk.split("\n")[1:]]
            dests, load_at = set(), []
            for i, l in enumerate(body):
                m = re.match(r"global_load_dwordx4 v\[(\d+):(\d+)\]", l)
                if m:
                    dests |= set(range(int(m.group(1)), int(m.group(2)) + 1))
                    load_at.append(i)
                m = re.match(r"global_load_ushort v(\d+)", l)
                if m:
                    dests.add(int(m.group(1)))
            assert len(load_at) >= 4, head
            bad = []
            barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier") and i > load_at[0])
            for i in range(load_at[0], barrier):                         # the prologue: first hand-issued load to the first phase's barrier
                m = re.match(r"v_mov_b32_e32 v(\d+), (?:v(\d+))?", body[i])
                if m and (int(m.group(1)) in dests or (m.group(2) is not None and int(m.group(2)) in dests)):
                    bad.append(body[i])
            assert not bad, f"{head}: register copies of hand-issued load destinations: {bad[:8]}"
    assert found == 8, f"expected the 8 instantiations of k_gemm_skinny_f4 (2 dtypes x 4 row tiles), found {found}"
