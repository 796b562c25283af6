#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of one HIP source kernel by kernel: `asm_compare.py parent.s new.s`, both from
`hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S`.

A kernel is IDENTICAL if its instructions (comments, directives and label numbers stripped) are the same text; EQUIVALENT if it has the
same instruction count, the same opcode histogram, the same ordered sequence of memory, LDS, MFMA, s_waitcnt (operands included), barrier
and branch instructions, and the same register, LDS, scratch and spill figures in the metadata -- registers may be numbered differently
and independent scalar / VALU instructions may be ordered differently; anything else FAILS.  Exit status 1 if a kernel fails or the two
sets of kernel names differ.  Kernels whose names match a regular expression given with --may-differ may be EQUIVALENT; every other kernel
has to be IDENTICAL."""
import collections
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")
ORDERED = re.compile(r"^(global_|buffer_|ds_|v_mfma|s_waitcnt|s_barrier|s_load|s_buffer_load|s_cbranch|s_branch)")
MODIFIER = re.compile(r"\boffset:\d+|\bnt\b|\bsc[01]\b|\blds\b")


def kernels(path):
    text = open(path).read()
    meta = {}
    for rec in text[text.index("amdhsa.kernels:"):].split("\n  - ")[1:]:
        fields = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)$", rec, flags=re.M))
        if ".name" in fields and ".symbol" in fields:
            meta[fields[".name"]] = tuple(fields[k] for k in META)
    out = {}
    for name in meta:
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), text, flags=re.S | re.M).group(1)
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in body.split("\n") if re.match(r"\t[a-z]", l)]
        out[name] = (ins, meta[name])
    return out


def ordered(ins):
    seq = []
    for i in ins:
        op = i.split()[0]
        if ORDERED.match(op):
            seq.append(i if op == "s_waitcnt" else " ".join([op] + MODIFIER.findall(i)))
    return seq


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--may-differ=")]
    may = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--may-differ=")]
    a, b = kernels(args[0]), kernels(args[1])
    bad = sorted(set(a) ^ set(b))
    for n in bad:
        print("ONLY IN %s: %s" % ("parent" if n in a else "new", n))
    tally = collections.Counter()
    for n in sorted(set(a) & set(b)):
        (ia, ma), (ib, mb) = a[n], b[n]
        if ia == ib and ma == mb:
            tally["identical"] += 1
            continue
        ops = lambda ins: collections.Counter(i.split()[0] for i in ins)
        same = len(ia) == len(ib) and ops(ia) == ops(ib) and ordered(ia) == ordered(ib) and ma == mb
        ok = same and any(re.search(p, n) for p in may)
        tally["equivalent" if ok else "FAILED"] += 1
        print("%s %s: %d / %d instructions, metadata %s / %s" % ("equivalent" if ok else "FAILED", n, len(ia), len(ib), ma, mb))
    print("%d kernels: %d identical, %d equivalent (register numbering / order of independent instructions), %d failed, %d unmatched names"
          % (len(set(a) | set(b)), tally["identical"], tally["equivalent"], tally["FAILED"], len(bad)))
    return 1 if bad or tally["FAILED"] else 0


if __name__ == "__main__":
    sys.exit(main())
