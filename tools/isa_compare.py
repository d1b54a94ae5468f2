#!/usr/bin/env python3
"""Compare the gfx950 assembly of the tile kernels before and after a source-only change, kernel by kernel.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S old/tavb_mfma.hip -o old.s        (and one .s per new file)
    python tools/isa_compare.py old.s new_wide.s new_skinny.s new_select.s [--diff 'mfma_scan_kernel<0,4,8,6,4,false,false,true>']

One line per kernel of the first file: `same`, `differs (N lines)` or `missing`, then any kernel only the new files have.  A file is cut
into kernels at their function labels (label .. .Lfunc_end) and kernels are matched by name and template arguments, read off the mangled
symbol.  Before the comparison symbol names, the function index of local labels (.LBB<n>_<m>, .Lfunc_end<n>) and comments are
normalised away; the instructions are compared as text, nothing is searched for.  Of the kernel descriptor the register, LDS and scratch
fields are compared (DESCRIPTOR): a change there is reported even when it is the only one.  Exit status 1 when a kernel is missing.
"""
import argparse
import difflib
import re
import sys

DESCRIPTOR = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
# template arguments of the OLD side that the new side no longer has: kernel name -> argument index.  (skinny_scan_kernel lost ABL two
# changes ago: {"skinny_scan_kernel": 3} compares against a parent that still has it.)
DROPPED_ARGS = {}
# template arguments the NEW side gained at the end of the list, and the value that names the old kernel: kernel name -> (arguments the old side
# has, value).  (skinny_scan_kernel gained MASKED in the last change: {"skinny_scan_kernel": (6, "false")} compares against a parent without it.
# The 128/256-query kernel's masked form is a kernel of its own, mfma_scan_masked_kernel: mfma_scan_kernel's names did not change.)
ADDED_ARGS = {}

def kernel_id(symbol):
    """'_ZN4tavb12_GLOBAL__N_116mfma_scan_kernelILi0ELi4E...EEvNS0_...' -> ('mfma_scan_kernel', ['0', '4', ...])"""
    pos, name = symbol.index("N") + 1, None
    while symbol[pos].isdigit():  # nested name: <length><identifier> ...
        m = re.match(r"\d+", symbol[pos:])
        n = int(m.group())
        name = symbol[pos + m.end() : pos + m.end() + n]
        pos += m.end() + n
    args = []
    if symbol[pos] == "I":
        pos += 1
        while symbol[pos] != "E":
            pack = re.match(r"J(PKj)?E", symbol[pos:])  # a trailing parameter pack (the mask argument of skinny_scan_kernel): says nothing MASKED does not
            if pack is not None:
                pos += pack.end()
                continue
            pack = re.match(r"JNS\d*_(\d+)", symbol[pos:])  # ... unless it is a struct (ScopePlanes: the per-query mode of MASKED = true), which names the mode
            if pack is not None:
                start = pos + pack.end()
                args.append(symbol[start : start + int(pack.group(1))])
                pos = start + int(pack.group(1)) + 2  # the struct's and the pack's closing E
                continue
            m = re.match(r"Li(\d+)E|Ln(\d+)E|Lb([01])E|(f)|(DF16_)", symbol[pos:])
            if m is None:
                raise ValueError(f"template argument not understood at {symbol[pos:]!r}")
            i, neg, b, f32, f16 = m.groups()
            args.append(i if i is not None else "-" + neg if neg is not None else ("false", "true")[int(b)] if b is not None else "float" if f32 else "_Float16")
            pos += m.end()
    return name, args


def kernels(path, old_side):
    """{display name: (normalised instruction lines, {descriptor field: value})}"""
    out, lines = {}, open(path).read().split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"(_Z\w+):", lines[i])
        if m is None:
            i += 1
            continue
        symbol, body, desc = m.group(1), [], {}
        i += 1
        while not lines[i].startswith(".Lfunc_end"):
            line = lines[i].split(";")[0].rstrip()
            i += 1
            d = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", line)
            if d is not None:
                if d.group(1) in DESCRIPTOR:
                    desc[d.group(1)] = d.group(2)
                continue
            if not line.strip() or re.match(r"\s*\.(section|text|p2align|end_amdhsa_kernel)\b", line):
                continue
            line = line.replace(symbol, "KERNEL")
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        name, args = kernel_id(symbol)
        if old_side and name in DROPPED_ARGS and len(args) > ADDED_ARGS.get(name, (len(args),))[0]:
            del args[DROPPED_ARGS[name]]
        if not old_side and name in ADDED_ARGS and len(args) == ADDED_ARGS[name][0] + 1 and args[-1] == ADDED_ARGS[name][1]:
            del args[-1]
        out[name + ("<" + ",".join(args) + ">" if args else "")] = (body, desc)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old", help="assembly of the parent's file")
    ap.add_argument("new", nargs="+", help="assembly of the files that replace it")
    ap.add_argument("--diff", metavar="KERNEL", help="also print the unified diff of this kernel's normalised instructions")
    a = ap.parse_args()
    old, new = kernels(a.old, True), {}
    for path in a.new:
        new.update(kernels(path, False))
    missing = 0
    for k, (body, desc) in old.items():
        if k not in new:
            print(f"{k}: missing")
            missing += 1
            continue
        nbody, ndesc = new[k]
        changed = [ln for ln in difflib.unified_diff(body, nbody, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
        fields = [f"{f} {desc.get(f)} -> {ndesc.get(f)}" for f in DESCRIPTOR if desc.get(f) != ndesc.get(f)]
        verdict = f"differs ({len(changed)} lines)" if changed or fields else "same"
        print(f"{k}: {verdict}" + (" [" + ", ".join(fields) + "]" if fields else ""))
        if a.diff == k:
            print("\n".join(difflib.unified_diff(body, nbody, "old", "new", lineterm="")))
    for k in new:
        if k not in old:
            print(f"{k}: only in the new files")
    print(f"{len(old)} kernels in {a.old}, {len(new)} in the new files, {missing} missing")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
