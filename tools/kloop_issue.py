#!/usr/bin/env python3
"""Instruction mix of the steady-state K step of the wide tile kernels, read off the gfx950 assembly.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S typeagent_py_amd/csrc/tavb_mfma_wide.hip -o wide.s
    python tools/kloop_issue.py wide.s ['mfma_scan_kernel<0,4,8,6,4,false,false,true>' ...] [--list] [--dump KERNEL]

The K step is the innermost loop of a kernel that holds MFMAs (the `#pragma unroll 1` loop of mfma_scan_kernel): the shortest span between
a label and a backward branch to it with at least one v_mfma inside.  Its instructions are counted by issue class, for the whole step and
per quarter (a quarter starts at its first MFMA; what stands in front of the first MFMA of the step counts to quarter 0).  Output is a
markdown table per kernel (profiles/r12_kloop_issue.md).  Without kernel names: every mfma_scan_kernel instantiation, whole step only.
"""
import argparse
import re
import sys

from isa_compare import kernels

CLASSES = ("MFMA", "ds_read", "buffer_load lds", "v_readlane / v_writelane", "v_readfirstlane", "other VALU", "SALU", "s_waitcnt / s_nop", "other")


def classify(line):
    op = line.split()[0]
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith(("ds_read", "ds_load")):
        return "ds_read"
    if op.startswith("buffer_load") and re.search(r"\blds\b", line):
        return "buffer_load lds"
    if op.startswith(("v_readlane", "v_writelane")):
        return "v_readlane / v_writelane"
    if op.startswith("v_readfirstlane"):
        return "v_readfirstlane"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "s_waitcnt / s_nop"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def k_step(body):
    """the instruction lines of the innermost loop that holds MFMAs, or None"""
    label_at = {}
    best = None
    for i, line in enumerate(body):
        m = re.match(r"(\.LBB_\d+):", line)
        if m:
            label_at[m.group(1)] = i
            continue
        m = re.match(r"\s*s_cbranch_\w+\s+(\.LBB_\d+)|\s*s_branch\s+(\.LBB_\d+)", line)
        if m:
            target = m.group(1) or m.group(2)
            if target in label_at:  # backward
                span = [ln for ln in body[label_at[target] : i + 1] if not re.match(r"\.LBB_\d+:", ln) and ln.strip()]
                if any(ln.split()[0].startswith("v_mfma") for ln in span) and (best is None or len(span) < len(best)):
                    best = span
    return best


def table(name, span, per_quarter):
    n_mfma = sum(1 for ln in span if ln.split()[0].startswith("v_mfma"))
    qm = n_mfma // 4 if n_mfma % 4 == 0 else n_mfma
    cols = [dict.fromkeys(CLASSES, 0) for _ in range(4)]
    seen = 0
    for ln in span:
        c = classify(ln)
        if c == "MFMA":
            seen += 1
        q = min(3, max(0, (seen - 1) // qm)) if seen else 0
        cols[q][c] += 1
    out = [f"`{name}`: {len(span)} instructions, {n_mfma} MFMAs", ""]
    if per_quarter:
        out += ["| class | q0 | q1 | q2 | q3 | step |", "|---|---|---|---|---|---|"]
        for c in CLASSES:
            out.append(f"| {c} | " + " | ".join(str(col[c]) for col in cols) + f" | {sum(col[c] for col in cols)} |")
        out.append("| all | " + " | ".join(str(sum(col.values())) for col in cols) + f" | {len(span)} |")
    else:
        out += ["| " + " | ".join(CLASSES) + " |", "|" + "---|" * len(CLASSES), "| " + " | ".join(str(sum(col[c] for col in cols)) for c in CLASSES) + " |"]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", nargs="*")
    ap.add_argument("--list", action="store_true", help="print the kernel names of the file")
    ap.add_argument("--dump", metavar="KERNEL", help="print the K step of this kernel, one instruction per line")
    a = ap.parse_args()
    ks = kernels(a.asm, False)
    if a.list:
        print("\n".join(ks))
        return 0
    if a.dump:
        print("\n".join(k_step(ks[a.dump][0])))
        return 0
    for name in a.kernel or [k for k in ks if k.startswith("mfma_scan_kernel")]:
        span = k_step(ks[name][0])
        if span is None:
            print(f"`{name}`: no loop with MFMAs\n")
            continue
        print(table(name, span, bool(a.kernel)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
