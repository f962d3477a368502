#!/usr/bin/env python
"""Is the hand-scheduled part of a kernel the same in two device listings, whatever the register allocator did around it?

    python scripts/isa_regions.py OLD.s OLD_KERNEL NEW.s NEW_KERNEL [--whole] [-o report.txt]      (the report is appended to)

The listings come from hipcc <the Makefile's flags of the file> --cuda-device-only -S.  A kernel is cut at its ``sched_barrier`` comments;
the regions between the first and the last one (for conv_wgrad_wino_f32: the tile loop) are compared one by one, as sequences of
instructions with every register NUMBER masked (v12 -> v, s[20:23] -> s[4], a[252:255] -> a[4]) and labels masked: opcodes, operand
kinds, tuple widths, modifiers, immediates, offsets and wait counts must agree, in order.  Instructions that only the scalar unit sees
(s_* other than s_waitcnt / s_barrier / s_nop) are listed apart: where a loop-carried value lives is the allocator's business.  Exit
status 1 unless every region agrees."""
import argparse
import difflib
import re
import sys


def body(path, kernel):
    text = open(path).read()
    m = re.search(r"^" + re.escape(kernel) + r":.*?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
    if not m:
        sys.exit("%s: no kernel %s" % (path, kernel))
    return m.group(1).split("\n")


def mask(line):
    t = re.sub(r";.*$", "", line).strip()
    t = re.sub(r"\b([vsa])\[(\d+):(\d+)\]", lambda m: "%s[%d]" % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1), t)
    t = re.sub(r"\b([vsa])\d+\b", r"\1", t)
    t = re.sub(r"\.LBB\d+_\d+", ".L", t)
    return t


def regions(lines):
    """[[masked instruction, ...], ...]: one list per stretch between two sched_barrier comments"""
    out, cur, seen = [], None, False
    for l in lines:
        t = l.strip()
        if t.startswith("; sched_barrier"):
            if cur is not None:
                out.append(cur)
            cur, seen = [], True
            continue
        if not seen or not t or t.startswith((";", ".")) and not t.startswith(".LBB"):
            continue
        m = mask(t)
        if m:
            cur.append(m)
    return out          # what follows the last sched_barrier is not a region


def split(seq):
    scalar = lambda t: t.startswith("s_") and not t.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_cbranch", "s_branch"))
    return [t for t in seq if not scalar(t)], sorted(t.split()[0] for t in seq if scalar(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("old_kernel")
    ap.add_argument("new")
    ap.add_argument("new_kernel")
    ap.add_argument("-o", "--out")
    ap.add_argument("--whole", action="store_true", help="compare the two kernels' whole bodies instead, registers and all, with only the kernels' "
                    "own names and the function number in local labels masked (for an instantiation that was merely renamed)")
    a = ap.parse_args()
    if a.whole:
        def norm(path, kernel):
            out = []
            for l in body(path, kernel):
                t = re.sub(r";.*$", "", l).rstrip()
                if t.strip() and not t.strip().startswith((".file", ".ident", ".loc")):
                    out.append(re.sub(r"\.LBB\d+_", ".LBB_", t).replace(kernel, "KERNEL"))
            return out
        o, n = norm(a.old, a.old_kernel), norm(a.new, a.new_kernel)
        report = "%s\n  against %s\n  whole body, %d / %d lines: %s\n" % (a.old_kernel, a.new_kernel, len(o), len(n), "identical" if o == n else "DIFFERENT")
        sys.stdout.write(report)
        if a.out:
            open(a.out, "a").write(report)
        return 0 if o == n else 1
    ro, rn = regions(body(a.old, a.old_kernel)), regions(body(a.new, a.new_kernel))
    rows = ["%s\n  against %s" % (a.old_kernel, a.new_kernel), "regions between sched_barriers: %d / %d (aligned at the last one)" % (len(ro), len(rn))]
    k = min(len(ro), len(rn))       # a kernel with sched_barriers of its own in front of the loop has more regions: the loop's are the last ones
    ro, rn = ro[len(ro) - k:], rn[len(rn) - k:]
    same = k > 0
    for k, (o, n) in enumerate(zip(ro, rn)):
        (vo, so), (vn, sn) = split(o), split(n)
        mf = sum(1 for t in vn if t.startswith("v_mfma"))
        ok = vo == vn
        same &= ok
        rows.append("  region %d: %d instructions (%d MFMA) besides %d / %d scalar-unit ones: %s" % (
            k, len(vn), mf, len(so), len(sn), "same sequence" if ok else "DIFFERENT (old %d instructions)" % len(vo)))
        if so != sn:
            rows.append("    scalar-unit opcodes old: %s" % " ".join(so))
            rows.append("    scalar-unit opcodes new: %s" % " ".join(sn))
        if not ok:
            for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, vo, vn, autojunk=False).get_opcodes():
                if tag != "equal":
                    rows.append("    at %d: old [%s] new [%s]" % (i1, "; ".join(vo[i1:i2]), "; ".join(vn[j1:j2])))
    rows.append("every region the same" if same else "NOT the same")
    report = "\n".join(rows) + "\n"
    sys.stdout.write(report)
    if a.out:
        open(a.out, "a").write(report)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
