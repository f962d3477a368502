#!/usr/bin/env python
"""Are the device listings of two source trees the same, kernel by kernel?  For refactors that must not move an instruction.

    python scripts/isa_same.py OLD_CSRC NEW_CSRC [file.hip ...] [-o report.txt]

Compiles every file (default: every entry of SRCS in either tree's Makefile) of both directories with the flags its Makefile gives that
file plus --cuda-device-only -S, drops comment lines, .file / .ident / .loc and the per-translation-unit __hip_cuid_ symbol, and prints
per kernel: mangled name, sgpr / vgpr / spilled-vgpr counts of the metadata, instructions, "identical" or "DIFFERENT".  A source that
only one tree has counts as one without kernels in the other.  Kernels are compared as a set and the rest of a listing as a bag of
lines: another order of instantiation is reported as that.  Exit status 1 unless every file has the same kernels, each identical, and
the same lines.  A kernel that one file lost and another gained is also compared across the move ("moved from ... to ...").

--sub-new REGEX REPL (repeatable) rewrites every line of the NEW tree's listings before the comparison: a kernel that gained a template
parameter has another mangled name, and with its default value's suffix taken out again (e.g. 'ELb0EEv9WgradArgs' 'EEv9WgradArgs') the
instantiations that existed before are compared with their old selves; the ones that are new stay listed as "only in the new tree"."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

def makefile(csrc):
    """SRCS of csrc/Makefile and a function name -> the CXXFLAGS of that file (the target-specific additions included)"""
    text = open(os.path.join(csrc, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", text, re.M).group(1).split()
    base = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    extra = {}
    for objs, more in re.findall(r"^((?:build/\w+\.o\s*)+):\s*CXXFLAGS\s*\+=\s*(.*)$", text, re.M):
        for o in objs.split():
            extra.setdefault(os.path.basename(o)[:-2] + ".hip", []).extend(more.split())
    return srcs, lambda name: base + extra.get(name, [])


def listing(csrc, name, tmp, subs=()):
    if not os.path.exists(os.path.join(csrc, name)):
        return []
    out = os.path.join(tmp, name + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *makefile(csrc)[1](name), "--cuda-device-only", "-S", name, "-o", out], cwd=csrc, check=True)
    keep = []
    for l in open(out):
        t = l.strip()
        if t.startswith(";") or t.startswith((".file", ".ident", ".loc")) or "__hip_cuid_" in l:
            continue
        for pat, repl in subs:
            l = re.sub(pat, repl, l)
        keep.append(l.rstrip())
    return keep


def kernels(lines):
    """mangled name -> (body lines, metadata dict) of every kernel in a normalised listing"""
    text = "\n".join(lines)
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"^    \.(name|sgpr_count|vgpr_count|vgpr_spill_count):\s+(\S+)", blk, re.M))
        meta[f["name"]] = f
    res = {}
    for name in meta:           # label .. .Lfunc_end: the instructions and the kernel descriptor
        m = re.search(r"^" + re.escape(name) + r":.*?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        # (.LBB<f>_<n>, and BB<f>_<n> in the loop comments: f is the function's ordinal in its file -- an instantiation added or taken away
        # in front renumbers the labels, not the code)
        res[name] = (re.sub(r"BB\d+_", "BB_", m.group(1)).split("\n"), meta[name])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="*")
    ap.add_argument("-o", "--out")
    ap.add_argument("--sub-new", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    args = ap.parse_args()
    if not args.files:
        old_srcs, new_srcs = makefile(args.old)[0], makefile(args.new)[0]
        args.files = new_srcs + [f for f in old_srcs if f not in new_srcs]
    rows, same, gone, came = [], True, {}, {}          # gone, came: kernel -> (file, kernel) of those only one tree has in that file
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        with concurrent.futures.ThreadPoolExecutor(8) as ex:          # the compiles run side by side
            jobs = [(ex.submit(listing, args.old, name, ta), ex.submit(listing, args.new, name, tb, args.sub_new)) for name in args.files]
        for name, (ja, jb) in zip(args.files, jobs):
            la, lb = ja.result(), jb.result()
            ka, kb = kernels(la), kernels(lb)
            whole = "identical" if la == lb else "the same lines in another order" if sorted(la) == sorted(lb) else "DIFFERENT"
            if la and lb:
                rows.append("%s: %d kernels, whole listing %s" % (name, len(kb), whole))
                same &= sorted(la) == sorted(lb) and all(k in ka and k in kb and ka[k] == kb[k] for k in set(ka) | set(kb))
            else:
                rows.append("%s (only in the %s tree): %d kernels" % (name, "old" if la else "new", len(ka) + len(kb)))
                same &= not ka and not kb
            for k in sorted(set(ka) | set(kb)):
                if k not in ka or k not in kb:
                    (gone if k in ka else came)[k] = (name, (ka if k in ka else kb)[k])
                    body, f = (ka if k in ka else kb)[k]
                    rows.append("  %s\n    sgpr %s vgpr %s vgpr_spill %s instructions %d  only in the %s tree" % (
                        k, f["sgpr_count"], f["vgpr_count"], f["vgpr_spill_count"],
                        sum(1 for l in body if l.startswith("\t") and not l.strip().startswith(".")), "old" if k in ka else "new"))
                    continue
                body, f = kb[k]
                ninstr = sum(1 for l in body if l.startswith("\t") and not l.strip().startswith("."))
                verdict = "identical" if ka[k] == kb[k] else "DIFFERENT (old: sgpr %s vgpr %s spill %s)" % (
                    ka[k][1]["sgpr_count"], ka[k][1]["vgpr_count"], ka[k][1]["vgpr_spill_count"])
                rows.append("  %s\n    sgpr %s vgpr %s vgpr_spill %s instructions %d  %s" % (
                    k, f["sgpr_count"], f["vgpr_count"], f["vgpr_spill_count"], ninstr, verdict))
    for k in sorted(set(gone) & set(came)):          # a kernel that changed files is compared with itself across the move
        rows.append("moved from %s to %s: %s\n    %s" % (gone[k][0], came[k][0], k, "identical" if gone[k][1] == came[k][1] else "DIFFERENT"))
    report = ("device listings (hipcc <the Makefile's CXXFLAGS of each file> --cuda-device-only -S), normalised, old tree against new\n"
              + "".join("new tree's lines rewritten: s/%s/%s/\n" % tuple(sr) for sr in args.sub_new) + "\n".join(rows)
              + "\n%s\n" % ("every kernel identical" if same else "NOT the same"))
    sys.stdout.write(report)
    if args.out:
        open(args.out, "w").write(report)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
