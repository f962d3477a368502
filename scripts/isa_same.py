#!/usr/bin/env python
"""Are the device listings of two source trees the same, kernel by kernel?  For refactors of the Winograd kernels, which must not move
an instruction.

    python scripts/isa_same.py OLD_CSRC NEW_CSRC [file.hip ...] [-o report.txt]

Compiles every file (default: the four Winograd sources) of both directories with the Makefile's flags for them plus
--cuda-device-only -S, drops comment lines, .file / .ident / .loc and the per-translation-unit __hip_cuid_ symbol, and prints per
kernel: mangled name, sgpr / vgpr / spilled-vgpr counts of the metadata, instructions, "identical" or "DIFFERENT".  Exit status 1
unless the whole normalised listings are equal."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

FILES = ["conv_wino.hip", "conv_wino_res.hip", "conv_wino_ring.hip", "conv_wgrad_wino.hip"]
FLAGS = "-O3 -fPIC -std=c++17 --offload-arch=gfx950 -Wall -Wno-unused-result -ffp-contract=off -fno-slp-vectorize".split()


def listing(csrc, name, tmp):
    out = os.path.join(tmp, name + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *FLAGS, "--cuda-device-only", "-S", name, "-o", out], cwd=csrc, check=True)
    keep = []
    for l in open(out):
        t = l.strip()
        if t.startswith(";") or t.startswith((".file", ".ident", ".loc")) or "__hip_cuid_" in l:
            continue
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
        res[name] = (m.group(1).split("\n"), meta[name])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="*", default=FILES)
    ap.add_argument("-o", "--out")
    args = ap.parse_args()
    rows, same = [], True
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        with concurrent.futures.ThreadPoolExecutor(8) as ex:          # the compiles run side by side
            jobs = [(ex.submit(listing, args.old, name, ta), ex.submit(listing, args.new, name, tb)) for name in args.files]
        for name, (ja, jb) in zip(args.files, jobs):
            la, lb = ja.result(), jb.result()
            ka, kb = kernels(la), kernels(lb)
            rows.append("%s: %d kernels, whole listing %s" % (name, len(kb), "identical" if la == lb else "DIFFERENT"))
            same &= la == lb and sorted(ka) == sorted(kb)
            for k in sorted(set(ka) | set(kb)):
                if k not in ka or k not in kb:
                    rows.append("  %s\n    only in the %s tree" % (k, "old" if k in ka else "new"))
                    continue
                body, f = kb[k]
                ninstr = sum(1 for l in body if l.startswith("\t") and not l.strip().startswith("."))
                verdict = "identical" if ka[k] == kb[k] else "DIFFERENT (old: sgpr %s vgpr %s spill %s)" % (
                    ka[k][1]["sgpr_count"], ka[k][1]["vgpr_count"], ka[k][1]["vgpr_spill_count"])
                rows.append("  %s\n    sgpr %s vgpr %s vgpr_spill %s instructions %d  %s" % (
                    k, f["sgpr_count"], f["vgpr_count"], f["vgpr_spill_count"], ninstr, verdict))
    report = "device listings (hipcc %s --cuda-device-only -S), normalised, old tree against new\n" % " ".join(FLAGS) + "\n".join(rows) + "\n"
    sys.stdout.write(report)
    if args.out:
        open(args.out, "w").write(report)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
