#!/usr/bin/env python
"""Everything the host layer of the convolutions decides, as text: for refactors of csrc/conv_plan.hip and csrc/aesr_api.hip, which must not
change a plan, a workspace size, a kernel choice, a status code or an error message.

    python scripts/plan_dump.py LIB.so [-o dump.txt] [--seed 1] [--count 300]

ctypes only (signatures parsed from include/*.h), no torch, and only where the HIP runtime sees NO GPU: the refusal block drives launch
entry points with placeholder pointers.  The library is loaded in child processes with AESR_PLAN_DEBUG=1, one per AESR_WINO_RING mode
(unset, 1, 0) plus one for the refusals.  Per shape (the layer table and the oversized shapes of tests/host_sanitized_sweep.py and a seeded
random set) one line per query with the value returned; per mode every "[aesr plan]" / "[plan_wgrad]" line the library printed; then the
status code and aesr_last_error_string() of calls the host code refuses (null pointers, illegal filters, channel counts, odd and
oversized shapes, bad jobs in job tables) -- and of a few it accepts, which end at the first HIP call for want of a device.  Two libraries
agree when their dumps are equal byte for byte: the last line printed is the number of shapes, the line count and the SHA-256 of the dump."""
import argparse
import ast
import ctypes
import hashlib
import os
import random
import re
import subprocess
import sys
from ctypes import c_char_p, c_double, c_float, c_int, c_size_t, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000          # a placeholder "device pointer": never dereferenced on the host


def sweep_tables():
    """BASELINE and HUGE of tests/host_sanitized_sweep.py (a script, not a module: its two literals are evaluated, nothing else runs)"""
    tree = ast.parse(open(os.path.join(ROOT, "tests", "host_sanitized_sweep.py")).read())
    got = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) in ("BASELINE", "HUGE"):
            got[node.targets[0].id] = eval(compile(ast.Expression(node.value), "sweep", "eval"))
    return [(n, h, h, ci, co) for n, h, ci, co in got["BASELINE"]], list(got["HUGE"])


def shapes(seed, count):
    base, huge = sweep_tables()
    rng = random.Random(seed)
    rand = []
    while len(rand) < count:
        n = rng.choice([1, 1, 2, 3, 5, 7, 12, 16, 33])
        h, w = rng.randint(1, 300), rng.randint(1, 300)
        if rng.random() < 0.3:
            w = h
        ci = rng.choice([1, 3, 4, 8, 16, 32, 48, 64, 96, 128, 256, 512])
        co = rng.choice([1, 4, 8, 16, 32, 64, 96, 128, 256, 512])
        if n * h * w * max(ci, co) <= (1 << 29):
            rand.append((n, h, w, ci, co))
    return base + huge + rand, huge


class Lib:
    """the library with the argument types of every function declared in include/*.h; call(name, **kw): parameters by name, the rest 0 / NULL"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.params = {}
        for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
            for res, name, args in re.findall(r"^([a-z_ ]+?[ *]+)(aesr_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
                if not hasattr(self.lib, name):
                    continue
                names, types = [], []
                for a in [a.strip() for a in args.split(",") if a.strip() != "void"]:
                    names.append(re.findall(r"\w+", a)[-1])
                    types.append(c_void_p if "*" in a else c_float if "float" in a else c_double if "double" in a else c_size_t if "size_t" in a else c_int)
                f = getattr(self.lib, name)
                f.argtypes = types
                f.restype = c_char_p if "char" in res else c_size_t if "size_t" in res else c_int
                self.params[name] = names

    def call(self, name, **kw):
        unknown = set(kw) - set(self.params[name])
        assert not unknown, (name, unknown)
        return getattr(self.lib, name)(*[kw.get(p, 0 if t is not c_void_p else None) for p, t in zip(self.params[name], getattr(self.lib, name).argtypes)])


def child_queries(L, seed, count):
    q = L.lib
    for n, h, w, ci, co in shapes(seed, count)[0]:
        row = ["%d %d %d %d %d" % (n, h, w, ci, co)]
        for ks, pad in ((1, 0), (3, 1)):
            row.append("k%d fwd_ws=%d dgrad_ws=%d wgrad_ws=%d" % (ks, q.aesr_conv2d_workspace_floats(n, h, w, ci, co, ks, pad),
                       q.aesr_conv2d_dgrad_workspace_floats(n, h, w, ci, co, ks, pad), q.aesr_conv2d_wgrad_workspace_floats(n, h, w, ci, co, ks, pad)))
        for tr in (0, 1):
            row.append("t%d wino_kernel=%d wino_ws=%d wino_packed=%d packed=%d,%d" % (
                tr, q.aesr_conv2d_wino_kernel(n, h, w, ci, co, 3, 1, tr), q.aesr_conv2d_wino_workspace_floats(n, h, w, ci, co, tr),
                q.aesr_conv2d_wino_packed_floats(co, ci, tr), q.aesr_conv2d_packed_floats(co, ci, 1, tr), q.aesr_conv2d_packed_floats(co, ci, 3, tr)))
        row.append("fwd_bn=%d" % q.aesr_conv2d_wino_fwd_bn_supported(n, h, w, ci, co))
        for r in row[1:]:
            print(row[0] + " | " + r)


def child_refusals(L, seed, count):
    def refuse(tag, name, **kw):
        rc = L.call(name, **kw)
        print("%s %s -> %d | %s" % (name, tag, rc, (L.lib.aesr_last_error_string() or b"").decode()))

    P = FAKE
    conv = dict(N=2, H=8, W=8, Cin=32, Cout=32, KS=3, pad=1)
    wino = dict(N=2, H=8, W=8, Cin=32, Cout=32)
    ptrs = {        # the pointer parameters a call needs to get past its null check
        "aesr_conv2d_fwd": dict(packed=P, out=P), "aesr_conv2d_fwd_ws": dict(packed=P, out=P, workspace=P),
        "aesr_conv2d_dgrad": dict(dy=P, packed_t=P, dx=P), "aesr_conv2d_dgrad_ws": dict(dy=P, packed_t=P, dx=P, workspace=P),
        "aesr_conv2d_wgrad": dict(x=P, dy=P, dw=P, db=P, workspace=P), "aesr_conv2d_wgrad_partial": dict(x=P, dy=P, workspace=P),
    }
    ptrs["aesr_conv2d_fwd"]["in"] = ptrs["aesr_conv2d_fwd_ws"]["in"] = P
    wptrs = {
        "aesr_conv2d_wino_fwd": dict(upacked=P, out=P), "aesr_conv2d_wino_fwd_ws": dict(upacked=P, out=P, workspace=P, workspace_floats=1 << 20),
        "aesr_conv2d_wino_dgrad": dict(dy=P, upacked_t=P, dx=P), "aesr_conv2d_wino_dgrad_ws": dict(dy=P, upacked_t=P, dx=P, workspace=P, workspace_floats=1 << 20),
        "aesr_conv2d_wino_fwd_bn": dict(upacked=P, bn_scale=P, bn_shift=P, out=P), "aesr_conv2d_wino_fwd_up2": dict(in_half=P, upacked=P, out=P),
        "aesr_conv2d_wino_dgrad_sum2": dict(dy=P, upacked_t=P, dx_half=P),
    }
    for name in ("aesr_conv2d_wino_fwd", "aesr_conv2d_wino_fwd_ws", "aesr_conv2d_wino_fwd_bn"):
        wptrs[name]["in"] = P
    # a null pointer (everything NULL, then one pointer at a time missing)
    for name, pp in list(ptrs.items()) + list(wptrs.items()):
        shape = conv if name in ptrs else wino
        refuse("all-null", name, **shape)
        for miss in pp:
            if miss != "workspace_floats":
                refuse("null-" + miss, name, **dict(shape, **{k: v for k, v in pp.items() if k != miss}))
    for name in ("aesr_conv2d_pack", "aesr_conv2d_pack_many", "aesr_conv2d_wino_pack_many", "aesr_weight_prep_many", "aesr_conv2d_wgrad_reduce_many",
                 "aesr_conv2d_wgrad_up2", "aesr_conv2d_cout1_dgrad", "aesr_conv2d_cout1_dgrad_pre", "aesr_bn_fused1_fwd", "aesr_bn_fused1_bwd",
                 "aesr_bn_fused1_fwd_p2p", "aesr_bn_fused1_bwd_p2p"):
        refuse("all-null", name)
    thin = dict(dy=P, dx=P, N=2, H=8, W=8, Cin=32, mask_act=1)
    refuse("null-workspace", "aesr_conv2d_cout1_dgrad", w=P, **thin)
    refuse("null-w", "aesr_conv2d_cout1_dgrad", workspace=P, **thin)
    refuse("Cin=12", "aesr_conv2d_cout1_dgrad", w=P, workspace=P, **dict(thin, Cin=12))
    refuse("null-w", "aesr_conv2d_cout1_dgrad_pre", **thin)
    refuse("Cin=12", "aesr_conv2d_cout1_dgrad_pre", w_flipped=P, **dict(thin, Cin=12))
    refuse("KS=2", "aesr_conv2d_pack", w=P, packed=P, Cout=32, Cin=32, KS=2)
    # illegal filter / padding, channel counts, sizes below the filter, odd sizes of the folded-upsampling forms
    for name, pp in ptrs.items():
        for tag, bad in (("KS=2", dict(KS=2)), ("KS=3,pad=3", dict(pad=3)), ("pad=-1", dict(pad=-1)), ("Cin=6", dict(Cin=6)), ("Cout=6", dict(Cout=6)),
                         ("1x1,pad=0", dict(H=1, W=1, pad=0)), ("Cin=0", dict(Cin=0))):
            refuse(tag, name, **dict(conv, **pp, **bad))
    for name, pp in wptrs.items():
        for tag, bad in (("Cin=24", dict(Cin=24)), ("Cout=48", dict(Cout=48)), ("H=7", dict(H=7))):
            if tag != "H=7" or name.endswith(("up2", "sum2")):
                refuse(tag, name, **dict(wino, **pp, **bad))
    refuse("pool,H=1", "aesr_conv2d_wino_fwd_bn", pool=1, **dict(wino, H=1, **wptrs["aesr_conv2d_wino_fwd_bn"]))
    refuse("H=7", "aesr_conv2d_wgrad_up2", x_half=P, dy=P, dw=P, db=P, workspace=P, **dict(wino, H=7))
    refuse("Cin=48", "aesr_conv2d_wgrad_up2", x_half=P, dy=P, dw=P, db=P, workspace=P, **dict(wino, Cin=48))
    refuse("x_up2,H=7", "aesr_conv2d_wgrad_partial", x_up2=1, **dict(conv, H=7, **ptrs["aesr_conv2d_wgrad_partial"]))
    refuse("x_up2,k1", "aesr_conv2d_wgrad_partial", x_up2=1, **dict(conv, KS=1, pad=0, **ptrs["aesr_conv2d_wgrad_partial"]))
    for tag, bad in (("KS=2", dict(KS=2)), ("pad=3", dict(pad=3)), ("N=0", dict(N=0))):
        for name in ("aesr_conv2d_workspace_floats", "aesr_conv2d_dgrad_workspace_floats", "aesr_conv2d_wgrad_workspace_floats"):
            refuse(tag, name, **dict(conv, **bad))
    # tensors beyond the kernels' offsets, with every pointer in place
    for n, h, w, ci, co in shapes(seed, count)[1]:
        big = dict(N=n, H=h, W=w, Cin=ci, Cout=co)
        for name, pp in list(ptrs.items()) + list(wptrs.items()):
            refuse("%dx%dx%dx%d->%d" % (n, h, w, ci, co), name, **dict(conv if name in ptrs else {}, **pp, **big))

    # job tables: a bad job in the first chunk is refused before anything is launched; one in the second chunk is met only after the first
    # chunk's launch, which has no device to run on here
    class PackJob(ctypes.Structure):
        _fields_ = [("w", c_void_p), ("packed", c_void_p), ("Cout", c_int), ("Cin", c_int), ("KS", c_int), ("transpose", c_int)]

    class PrepJob(ctypes.Structure):
        _fields_ = [("w", c_void_p), ("aux0", c_void_p), ("aux1", c_void_p), ("out", c_void_p), ("kind", c_int), ("Cout", c_int), ("Cin", c_int),
                    ("KS", c_int), ("transpose", c_int)]

    class ReduceJob(ctypes.Structure):
        _fields_ = [("workspace", c_void_p), ("dw", c_void_p), ("db", c_void_p), ("N", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int),
                    ("Cout", c_int), ("KS", c_int), ("pad", c_int)]

    def table(tag, name, cls, good, bad, at, n):
        jobs = (cls * n)(*[cls(*(bad if i == at else good)) for i in range(n)])
        refuse("%s at job %d of %d" % (tag, at, n), name, jobs_host=ctypes.addressof(jobs), njobs=n)

    for at, n in ((1, 3), (33, 40)):
        table("KS=2", "aesr_conv2d_pack_many", PackJob, (P, P, 32, 32, 3, 0), (P, P, 32, 32, 2, 0), at, n)
        table("null-w", "aesr_conv2d_pack_many", PackJob, (P, P, 32, 32, 3, 0), (None, P, 32, 32, 3, 0), at, n)
        table("KS=1", "aesr_conv2d_wino_pack_many", PackJob, (P, P, 32, 32, 3, 1), (P, P, 32, 32, 1, 1), at, n)
        table("pack,KS=2", "aesr_weight_prep_many", PrepJob, (P, None, None, P, 0, 32, 32, 3, 0), (P, None, None, P, 0, 32, 32, 2, 0), at, n)
        table("wino,KS=1", "aesr_weight_prep_many", PrepJob, (P, None, None, P, 1, 32, 32, 3, 0), (P, None, None, P, 1, 32, 32, 1, 0), at, n)
        table("fold,no-aux0", "aesr_weight_prep_many", PrepJob, (P, P, P, P, 2, 32, 4, 3, 0), (P, None, P, P, 2, 32, 4, 3, 0), at, n)
        table("kind=9", "aesr_weight_prep_many", PrepJob, (P, None, None, P, 3, 1, 32, 3, 0), (P, None, None, P, 9, 1, 32, 3, 0), at, n)
        table("null-out", "aesr_weight_prep_many", PrepJob, (P, None, None, P, 3, 1, 32, 3, 0), (P, None, None, None, 3, 1, 32, 3, 0), at, n)
    for at, n in ((1, 3), (17, 20)):
        good = (P, P, P, 2, 8, 8, 32, 32, 3, 1)
        table("KS=2", "aesr_conv2d_wgrad_reduce_many", ReduceJob, good, (P, P, P, 2, 8, 8, 32, 32, 2, 1), at, n)
        table("pad=3", "aesr_conv2d_wgrad_reduce_many", ReduceJob, good, (P, P, P, 2, 8, 8, 32, 32, 3, 3), at, n)
        table("1x1,pad=0", "aesr_conv2d_wgrad_reduce_many", ReduceJob, good, (P, P, P, 2, 1, 1, 32, 32, 3, 0), at, n)
        table("huge", "aesr_conv2d_wgrad_reduce_many", ReduceJob, good, (P, P, P, 64, 1024, 1024, 64, 64, 3, 1), at, n)
        table("null-dw", "aesr_conv2d_wgrad_reduce_many", ReduceJob, good, (P, None, P, 2, 8, 8, 32, 32, 3, 1), at, n)


def child(args):
    try:
        hip, n = ctypes.CDLL("libamdhip64.so"), c_int(0)
        if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0:
            print("REFUSED: %d GPU(s) visible -- this dump drives launch entry points with placeholder pointers and runs on CPU-only machines" % n.value)
            return 3
    except OSError:
        pass
    (child_refusals if args.child == "refusals" else child_queries)(Lib(args.lib), args.seed, args.count)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("-o", "--out")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--count", type=int, default=300)
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = []
    for mode in ("unset", "1", "0", "refusals"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("AESR_")}
        env["AESR_PLAN_DEBUG"] = "1"
        if mode in ("1", "0"):
            env["AESR_WINO_RING"] = mode
        r = subprocess.run([sys.executable, os.path.abspath(__file__), os.path.abspath(args.lib), "--seed", str(args.seed), "--count", str(args.count),
                            "--child", mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return r.returncode or 1
        out.append("==== " + ("refusals" if mode == "refusals" else "AESR_WINO_RING " + mode) + "\n" + r.stdout)
        out.append("==== plans printed\n" + "".join(l + "\n" for l in r.stderr.split("\n") if l.startswith(("[aesr plan]", "[plan_wgrad]"))))
    text = "".join(out)
    if args.out:
        open(args.out, "w").write(text)
    print("%d shapes, %d lines, sha256 %s" % (len(shapes(args.seed, args.count)[0]), text.count("\n"), hashlib.sha256(text.encode()).hexdigest()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
