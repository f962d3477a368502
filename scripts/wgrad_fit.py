#!/usr/bin/env python
"""Fixed cost of a conv_wgrad_wino_f32 launch in the c2 step (12 triplets): t = a * visits + b over the ten launches of a step, from a
rocprofv3 --kernel-trace .db of bench.py.  A launch visits ceil(ntiles / S) tiles per workgroup (ntiles = N ceil(H/16) ceil(W/8),
S = 256 / ((Cin/32)(Cout/32)), plan_wgrad_wino).  Steps are delimited by the marker kernel; the fit is made on the mean over the last
STEPS steps and on each of them alone (the spread of a and b over single steps is the trace's own run-to-run difference).
    wgrad_fit.py results.db [STEPS=4] [marker]"""
import sqlite3
import sys

import numpy as np

# the 3x3 layers with >= 32 channels in backward order: Cin, Cout, size, images
LAYERS = [(32, 32, 160, 36), (32, 32, 80, 36), (64, 32, 80, 36), (64, 64, 40, 36), (128, 64, 40, 36), (128, 128, 40, 24), (64, 128, 40, 24),
          (64, 64, 81, 24), (32, 64, 81, 24), (32, 32, 162, 24)]


def visits(cin, cout, size, n):
    ntiles = n * -(-size // 16) * -(-size // 8)
    s = 256 // ((cin // 32) * (cout // 32))
    return -(-ntiles // s)


def fit(v, t):
    A = np.stack([v, np.ones_like(v)], 1)
    (a, b), res = np.linalg.lstsq(A, t, rcond=None)[:2]
    return a, b, float(np.sqrt(res[0] / len(v))) if len(res) else 0.0


def main():
    db = sqlite3.connect(sys.argv[1])
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    marker = sys.argv[3] if len(sys.argv) > 3 else "adam_step_kernel"
    rows = list(db.execute("select name, start, end from kernels order by start"))
    ends = [i for i, r in enumerate(rows) if r[0].startswith(marker)]
    v = np.array([visits(*l) for l in LAYERS], dtype=np.float64)
    per_step = []
    for k in range(steps):
        seg = rows[ends[-2 - k] + 1: ends[-1 - k] + 1]
        t = [(e - s) / 1e3 for name, s, e in seg if "conv_wgrad_wino_f32" in name]
        assert len(t) == len(LAYERS), "%d launches of conv_wgrad_wino_f32 in a step, expected %d (c2, 12 triplets)" % (len(t), len(LAYERS))
        per_step.append(t)
    per_step = np.array(per_step)
    mean = per_step.mean(0)
    a, b, rms = fit(v, mean)
    print("layer (backward order)   N  visits   us (mean of %d steps)   min    max   model %.3f*visits + %.2f" % (steps, a, b))
    for l, vv, m, lo, hi in zip(LAYERS, v, mean, per_step.min(0), per_step.max(0)):
        print("%4d->%-4d @%-4d        %3d  %5d   %8.1f            %6.1f %6.1f   %6.1f" % (l[0], l[1], l[2], l[3], vv, m, lo, hi, a * vv + b))
    print("fit on the mean: a = %.3f us per visit, b = %.2f us per launch (rms residual %.2f us); sum over the ten launches %.1f us, of which b: %.1f us"
          % (a, b, rms, mean.sum(), 10 * b))
    singles = [fit(v, t)[:2] for t in per_step]
    print("single steps: a = %s | b = %s" % (" ".join("%.3f" % s[0] for s in singles), " ".join("%.2f" % s[1] for s in singles)))
    print("run-to-run: a %.3f .. %.3f (spread %.3f), b %.2f .. %.2f (spread %.2f)" % (
        min(s[0] for s in singles), max(s[0] for s in singles), max(s[0] for s in singles) - min(s[0] for s in singles),
        min(s[1] for s in singles), max(s[1] for s in singles), max(s[1] for s in singles) - min(s[1] for s in singles)))


if __name__ == "__main__":
    main()
