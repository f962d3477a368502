#!/usr/bin/env python
"""Times the thick-slice simulation (aesr_thick_slices, csrc/thick_slices.hip) on brain-sized volumes: 176 x 208 x 176 (OASIS) at
downsample steps 3 and 6 (thickness 3 and 6), 256 x 256 x 200 (dHCP) at step 5 (thickness 2.5), and each volume's full-Z blur (z_step 1, the
dataset-creation use).  Needs the GPU; prints a table (kept in profiles/thick_slices.txt).

- call:   HIP events around ``datasets.common_brains.thick_slices`` on a device tensor (weights on the host, the output's allocation, one
          launch), after ``--warmup`` calls; median / min / max of ``--reps`` calls.
- kernel: HIP events around ``--batch`` back-to-back calls of the C entry point into one preallocated output, divided by ``--batch``
          (the launch latency of a single call is hidden behind the previous kernel); median / min / max of ``--reps`` such batches.
          ``rocprofv3 --kernel-trace --stats -- python scripts/thick_slices_bench.py --reps 20 --no-cpu`` gives the same figure from the
          profiler (the stats table names thick_slices_kernel<float4, 64> / <float, 256>).
- bytes:  algorithmic, (Z + Zo) H W x 4 B; the share of the 8 TB/s HBM peak is those bytes over the kernel time.
- cpu:    if scipy is importable, the reference's function on the same array on this machine's host, once: its per-column loop
          (``gaussian_filter1d`` per (y, x), datasets/common_brains.py:37-44) and the one ``axis=0`` call that equals it; the largest
          difference between the device result and scipy's is printed with it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import _hip  # noqa: E402
from superresolution_aniso_mri_amd.datasets import common_brains as cb  # noqa: E402
from superresolution_aniso_mri_amd.datasets.common import gaussian_weights  # noqa: E402

HBM_PEAK = 8.0e12
CASES = [("OASIS 176x208x176 step 3", (176, 208, 176), 3.0, 3), ("OASIS 176x208x176 step 6", (176, 208, 176), 6.0, 6),
         ("dHCP  256x256x200 step 5", (256, 256, 200), 2.5, 5), ("OASIS 176x208x176 full Z", (176, 208, 176), 3.0, 1),
         ("dHCP  256x256x200 full Z", (256, 256, 200), 2.5, 1)]


def event_times(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "thick_slices_bench.py measures on the GPU; there is no CPU fallback"
    print("device: %s; %d warm-up calls, %d samples; kernel = %d back-to-back launches / %d" % (torch.cuda.get_device_name(0), args.warmup,
                                                                                                args.reps, args.batch, args.batch))
    print("%-26s | %-26s | %-26s | %8s %8s | %s" % ("case", "call med/min/max [us]", "kernel med/min/max [us]", "GB/s", "of 8TB/s", "MB moved"))
    g = torch.Generator().manual_seed(1)
    vols = {}
    for name, shape, th, k in CASES:
        if shape not in vols:
            vols[shape] = torch.rand(*shape, generator=g).cuda()
        x = vols[shape]
        Z, H, W = shape
        y = cb.thick_slices(x, th, k)
        nbytes = 4.0 * (x.numel() + y.numel())
        w, r = gaussian_weights(th / cb.FWHM)
        w = np.ascontiguousarray(w, np.float64)
        wp = w.ctypes.data_as(_hip.DP)

        def batch():
            for _ in range(args.batch):
                _hip.lib.aesr_thick_slices(_hip.ptr(x), _hip.ptr(y), Z, H, W, k, wp, r, _hip.stream())
        tc = event_times(lambda: cb.thick_slices(x, th, k), args.warmup, args.reps)
        tk = [t / args.batch for t in event_times(batch, 2, args.reps)]
        med = statistics.median(tk)
        print("%-26s | %8.1f %8.1f %8.1f | %8.2f %8.2f %8.2f | %8.1f %7.1f%% | %.1f (radius %d, out %s)" % (
            name, statistics.median(tc) * 1e6, min(tc) * 1e6, max(tc) * 1e6, med * 1e6, min(tk) * 1e6, max(tk) * 1e6, nbytes / med / 1e9,
            100 * nbytes / med / HBM_PEAK, nbytes / 1e6, r, tuple(y.shape)))
    if args.no_cpu:
        return
    try:
        import scipy
        from scipy.ndimage import gaussian_filter1d
    except ImportError:
        print("cpu: NOT MEASURED (scipy is not importable here)")
        return
    for name, shape, th, k in CASES[:3]:
        host = vols[shape].cpu().numpy()
        sigma = th / 2.355
        t0 = time.perf_counter()
        one = gaussian_filter1d(host, sigma, axis=0)
        t_axis = time.perf_counter() - t0
        t0 = time.perf_counter()
        loop = np.zeros_like(host)
        for yy in range(host.shape[1]):
            for xx in range(host.shape[2]):
                loop[:, yy, xx] = gaussian_filter1d(host[:, yy, xx], sigma)
        t_loop = time.perf_counter() - t0
        dev = cb.thick_slices(vols[shape], th, k).cpu().numpy()
        print("cpu: %-26s scipy %s on this host, once: the reference's per-column loop %.2f s, one axis=0 call %.3f s (equal: %s); "
              "max |device - scipy[::%d]| = %.3g" % (name, scipy.__version__, t_loop, t_axis, bool(np.array_equal(one, loop)), k,
                                                      float(np.abs(dev.astype(np.float64) - one[::k]).max())))


if __name__ == "__main__":
    main()
