#!/usr/bin/env python
"""Times the conventional through-plane baselines (aesr_z_expand / aesr_bspline_prefilter_z, csrc/z_expand.hip) on a cardiac frame
30 x 224 x 224 at factor 7 and a brain volume 59 x 208 x 176 at factor 3, for nearest, linear, bspline and lanczos (radius 5), ITK alignment.
Needs the GPU; prints a table (kept in profiles/z_expand.txt).

- call:   HIP events around ``evaluate.z_interp.z_expand`` on a device tensor (tables on the host, the output's allocation, one launch --
          bspline: the coefficient workspace's allocation and the pre-filter launch too), after ``--warmup`` calls; median / min / max of
          ``--reps`` calls.
- kernel: HIP events around ``--batch`` back-to-back calls of the C entry point into one preallocated output, divided by ``--batch`` (the
          launch latency of a single call is hidden behind the previous kernel); median / min / max of ``--reps`` such batches.  bspline has
          two rows: the expansion from ready coefficients, and the pre-filter alone.
- bytes:  algorithmic, (1 + f) Z H W x 4 B for every method (the issue's bound: samples in, slices out); the share of the 8 TB/s HBM peak is
          those bytes over the kernel time.  The bspline expansion really reads 8-byte coefficients ((2 + f) Z H W x 4 B) and the pre-filter
          moves 3 x 4 + 3 x 8 bytes per sample (the exact initialisation reads the line twice, the causal pass once more, the anti-causal pass
          re-reads what the causal one wrote);
          their rows give both the nominal and, in brackets, the real share.
- cpu:    if scipy is importable, the same expansion on this machine's host, once, as context: ``map_coordinates`` order 1 / ``nearest`` and
          ``spline_filter1d`` + ``map_coordinates`` order 3 / ``mirror`` on the whole volume along z (1-D calls per column would be the
          reference's SimpleITK cost model; one vectorised call per volume is the kinder comparison)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import _hip  # noqa: E402
from superresolution_aniso_mri_amd.evaluate import z_interp  # noqa: E402

HBM_PEAK = 8.0e12
CASES = [("cardiac 30x224x224 f=7", (30, 224, 224), 7), ("brain   59x208x176 f=3", (59, 208, 176), 3)]


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
    assert torch.cuda.is_available(), "z_expand_bench.py measures on the GPU; there is no CPU fallback"
    print("device: %s; %d warm-up calls, %d samples; kernel = %d back-to-back launches / %d" % (torch.cuda.get_device_name(0), args.warmup,
                                                                                                args.reps, args.batch, args.batch))
    print("%-24s %-18s | %-26s | %-26s | %8s %8s | %s" % ("case", "method", "call med/min/max [us]", "kernel med/min/max [us]", "GB/s", "of 8TB/s",
                                                         "MB (1 + f) Z H W x 4"))
    g = torch.Generator().manual_seed(1)
    vols = {}
    for name, shape, f in CASES:
        x = vols.setdefault(shape, torch.rand(*shape, generator=g).cuda())
        Z, H, W = shape
        Zo = z_interp.out_slices(Z, f, "itk")
        nominal = 4.0 * Z * H * W * (1 + f)
        x4 = x.unsqueeze(0)
        coef = z_interp.bspline_coefficients(x4)
        y = torch.empty((Zo, H, W), device="cuda")
        for method in z_interp.METHODS:
            base, w, boundary, needs_coef = z_interp.phase_tables(method, f, "itk", 5)
            base, w = np.ascontiguousarray(base, np.int32), np.ascontiguousarray(w, np.float64)
            bp, wp = base.ctypes.data_as(_hip.IP), w.ctypes.data_as(_hip.DP)

            def batch():
                for _ in range(args.batch):
                    _hip.lib.aesr_z_expand(None if needs_coef else _hip.ptr(x), _hip.ptr(coef) if needs_coef else None, _hip.ptr(y), 1, Z, H, W, f,
                                           Zo, w.shape[1], bp, wp, boundary, 0, _hip.stream())

            def prefilter():
                for _ in range(args.batch):
                    _hip.lib.aesr_bspline_prefilter_z(_hip.ptr(x), _hip.ptr(coef), 1, Z, H, W, _hip.stream())
            tc = event_times(lambda: z_interp.z_expand(x, f, method), args.warmup, args.reps)
            rows = [(method + (" (expansion)" if needs_coef else ""), batch, 4.0 * Z * H * W * (2 + f) if needs_coef else nominal)]
            if needs_coef:
                rows.append(("bspline (pre-filter)", prefilter, Z * H * W * (3 * 4.0 + 3 * 8.0)))
            for label, fn, real in rows:
                tk = [t / args.batch for t in event_times(fn, 2, args.reps)]
                med = statistics.median(tk)
                extra = "" if real == nominal else " [really %.1f MB: %.1f%%]" % (real / 1e6, 100 * real / med / HBM_PEAK)
                print("%-24s %-18s | %8.1f %8.1f %8.1f | %8.2f %8.2f %8.2f | %8.1f %7.1f%% | %.1f%s" % (
                    name, label, statistics.median(tc) * 1e6, min(tc) * 1e6, max(tc) * 1e6, med * 1e6, min(tk) * 1e6, max(tk) * 1e6,
                    nominal / med / 1e9, 100 * nominal / med / HBM_PEAK, nominal / 1e6, extra))
    if args.no_cpu:
        return
    try:
        import scipy
        from scipy import ndimage as ndi
    except ImportError:
        print("cpu: NOT MEASURED (scipy is not importable here)")
        return
    for name, shape, f in CASES:
        host = vols[shape].cpu().numpy()
        Z, H, W = shape
        zz = ((np.arange(Z * f) + 0.5) / f - 0.5)[:, None, None] * np.ones((1, H, W))
        yy, xx = np.broadcast_to(np.arange(H)[None, :, None], zz.shape), np.broadcast_to(np.arange(W)[None, None, :], zz.shape)
        t0 = time.perf_counter()
        lin = ndi.map_coordinates(host, [zz, yy, xx], order=1, mode="nearest")
        t_lin = time.perf_counter() - t0
        t0 = time.perf_counter()
        c = ndi.spline_filter1d(host, order=3, axis=0, mode="mirror", output=np.float64)
        t_pre = time.perf_counter() - t0
        dev = z_interp.z_expand(vols[shape], f, "linear").cpu().numpy()
        devc = z_interp.bspline_coefficients(vols[shape].unsqueeze(0))[0].cpu().numpy()
        print("cpu: %-24s scipy %s on this host, once: map_coordinates order 1 %.2f s, spline_filter1d %.3f s; max |device - scipy| linear %.3g, "
              "coefficients %.3g" % (name, scipy.__version__, t_lin, t_pre, float(np.abs(dev.astype(np.float64) - lin).max()),
                                     float(np.abs(devc - c).max())))


if __name__ == "__main__":
    main()
