#!/usr/bin/env python
"""Times the long-axis view kernel against the torch composition that does the same job, and the long-axis metric calls beside
their axis-0 times.  Needs the GPU; prints a table (kept as profiles/long_axis_views.txt).

Per volume size and axis, alternating within one process, device-synchronised, every variant repeated until it has run for
``--seconds``:
  (a) aesr_long_axis_views: both views + the black flags, one call;
  (b) torch: swapaxes(0, k).contiguous() of both volumes + (view == 0).flatten(1).all(1)          [measured twice: b1, b2 = its spread]
  and compute_{ssim,psnr,vif}_for_batch(eval_axis=k) beside eval_axis=0 on the same volume (host time included: they end in a copy
  of the per-slice scores).
Algorithmic bytes of (a): 4 B x Z x H x W x 2 volumes x (read + write); its share of the 8 TB/s HBM peak is those bytes over the time.
The outputs of (a) and (b) are compared bit for bit before anything is timed."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import _hip  # noqa: E402
from superresolution_aniso_mri_amd.evaluate import metrics  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, seconds, chunk):
    """Mean seconds per call over chunks of ``chunk`` calls, each ended by a device synchronise, until ``seconds`` have passed."""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(chunk):
            fn()
        torch.cuda.synchronize()
        n += chunk
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.5, help="run time per variant and round")
    ap.add_argument("--rounds", type=int, default=2, help="alternating rounds (a, b1, b2, a, b1, b2, ...)")
    ap.add_argument("--sizes", default="10x224x224,30x224x224,128x256x256")
    ap.add_argument("--no-metrics", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "long_axis_bench.py measures on the GPU; there is no CPU fallback"
    print("device: %s" % torch.cuda.get_device_name(0))
    print("%-13s %4s | %9s %9s %9s | %8s %8s | %9s %7s | %s" % ("volume", "axis", "a [us]", "b1 [us]", "b2 [us]", "b/a", "spread", "a GB/s", "of 8TB/s",
                                                                 "a not slower than b by more than the spread"))
    rows = []
    for size in args.sizes.split(","):
        Z, H, W = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(Z * 7 + H)
        ref = torch.rand(Z, H, W, generator=g)
        ref[:, :5, :] = 0.0
        ref[:, :, -7:] = 0.0
        rec = (0.9 * ref + 0.05 * torch.randn(Z, H, W, generator=g) + 0.03).clamp(0, 1)
        ref, rec = ref.cuda(), rec.cuda()
        for axis in (1, 2):
            shape = (H, Z, W) if axis == 1 else (W, H, Z)
            rv, cv = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
            black = torch.empty(shape[0], device="cuda", dtype=torch.uint8)
            st = _hip.stream()

            def a():
                _hip.check(_hip.lib.aesr_long_axis_views(_hip.ptr(ref), _hip.ptr(rec), _hip.ptr(rv), _hip.ptr(cv), _hip.ptr(black), Z, H, W, axis, st),
                           "aesr_long_axis_views")

            def b():
                v = torch.swapaxes(ref, 0, axis).contiguous()
                c = torch.swapaxes(rec, 0, axis).contiguous()
                return v, c, (v == 0).flatten(1).all(1)
            a()
            v, c, k = b()
            assert torch.equal(rv.view(torch.int32), v.view(torch.int32)) and torch.equal(cv.view(torch.int32), c.view(torch.int32))
            assert torch.equal(black.bool(), k)
            for fn in (a, b):                       # warm-up
                timed(fn, 0.2, 20)
            t = {"a": [], "b1": [], "b2": []}
            for _ in range(args.rounds):
                t["a"].append(timed(a, args.seconds, 50)[0])
                t["b1"].append(timed(b, args.seconds, 50)[0])
                t["b2"].append(timed(b, args.seconds, 50)[0])
            ta, tb1, tb2 = (sum(t[k]) / len(t[k]) for k in ("a", "b1", "b2"))
            tb, spread = 0.5 * (tb1 + tb2), abs(tb1 - tb2)
            nbytes = 4.0 * Z * H * W * 2 * 2
            ok = ta <= tb + spread
            print("%-13s %4d | %9.2f %9.2f %9.2f | %8.2f %7.2f%% | %9.1f %6.1f%% | %s" % (size, axis, ta * 1e6, tb1 * 1e6, tb2 * 1e6, tb / ta,
                                                                                       100 * spread / tb, nbytes / ta / 1e9,
                                                                                       100 * nbytes / ta / HBM_PEAK, "yes" if ok else "NO"))
            rows.append((size, axis, ok))
        if not args.no_metrics:
            fns = (("ssim", metrics.compute_ssim_for_batch), ("psnr", metrics.compute_psnr_for_batch), ("vif", metrics.compute_vif_for_batch))
            for name, fn in fns:
                line = "  compute_%s_for_batch %-13s" % (name, size)
                for axis in (0, 1, 2):
                    fn(ref, rec, eval_axis=axis)
                    per, _ = timed(lambda: fn(ref, rec, eval_axis=axis), min(args.seconds, 1.0), 5)
                    line += "  eval_axis=%d %9.1f us" % (axis, per * 1e6)
                print(line)
    big = [ok for size, axis, ok in rows if size == "128x256x256"]
    if big:
        print("condition (128x256x256: a not slower than b by more than b's spread): %s" % ("met" if all(big) else "NOT met"))


if __name__ == "__main__":
    main()
