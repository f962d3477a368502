#!/usr/bin/env python
"""Times shape-based interpolation of label maps (aesr_shape_signed_distances / aesr_shape_interpolate, csrc/shape_interp.hip) on one
30 x 224 x 224 label volume with four classes (the background and three structures) at in-plane spacing (1.4, 1.4) mm, 6 slices put into
every gap (204 output slices).  Needs the GPU; prints a table (kept in profiles/shape_interp.txt).  No target is set: this is what is measured.

- signed distances / blend: HIP events around one call of the C entry point into preallocated buffers, after ``--warmup`` calls; median /
  min / max of ``--reps`` calls.
- call: host clock around ``evaluate.shape_interp.shape_interpolate`` on a device tensor, device synchronised: the class list
  (``torch.unique``), the allocations, the upload of the grid's tables and the three launches.
- parity: the fixture's cases (tests/golden/shape_interp.npz) against the numpy restatement of tests/test_shape_interp_golden.py: map values
  that differ in bits, labels that differ from the rule on the device's maps (the tests hold both to 0).
- cpu: if scipy is importable, ``distance_transform_edt`` twice per class and slice for the same maps on this machine's host, once, and
  the worst difference of the device's maps from them."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from superresolution_aniso_mri_amd import _hip  # noqa: E402
from superresolution_aniso_mri_amd.evaluate import shape_interp  # noqa: E402
from superresolution_aniso_mri_amd.evaluate.z_grid import target_grid  # noqa: E402

SHAPE, SPACING_YX, CLASSES, PER_GAP = (30, 224, 224), (1.4, 1.4), (0, 1, 2, 3), 6


def label_volume(shape, rng):
    """floor(4 * 0.999 * smooth blobs): nested structures that move and change size along z"""
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    f = np.zeros(shape)
    for _ in range(4):
        c, s, a = rng.uniform(0.25, 0.75, 3) * np.array(shape), rng.uniform(0.15, 0.3), rng.uniform(0.5, 1.0)
        f += a * np.exp(-sum(((g - ci) / (s * n)) ** 2 for g, ci, n in zip(grids, c, shape)) / 2)
    return np.floor(4 * 0.999 * f / f.max()).astype(np.uint8)


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


def row(label, times, unit=1e3, note=""):
    print("%-52s | %9.3f %9.3f %9.3f %s" % (label, statistics.median(times) * unit, min(times) * unit, max(times) * unit, note))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "shape_interp_bench.py measures on the GPU; there is no CPU fallback"
    Z, H, W = SHAPE
    C = len(CLASSES)
    vol = label_volume(SHAPE, np.random.default_rng(7))
    assert sorted(np.unique(vol).tolist()) == list(CLASSES)
    lab = torch.from_numpy(vol).cuda()[None]
    grid = target_grid(Z, 1.0, 1.0 / (PER_GAP + 1))
    J = grid.J
    print("device: %s; %d warm-up calls, %d samples; %d x %d x %d, classes %s, spacing (y, x) %s, %d slices per gap -> %d slices" % (
        torch.cuda.get_device_name(0), args.warmup, args.reps, Z, H, W, list(CLASSES), list(SPACING_YX), PER_GAP, J))
    nbytes = int(_hip.lib.aesr_shape_workspace_bytes(1, Z, H, W, C))
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    sdm = torch.empty((1, C, Z, H, W), device="cuda", dtype=torch.float64)
    out = torch.empty((1, J, H, W), device="cuda", dtype=torch.uint8)
    gap, alpha = shape_interp.grid_tables(grid, "cuda")
    cls = _hip.int_array(CLASSES)

    def maps():
        _hip.check(_hip.lib.aesr_shape_signed_distances(_hip.ptr(lab), _hip.ptr(sdm), _hip.ptr(ws), nbytes, 1, Z, H, W, cls, C, SPACING_YX[0],
                                                        SPACING_YX[1], _hip.stream()), "aesr_shape_signed_distances")

    def blend():
        _hip.check(_hip.lib.aesr_shape_interpolate(_hip.ptr(sdm), _hip.ptr(gap), _hip.ptr(alpha), _hip.ptr(out), 1, C, Z, H, W, J, cls, _hip.stream()),
                   "aesr_shape_interpolate")
    print("maps %.1f MB, workspace %.1f MB, output %.1f MB (%s stores); voxels per class %s" % (
        sdm.numel() * 8 / 1e6, nbytes / 1e6, out.numel() / 1e6, shape_interp.store_path(out, H * W), [int((vol == c).sum()) for c in CLASSES]))
    print("%-52s | %9s %9s %9s" % ("", "med [ms]", "min [ms]", "max [ms]"))
    t_maps = event_times(maps, args.warmup, args.reps)
    row("aesr_shape_signed_distances (2 launches)", t_maps, note="%.1f Mpixel-maps/s" % (C * Z * H * W / statistics.median(t_maps) / 1e6))
    t_blend = event_times(blend, args.warmup, args.reps)
    row("aesr_shape_interpolate (1 launch)", t_blend, note="%.1f GB/s of map values loaded (a map slice serves up to %d output slices: mostly cache hits), %.1f Mvoxel/s written" % (
        2 * C * 8 * J * H * W / statistics.median(t_blend) / 1e9, 2 * (PER_GAP + 1), J * H * W / statistics.median(t_blend) / 1e6))

    def whole():
        t0 = time.perf_counter()
        res = shape_interp.shape_interpolate(lab[0], num_interpolations=PER_GAP, spacing_yx=SPACING_YX)
        torch.cuda.synchronize()
        whole.out = res
        return time.perf_counter() - t0
    for _ in range(args.warmup):
        whole()
    row("call: shape_interpolate, device tensor in", [whole() for _ in range(args.reps)], note="(host clock)")
    assert torch.equal(whole.out, out[0]) and torch.equal(whole.out[::PER_GAP + 1], lab[0])

    import test_shape_interp_golden as tm
    bits, labels, n_maps, n_labels = 0, 0, 0, 0
    for name in tm.case_names():
        c = tm.case(name)
        dev = torch.from_numpy(c["labels"]).cuda()
        got, _ = shape_interp.signed_distance_maps(dev, c["spacing"], c["classes"])
        got = got.cpu().numpy()
        from superresolution_aniso_mri_amd.evaluate.z_grid import ZGrid
        g = ZGrid(c["labels"].shape[1], 1.0, 1.0, c["gap"] + c["alpha"], c["gap"].astype(np.int64), c["alpha"])
        lab_dev = shape_interp.shape_interpolate(dev, grid=g, spacing_yx=c["spacing"], classes=c["classes"]).cpu().numpy()
        want_maps, _ = tm.restated(name)
        bits += int((got.view(np.int64) != want_maps.view(np.int64)).sum())
        labels += int((lab_dev != tm.blend_np(got, c["gap"], c["alpha"], c["classes"])[0]).sum())
        n_maps, n_labels = n_maps + got.size, n_labels + lab_dev.size
    print("parity: %d of %d map values of the fixture's cases differ in bits from the numpy restatement; %d of %d labels differ from the rule "
          "on the device's maps" % (bits, n_maps, labels, n_labels))
    if args.no_cpu:
        return
    try:
        import scipy
        from scipy import ndimage as ndi
    except ImportError:
        print("cpu: NOT MEASURED (scipy is not importable here)")
        return
    maps()
    dev_maps = sdm.cpu().numpy()[0]
    big = float(np.sqrt((H * SPACING_YX[0]) ** 2 + (W * SPACING_YX[1]) ** 2))
    t0 = time.perf_counter()
    host = np.empty((C, Z, H, W))
    for ci, c in enumerate(CLASSES):
        for z in range(Z):
            M = vol[z] == c
            if M.all() or not M.any():
                host[ci, z] = big if M.all() else -big
            else:
                host[ci, z] = np.where(M, ndi.distance_transform_edt(M, sampling=SPACING_YX), -ndi.distance_transform_edt(~M, sampling=SPACING_YX))
    t_host = time.perf_counter() - t0
    print("cpu: scipy %s on this host, once: %.3f s for the same %d x %d maps (distance_transform_edt twice per class and slice); worst "
          "|device - scipy| %.3g (BIG = %.1f)" % (scipy.__version__, t_host, C, Z, float(np.abs(dev_maps - host).max()), big))


if __name__ == "__main__":
    main()
