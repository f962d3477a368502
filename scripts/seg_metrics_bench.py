#!/usr/bin/env python
"""Times the segmentation scores (aesr_surface_borders / aesr_surface_distances, csrc/seg_metrics.hip) on one 70 x 224 x 224 pair of label
volumes with three foreground classes at spacing (10, 1.4, 1.4) mm, 3-D borders, connectivity 1.  Needs the GPU; prints a table (kept in
profiles/seg_metrics.txt).

- phase one / phase two: HIP events around one call of the C entry point into preallocated buffers (phase two from phase one's
  workspace and a host copy of its counts made beforehand), after ``--warmup`` calls; median / min / max of ``--reps`` calls.
- call: host clock around ``evaluate.seg_metrics.segmentation_scores`` on device tensors, device synchronised: both phases, the
  allocations, the copy of the counts in between, the download of the packed lists and numpy's percentile.
- parity: the packed lists of the test fixture's cases against the numpy restatement of tests/test_seg_metrics_golden.py, worst relative
  difference (the tests hold it to 1e-12).
- cpu: if scipy is importable, the reference's route on this machine's host, once: per class and direction ``binary_erosion`` and
  ``distance_transform_edt`` (what kwatsch/medpy_metrics.py does for hd, hd95 and assd, which each repeat it), and the worst relative
  difference of the device's hd / hd95 / assd from the values computed that way."""
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
from superresolution_aniso_mri_amd import _hip, ops  # noqa: E402
from superresolution_aniso_mri_amd.evaluate import seg_metrics  # noqa: E402

SHAPE, SPACING, CLASSES = (70, 224, 224), (10.0, 1.4, 1.4), (1, 2, 3)


def label_pair(shape, rng):
    """floor(4 * 0.999 * smooth blob) twice, the second with every blob moved a little: a segmentation and its reference"""
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    blobs = [(rng.uniform(0.25, 0.75, 3) * np.array(shape), rng.uniform(0.15, 0.3), rng.uniform(0.5, 1.0)) for _ in range(4)]
    out = []
    for jitter in (0.0, 1.0):
        f = np.zeros(shape)
        for c, s, a in blobs:
            c = c + jitter * rng.standard_normal(3) * np.array([1.0, 3.0, 3.0])
            f += a * np.exp(-sum(((g - ci) / (si * n)) ** 2 for g, ci, si, n in zip(grids, c, (s, s, s), shape)) / 2)
        out.append(np.floor(4 * 0.999 * f / f.max()).astype(np.float32))
    return out[1], out[0]


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
    print("%-44s | %9.3f %9.3f %9.3f %s" % (label, statistics.median(times) * unit, min(times) * unit, max(times) * unit, note))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seg_metrics_bench.py measures on the GPU; there is no CPU fallback"
    Z, H, W = SHAPE
    C = len(CLASSES)
    res, ref = label_pair(SHAPE, np.random.default_rng(7))
    r, g = torch.from_numpy(res).cuda()[None], torch.from_numpy(ref).cuda()[None]
    print("device: %s; %d warm-up calls, %d samples; %d x %d x %d, classes %s, spacing %s, ndim 3, connectivity 1" % (
        torch.cuda.get_device_name(0), args.warmup, args.reps, Z, H, W, list(CLASSES), list(SPACING)))
    nbytes = ops.surface_workspace_bytes(1, Z, H, W, C)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    counts = torch.empty((1, C, 7), device="cuda", dtype=torch.int64)
    cls = _hip.int_array(CLASSES)

    def phase_one():
        _hip.check(_hip.lib.aesr_surface_borders(_hip.ptr(r), _hip.ptr(g), _hip.ptr(ws), _hip.ptr(counts), 1, Z, H, W, cls, C, 3, 1, _hip.stream()),
                   "aesr_surface_borders")
    phase_one()
    host = counts.cpu().numpy()
    total = int(ops.surface_list_lengths(host).sum())
    dist = torch.empty(total, device="cuda", dtype=torch.float64)
    stats = torch.empty((1, C, 2, 2), device="cuda", dtype=torch.float64)
    sp = _hip.double_array(SPACING)

    def phase_two():
        _hip.check(_hip.lib.aesr_surface_distances(_hip.ptr(ws), _hip.ptr(counts), host.ctypes.data_as(_hip.LLP), _hip.ptr(dist), total,
                                                   _hip.ptr(stats), 1, Z, H, W, C, 3, sp, _hip.stream()), "aesr_surface_distances")
    print("workspace %.1f MB; voxels per class (result / reference) %s; border voxels %s; %d distances" % (
        nbytes / 1e6, host[0, :, :2].tolist(), host[0, :, 5:].tolist(), total))
    print("%-44s | %9s %9s %9s" % ("", "med [ms]", "min [ms]", "max [ms]"))
    row("phase one: aesr_surface_borders (2 launches)", event_times(phase_one, args.warmup, args.reps))
    row("phase two: aesr_surface_distances (5 launches)", event_times(phase_two, args.warmup, args.reps))

    def whole():
        t0 = time.perf_counter()
        out = seg_metrics.segmentation_scores(r, g, SPACING, classes=CLASSES)
        torch.cuda.synchronize()
        whole.out = out
        return time.perf_counter() - t0
    for _ in range(args.warmup):
        whole()
    row("call: segmentation_scores, device tensors in", [whole() for _ in range(args.reps)], note="(host clock)")
    dev = whole.out
    print("device scores: dice %s hd %s hd95 %s assd %s" % tuple(np.array2string(dev[k][0], precision=6) for k in ("dice", "hd", "hd95", "assd")))

    import test_seg_metrics_golden as tm
    worst, n = 0.0, 0
    for name in tm.case_names():
        rr, gg, spc, classes, empty, rank = tm.case_frames(name)
        for nd, k in ((3, 1), (3, rank), (2, 2)) if rank == 3 else ((2, 1), (2, 2)):
            out = seg_metrics.surface_distance_lists(rr, gg, spc, classes=classes, ndim=nd, connectivity=k)
            for fr in range(rr.shape[0]):
                for ci, c in enumerate(classes):
                    if c in empty:
                        continue
                    for d, (X, Y) in enumerate(((rr[fr] == c, gg[fr] == c), (gg[fr] == c, rr[fr] == c))):
                        want = tm.surface_distances_np(X, Y, spc, nd, k)
                        o = int(out["offsets"][fr, ci, d])
                        got = out["distances"][o:o + int(out["lengths"][fr, ci, d])]
                        assert got.shape == want.shape
                        fin = np.isfinite(want)
                        assert np.array_equal(np.isfinite(got), fin)
                        if fin.any():
                            worst = max(worst, float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(want[fin], 1e-300))))
                        n += len(want)
    print("parity: %d distances of the fixture's cases against the numpy restatement, worst relative difference %.3g" % (n, worst))
    if args.no_cpu:
        return
    try:
        import scipy
        from scipy import ndimage as ndi
    except ImportError:
        print("cpu: NOT MEASURED (scipy is not importable here)")
        return
    per_class, worst = [], 0.0
    for ci, c in enumerate(CLASSES):
        A, B = res == c, ref == c
        t0 = time.perf_counter()
        fp = ndi.generate_binary_structure(3, 1)
        bA, bB = A ^ ndi.binary_erosion(A, structure=fp, iterations=1), B ^ ndi.binary_erosion(B, structure=fp, iterations=1)
        d_ab = ndi.distance_transform_edt(~bB, sampling=SPACING)[bA]
        d_ba = ndi.distance_transform_edt(~bA, sampling=SPACING)[bB]
        host_scores = (max(d_ab.max(), d_ba.max()), np.percentile(np.hstack((d_ab, d_ba)), 95), (d_ab.mean() + d_ba.mean()) / 2)
        per_class.append(time.perf_counter() - t0)
        for key, want in zip(("hd", "hd95", "assd"), host_scores):
            worst = max(worst, abs(dev[key][0, ci] - want) / want)
    print("cpu: scipy %s on this host, once, both directions of one class: %s s (classes %s), %.2f s for all three; worst relative difference "
          "of the device's hd / hd95 / assd from scipy's %.3g" % (scipy.__version__, " ".join("%.2f" % t for t in per_class), list(CLASSES),
                                                                  sum(per_class), worst))


if __name__ == "__main__":
    main()
