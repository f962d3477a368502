#!/usr/bin/env python
"""Times oblique reslicing (aesr_reslice_affine / aesr_reslice_grid, csrc/reslice.hip) on a super-resolved cardiac cine, 30 frames of
90 x 224 x 224 at 1.4 x 1.4 x 1.1 mm:
  lax      -> 30 x 3 x 256 x 256: a long-axis stack (1.25 x 1.25 x 6 mm) through the volume's centre, tilted off its z axis
  rotated  -> 30 x 90 x 224 x 224: a grid of the same size turned 30 degrees about the oblique axis (1, 2, 3) through the centre
Needs the GPU; prints a table and appends it to ``--out`` (profiles/reslice.txt, which also holds hand-written notes and compiler remarks).

- call:   HIP events around ``evaluate.reslice.reslice_affine`` / ``reslice_grid`` on device tensors (the matrix on the host, the output's
          allocation, one launch), after ``--warmup`` calls; median / min / max of ``--reps`` calls.
- kernel: HIP events around ``--batch`` back-to-back calls of the C entry point into one preallocated output, divided by ``--batch``; median /
          min / max of ``--reps`` such batches.  Rows: affine linear, affine nearest, grid linear, and affine linear with ``out`` moved by 4
          bytes (the kernel has one path: the alignment should not matter).
- bytes:  algorithmic: every output voxel written once and every source voxel that some corner touches read once, for each of the N
          frames (counted on the host from the same float64 coordinates), plus the 12-byte grid entries on the grid path; the share of the
          8 TB/s HBM peak is those bytes over the kernel time.
- torch:  ``torch.nn.functional.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True)`` on the same device, with the grid
          expanded over the frames ([N, 1, Z, H, W] input) and with the frames as channels ([1, N, Z, H, W] input, one grid), and the largest
          difference between its result and the kernel's.
- taps:   the higher-order interpolators of csrc/reslice_taps.hip on the same two workloads, each launch timed alone: the B-spline's
          pre-filter (``aesr_bspline_prefilter_3d``, three passes) apart from its 64-tap gather, ``lanczos`` and ``cosine`` at radius 5
          (1000 taps).  GMAC/s: fp64 multiply-adds of the tap sum (taps x frames x voxels inside the source) over the kernel time;
          "x linear": the kernel time over the trilinear kernel's, measured again in the same run.  Beside them
          ``scipy.ndimage.map_coordinates(order=3, mode='mirror')`` on the host for ONE frame (``--no-scipy`` skips it)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import _hip  # noqa: E402
from superresolution_aniso_mri_amd.evaluate import reslice as rl  # noqa: E402

HBM_PEAK = 8.0e12
N, SAX_SHAPE, SAX_SPACING = 30, (90, 224, 224), (1.4, 1.4, 1.1)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def centred(shape, spacing, direction, centre):
    """the Geometry of a [z, y, x] grid whose centre voxel sits at ``centre`` (mm)"""
    half = np.array([(shape[2] - 1) / 2, (shape[1] - 1) / 2, (shape[0] - 1) / 2]) * np.asarray(spacing)
    return rl.Geometry(spacing, np.asarray(centre) - np.asarray(direction) @ half, direction)


def cases():
    sax = centred(SAX_SHAPE, SAX_SPACING, rotation((1, 2, 3), 0.7), (10.0, -20.0, 30.0))
    ex = np.array([np.cos(0.6), np.sin(0.6), 0.0])
    ey = rotation(ex, 0.3) @ np.array([0.0, 0.0, 1.0])
    lax = centred((3, 256, 256), (1.25, 1.25, 6.0), sax.direction @ np.stack([ex, ey, np.cross(ex, ey)], axis=1), (10.0, -20.0, 30.0))
    turned = centred(SAX_SHAPE, SAX_SPACING, sax.direction @ rotation((1, 2, 3), np.pi / 6), (10.0, -20.0, 30.0))
    return [("lax     30x3x256x256", rl.affine_between(sax, lax), (3, 256, 256)), ("rotated 30x90x224x224", rl.affine_between(sax, turned), SAX_SHAPE)]


def coordinates(M, shape):
    zo, yo, xo = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    return np.stack([((M[a, 0] * xo + M[a, 1] * yo) + M[a, 2] * zo) + M[a, 3] for a in range(3)], axis=-1)


def touched_voxels(c, src_shape):
    """how many source voxels some corner of some output voxel reads"""
    Z, Y, X = src_shape
    seen = np.zeros(Z * Y * X, dtype=bool)
    i0 = np.floor(c).astype(np.int64).reshape(-1, 3)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ix, iy, iz = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                ok = (ix >= 0) & (ix < X) & (iy >= 0) & (iy < Y) & (iz >= 0) & (iz < Z)
                seen[(iz[ok] * Y + iy[ok]) * X + ix[ok]] = True
    return int(seen.sum())


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--no-scipy", dest="scipy", action="store_false", help="skip the host's map_coordinates(order=3) row (seconds per case)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reslice.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "reslice_bench.py measures on the GPU; there is no CPU fallback"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("device: %s; %d warm-up calls, %d samples; kernel = %d back-to-back launches / %d" % (torch.cuda.get_device_name(0), args.warmup, args.reps,
                                                                                          args.batch, args.batch))
    say("%-22s %-26s | %-29s | %-29s | %8s %8s | %s" % ("case", "path", "call med/min/max [us]", "kernel med/min/max [us]", "GB/s", "of 8TB/s", "MB moved"))
    x = torch.rand((N,) + SAX_SHAPE, generator=torch.Generator().manual_seed(1)).cuda()
    Zs, Hs, Ws = SAX_SHAPE
    size = np.array(SAX_SHAPE[::-1], dtype=np.float64)
    for name, M, shape in cases():
        Zo, Ho, Wo = shape
        c = coordinates(M, shape)
        n_out, n_src = Zo * Ho * Wo, touched_voxels(c, SAX_SHAPE)
        grid = torch.from_numpy((c / ((size - 1) / 2) - 1).astype(np.float32)).cuda()
        n_inside = int(((c >= -0.5) & (c < size - 0.5)).all(axis=-1).sum())          # the voxels the higher-order kernels compute
        zyx = np.ascontiguousarray(np.moveaxis(c[..., ::-1], -1, 0))
        del c
        m = np.ascontiguousarray(M[:3], np.float64)
        mp = m.ctypes.data_as(_hip.DP)
        spare = torch.empty(N * n_out + 4, device="cuda")          # 16-byte aligned; [1:] is the same buffer 4 bytes later
        y, y4 = spare[:N * n_out], spare[1:N * n_out + 1]
        assert y.data_ptr() % 16 == 0 and y4.data_ptr() % 16 == 4

        def affine(out, interp):
            def run():
                for _ in range(args.batch):
                    _hip.check(_hip.lib.aesr_reslice_affine(_hip.ptr(x), _hip.ptr(out), N, Zs, Hs, Ws, Zo, Ho, Wo, mp, interp, _hip.stream()), "affine")
            return run

        def by_grid():
            for _ in range(args.batch):
                _hip.check(_hip.lib.aesr_reslice_grid(_hip.ptr(x), _hip.ptr(grid), _hip.ptr(y), N, Zs, Hs, Ws, Zo, Ho, Wo, 1, _hip.stream()), "grid")
        moved = 4.0 * N * (n_out + n_src)
        rows = [("affine linear", lambda: rl.reslice_affine(x, M, shape, "linear"), affine(y, 1), moved),
                ("affine nearest", lambda: rl.reslice_affine(x, M, shape, "nearest"), affine(y, 0), moved),
                ("grid linear", lambda: rl.reslice_grid(x, grid, "linear"), by_grid, moved + 12.0 * n_out),
                ("affine linear, out + 4 bytes", None, affine(y4, 1), moved)]
        say("%-22s %d of %d source voxels touched per frame, %d output voxels" % (name, n_src, Zs * Hs * Ws, n_out))
        for label, call, kernel, nbytes in rows:
            tc = event_times(call, args.warmup, args.reps) if call else None
            tk = [t / args.batch for t in event_times(kernel, 1, args.reps)]
            med = statistics.median(tk)
            call_txt = "%9.1f %9.1f %9.1f" % (statistics.median(tc) * 1e6, min(tc) * 1e6, max(tc) * 1e6) if tc else "%29s" % "-"
            say("%-22s %-26s | %s | %9.1f %9.1f %9.1f | %8.1f %7.1f%% | %.1f" % (name, label, call_txt, med * 1e6, min(tk) * 1e6, max(tk) * 1e6,
                                                                            nbytes / med / 1e9, 100 * nbytes / med / HBM_PEAK, nbytes / 1e6))
        # the higher-order interpolators (csrc/reslice_taps.hip) beside the trilinear row of this run
        t_linear = statistics.median([t / args.batch for t in event_times(affine(y, 1), 1, args.reps)])
        coef = rl.bspline_coefficients_3d(x)

        def taps(kernel, radius):
            src_p, coef_p = (None, _hip.ptr(coef)) if kernel == _hip.TAPS_BSPLINE3 else (_hip.ptr(x), None)
            return lambda: _hip.check(_hip.lib.aesr_reslice_taps_affine(src_p, coef_p, _hip.ptr(y), N, Zs, Hs, Ws, Zo, Ho, Wo, mp, kernel, radius, 0,
                                                                          _hip.stream()), "taps")

        def prefilter():
            _hip.check(_hip.lib.aesr_bspline_prefilter_3d(_hip.ptr(x), _hip.ptr(coef), N, Zs, Hs, Ws, _hip.stream()), "prefilter")
        reps = max(3, args.reps // 4)
        say("%-22s %-26s | %-29s | %10s %10s | %s" % (name, "path (%d of %d voxels inside)" % (n_inside, n_out), "kernel med/min/max [us]", "GMAC/s",
                                                      "x linear", "fp64 multiply-adds"))
        for label, fn, macs in (("bspline pre-filter (3 passes)", prefilter, None), ("bspline gather", taps(_hip.TAPS_BSPLINE3, 5), 64.0 * N * n_inside),
                                ("lanczos r=5", taps(_hip.TAPS_LANCZOS, 5), 1000.0 * N * n_inside), ("cosine r=5", taps(_hip.TAPS_COSINE, 5), 1000.0 * N * n_inside)):
            tk = event_times(fn, 1, reps)
            med = statistics.median(tk)
            rate = "%10.1f" % (macs / med / 1e9) if macs else "%10s" % "-"
            say("%-22s %-26s | %9.1f %9.1f %9.1f | %s %10.2f | %s" % (name, label, med * 1e6, min(tk) * 1e6, max(tk) * 1e6, rate, med / t_linear,
                                                                   "%.3g" % macs if macs else "-"))
        del coef
        torch.cuda.empty_cache()
        if args.scipy:
            from scipy import ndimage
            import time
            frame = x[0].cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            ndimage.map_coordinates(frame, zyx, order=3, mode="mirror", output=np.float64)
            say("%-22s %-50s | %9.1f us for ONE frame (pre-filter included)" % (name, "scipy.ndimage.map_coordinates(order=3) on the host",
                                                                               (time.perf_counter() - t0) * 1e6))
        del zyx
        ours = rl.reslice_affine(x, M, shape, "linear")
        g5 = grid.unsqueeze(0)
        forms = (("torch grid_sample, grid expanded over the frames", lambda: torch.nn.functional.grid_sample(
                      x.unsqueeze(1), g5.expand(N, -1, -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)),
                 ("torch grid_sample, frames as channels", lambda: torch.nn.functional.grid_sample(
                      x.unsqueeze(0), g5, mode="bilinear", padding_mode="zeros", align_corners=True)))
        for label, fn in forms:
            tt = event_times(fn, 1, max(3, args.reps // 4))
            diff = float((fn().reshape(ours.shape) - ours).abs().max())
            say("%-22s %-50s | %9.1f %9.1f %9.1f us | max |torch - kernel| = %.3g" % (name, label, statistics.median(tt) * 1e6, min(tt) * 1e6,
                                                                                   max(tt) * 1e6, diff))
        del ours, grid, g5, spare, y, y4
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    # appended: the file also holds the prose around earlier runs and the compiler's resource-usage remarks, which a run must not erase
    with open(args.out, "a") as f:
        f.write("\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
