#!/usr/bin/env python
"""Generate tests/golden/reslice_taps.npz for the higher-order affine reslice (include/aesr_hip_reslice_taps.h).  A script, not a test (pytest does not
collect it); scipy and numpy only.  Only data is written, per case:

  vol       uint16 counts of 1/1024 in [0, 1] (exact in fp32), [N, Z, Y, X]
  matrix    float64 [3, 4]: source (x, y, z) = matrix @ (xo, yo, zo, 1)
  coef      ``scipy.ndimage.spline_filter(vol, order=3, mode='mirror', output=float64)`` per frame
  bspline   ``scipy.ndimage.map_coordinates(vol, positions, order=3, mode='mirror')`` in float64 with the inside rule applied (0 wherever
            -0.5 <= p < size - 0.5 fails on an axis); positions in the contract's operation order
  lanczos3, lanczos5, cosine5
            the numpy restatement of tests/test_reslice_taps_golden.py: the windowed sincs have no second implementation on this machine
            (SimpleITK is not installed) and are pinned by their closed form

Cases (tests/test_reslice_taps_golden.py: CASES):
  oblique    (5, 9, 11) -> (2, 7, 13), an oblique cut
  oneslice   (1, 3, 2) -> (2, 4, 5): one source slice, every z position within [-0.5, 0.5) or outside
  halfvoxel  (2, 2, 2) -> (3, 3, 3), scale 0.4 and shift -0.3: positions -0.3, 0.1, 0.5 per axis, some in [-0.5, 0)
  frames     3 frames of (7, 12, 10) -> (3, 9, 66): output rows cross a wave boundary
  identity   (4, 6, 7) -> (4, 6, 7)
  flip       (4, 6, 7) -> (7, 6, 4): exact integers, (z, y, x) = (xo, Y - 1 - yo, zo)
  samegrid   (4, 6, 7) -> (4, 6, 7): an oblique geometry onto its own grid, the matrix composed as inv(T R S) @ (T R S) in float64: the identity
             with rounding noise, so some positions are -1e-17 where the exact value is 0 and p - floor(p) rounds to exactly 1.0 (asserted here)
  halfgrid   (4, 6, 7) -> (7, 11, 13): the same geometry onto a grid of half the spacing with the same origin
In each oblique case between 10 % and 60 % of the output voxels are outside (asserted here): both branches of the inside rule run.

Run:  python tests/make_golden_reslice_taps.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_reslice_taps_golden as tt  # noqa: E402

MATRICES = {
    "oblique": [[0.83, 0.21, 1.9, -0.7], [-0.17, 1.31, 0.6, -0.9], [0.05, -0.12, 2.6, 1.2]],
    "oneslice": [[0.45, 0.05, 0.1, -0.2], [0.1, 0.61, 0.2, -0.1], [0.02, 0.21, 0.3, -0.45]],
    "halfvoxel": [[0.4, 0.0, 0.0, -0.3], [0.0, 0.4, 0.0, -0.3], [0.0, 0.0, 0.4, -0.3]],
    "frames": [[0.151, 0.09, 0.7, -0.6], [-0.031, 1.37, 0.9, -0.8], [0.047, 0.33, 1.9, -0.2]],
    "identity": [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
    "flip": [[0.0, 0.0, 1.0, 0.0], [0.0, -1.0, 0.0, 5.0], [1.0, 0.0, 0.0, 0.0]],
}


def index_to_world(spacing, origin, direction):
    S, R, T = np.eye(4), np.eye(4), np.eye(4)
    S[:3, :3], R[:3, :3], T[:3, 3] = np.diag(spacing), direction, origin
    return T @ R @ S


def composed(ref_spacing):
    """``inv(T R S) @ (T_r R S_r)`` for a stack of 1.4 x 1.4 x 2.5 mm turned 0.3 rad about (1, 2, 3) and a grid of ``ref_spacing`` with the same
    origin and direction: exact up to the rounding noise of the inverse and the products, which is the point of the case"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    R = np.eye(3) + np.sin(0.3) * K + (1.0 - np.cos(0.3)) * (K @ K)
    origin = (-120.3, -85.1, 40.7)
    return (np.linalg.inv(index_to_world((1.4, 1.4, 2.5), origin, R)) @ index_to_world(ref_spacing, origin, R))[:3]


MATRICES["samegrid"] = composed((1.4, 1.4, 2.5))
MATRICES["halfgrid"] = composed((0.7, 0.7, 1.25))


def main():
    rs = np.random.RandomState(20240611)
    rec = {"names": np.array(list(tt.CASES))}
    for name, (frames, src_shape, out_shape, oblique) in tt.CASES.items():
        counts = rs.randint(0, 1025, size=(frames,) + src_shape).astype(np.uint16)
        vol = (counts / tt.Q).astype(np.float32)
        M = np.array(MATRICES[name], dtype=np.float64)
        pos = tt.positions(M, out_shape)
        ok = tt.inside(pos, src_shape)
        outside = 1.0 - ok.mean()
        assert (0.10 <= outside <= 0.60) if oblique else outside == 0.0, (name, outside)
        if name in tt.NOISY:          # some positions are -1e-17 where the exact value is 0: p - floor(p) rounds to 1.0 there
            rounds_up = (pos - np.floor(pos)) == 1.0
            assert rounds_up.sum() >= 3 and (pos[rounds_up] < 0).all(), (name, int(rounds_up.sum()))
        coef = np.stack([ndimage.spline_filter(f.astype(np.float64), order=3, mode="mirror", output=np.float64) for f in vol])
        zyx = np.stack([pos[..., 2], pos[..., 1], pos[..., 0]])
        zyx = np.where(ok[None], zyx, 0.0)
        spline = np.stack([np.where(ok, ndimage.map_coordinates(f.astype(np.float64), zyx, order=3, mode="mirror", output=np.float64), 0.0) for f in vol])
        rec.update({"%s/vol" % name: counts, "%s/matrix" % name: M, "%s/coef" % name: coef, "%s/bspline" % name: spline})
        for kernel, radius in tt.SINCS:
            rec["%s/%s%d" % (name, kernel, radius)] = np.stack([tt.gather(f.astype(np.float64), pos, kernel, radius) for f in vol])
        print("%-10s %d x %s -> %s: %.1f %% outside" % (name, frames, src_shape, out_shape, 100 * outside))
    path = os.path.join(HERE, "golden", "reslice_taps.npz")
    np.savez_compressed(path, **rec)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
