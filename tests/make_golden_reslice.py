#!/usr/bin/env python
"""Generate tests/golden/reslice.npz: the REFERENCE's own ``evaluate/cardiac/resample_sax_to_lax.py`` -- ``make_lax_identity_grid`` and
``make_transform`` on float32 S / R / T matrices, then the body of its frame loop, ``grid_sample(vol[None, None], grid[None],
align_corners=True)`` on the CPU -- plus torch's ``mode='nearest'`` result on the same grid.  A script, not a test (pytest does not collect
it); it needs the reference checkout (``AESR_REFERENCE``, see oracle/make_golden.py), which the GPU box does not have.  Only data is
written: the volumes (uint16 counts of 1/1024: exact in fp32), the six 4x4 matrices in float64, the shapes, the reference's grid, its
output and the nearest output.

The module is loaded from its file with ``SimpleITK`` and ``kwatsch.create_nifti_from_dicom`` answered by empty stand-ins
(``oracle.make_golden._any_stub``): neither is used by the two grid functions.  The frame loop itself (``np.arange(n).astype(np.int)``) does
not run on current numpy, so its body is called here per frame.

Cases (tests/test_reslice_golden.py: CASES):
  oblique    SAX (13, 40, 36) at 1.4 x 1.4 x 2.5 mm, rotated 0.7 rad about (1, 2, 3), origin (-120.3, -85.1, 40.7); LAX (3, 33, 47) at
             1.1 x 1.1 x 6 mm through the SAX centre, its rows tilted off the SAX z axis: interior, the fading one-voxel border and the
             all-zero outside in one case
  oblique4d  the same geometry, 3 frames
  odd        SAX (5, 9, 11), LAX (2, 7, 13): no side is a multiple of 4
  outside    the oblique LAX grid moved 500 mm along its normal: every output exactly 0

Run:  python tests/make_golden_reslice.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

Q = 1024.0
HALF_MARGIN = 1e-4          # nearest: a coordinate this close to a half-integer may round either way (fp32 against fp64 unnormalisation)


def import_reference_module():
    mg._any_stub("SimpleITK")
    mg._any_stub("kwatsch.create_nifti_from_dicom")
    path = os.path.join(mg.REF, "evaluate", "cardiac", "resample_sax_to_lax.py")
    spec = importlib.util.spec_from_file_location("reference_resample_sax_to_lax", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rotation(axis, angle):
    """Rodrigues: float64 [3, 3]"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def srt(spacing, direction, origin):
    """(S, R, T) float64 [4, 4] each: world = T @ R @ S @ index"""
    S, R, T = np.eye(4), np.eye(4), np.eye(4)
    S[:3, :3] = np.diag(spacing)
    R[:3, :3] = direction
    T[:3, 3] = origin
    return S, R, T


def lax_through_centre(sax_shape, sax_srt, lax_shape, lax_spacing, turn, tilt, shift_mm=0.0):
    """A LAX grid whose centre voxel sits on the SAX volume's centre (+ shift_mm along the LAX normal).  In the SAX frame its x axis is
    the SAX x axis turned by ``turn`` about z, its y axis the SAX z axis tilted by ``tilt`` about that x axis: the plane holds the long
    axis of the heart, as a 2- / 4-chamber view does."""
    S, R, T = sax_srt
    ex = np.array([np.cos(turn), np.sin(turn), 0.0])
    ey = rotation(ex, tilt) @ np.array([0.0, 0.0, 1.0])
    ez = np.cross(ex, ey)
    direction = R[:3, :3] @ np.stack([ex, ey, ez], axis=1)
    centre_sax = (T @ R @ S @ np.array([(sax_shape[2] - 1) / 2, (sax_shape[1] - 1) / 2, (sax_shape[0] - 1) / 2, 1.0]))[:3]
    half = np.array([(lax_shape[2] - 1) / 2, (lax_shape[1] - 1) / 2, (lax_shape[0] - 1) / 2]) * np.asarray(lax_spacing)
    origin = centre_sax - direction @ half + shift_mm * direction[:, 2]
    return srt(lax_spacing, direction, origin)


def volume(rs, shape):
    """MRI-like [Z, Y, X] in [0, 1], multiples of 1/1024, bright up to the faces (so the fading border is visible)"""
    z, h, w = shape
    zz, yy, xx = np.mgrid[0:z, 0:h, 0:w].astype(np.float64)
    vol = 0.1 + np.zeros(shape)
    for _ in range(6):
        cz, cy, cx = rs.uniform(0, z), rs.uniform(0, h), rs.uniform(0, w)
        sz, sg, amp = rs.uniform(0.3, 0.9) * z, rs.uniform(0.1, 0.3) * min(h, w), rs.uniform(0.1, 0.4)
        vol += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg) - (zz - cz) ** 2 / (2 * sz * sz))
    vol = np.clip(vol + 0.03 * rs.randn(*shape), 0, 1)          # the noise of the sibling fixtures (tests/make_golden_long_axis.py)
    return np.round(vol * Q).astype(np.uint16)


def main():
    ref = import_reference_module()
    rs = np.random.RandomState(20241019)
    sax_big = srt((1.4, 1.4, 2.5), rotation((1, 2, 3), 0.7), (-120.3, -85.1, 40.7))
    sax_odd = srt((1.7, 1.3, 4.0), rotation((3, -1, 2), -0.4), (12.5, -7.25, -30.0))
    geo = {
        "oblique": ((13, 40, 36), sax_big, (3, 33, 47), lax_through_centre((13, 40, 36), sax_big, (3, 33, 47), (1.1, 1.1, 6.0), 0.6, 0.45), 1),
        "oblique4d": ((13, 40, 36), sax_big, (3, 33, 47), lax_through_centre((13, 40, 36), sax_big, (3, 33, 47), (1.1, 1.1, 6.0), 0.6, 0.45), 3),
        "odd": ((5, 9, 11), sax_odd, (2, 7, 13), lax_through_centre((5, 9, 11), sax_odd, (2, 7, 13), (1.2, 1.9, 3.0), -0.8, 0.3), 1),
        "outside": ((13, 40, 36), sax_big, (3, 33, 47), lax_through_centre((13, 40, 36), sax_big, (3, 33, 47), (1.1, 1.1, 6.0), 0.6, 0.45, 500.0), 1),
    }
    rec = {"tags": np.array(list(geo))}
    for tag, (sax_shape, sax_srt, lax_shape, lax_srt, frames) in geo.items():
        mats64 = np.stack(list(lax_srt) + list(sax_srt))          # S_lax, R_lax, T_lax, S_sax, R_sax, T_sax
        mats32 = [torch.from_numpy(m.astype(np.float32)) for m in mats64]
        ident = ref.make_lax_identity_grid(lax_shape)
        grid = ref.make_transform(ident, lax_shape, sax_shape, *mats32)
        assert grid.dtype == torch.float32 and tuple(grid.shape) == lax_shape + (3,)
        vols = np.stack([volume(rs, sax_shape) for _ in range(frames)])
        lin, near = [], []
        for f in range(frames):
            v = torch.from_numpy((vols[f] / Q).astype(np.float32))
            lin.append(torch.nn.functional.grid_sample(v[None, None], grid[None], align_corners=True).squeeze().numpy())
            near.append(torch.nn.functional.grid_sample(v[None, None], grid[None], mode="nearest", align_corners=True).squeeze().numpy())
        lin, near = np.stack(lin).astype(np.float32), np.stack(near).astype(np.float32)
        rec["%s/vol" % tag] = vols if frames > 1 else vols[0]
        rec["%s/matrices" % tag] = mats64
        rec["%s/sax_shape" % tag] = np.array(sax_shape, dtype=np.int64)
        rec["%s/lax_shape" % tag] = np.array(lax_shape, dtype=np.int64)
        rec["%s/grid" % tag] = grid.numpy()
        rec["%s/linear" % tag] = lin if frames > 1 else lin[0]
        rec["%s/nearest" % tag] = near if frames > 1 else near[0]
        if tag == "odd":
            rec["odd/ident"] = ident.numpy()
            rec["odd/ident_first"] = ref.make_identity_grid(lax_shape, stackdim="first").numpy()
        # what the case exercises
        size = np.array(sax_shape[::-1], dtype=np.float64)
        c = (grid.numpy().astype(np.float64) + 1) / 2 * (size - 1)
        inside = np.all((c >= 0) & (c <= size - 1), axis=-1).mean()
        border = (np.all((c > -1) & (c < size), axis=-1)).mean() - inside
        near_half = (np.abs(c - np.floor(c) - 0.5) < HALF_MARGIN).any(axis=-1).mean()
        print("%-10s inside %.3f, fading border %.3f, outside %.3f; within %.0e of a half-integer %.4f; nonzero outputs %.3f"
              % (tag, inside, border, 1 - inside - border, HALF_MARGIN, near_half, float((lin != 0).mean())))
        assert near_half <= 0.01, tag
    out = os.path.join(HERE, "golden", "reslice.npz")
    np.savez_compressed(out, **rec)
    print("reslice.npz: %d bytes" % os.path.getsize(out))


if __name__ == "__main__":
    main()
