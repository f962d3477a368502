#!/usr/bin/env python
"""Writes tests/golden/shape_interp.npz: small label volumes and what shape-based interpolation (include/aesr_hip_shape.h) makes of them when the
signed distance maps come from scipy.  scipy and numpy only; run from the repository root:  python tests/make_golden_shape_interp.py

Per case: the label volume (uint8 [N, Z, H, W]), classes, spacing (sy, sx), the grid (gap, alpha), scipy's signed maps --
+-``distance_transform_edt(mask or ~mask, sampling=(sy, sx))`` per slice, +-BIG where the set to minimise over is empty --, the labels the
blend and arg-max rule gives on those maps in numpy fp64, and the margin between the best and the second-best blended value of every voxel.

Volumes are overlapping discs and boxes that move and shrink from slice to slice (seeded RandomState).  Labels are compared only where the
margin exceeds 1e-9 * BIG, and that rule may leave out at most 0.1 % of a case: a volume whose blended maps tie (a pixel as deep inside a
class in one slice as it is outside it in the next, at alpha 1/2) says nothing about a kernel, so a case takes the first seed, counted up
from its own, whose volume meets the cap -- judged on scipy's maps alone, and asserted for the numpy restatement of
tests/test_shape_interp_golden.py as well before anything is written."""
import os
import sys

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import test_shape_interp_golden as tm  # noqa: E402
from superresolution_aniso_mri_amd.evaluate.z_grid import target_grid  # noqa: E402

OUT = os.path.join(HERE, "golden", "shape_interp.npz")
YCHUNK = 128          # SHP_YCHUNK of csrc/shape_interp.hip: the y pass stages this many rows at a time

# name: (N, Z, H, W, classes, (sy, sx), grid, special)
CASES = [
    ("w1", 1, 2, 9, 1, [0, 1], (1.0, 1.0), ("n", 1), None),                          # one column; H W % 4 != 0
    ("w63", 1, 3, 5, 63, [0, 1], (1.25, 1.5), ("n", 1), None),                       # one ballot word, not full
    ("w64", 1, 2, 4, 64, [0, 1, 2, 3], (1.0, 1.0), ("n", 6), None),                  # exactly one word; H W % 4 == 0
    ("w65", 1, 2, 3, 65, [0, 1], (1.0, 1.0), ("n", 1), None),                        # one pixel in the second word
    ("w130", 1, 2, 4, 130, [0, 2], (1.25, 1.5), ("n", 6), None),                     # three words
    ("h1", 1, 2, 1, 37, [0, 1], (1.0, 1.0), ("n", 1), None),                         # one row
    ("ychunk", 1, 2, YCHUNK + 1, 8, [0, 1], (1.0, 1.0), ("n", 1), None),             # the y pass takes a second chunk of one row
    ("z1", 1, 1, 7, 9, [0, 1], (1.25, 1.5), ("n", 1), None),                         # a single slice: J = 1
    ("bgonly", 1, 2, 5, 6, [0], (1.0, 1.0), ("n", 6), "empty"),                      # C = 1: background only
    ("eight", 1, 3, 12, 14, [0, 1, 2, 3, 4, 5, 6, 7], (1.0, 1.0), ("n", 6), None),   # C = 8
    ("oneslice", 1, 3, 10, 12, [0, 1, 2], (1.25, 1.5), ("n", 6), "oneslice"),        # class 2 in one slice only; class 1 fills a slice
    ("z7", 1, 7, 12, 20, [0, 1, 2, 3], (1.0, 1.0), ("n", 6), None),                  # Z = 7, 43 output slices
    ("frames", 2, 5, 10, 12, [0, 1, 2, 5], (1.25, 1.5), ("target", 10.0, 1.4), None),  # N = 2, the 29 slices of 10 mm at 1.4 mm
]


def volume(rng, N, Z, H, W, classes, special):
    """discs and boxes, one per foreground class, later classes painted over earlier ones; each moves and shrinks linearly along z"""
    lab = np.full((N, Z, H, W), classes[0], dtype=np.uint8)
    if special == "empty":
        return lab
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for n in range(N):
        for k, c in enumerate(classes[1:]):
            cy, cx = rng.uniform(0.25, 0.75) * (H - 1), rng.uniform(0.25, 0.75) * (W - 1)
            vy, vx = rng.uniform(-1.0, 1.0) * H / (4.0 * max(Z, 1)), rng.uniform(-1.0, 1.0) * W / (4.0 * max(Z, 1))
            r0 = rng.uniform(0.3, 0.55) * max(min(H, W), 4)
            r0 = max(r0, 0.3 * max(H, W)) if min(H, W) == 1 else r0
            shrink = rng.uniform(0.3, 0.7)
            box = rng.rand() < 0.5
            for z in range(Z):
                t = z / float(max(Z - 1, 1))
                r = r0 * (1.0 - shrink * t)
                dy, dx = yy - (cy + vy * z), xx - (cx + vx * z)
                inside = (np.maximum(np.abs(dy), np.abs(dx) * 0.8) <= r) if box else (dy * dy + dx * dx <= r * r)
                lab[n, z][inside] = c
    if special == "oneslice":
        keep = lab[0, 1] == classes[2]
        assert keep.any()
        lab[lab == classes[2]] = classes[0]
        lab[0, 1][keep] = classes[2]          # class 2 lives in slice 1 alone
        lab[0, 2] = classes[1]                # class 1 fills slice 2
    return lab


def scipy_maps(lab, classes, sy, sx):
    N, Z, H, W = lab.shape
    big = tm.big_of(H, W, sy, sx)
    out = np.empty((N, len(classes), Z, H, W), dtype=np.float64)
    for n in range(N):
        for z in range(Z):
            for ci, c in enumerate(classes):
                M = lab[n, z] == c
                if M.all():
                    out[n, ci, z] = big
                elif not M.any():
                    out[n, ci, z] = -big
                else:
                    out[n, ci, z] = np.where(M, ndi.distance_transform_edt(M, sampling=(sy, sx)), -ndi.distance_transform_edt(~M, sampling=(sy, sx)))
    return out


def make_grid(Z, spec):
    return target_grid(Z, 1.0, 1.0 / (spec[1] + 1)) if spec[0] == "n" else target_grid(Z, spec[1], spec[2])


def main():
    rec, names = {}, []
    for index, (name, N, Z, H, W, classes, (sy, sx), gspec, special) in enumerate(CASES):
        grid = make_grid(Z, gspec)
        big = tm.big_of(H, W, sy, sx)
        for seed in range(1000 * index, 1000 * index + 500):
            lab = volume(np.random.RandomState(seed), N, Z, H, W, classes, special)
            if special != "empty" and any(not (lab == c).any() for c in classes):
                continue          # every class of the list occurs somewhere
            sdm = scipy_maps(lab, classes, sy, sx)
            out, margin = tm.blend_np(sdm, grid.gap, grid.alpha, classes)
            if (~(margin > tm.MARGIN * big)).mean() <= tm.LEFT_OUT_CAP:
                break
        else:
            raise SystemExit("%s: no seed gives a volume that meets the cap" % name)
        changed = sum(int((lab[:, z] != lab[:, z + 1]).sum()) for z in range(Z - 1))
        assert Z == 1 or special == "empty" or changed > 0, name
        rec.update({name + "/labels": lab, name + "/classes": np.asarray(classes, dtype=np.int64), name + "/spacing": np.asarray([sy, sx]),
                    name + "/gap": grid.gap.astype(np.int64), name + "/alpha": grid.alpha.astype(np.float64), name + "/sdm": sdm,
                    name + "/out": out, name + "/margin": margin, name + "/seed": np.asarray(seed)})
        names.append(name)
        print("%-9s seed %5d  N %d Z %d H %3d W %3d C %d  J %2d  pixels that change between slices %4d  voxels under the margin %d of %d"
              % (name, seed, N, Z, H, W, len(classes), grid.J, changed, int((~(margin > tm.MARGIN * big)).sum()), margin.size))
    assert names == tm.CASES
    rec["names"] = np.asarray(names)
    # the restatement meets the conditions on this fixture before it is written: maps within the bound, labels under the margin rule, the cap
    tm._CACHE.clear()
    tm._CACHE["rec"] = rec
    for name in names:
        c = tm.case(name)
        maps, labels = tm.restated(name)
        assert np.abs(maps - c["sdm"]).max() <= tm.MAP_BOUND * c["big"], name
        tm.assert_labels_match_fixture(labels, c, name)
    np.savez_compressed(OUT, **rec)
    print("%s: %d cases, %.1f KB" % (OUT, len(names), os.path.getsize(OUT) / 1024.0))


if __name__ == "__main__":
    main()
