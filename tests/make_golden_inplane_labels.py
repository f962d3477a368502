#!/usr/bin/env python
"""Generate tests/golden/inplane_labels.npz: the REFERENCE's own ``datasets.common.apply_2d_zoom_3d`` / ``apply_2d_zoom_4d`` with
``order=0, do_blur=False, as_type=int`` -- how its ``ACDCImage`` resamples a label map (scipy.ndimage.zoom(order=0) on the CPU).  A script,
not a test (pytest does not collect it); it needs the reference checkout (``AESR_REFERENCE``, see oracle/make_golden.py), which the GPU box
does not have.  Only data is written.

The reference is imported by ``tests/make_golden_inplane.py::import_reference_common`` (its checkout ahead on ``sys.path``, ``__file__``
asserted to lie under it, empty stand-ins for packages the path never calls, ``np.int = int``).

Label volumes hold the values 1 .. 4 -- no 0, so that the 0 of a dead last row / column (scipy's ``constant`` boundary where rounding puts
the last coordinate past the edge) is visible.  Cases: the (size, spacing) pairs of the small cases of tests/golden/inplane.npz, among
them the two dead-line pairs (``d_quirk``, ``d_quirk224``); ``t_ties`` (13 x 9 at 2.66 mm -> 25 x 17: every second coordinate is an exact
.5) and the 4-D case.  The script asserts that dead lines and ties occur.

Per case: ``<tag>/in`` (uint8), ``<tag>/out`` (int64, what the reference returned), ``<tag>/spacing``, ``<tag>/new_spacing``; ``tags``.

Run:  python tests/make_golden_inplane_labels.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_inplane as mgi  # noqa: E402

CASES = [  # tag, shape, spacing, new_spacing
    ("a_in_125", (3, 60, 70), (10.0, 1.25, 1.25), (10.0, 1.4, 1.4)),
    ("a_in_168", (2, 62, 68), (8.0, 1.68, 1.68), (1.4, 1.4)),
    ("a_back_125", (2, 54, 62), (8.0, 1.4, 1.4), (8.0, 1.25, 1.25)),
    ("a_back_15625", (3, 67, 76), (1.4, 1.4), (1.5625, 1.5625)),
    ("b_nonsquare", (2, 101, 77), (8.0, 1.37, 1.41), (1.4, 1.4)),
    ("c_radius2", (2, 50, 44), (8.0, 0.7, 0.7), (1.4, 1.4)),
    ("d_quirk", (2, 47, 61), (8.0, 1.25, 0.7), (1.4, 1.4)),
    ("d_quirk224", (1, 229, 26), (8.0, 1.37, 1.25), (1.4, 1.4)),
    ("e_tiny_identity", (2, 13, 9), (8.0, 1.4, 1.4), (1.4, 1.4)),
    ("e_tiny_10", (2, 13, 9), (8.0, 1.0, 1.0), (1.4, 1.4)),
    ("e_tiny_21", (2, 13, 9), (8.0, 2.1, 2.1), (1.4, 1.4)),
    ("e_tiny_mixed", (2, 13, 9), (8.0, 0.9, 1.9), (1.4, 1.4)),
    ("t_ties", (2, 13, 9), (8.0, 2.66, 2.66), (1.4, 1.4)),
    ("g_4d", (3, 4, 40, 48), (8.0, 1.5625, 1.5625), (1.4, 1.4)),
]
DEAD = {"d_quirk": (True, True), "d_quirk224": (True, True)}          # (dead last row, dead last column); every other case has none


def labels(rs, shape):
    """Values 1 .. 4: background 1 and three discs per slice; the last row and column carry all four, so a dead line differs from any."""
    h, w = shape[-2:]
    n = int(np.prod(shape[:-2]))
    yy, xx = np.mgrid[0:h, 0:w]
    lab = np.ones((n, h, w), np.uint8)
    for s in range(n):
        for v in (2, 3, 4):
            cy, cx, r = rs.uniform(0.2 * h, 0.8 * h), rs.uniform(0.2 * w, 0.8 * w), rs.uniform(0.12, 0.3) * min(h, w)
            lab[s][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = v
        lab[s, -1, :] = 1 + (np.arange(w) + s) % 4
        lab[s, :, -1] = 1 + (np.arange(h) + s) % 4
    return lab.reshape(shape)


def has_tie(n, n_out):
    c = np.arange(n_out, dtype=np.float64) * (np.float64(n - 1) / np.float64(n_out - 1))
    return bool((c - np.floor(c) == 0.5).any())


def main():
    dc = mgi.import_reference_common()
    rs = np.random.RandomState(20241021)
    rec, tags, ties, dead = {}, [], 0, 0
    for tag, shape, spacing, new_spacing in CASES:
        lab = labels(rs, shape)
        fn = dc.apply_2d_zoom_4d if lab.ndim == 4 else dc.apply_2d_zoom_3d
        given = lab.astype(np.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = fn(given, spacing, new_spacing, order=0, do_blur=False, as_type=int)
        assert np.array_equal(given, lab), "the reference changed its input"
        assert out.dtype == np.int64 and set(np.unique(out)) <= {0, 1, 2, 3, 4}
        flat = out.reshape((-1,) + out.shape[-2:])
        row, col = DEAD.get(tag, (False, False))
        assert bool((flat[:, -1, :] == 0).all()) == row and bool((flat[:, :, -1] == 0).all()) == col, tag
        assert (flat[:, :-1, :-1] > 0).all(), tag          # a 0 can only come from a dead line
        dead += int(row) + int(col)
        ties += int(has_tie(shape[-2], out.shape[-2])) + int(has_tie(shape[-1], out.shape[-1]))
        rec[tag + "/in"], rec[tag + "/out"] = lab, out
        rec[tag + "/spacing"], rec[tag + "/new_spacing"] = np.array(spacing, np.float64), np.array(new_spacing, np.float64)
        tags.append(tag)
        print("  %-18s %s -> %s" % (tag, lab.shape, out.shape))
    assert dead >= 4 and ties >= 2 and has_tie(13, 25) and has_tie(9, 17), (dead, ties)
    assert rec["t_ties/out"].shape == (2, 25, 17) and rec["g_4d/out"].ndim == 4
    rec["tags"] = np.array(tags)
    path = os.path.join(HERE, "golden", "inplane_labels.npz")
    np.savez_compressed(path, **rec)
    print("inplane_labels.npz: %d bytes, %d cases, %d dead lines, %d axes with exact ties" % (os.path.getsize(path), len(tags), dead, ties))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
