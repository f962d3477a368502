#!/usr/bin/env python
"""Generate tests/golden/inplane.npz: the REFERENCE's own ``datasets.common.apply_2d_zoom_3d`` / ``apply_2d_zoom_4d`` (scipy on the CPU).
A script, not a test (pytest does not collect it); it needs the reference checkout (``AESR_REFERENCE``, see oracle/make_golden.py), which
the GPU box does not have.  Only data is written.

This repository has a root package named ``datasets`` too (the import-path shim), so the reference checkout is put AHEAD of the
repository root on ``sys.path`` (``oracle.make_golden.import_reference()`` does that) and ``datasets.common.__file__`` is asserted to lie
under the reference before anything is called.  Packages the module imports at its top and this path never calls (SimpleITK,
torchvision.datasets, ...) are answered with empty stand-ins.  The ONE behavioural shim: ``np.int = int`` -- the reference compares
``as_type == np.int``, a name numpy 2 no longer has.  scipy's deprecation warning for ``ndimage.interpolation`` is silenced.

Per case: ``<tag>/in`` (uint16 counts of 1/1024 for images, int64 for labels), ``<tag>/out`` (what the reference returned), ``<tag>/spacing``,
``<tag>/new_spacing``, ``<tag>/do_blur``, ``<tag>/labels``; ``tags`` lists the cases.  The reference blurs into the array it is given, so it
gets a copy.  Every array is handed over as float32 -- the labels 0..3 too (``do_blur=False``, ``as_type=int``: rounded and cast by the
reference): an integer-typed array would have scipy truncate the interpolated values, a case the device path does not reproduce.

Run:  python tests/make_golden_inplane.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

Q = 1024.0          # intensities are multiples of 1/1024: exact in fp32, stored as uint16 counts


def import_reference_common():
    np.int = int
    mg.import_reference()
    tv = sys.modules["torchvision"]
    for sub in ("datasets", "transforms", "utils"):
        setattr(tv, sub, mg._any_stub("torchvision." + sub))
    for _ in range(64):
        try:
            import datasets.common as dc
            break
        except ModuleNotFoundError as e:
            mg._any_stub(e.name)
    else:
        raise RuntimeError("could not import the reference's datasets.common")
    ref = os.path.realpath(mg.REF)
    assert os.path.realpath(dc.__file__).startswith(ref + os.sep), "datasets.common came from %s, not from the reference" % dc.__file__
    return dc


def image(rs, shape):
    """MRI-like slices in [0, 1]: a few blobs per slice plus noise, as uint16 counts of 1/1024."""
    h, w = shape[-2:]
    n = int(np.prod(shape[:-2]))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, h, w))
    for s in range(n):
        for _ in range(5):
            cy, cx = rs.uniform(0.1 * h, 0.9 * h), rs.uniform(0.1 * w, 0.9 * w)
            sg, amp = rs.uniform(0.05, 0.3) * min(h, w) + 0.7, rs.uniform(0.2, 0.8)
            out[s] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
        out[s] += 0.04 * rs.randn(h, w)
    return np.round(np.clip(out, 0, 1) * Q).astype(np.uint16).reshape(shape)


CASES = [  # tag, shape, spacing, new_spacing
    ("a_full", (1, 216, 256), (8.0, 1.5625, 1.5625), (1.4, 1.4)),
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
    ("g_4d", (3, 4, 40, 48), (8.0, 1.5625, 1.5625), (1.4, 1.4)),
]
LABEL_CASES = [
    ("f_labels_15625", (3, 40, 36), (8.0, 1.5625, 1.5625), (1.4, 1.4)),
    ("f_labels_125", (2, 40, 36), (8.0, 1.25, 1.25), (1.4, 1.4)),
]
# (tag, dead last row, dead last column) for the cases that have such a line; every other case must have none
DEAD = {"d_quirk": (True, True), "d_quirk224": (True, True)}          # 26 -> 23 at 1.25 mm ends in a dead column too


def main():
    dc = import_reference_common()
    rs = np.random.RandomState(20241016)
    rec, tags = {}, []

    def run(tag, arr, spacing, new_spacing, do_blur, as_type):
        fn = dc.apply_2d_zoom_4d if arr.ndim == 4 else dc.apply_2d_zoom_3d
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = fn(arr.copy(), spacing, new_spacing, order=1, do_blur=do_blur, as_type=as_type)
        tags.append(tag)
        rec[tag + "/spacing"], rec[tag + "/new_spacing"] = np.array(spacing, np.float64), np.array(new_spacing, np.float64)
        rec[tag + "/do_blur"], rec[tag + "/labels"] = np.array(do_blur), np.array(as_type is int)
        rec[tag + "/out"] = out
        return out

    for tag, shape, spacing, new_spacing in CASES:
        counts = image(rs, shape)
        rec[tag + "/in"] = counts
        out = run(tag, (counts / Q).astype(np.float32), spacing, new_spacing, True, np.float32)
        assert out.dtype == np.float32, out.dtype
        row, col = DEAD.get(tag, (False, False))
        flat = out.reshape((-1,) + out.shape[-2:])
        assert bool((flat[:, -1, :] == 0).all()) == row and bool((flat[:, :, -1] == 0).all()) == col, tag
        assert flat[:, :-1, :-1].max() > 0.1
    assert rec["a_full/out"].shape == (1, 241, 286) and rec["d_quirk/out"].shape == (2, 42, 30) and rec["d_quirk224/out"].shape == (1, 224, 23)
    for tag, shape, spacing, new_spacing in LABEL_CASES:
        lab = np.zeros(shape, np.int64)
        h, w = shape[-2:]
        yy, xx = np.mgrid[0:h, 0:w]
        for s in range(shape[0]):
            for v in (1, 2, 3):
                cy, cx, r = rs.uniform(0.3 * h, 0.7 * h), rs.uniform(0.3 * w, 0.7 * w), rs.uniform(0.1, 0.25) * min(h, w)
                lab[s][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = v
        rec[tag + "/in"] = lab
        out = run(tag, lab.astype(np.float32), spacing, new_spacing, False, int)
        assert out.dtype == np.int64 and set(np.unique(out)) <= {0, 1, 2, 3}
    rec["tags"] = np.array(tags)
    path = os.path.join(HERE, "golden", "inplane.npz")
    np.savez_compressed(path, **rec)
    print("inplane.npz: %d bytes, %d cases" % (os.path.getsize(path), len(tags)))
    for tag in tags:
        print("  %-18s %s -> %s" % (tag, rec[tag + "/in"].shape, rec[tag + "/out"].shape))


if __name__ == "__main__":
    main()
