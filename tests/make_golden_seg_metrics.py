#!/usr/bin/env python
"""Generate tests/golden/seg_metrics.npz from the REFERENCE's own kwatsch/medpy_metrics.py (imported from the reference checkout,
``AESR_REFERENCE`` as in oracle/make_golden.py; nothing of it is copied).  A script, not a test; the GPU box does not have the
reference.  Only data is written: the label volumes and, per class, neighbourhood dimension, connectivity and direction, the list the
reference's ``__surface_distances`` returns and its dc / jc / precision / recall / specificity / ravd / hd / hd95 / asd / assd.

Keys.  ``cases`` names the cases; per case ``<case>/result``, ``<case>/reference`` (fp32 class ids, [H, W], [Z, H, W] or [N, Z, H, W]),
``<case>/spacing`` (one entry per axis of a frame), ``<case>/classes``, ``<case>/empty`` (classes absent from one side on purpose).
Per frame n and class c: ``<case>/n<n>/c<c>/overlap`` = (dc, jc, precision, recall, specificity, ravd), NaN where the reference raises;
and per ``d<ndim>/k<connectivity>``: ``sds_rg`` (result -> reference), ``sds_gr``, ``scores`` = (hd, hd95, asd_rg, asd_gr, assd).
``d2`` of a volume with Z > 1 scores every slice as an image of its own: the reference is called per slice and the lists are
concatenated in slice order; it is recorded only where no slice holds the class on one side alone (the reference raises there).
Label maps are floor(K * 0.999 * smooth blob), as the multi-channel fixtures make them."""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "golden", "seg_metrics.npz")


def reference_module():
    path = os.path.join(mg.REF, "kwatsch", "medpy_metrics.py")
    spec = importlib.util.spec_from_file_location("reference_medpy_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    assert os.path.realpath(mod.__file__).startswith(os.path.realpath(mg.REF) + os.sep)
    return mod


def blob(shape, rng, centres=None, jitter=0.0):
    """a smooth field in [0, 1] with maximum 1: a few Gaussians; returns (field, centres) so that a second field can sit nearby"""
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    if centres is None:
        centres = [(rng.uniform(0.15, 0.85, len(shape)) * np.array(shape), rng.uniform(0.18, 0.35), rng.uniform(0.5, 1.0)) for _ in range(4)]
    out = np.zeros(shape)
    for c, s, a in centres:
        c = c + jitter * rng.standard_normal(len(shape)) * np.minimum(np.array(shape) * 0.08, 2.0)
        sig = np.maximum(np.array(shape) * s, 1.2)
        out += a * np.exp(-sum(((g - ci) / si) ** 2 for g, ci, si in zip(grids, c, sig)) / 2)
    return out / out.max(), centres


def label_pair(shape, K, rng):
    ref, centres = blob(shape, rng)
    res, _ = blob(shape, rng, centres, jitter=1.0)
    return np.floor(K * 0.999 * res).astype(np.float32), np.floor(K * 0.999 * ref).astype(np.float32)


def cases():
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, res, ref, spacing, classes, empty=()):
        out.append(dict(name=name, result=res, reference=ref, spacing=np.asarray(spacing, dtype=np.float64),
                        classes=np.asarray(classes, dtype=np.int64), empty=np.asarray(empty, dtype=np.int64)))

    r, g = label_pair((6, 20, 18), 4, rng)
    add("aniso", r, g, (10.0, 1.4, 1.4), (1, 2, 3))
    r, g = label_pair((5, 7, 67), 4, rng)
    add("ties", r, g, (1.0, 1.0, 1.0), (1, 2, 3))
    r, g = label_pair((12, 64, 80), 4, rng)
    add("multiwg", r, g, (2.5, 1.25, 1.25), (1, 2, 3))
    r, g = label_pair((9, 13), 4, rng)
    add("img2d", r, g, (1.5, 0.75), (1, 2, 3))
    add("z1", r[None], g[None], (3.0, 1.5, 0.75), (1, 2, 3))
    fr = [label_pair((6, 20, 18), 4, rng) for _ in range(3)]
    add("frames", np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), (10.0, 1.4, 1.4), (1, 2, 3))
    r, g = label_pair((4, 10, 12), 8, rng)
    add("eight", r, g, (2.0, 1.0, 1.5), tuple(range(8)))
    one = np.zeros((4, 5, 6), dtype=np.float32)
    one[2, 1, 4] = 1
    add("extreme", np.ones((4, 5, 6), dtype=np.float32), one, (2.0, 1.0, 1.0), (1,))
    full = np.ones((5, 8, 9), dtype=np.float32)
    full[2, 3:5, 4:6] = 0
    cross = np.zeros((5, 8, 9), dtype=np.float32)
    cross[:, 4, 4] = cross[2, :, 4] = cross[2, 4, :] = 1
    add("faces", full, cross, (1.0, 0.5, 0.5), (1,))
    r, g = label_pair((6, 20, 18), 3, rng)
    g[g == 2] = 1
    add("oneside", r, g, (10.0, 1.4, 1.4), (1, 2), empty=(2,))
    return out


def frames_of(case):
    r, g = case["result"], case["reference"]
    if r.ndim == len(case["spacing"]):
        return [(r, g)]
    return list(zip(r, g))


def overlap(ref, a, b):
    def safe(fn):
        try:
            return float(fn(a, b))
        except (ZeroDivisionError, RuntimeError):
            return float("nan")
    return np.array([safe(ref.dc), safe(ref.jc), safe(ref.precision), safe(ref.recall), safe(ref.specificity), safe(ref.ravd)])


def main():
    ref = reference_module()
    sds = getattr(ref, "__surface_distances")
    rec = {"cases": np.asarray([c["name"] for c in cases()])}
    sliced = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for case in cases():
            name = case["name"]
            for k in ("result", "reference", "spacing", "classes", "empty"):
                rec["%s/%s" % (name, k)] = case[k]
            rank = len(case["spacing"])
            for n, (r, g) in enumerate(frames_of(case)):
                for c in case["classes"]:
                    a, b = r == c, g == c
                    key = "%s/n%d/c%d" % (name, n, c)
                    rec[key + "/overlap"] = overlap(ref, a, b)
                    if c in case["empty"]:
                        assert a.any() != b.any(), "%s: class %d was to be present on one side only" % (name, c)
                        continue
                    # what the tests rely on: every other requested class is non-empty on both sides
                    assert a.any() and b.any(), "%s frame %d: class %d is empty on a side" % (name, n, c)
                    modes = [2] if rank == 2 else [3, 2]
                    for nd in modes:
                        for conn in range(1, nd + 1):
                            if nd == rank:
                                rg = sds(a, b, tuple(case["spacing"]), conn)
                                gr = sds(b, a, tuple(case["spacing"]), conn)
                                scores = [ref.hd(a, b, tuple(case["spacing"]), conn), ref.hd95(a, b, tuple(case["spacing"]), conn),
                                          ref.asd(a, b, tuple(case["spacing"]), conn), ref.asd(b, a, tuple(case["spacing"]), conn),
                                          ref.assd(a, b, tuple(case["spacing"]), conn)]
                            else:
                                if any(az.any() != bz.any() for az, bz in zip(a, b)):
                                    continue          # a slice holds the class on one side only: the reference raises for that slice
                                sp = tuple(case["spacing"][1:])
                                rg = np.concatenate([sds(az, bz, sp, conn) for az, bz in zip(a, b) if az.any()])
                                gr = np.concatenate([sds(bz, az, sp, conn) for az, bz in zip(a, b) if az.any()])
                                scores = [max(rg.max(), gr.max()), np.percentile(np.hstack((rg, gr)), 95), rg.mean(), gr.mean(),
                                          (rg.mean() + gr.mean()) / 2]
                                sliced += a.shape[0] > 1
                            sub = "%s/d%d/k%d" % (key, nd, conn)
                            rec[sub + "/sds_rg"], rec[sub + "/sds_gr"] = np.asarray(rg, np.float64), np.asarray(gr, np.float64)
                            rec[sub + "/scores"] = np.asarray(scores, dtype=np.float64)
    assert sliced >= 4, "too few slice-wise (ndim = 2 on a volume) records: %d" % sliced
    np.savez_compressed(OUT, **rec)
    print("%s: %d arrays, %d slice-wise records, %.1f KB" % (OUT, len(rec), sliced, os.path.getsize(OUT) / 1024.0))


if __name__ == "__main__":
    main()
