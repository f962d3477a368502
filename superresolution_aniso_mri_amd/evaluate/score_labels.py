"""Score label volumes against reference label volumes on the device.

    python -m superresolution_aniso_mri_amd.evaluate.score_labels --pred DIR|FILE --ref DIR|FILE [--classes 1 2 3] [--ndim 2|3]
                                                                   [--connectivity k] [--spacing Z Y X] [--out scores.npz]
                                                                   [--objects] [--largest_component]

Files are NIfTI (.nii, .nii.gz), MetaImage (.mha, .mhd) or .npy; with directories they are matched by name and a file without a partner is
an error.  The spacing comes from the header of the reference file; .npy has none and needs --spacing.  A 4-D file is a series of frames.
Prints one table (mean over files and frames per class, and the mean over classes) and writes every array with --out.
--objects adds the object-wise scores of evaluate/object_metrics.py (obj_tpr, obj_fpr, obj_assd and what they are made of) to the table and
to --out; --largest_component keeps only the largest connected component of every class of the prediction before anything is scored."""
import argparse
import os
import sys

import numpy as np

from .. import volume_io
from . import seg_metrics
from .object_metrics import OBJECT_KEYS

EXTENSIONS = (".nii.gz", ".nii", ".mha", ".mhd", ".npy")
TABLE_KEYS = ("dice", "jc", "hd", "hd95", "assd", "ravd")
OBJECT_TABLE_KEYS = ("obj_tpr", "obj_fpr", "obj_assd")


def _stem(name):
    low = name.lower()
    for ext in EXTENSIONS:
        if low.endswith(ext):
            return name[:-len(ext)]
    return None


def _files(path):
    """{stem: path} of one file or of the volume files of a directory"""
    if os.path.isdir(path):
        found = {}
        for name in sorted(os.listdir(path)):
            stem = _stem(name)
            if stem is not None and os.path.isfile(os.path.join(path, name)):
                if stem in found:
                    raise ValueError("%s holds %s twice (different formats)" % (path, stem))
                found[stem] = os.path.join(path, name)
        return found
    if not os.path.isfile(path) or _stem(os.path.basename(path)) is None:
        raise ValueError("%s is neither a directory nor a volume file (%s)" % (path, ", ".join(EXTENSIONS)))
    return {_stem(os.path.basename(path)): path}


def match_files(pred, ref):
    """[(name, pred_path, ref_path)]; two single files are a pair whatever their names"""
    p, r = _files(pred), _files(ref)
    if not os.path.isdir(pred) and not os.path.isdir(ref):
        return [(next(iter(r)), next(iter(p.values())), next(iter(r.values())))]
    lonely = sorted(set(p) ^ set(r))
    if lonely:
        raise ValueError("no partner for: %s" % ", ".join(lonely))
    if not p:
        raise ValueError("no volume files in %s" % pred)
    return [(k, p[k], r[k]) for k in sorted(p)]


def read_labels(path, spacing=None):
    """(array [N, Z, H, W] float32, spacing (z, y, x)); ``spacing`` overrides the header and is required for .npy"""
    if path.lower().endswith(".npy"):
        if spacing is None:
            raise ValueError("%s: a .npy file carries no spacing, give --spacing Z Y X" % path)
        arr = np.load(path)
    else:
        vol = volume_io.read_volume(path)
        arr = vol.array
        if spacing is None:
            spacing = (vol.spacing[2], vol.spacing[1], vol.spacing[0])
    if arr.ndim == 3:
        arr = arr[None]
    if arr.ndim != 4:
        raise ValueError("%s: label volumes are [z, y, x] or [t, z, y, x], got shape %s" % (path, arr.shape))
    return np.ascontiguousarray(arr, dtype=np.float32), tuple(float(s) for s in spacing)


def score_files(pairs, classes=None, ndim=3, connectivity=1, spacing=None, objects=False, largest_component=False):
    """pairs of match_files -> dict of arrays [frames of all files, C] (the keys of segmentation_scores) + names, frame_of.
    ``objects``: the keys of object_metrics.object_scores as well; ``largest_component``: the prediction is cleaned first."""
    rows, names = [], []
    if classes is None:          # one class list for every file: 1 ... the largest label of any reference
        top = max(float(read_labels(rpath, spacing)[0].max()) for _, _, rpath in pairs)
        if not top >= 1:
            raise ValueError("the reference volumes hold no label >= 1")
        classes = list(range(1, int(top) + 1))
    for name, ppath, rpath in pairs:
        ref, sp = read_labels(rpath, spacing)
        pred, _ = read_labels(ppath, sp)
        if pred.shape != ref.shape:
            raise ValueError("%s: prediction %s and reference %s differ in shape" % (name, pred.shape, ref.shape))
        if largest_component:
            from .components import keep_largest_component
            pred = keep_largest_component(pred, classes=classes, ndim=ndim, connectivity=connectivity)
        row = seg_metrics.segmentation_scores(pred, ref, sp, classes=classes, ndim=ndim, connectivity=connectivity)
        if objects:
            from .object_metrics import object_scores
            obj = object_scores(pred, ref, sp, classes=classes, ndim=ndim, connectivity=connectivity)
            row.update({k: obj[k] for k in OBJECT_KEYS})
        rows.append(row)
        names += [name] * ref.shape[0]
    out = {k: np.concatenate([row[k] for row in rows]) for k in rows[0] if k != "classes"}
    out["classes"] = rows[0]["classes"]
    out["names"] = np.asarray(names)
    return out


def format_table(scores):
    keys = TABLE_KEYS + tuple(k for k in OBJECT_TABLE_KEYS if k in scores)
    lines = ["%-8s" % "class" + "".join("%12s" % k for k in keys)]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # a class that is empty everywhere: the mean of nothing is NaN
        means = {k: np.nanmean(scores[k], axis=0) for k in keys}
        for i, c in enumerate(scores["classes"]):
            lines.append("%-8d" % c + "".join("%12.4f" % means[k][i] for k in keys))
        lines.append("%-8s" % "mean" + "".join("%12.4f" % np.nanmean(means[k]) for k in keys))
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred", required=True)
    ap.add_argument("--ref", required=True)
    ap.add_argument("--classes", type=int, nargs="+", default=None)
    ap.add_argument("--ndim", type=int, choices=(2, 3), default=3)
    ap.add_argument("--connectivity", type=int, default=1)
    ap.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("Z", "Y", "X"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--objects", action="store_true", help="add the object-wise scores (obj_tpr, obj_fpr, obj_asd, obj_assd)")
    ap.add_argument("--largest_component", action="store_true", help="keep the largest component of every class of the prediction")
    args = ap.parse_args(argv)
    try:
        pairs = match_files(args.pred, args.ref)
        scores = score_files(pairs, args.classes, args.ndim, args.connectivity, args.spacing, args.objects, args.largest_component)
    except ValueError as e:
        ap.error(str(e))
    print("%d file(s), %d frame(s), ndim=%d, connectivity=%d" % (len(pairs), len(scores["names"]), args.ndim, args.connectivity))
    print(format_table(scores))
    if args.out:
        np.savez(args.out, **scores)
    return scores


if __name__ == "__main__":
    main(sys.argv[1:])
