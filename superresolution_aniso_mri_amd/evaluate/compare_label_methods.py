"""Label-map interpolation methods side by side on held-out slices: the nearest slice, shape-based interpolation
(``evaluate.shape_interp``) and, with an experiment, the multi-channel model.

    python -m superresolution_aniso_mri_amd.evaluate.compare_label_methods --labels_dir L --downsample_steps K
                                                    [--exper_dir E --volumes_dir V --model_nbr M] [--classes 1 2 3] [--spacing Z Y X] [--out scores.npz]

Every label volume of L (.nii / .nii.gz / .mha / .mhd / .npy; each frame of a 4-D file counts as a volume) keeps every K-th slice; the
slices in between are interpolated by each method, cut and extended as ``create_simple_interpolation(generate_inbetween_slices=True)``
does, and scored against the full label volume by ``seg_metrics.segmentation_scores``.  With --exper_dir and --volumes_dir (the images,
matched to the label files by name) the model of E is scored through ``seg_metrics.score_label_supervolume`` on the same reference.
Prints one table -- mean Dice, HD95 and ASSD per method and class -- and writes every table with --out (keys ``<method>/<score>``)."""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

from . import seg_metrics
from .score_labels import _files, read_labels

TABLE_KEYS = ("dice", "hd95", "assd")
BASELINES = ("nearest", "shape")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Score nearest-slice and shape-based interpolation (and a multi-channel model) on held-out label slices")
    p.add_argument("--labels_dir", required=True)
    p.add_argument("--downsample_steps", type=int, required=True)
    p.add_argument("--exper_dir", default=None, help="experiment of a multi-channel model: scored beside the baselines (needs --volumes_dir)")
    p.add_argument("--volumes_dir", default=None, help="the image volumes of the label volumes, matched by name")
    p.add_argument("--model_nbr", type=int, default=None, help="checkpoint to score (default: the latest)")
    p.add_argument("--classes", type=int, nargs="+", default=None, help="classes scored (default: 1 ... the largest label)")
    p.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("Z", "Y", "X"), help="spacing of .npy volumes (they carry none)")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if args.downsample_steps < 2:
        p.error("--downsample_steps must be at least 2")
    if (args.exper_dir is None) != (args.volumes_dir is None):
        p.error("--exper_dir and --volumes_dir go together: the model needs the images of the label volumes")
    if args.model_nbr is not None and args.exper_dir is None:
        p.error("--model_nbr needs --exper_dir")
    return p, args


def baseline_volumes(ref, downsample_steps, spacing):
    """ref: CUDA fp32 [Z, H, W] class ids -> {"nearest": .., "shape": ..}, CUDA fp32 volumes as deep as ``ref``"""
    from .common import create_simple_interpolation
    from .shape_interp import shape_baseline
    near = create_simple_interpolation(ref, spacing, expand_factor=downsample_steps, interpol_filter="nearest", generate_inbetween_slices=True,
                                       align="grid").array
    return {"nearest": near, "shape": shape_baseline(ref, downsample_steps, spacing).to(torch.float32)}


def compare(label_files, downsample_steps, classes=None, spacing=None, trainer=None, image_files=None):
    """{method: {score: [volumes, C]}, "classes", "names"} over the frames of ``label_files`` ({stem: path})."""
    if classes is None:
        top = max(float(read_labels(path, spacing)[0].max()) for path in label_files.values())
        if not top >= 1:
            raise ValueError("the label volumes hold no label >= 1")
        classes = list(range(1, int(top) + 1))
    rows, names = {}, []
    for stem in sorted(label_files):
        labels, sp = read_labels(label_files[stem], spacing)
        images = None
        if trainer is not None:
            if stem not in image_files:
                raise ValueError("--volumes_dir holds no image volume named %s" % stem)
            images, _ = read_labels(image_files[stem], sp)
            if images.shape != labels.shape:
                raise ValueError("%s: image %s and labels %s differ in shape" % (stem, images.shape, labels.shape))
        for t in range(labels.shape[0]):
            ref = torch.from_numpy(labels[t]).to("cuda")
            if trainer is None:
                got = {m: seg_metrics.segmentation_scores(v, ref, sp, classes=classes) for m, v in baseline_volumes(ref, downsample_steps, sp).items()}
            else:
                from ..data_device import rescale_intensities
                img = torch.from_numpy(np.asarray(rescale_intensities(images[t], (0, 100)), dtype=np.float32))
                got = seg_metrics.score_label_supervolume(trainer, img, torch.from_numpy(labels[t]), downsample_steps, sp, classes=classes,
                                                          baselines=BASELINES)
            for m, table in got.items():
                rows.setdefault(m, []).append(table)
            names.append(stem if labels.shape[0] == 1 else "%s#%d" % (stem, t))
    out = {m: {k: np.concatenate([r[k] for r in tables]) for k in seg_metrics.SCORE_KEYS} for m, tables in rows.items()}
    out["classes"] = np.asarray(classes, dtype=np.int64)
    out["names"] = np.asarray(names)
    return out


def methods_of(results):
    return [m for m in ("model",) + BASELINES if m in results]


def format_table(results, downsample_steps):
    lines = ["held-out label slices at %dx, %d volume(s)" % (downsample_steps, len(results["names"])),
             "%-10s%-8s" % ("method", "class") + "".join("%12s" % k for k in TABLE_KEYS)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # a class that is empty everywhere: the mean of nothing is NaN
        for m in methods_of(results):
            means = {k: np.nanmean(results[m][k], axis=0) for k in TABLE_KEYS}
            for i, c in enumerate(results["classes"]):
                lines.append("%-10s%-8d" % (m, c) + "".join("%12.4f" % means[k][i] for k in TABLE_KEYS))
            lines.append("%-10s%-8s" % (m, "mean") + "".join("%12.4f" % np.nanmean(means[k]) for k in TABLE_KEYS))
    return "\n".join(lines)


def main(argv=None):
    p, args = parse_args(argv)
    trainer, image_files = None, None
    try:
        label_files = _files(args.labels_dir)
        if not label_files:
            raise ValueError("no volume files in %s" % args.labels_dir)
        if args.exper_dir is not None:
            from ..kwatsch.get_trainer import get_trainer_dynamic
            from .compare_methods import latest_model
            exper_dir = os.path.expanduser(args.exper_dir)
            image_files = _files(args.volumes_dir)
            trainer, _ = get_trainer_dynamic(src_path=exper_dir, model_nbr=latest_model(exper_dir) if args.model_nbr is None else args.model_nbr,
                                             eval_mode=True)
        results = compare(label_files, args.downsample_steps, args.classes, args.spacing, trainer, image_files)
    except ValueError as e:
        p.error(str(e))
    print(format_table(results, args.downsample_steps))
    if args.out:
        flat = {"%s/%s" % (m, k): v for m in methods_of(results) for k, v in results[m].items()}
        np.savez(args.out, classes=results["classes"], names=results["names"], **flat)
    return results


if __name__ == "__main__":
    main(sys.argv[1:])
