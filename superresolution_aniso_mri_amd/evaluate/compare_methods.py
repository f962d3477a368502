"""The model beside the conventional through-plane baselines on the same held-out slices: what the reference's result tables put side by
side (evaluate/create_HR_images.py:309-329 -- ``create_super_volume`` and ``create_simple_interpolation`` with linear, B-spline and Lanczos
interpolation -- scored by the same functions).

    python -m superresolution_aniso_mri_amd.evaluate.compare_methods --exper_dir E --volumes_dir D --downsample_steps K

Every volume of D (.npy / .nii / .nii.gz / .mha / .mhd; each frame of a 4-D file counts as a volume) is rescaled to [0, 1] by its minimum
and maximum; every K-th slice is kept, the slices in between are synthesised by the model of E (``--model_nbr``, default the latest
checkpoint) and by each baseline, and all of them are scored against the originals by ``find_best_model.evaluate_interpolation_performance``
(SSIM, PSNR, VIF; ``--eval_axis`` 1 / 2 for the long-axis views).  Prints one table and writes one ``save_metrics`` file per method:
``E/results/<method>_<K>x[_axis<a>].npz``."""
import argparse
import glob
import os

import numpy as np

from . import common as _common
from . import find_best_model as _fbm

BASELINES = ("linear", "bspline", "lanczos")


def load_volumes(volumes_dir):
    """{i: {'image': [z,y,x] float32 in [0,1], 'patient_id', 'spacing' [z,y,x]}}: the dict ``evaluate_interpolation_performance`` reads."""
    from .. import volume_io
    from ..data_device import rescale_intensities
    out = {}
    for name in sorted(os.listdir(volumes_dir)):
        f, low = os.path.join(volumes_dir, name), name.lower()
        if low.endswith(".npy"):
            arr, spacing = np.load(f), (1.0, 1.0, 1.0)
        elif low.endswith((".nii", ".nii.gz", ".mha", ".mhd")):
            v = volume_io.read_volume(f)
            arr, spacing = v.array, tuple(v.spacing[:3][::-1])
        else:
            continue
        arr = np.asarray(arr, dtype=np.float32)
        if arr.ndim not in (3, 4):
            raise ValueError("%s: expected a [z,y,x] or [t,z,y,x] volume, got shape %s" % (f, arr.shape))
        for t, frame in enumerate(arr[None] if arr.ndim == 3 else arr):
            out[len(out)] = {"image": np.asarray(rescale_intensities(frame, (0, 100)), dtype=np.float32),
                             "patient_id": name if arr.ndim == 3 else "%s#%d" % (name, t), "spacing": np.asarray(spacing, dtype=np.float64)}
    if not out:
        raise FileNotFoundError("no volumes (.npy, .nii, .nii.gz, .mha, .mhd) in %s" % volumes_dir)
    return out


def latest_model(exper_dir):
    nbrs = [os.path.basename(m).replace(".models", "") for m in glob.glob(os.path.join(exper_dir, "models", "*.models"))]
    nbrs = [int(n) for n in nbrs if n.isdigit()]
    if not nbrs:
        raise ValueError("no checkpoints (models/<epoch>.models) in %s" % exper_dir)
    return max(nbrs)


def compare(exper_dir, volumes, downsample_steps, model_nbr=None, eval_axis=0, align="itk", ps_evaluate=None, eval_dataset=None,
            func_get_trainer=None):
    """{method: result lists of evaluate_interpolation_performance} for the model of ``exper_dir`` and BASELINES; writes the files."""
    if func_get_trainer is None:
        from ..kwatsch.get_trainer import get_trainer_dynamic as func_get_trainer
    exper_dir = os.path.expanduser(exper_dir)
    trainer, e_args = func_get_trainer(src_path=exper_dir, model_nbr=latest_model(exper_dir) if model_nbr is None else model_nbr, eval_mode=True)
    transform = None if ps_evaluate is None else _fbm.get_transforms(ps_evaluate, to_tensor=False)
    results = {}
    for method in (str(e_args.get("model", "ae")),) + BASELINES:
        results[method] = _fbm.evaluate_interpolation_performance(
            trainer if method not in BASELINES else None, e_args, volumes, transform=transform, downsample_steps=downsample_steps,
            eval_axis=eval_axis, interpol_filter=method if method in BASELINES else None, align=align)
    for method, res in results.items():
        _common.save_metrics(exper_dir, eval_dataset, {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}, downsample_steps, method,
                             eval_axis)
    return results


def format_table(results, downsample_steps, eval_axis=0):
    def mean(v):
        return float(np.mean(v)) if len(v) else float("nan")
    cols = ("ssim", "psnr", "vif") + (("ssim_synth", "psnr_synth", "vif_synth") if eval_axis == 0 else ())
    lines = ["held-out slices at %dx, eval_axis %d, %d volume(s)" % (downsample_steps, eval_axis, len(next(iter(results.values()))["ssim"])),
             "%-14s" % "method" + "".join("%12s" % c for c in cols)]
    for method, res in results.items():
        lines.append("%-14s" % method + "".join("%12.4f" % mean(res[c]) for c in cols))
    return "\n".join(lines)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Score the model and the linear / B-spline / Lanczos baselines on the same held-out slices")
    p.add_argument("--exper_dir", type=str, required=True)
    p.add_argument("--volumes_dir", type=str, required=True)
    p.add_argument("--downsample_steps", type=int, required=True)
    p.add_argument("--model_nbr", type=int, default=None, help="checkpoint to score (default: the latest)")
    p.add_argument("--eval_axis", type=int, choices=(0, 1, 2), default=0)
    p.add_argument("--align", choices=("itk", "grid"), default="itk",
                   help="grid of the baselines: itk = SimpleITK's ExpandImageFilter (default), grid = kept slices at every K-th slot")
    p.add_argument("--ps_evaluate", type=int, default=None, help="pad / centre-crop every slice to this size first")
    p.add_argument("--eval_dataset", type=str, default=None, help="prefix of the result files")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    results = compare(args.exper_dir, load_volumes(args.volumes_dir), args.downsample_steps, model_nbr=args.model_nbr, eval_axis=args.eval_axis,
                      align=args.align, ps_evaluate=args.ps_evaluate, eval_dataset=args.eval_dataset)
    print(format_table(results, args.downsample_steps, args.eval_axis))
    return results


if __name__ == "__main__":
    main()
