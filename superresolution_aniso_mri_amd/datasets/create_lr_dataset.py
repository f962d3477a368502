"""``python -m superresolution_aniso_mri_amd.datasets.create_lr_dataset --src DIR --out DIR --dataset OASIS|dHCP|ADNI --downsample_steps K``

The reference's ``create_lr_dataset`` (datasets/OASIS/dataset.py:104-122, datasets/dHCP/dataset.py:14-35) without its patient
spreadsheet: every ``.nii`` / ``.nii.gz`` volume under ``--src`` is blurred along z on the device (``simulate_thick_slices``, full Z:
``z_step = 1``) with the dataset's slice thickness (``K`` for OASIS / ADNI, ``K / 2`` for dHCP) and written under ``--out`` with the
reference's file suffix (``get_file_suffix_blurred``).  The header -- spacing, origin, direction -- is carried over untouched
(``volume_io``); the data are float32, as ``sitk.GetArrayFromImage(...).astype(np.float32)`` makes them in the reference."""
import argparse
import os

import numpy as np

from .. import volume_io
from .common_brains import BRAIN_DATASETS, default_slice_thickness, get_file_suffix_blurred, simulate_thick_slices


def blurred_name(name, dataset, downsample_steps):
    """File name of the blurred copy: the reference replaces the file's own suffix by ``get_file_suffix_blurred``."""
    for ext in (".nii.gz", ".nii"):
        if name.lower().endswith(ext):
            stem, suffix = name[:-len(ext)], name[-len(ext):]
            break
    else:
        raise ValueError("%s: not a .nii / .nii.gz file" % name)
    if dataset == "ADNI":                       # the reference's ADNI suffix is '_<K>mm.nii' whatever the source suffix
        return stem + get_file_suffix_blurred(dataset, suffix, downsample_steps)
    if suffix.lower() != ".nii.gz":
        raise ValueError("%s: the %s suffix is built from '.nii.gz' files" % (name, dataset))
    return stem + get_file_suffix_blurred(dataset, suffix, downsample_steps)


def create_lr_dataset(src, out, dataset, downsample_steps, slice_thickness=None):
    """-> list of the files written."""
    if dataset not in BRAIN_DATASETS:
        raise ValueError("dataset=%r: one of %s" % (dataset, ", ".join(BRAIN_DATASETS)))
    thickness = default_slice_thickness(dataset, downsample_steps) if slice_thickness is None else float(slice_thickness)
    os.makedirs(out, exist_ok=True)
    written = []
    for name in sorted(os.listdir(src)):
        if not name.lower().endswith((".nii", ".nii.gz")):
            continue
        vol = volume_io.read_volume(os.path.join(src, name))
        if vol.array.ndim != 3:
            raise ValueError("%s: a brain volume is 3-D, got shape %s" % (name, vol.array.shape))
        img_lr = simulate_thick_slices(np.asarray(vol.array, dtype=np.float32), thickness)
        dst = os.path.join(out, blurred_name(name, dataset, downsample_steps))
        volume_io.write_volume(dst, vol, img_lr)
        print("INFO - saved image to {}".format(dst))
        written.append(dst)
    if not written:
        raise FileNotFoundError("no .nii / .nii.gz volumes in %s" % src)
    return written


def main(argv=None):
    p = argparse.ArgumentParser(description="Write thick-slice (blurred, full-Z) copies of isotropic brain volumes")
    p.add_argument("--src", required=True, help="directory of .nii / .nii.gz volumes")
    p.add_argument("--out", required=True, help="directory the blurred volumes are written to")
    p.add_argument("--dataset", required=True, choices=list(BRAIN_DATASETS))
    p.add_argument("--downsample_steps", type=int, required=True)
    p.add_argument("--thick_slices", type=float, default=None, metavar="MM", help="slice thickness (default: the dataset's: K, dHCP K / 2)")
    a = p.parse_args(argv)
    return create_lr_dataset(a.src, a.out, a.dataset, a.downsample_steps, a.thick_slices)


if __name__ == "__main__":
    main()
