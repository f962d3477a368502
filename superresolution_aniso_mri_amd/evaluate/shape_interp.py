"""Shape-based interpolation of label maps between slices (Raya & Udupa 1990, Herman et al. 1992) on the device: the conventional baseline
for a denser segmentation, and what a model that super-resolves label maps has to beat (copying the nearest slice is not).

Per class and slice the signed Euclidean distance to the class boundary (positive inside, in mm of the in-plane spacing); the maps of the
two neighbouring slices are blended linearly at the output slice's position and the class with the largest blended value wins, ties going
to the smallest class value.  csrc/shape_interp.hip computes both steps, include/aesr_hip_shape.h states the definitions, and
``evaluate.z_grid`` says where the output slices sit -- the integer grid of ``num_interpolations`` and the grid of a target slice spacing
are one code path.  A class that a slice does not hold has the distance ``-BIG`` everywhere in it (``BIG`` = the slice's diagonal, DESIGN.md
section 6b): such a class ends at the slice that has it, it does not taper.

    python -m superresolution_aniso_mri_amd.evaluate.shape_interp --labels_dir L --output_dir O (--num_interpolations n | --target_spacing_z MM)
                                                                   [--method shape|nearest] [--spacing_z MM --spacing Y X for .npy]

reads every label file of L (NIfTI, MetaImage, .npy; every frame of a 4-D file) and writes it to O with the new z spacing as
``<name>_ni0<n>`` or ``<name>_sz<MM>``.  There is no CPU fallback: numpy arrays go through the device and come back as numpy."""
import argparse
import os
import sys

import numpy as np
import torch

from .. import _hip
from .._hip import check, lib, ptr, stream
from .z_grid import ZGrid, target_grid

MAX_CLASSES = _hip.SHAPE_MAX_CLASSES
MAX_W = _hip.SHAPE_MAX_W
METHODS = ("shape", "nearest")
NO_FALLBACK = "shape-based interpolation is HIP kernels: it needs the GPU, there is no CPU fallback"


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def _present(labels):
    """sorted label values of a numpy array or tensor as Python numbers"""
    if torch.is_tensor(labels):
        return [v for v in torch.unique(labels.detach()).cpu().tolist()]
    return [v for v in np.unique(np.asarray(labels)).tolist()]


def check_classes(classes, present):
    """The class list of a call: ``classes`` (or, for None, the values present) as ascending ints in 0..255, 1 to 8 of them, holding every
    value of ``present``.  ValueError otherwise.  The background is a class like any other."""
    for v in present:
        if not (float(v) == int(v) and 0 <= int(v) <= 255):
            raise ValueError("label value %r is not an integer in 0..255" % (v,))
    present = sorted({int(v) for v in present})
    if classes is None:
        classes = present
    else:
        classes = list(classes)
        for c in classes:
            if int(c) != c or not 0 <= int(c) <= 255:
                raise ValueError("class value %r is not an integer in 0..255" % (c,))
        classes = [int(c) for c in classes]
        if any(b <= a for a, b in zip(classes, classes[1:])):
            raise ValueError("classes must be ascending and distinct, got %r" % (classes,))
    if not 1 <= len(classes) <= MAX_CLASSES:
        raise ValueError("1 to %d classes per call are supported (the background counts), got %d: %r" % (MAX_CLASSES, len(classes), classes))
    foreign = [v for v in present if v not in classes]
    if foreign:
        raise ValueError("label value(s) %r are not in classes %r" % (foreign, classes))
    return classes


def _spacing_yx(spacing_yx):
    s = [float(v) for v in np.asarray(spacing_yx, dtype=np.float64).reshape(-1)]
    if len(s) != 2 or not all(np.isfinite(v) and v > 0 for v in s):
        raise ValueError("spacing_yx must be two positive finite numbers (y, x), got %r" % (spacing_yx,))
    return s


def _check_shape(labels):
    if not hasattr(labels, "shape") or len(labels.shape) not in (3, 4):
        raise ValueError("label volumes must be [Z, H, W] or [N, Z, H, W], got shape %s" % (tuple(getattr(labels, "shape", ())),))
    if min(int(s) for s in labels.shape) < 1:
        raise ValueError("nothing to interpolate: shape %s" % (tuple(labels.shape),))
    if int(labels.shape[-1]) > MAX_W:
        raise ValueError("lines of up to %d pixels are supported, got W=%d" % (MAX_W, int(labels.shape[-1])))


def _to_device(labels, classes):
    """numpy / CPU tensor / CUDA tensor -> (uint8 CUDA [N, Z, H, W] contiguous, classes, host data given, a 3-D volume given).  Every check
    that needs no device is made before the device is asked for."""
    _check_shape(labels)
    host = not (torch.is_tensor(labels) and labels.is_cuda)
    if host:
        arr = np.asarray(labels.detach().cpu() if torch.is_tensor(labels) else labels)
        classes = check_classes(classes, _present(arr))
        if not torch.cuda.is_available():
            raise NotImplementedError(NO_FALLBACK)
        dev = torch.from_numpy(np.ascontiguousarray(arr.astype(np.uint8))).to("cuda")
    else:
        classes = check_classes(classes, _present(labels))
        dev = labels.detach().to(torch.uint8).contiguous()
    return (dev[None] if dev.dim() == 3 else dev), classes, host, len(labels.shape) == 3


def resolve_grid(Z, num_interpolations=None, grid=None):
    """Exactly one of the two: ``num_interpolations=n`` is ``target_grid(Z, 1.0, 1.0 / (n + 1))``; a ``ZGrid`` must be for ``Z`` slices."""
    if (num_interpolations is None) == (grid is None):
        raise ValueError("exactly one of num_interpolations and grid must be given")
    if grid is None:
        n = num_interpolations
        if int(n) != n or int(n) < 0:
            raise ValueError("num_interpolations=%r: a number of slices per gap, 0 or more" % (n,))
        return target_grid(int(Z), 1.0, 1.0 / (int(n) + 1))
    if not isinstance(grid, ZGrid):
        raise ValueError("grid must be an evaluate.z_grid.ZGrid, got %r" % (type(grid).__name__,))
    if grid.Z != int(Z):
        raise ValueError("grid is for %d slices, the volume has %d" % (grid.Z, int(Z)))
    return grid


def store_path(out, HW):
    """Which stores ``aesr_shape_interpolate`` takes for this output, by the rule of include/aesr_hip_shape.h: "word4" (4 labels per lane, one
    32-bit store) when H * W is a multiple of 4 and ``out`` is 4-byte aligned, else "byte1".  The values do not depend on it."""
    return "word4" if int(HW) % 4 == 0 and out.data_ptr() % 4 == 0 else "byte1"


# ---- the two launches -----------------------------------------------------------------------------------------------------------------
def _sdm(lab4, classes, spacing_yx):
    """uint8 CUDA [N, Z, H, W] -> fp64 CUDA [N, C, Z, H, W]; two launches, no synchronisation"""
    N, Z, H, W = (int(s) for s in lab4.shape)
    C = len(classes)
    nbytes = int(lib.aesr_shape_workspace_bytes(N, Z, H, W, C))
    if nbytes == 0:
        raise ValueError("the library refuses %d volumes of %d x %d x %d with %d classes (2^31 elements or more, or W > %d)" % (N, Z, H, W, C, MAX_W))
    sdm = torch.empty((N, C, Z, H, W), device=lab4.device, dtype=torch.float64)
    ws = torch.empty(nbytes, device=lab4.device, dtype=torch.uint8)
    with torch.cuda.device(lab4.device):
        check(lib.aesr_shape_signed_distances(ptr(lab4), ptr(sdm), ptr(ws), nbytes, N, Z, H, W, _hip.int_array(classes), C, spacing_yx[0],
                                              spacing_yx[1], stream()), "aesr_shape_signed_distances")
    return sdm


def _blend(sdm, gap_dev, alpha_dev, classes, out=None):
    """fp64 CUDA [N, C, Z, H, W] and the device tables -> uint8 CUDA [N, J, H, W]; one launch"""
    N, C, Z, H, W = (int(s) for s in sdm.shape)
    J = int(gap_dev.numel())
    if out is None:
        out = torch.empty((N, J, H, W), device=sdm.device, dtype=torch.uint8)
    with torch.cuda.device(sdm.device):
        check(lib.aesr_shape_interpolate(ptr(sdm), ptr(gap_dev), ptr(alpha_dev), ptr(out), N, C, Z, H, W, J, _hip.int_array(classes), stream()),
              "aesr_shape_interpolate")
    return out


def grid_tables(grid, device):
    """(gap int32 [J], alpha fp64 [J]) of a ZGrid on the device: uploaded once per call"""
    gap = torch.from_numpy(np.ascontiguousarray(grid.gap, dtype=np.int32)).to(device)
    alpha = torch.from_numpy(np.ascontiguousarray(grid.alpha, dtype=np.float64)).to(device)
    return gap, alpha


def signed_distance_maps(labels, spacing_yx=(1.0, 1.0), classes=None):
    """labels: uint8 label volume [Z, H, W] or [N, Z, H, W] (a CUDA tensor; numpy / CPU data goes through the device and comes back as
    numpy).  Returns (sdm fp64 [C, Z, H, W] or [N, C, Z, H, W], classes): per class and slice the signed distance to the class boundary
    in the units of ``spacing_yx``, positive on the class; +-BIG where the class fills the slice or is absent from it.  ``classes``
    defaults to the sorted values present; more than 8, or a label value outside ``classes``, is a ValueError."""
    spacing_yx = _spacing_yx(spacing_yx)
    lab4, classes, host, single = _to_device(labels, classes)
    sdm = _sdm(lab4, classes, spacing_yx)
    sdm = sdm[0] if single else sdm
    return (sdm.cpu().numpy() if host else sdm), classes


def _frames_per_call(N, C, Z, H, W, J, max_bytes):
    one = 2 * C * Z * H * W * 8 + J * H * W          # the maps, the workspace of the same size, the output
    return max(1, min(N, int(max_bytes) // max(one, 1)))


def shape_interpolate(labels, *, num_interpolations=None, grid=None, spacing_yx=(1.0, 1.0), classes=None, max_workspace_bytes=1 << 30):
    """labels [Z, H, W] or [N, Z, H, W] -> uint8 [J, H, W] or [N, J, H, W]: the label volume at the slices of the grid -- exactly one of
    ``num_interpolations`` (n slices into every gap: ``target_grid(Z, 1.0, 1.0 / (n + 1))``) and ``grid`` (an ``evaluate.z_grid.ZGrid``
    for Z slices) -- by shape-based interpolation.  Slices with alpha 0 or 1 are the input slices, bit for bit.  numpy in, numpy out
    (through the device); a CUDA tensor in, a CUDA tensor out.  Frames are processed in chunks whose buffers stay under
    ``max_workspace_bytes``; the grid's tables are uploaded once."""
    spacing_yx = _spacing_yx(spacing_yx)
    _check_shape(labels)
    grid = resolve_grid(labels.shape[-3], num_interpolations, grid)
    lab4, classes, host, single = _to_device(labels, classes)
    N, Z, H, W = (int(s) for s in lab4.shape)
    gap, alpha = grid_tables(grid, lab4.device)
    out = torch.empty((N, grid.J, H, W), device=lab4.device, dtype=torch.uint8)
    step = _frames_per_call(N, len(classes), Z, H, W, grid.J, max_workspace_bytes)
    for n0 in range(0, N, step):
        sdm = _sdm(lab4[n0:n0 + step], classes, spacing_yx)
        _blend(sdm, gap, alpha, classes, out[n0:n0 + step])
        del sdm
    out = out[0] if single else out
    return out.cpu().numpy() if host else out


# ---- the evaluation protocol ----------------------------------------------------------------------------------------------------------
def baseline_plan(num_slices, downsample_steps):
    """The bookkeeping of the held-out-slice protocol (``create_simple_interpolation(generate_inbetween_slices=True)``): (indices of the
    kept slices, last = ``determine_last_slice``: the interpolated stack is cut behind it, remain = the trailing originals appended)."""
    from .common import determine_last_slice
    Z, f = int(num_slices), int(downsample_steps)
    if f < 2:
        raise ValueError("downsample_steps must be at least 2, got %r" % (downsample_steps,))
    if Z < 1:
        raise ValueError("a volume has one slice or more, got %r" % (num_slices,))
    return list(range(0, Z, f)), determine_last_slice(Z, f), (Z - 1) % f


def shape_baseline(labels_full, downsample_steps, spacing):
    """The protocol of ``score_label_supervolume``'s nearest baseline with shape-based interpolation: keep every ``downsample_steps``-th
    slice of ``labels_full`` [Z, H, W], interpolate the slices in between on the integer grid (``spacing`` is (z, y, x); the in-plane part
    scales the distances), cut behind ``determine_last_slice`` and append the remaining ORIGINAL slices.  As deep as ``labels_full``;
    uint8, numpy for host data, a CUDA tensor for a CUDA tensor."""
    if len(labels_full.shape) != 3:
        raise ValueError("shape_baseline expects a [z, y, x] volume, got shape %s" % (tuple(labels_full.shape),))
    s = [float(v) for v in np.asarray(spacing, dtype=np.float64).reshape(-1)]
    if len(s) != 3:
        raise ValueError("spacing must be (z, y, x), got %r" % (spacing,))
    f = int(downsample_steps)
    kept, last, remain = baseline_plan(labels_full.shape[0], f)
    new = shape_interpolate(labels_full[::f], num_interpolations=f - 1, spacing_yx=s[1:])[:last + 1]
    if remain:
        tail = labels_full[-remain:]
        if torch.is_tensor(new):
            new = torch.cat([new, tail.to(new.device, torch.uint8)])
        else:
            new = np.concatenate([new, np.asarray(tail.detach().cpu() if torch.is_tensor(tail) else tail).astype(np.uint8)])
    assert new.shape[0] == labels_full.shape[0] and len(kept) == last // f + 1
    return new


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Interpolate label volumes between slices: shape-based interpolation, or the nearest slice")
    p.add_argument("--labels_dir", required=True, help="directory (or one file) of label volumes: .nii, .nii.gz, .mha, .mhd, .npy")
    p.add_argument("--output_dir", required=True)
    target = p.add_mutually_exclusive_group(required=True)
    target.add_argument("--num_interpolations", type=int, default=None, help="slices put into every gap")
    target.add_argument("--target_spacing_z", type=float, default=None, metavar="MM", help="slices MM apart")
    p.add_argument("--method", choices=METHODS, default="shape")
    p.add_argument("--spacing_z", type=float, default=None, metavar="MM", help="slice spacing of .npy volumes (they carry none)")
    p.add_argument("--spacing", type=float, nargs=2, default=None, metavar=("Y", "X"), help="in-plane spacing of .npy volumes (default 1 1)")
    args = p.parse_args(argv)
    if args.num_interpolations is not None and not 0 <= args.num_interpolations <= 16:
        p.error("--num_interpolations %d: 0 to 16 slices per gap" % args.num_interpolations)
    if args.target_spacing_z is not None and not (np.isfinite(args.target_spacing_z) and args.target_spacing_z > 0):
        p.error("--target_spacing_z %r must be positive and finite" % args.target_spacing_z)
    if args.spacing_z is not None and not (np.isfinite(args.spacing_z) and args.spacing_z > 0):
        p.error("--spacing_z %r must be positive and finite" % args.spacing_z)
    if args.spacing is not None and not all(np.isfinite(v) and v > 0 for v in args.spacing):
        p.error("--spacing %r must be positive and finite" % (args.spacing,))
    return p, args


def output_name(name, num_interpolations=None, target_spacing_z=None):
    """<stem>_ni0<n><ext> or <stem>_sz<MM><ext>: the tags of generate_hr_volumes"""
    from .score_labels import EXTENSIONS
    tag = "ni0{}".format(num_interpolations) if target_spacing_z is None else "sz{:g}".format(target_spacing_z)
    for ext in EXTENSIONS:
        if name.lower().endswith(ext):
            return "%s_%s%s" % (name[:-len(ext)], tag, name[-len(ext):])
    raise ValueError("%s is not a volume file (%s)" % (name, ", ".join(EXTENSIONS)))


def interpolate_array(arr, spacing_zyx, method="shape", num_interpolations=None, target_spacing_z=None):
    """[z,y,x] or [t,z,y,x] label array -> (the interpolated array, same leading layout and dtype, the new z spacing)"""
    if arr.ndim not in (3, 4):
        raise ValueError("label volumes are [z, y, x] or [t, z, y, x], got shape %s" % (arr.shape,))
    Z = arr.shape[-3]
    if target_spacing_z is not None:
        grid = target_grid(Z, spacing_zyx[0], target_spacing_z)
        new_z = grid.target_spacing_z
    else:
        grid = target_grid(Z, 1.0, 1.0 / (num_interpolations + 1))
        new_z = spacing_zyx[0] / (num_interpolations + 1)
    if method == "shape":
        out = shape_interpolate(arr, grid=grid, spacing_yx=spacing_zyx[1:])
    elif target_spacing_z is not None:
        from ..generate_hr_volumes import expand_volume_on_grid
        out = expand_volume_on_grid(arr, grid, "nearest")
    else:
        from .common import create_simple_interpolation
        frames = [create_simple_interpolation(f, spacing_zyx, expand_factor=num_interpolations + 1, interpol_filter="nearest", align="grid").array
                  for f in (arr[None] if arr.ndim == 3 else arr)]
        out = frames[0] if arr.ndim == 3 else np.stack(frames)
    return np.asarray(out).astype(arr.dtype), new_z


def main(argv=None):
    from .. import volume_io
    from .score_labels import _files
    p, args = parse_args(argv)
    try:
        files = _files(args.labels_dir)
        if not files:
            raise ValueError("no volume files in %s" % args.labels_dir)
    except ValueError as e:
        p.error(str(e))
    os.makedirs(args.output_dir, exist_ok=True)
    written = []
    for stem in sorted(files):
        path = files[stem]
        name = os.path.basename(path)
        try:
            if name.lower().endswith(".npy"):
                if args.target_spacing_z is not None and args.spacing_z is None:
                    raise ValueError("%s: a .npy file carries no spacing; give its slice spacing with --spacing_z MM" % name)
                vol, arr = None, np.load(path)
                spacing = (args.spacing_z if args.spacing_z is not None else 1.0,) + tuple(args.spacing or (1.0, 1.0))
            else:
                vol = volume_io.read_volume(path)
                arr, spacing = vol.array, (vol.spacing[2], vol.spacing[1], vol.spacing[0])
            out, new_z = interpolate_array(arr, spacing, args.method, args.num_interpolations, args.target_spacing_z)
        except ValueError as e:
            p.error(str(e))
        dst = os.path.join(args.output_dir, output_name(name, args.num_interpolations, args.target_spacing_z))
        if vol is None:
            np.save(dst, out)
        else:
            new_spacing = list(vol.spacing[:out.ndim])
            new_spacing[2] = new_z
            volume_io.write_volume(dst, vol, out, new_spacing)
        print("%s: %s, %d -> %d slices, z spacing %g -> %g mm: %s" % (name, args.method, arr.shape[-3], out.shape[-3], spacing[0], new_z, dst))
        written.append((dst, out, new_z))
    return written


if __name__ == "__main__":
    main(sys.argv[1:])
