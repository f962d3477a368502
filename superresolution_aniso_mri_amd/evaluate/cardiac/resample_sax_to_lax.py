"""A short-axis (SAX) stack in the geometry of the patient's long-axis (LAX) scan, on the device -- the reference's
evaluate/cardiac/resample_sax_to_lax.py with its four functions, their argument names and order:

    grid = make_lax_identity_grid(lax_shape)                                    # [z, y, x, 4]: homogeneous LAX voxel indices (x, y, z, 1)
    grid = make_transform(grid, lax_shape, sax_shape, S_lax, R_lax, T_lax, S_sax, R_sax, T_sax)     # [z, y, x, 3], normalised to [-1, 1]
    lax_view = resample_sax_to_lax(sax, (T,) + lax_shape, grid)                 # [T, z, y, x] float32

``S``, ``R``, ``T`` are the 4x4 spacing, direction and translation matrices of an image (world = T @ R @ S @ index).  ``make_transform``
multiplies in the dtype it is given and in the reference's order (six products from the right, then the division by (size - 1) / 2), so
float32 matrices reproduce the reference's float32 grid; ``evaluate.reslice`` composes ONE float64 matrix instead and is what the
command line below uses.  Interpolation is trilinear, zero padding, ``align_corners=True`` (csrc/reslice.hip).

Deviations from the reference, on purpose:
  - its frame loop (``np.arange(n).astype(np.int)``: ``np.int`` no longer exists in current numpy, the loop does not run) is not
    reproduced: all frames go through ONE ``aesr_reslice_grid`` launch;
  - ``resample_sax_to_lax`` also takes a ``volume_io.Volume`` or a [T, Z, Y, X] array / tensor, not only a SimpleITK image, and a CUDA
    tensor in gives a CUDA tensor out (the reference always returns numpy);
  - ``make_transform`` raises ValueError for a SAX side of 1, where the reference divides by zero.

Command line:  python -m superresolution_aniso_mri_amd.evaluate.cardiac.resample_sax_to_lax --sax S.nii.gz --lax L.nii.gz --out O.nii.gz
[--interp linear|nearest|bspline|lanczos|cosine] [--radius 3|4|5] [--clamp01]: every frame of the SAX file on the grid of the LAX file
(float64 affine path), written with the LAX header.  ``cosine`` with radius 5 is the interpolator of the reference's
kwatsch/create_nifti_from_dicom.py (``sitk.sitkCosineWindowedSinc``); csrc/reslice_taps.hip."""
import argparse
import sys

import numpy as np
import torch

from .. import reslice as _reslice


def make_identity_grid(shape, stackdim='last', device='cpu'):
    """``shape`` = [z, y, x] -> float32 tensor whose entry at (z, y, x) is the coordinate (x, y, z), stacked along the last (default),
    the first or the given dimension."""
    if isinstance(stackdim, int):
        dim = stackdim
    elif stackdim == 'last':
        dim = len(shape)
    elif stackdim == 'first':
        dim = 0
    else:
        raise ValueError("stackdim=%r: expected 'last', 'first' or an int" % (stackdim,))
    axes = torch.meshgrid(*[torch.arange(0, int(s), dtype=torch.float32, device=device) for s in shape], indexing="ij")
    return torch.stack(axes[::-1], dim=dim)


def make_lax_identity_grid(target_shape):
    """``target_shape`` = [z, y, x] -> float32 [z, y, x, 4]: (x, y, z, 1) of every voxel."""
    grid = make_identity_grid(target_shape)
    return torch.cat([grid, torch.ones(grid.shape[:-1] + (1,))], dim=-1)


def _as_tensor(m, like):
    return m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m), device=like.device)


def make_transform(ident_grid, lax_shape, sax_shape,
                   tr_S_lax, tr_R_lax, tr_T_lax,
                   tr_S_sax, tr_R_sax, tr_T_sax):
    """Homogeneous LAX voxel indices -> world -> SAX voxel indices -> normalised to [-1, 1] over the SAX extent ``sax_shape`` = [z, y, x].
    Returns ``lax_shape + (3,)``: (x, y, z) for ``grid_sample(..., align_corners=True)`` / ``aesr_reslice_grid``."""
    lax_shape, sax_shape = tuple(int(s) for s in lax_shape), tuple(int(s) for s in sax_shape)
    if len(sax_shape) != 3 or min(sax_shape) < 2:
        raise ValueError("sax_shape=%r: every SAX side must be at least 2 (the normalisation divides by (size - 1) / 2)" % (sax_shape,))
    pts = ident_grid.reshape(lax_shape[0], -1, 4)
    chain = [_as_tensor(m, pts) for m in (tr_S_lax, tr_R_lax, tr_T_lax)]
    chain += [torch.inverse(_as_tensor(m, pts)) for m in (tr_T_sax, tr_R_sax, tr_S_sax)]
    for m in chain:
        pts = pts @ m.T
    half = (torch.tensor(sax_shape[::-1] + (2,), dtype=torch.float32, device=pts.device) - 1) / 2
    pts = pts / half.to(pts.dtype) - 1
    return pts.reshape(lax_shape + (4,))[..., :3]


def _frames_of(sax_image):
    """[T, Z, Y, X] numpy array or tensor of whatever ``resample_sax_to_lax`` was given"""
    if hasattr(sax_image, "array") and hasattr(sax_image, "spacing"):          # volume_io.Volume
        arr = sax_image.array
    elif torch.is_tensor(sax_image) or isinstance(sax_image, np.ndarray):
        arr = sax_image
    else:
        try:
            import SimpleITK as sitk
        except ImportError:
            raise TypeError("sax_image: expected a volume_io.Volume, a [T, Z, Y, X] array or tensor (SimpleITK is not installed), got %s"
                            % type(sax_image).__name__)
        arr = sitk.GetArrayFromImage(sax_image)
    if len(arr.shape) != 4:
        raise ValueError("sax_image: expected [T, Z, Y, X], got shape %s" % (tuple(arr.shape),))
    return arr


def resample_sax_to_lax(sax_image, target_shape, transformed_ident_grid):
    """``sax_image``: a ``volume_io.Volume``, a [T, Z, Y, X] array or CUDA tensor, or a SimpleITK image; ``target_shape`` = [T, z, y, x];
    ``transformed_ident_grid``: what ``make_transform`` returned.  -> float32 ``[T, *lax_shape]``: numpy, or a CUDA tensor for a CUDA
    tensor.  One launch for all frames."""
    target_shape = tuple(int(s) for s in target_shape)
    if len(target_shape) != 4:
        raise ValueError("target_shape=%r: expected [T, z, y, x]" % (target_shape,))
    frames = _frames_of(sax_image)
    grid_shape = tuple(int(s) for s in transformed_ident_grid.shape)
    if grid_shape != target_shape[1:] + (3,):
        raise ValueError("transformed_ident_grid has shape %s, target_shape %s needs %s" % (grid_shape, target_shape, target_shape[1:] + (3,)))
    if int(frames.shape[0]) != target_shape[0]:
        raise ValueError("sax_image has %d frames, target_shape %s has %d" % (int(frames.shape[0]), target_shape, target_shape[0]))
    return _reslice.reslice_grid(frames, transformed_ident_grid, "linear")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m superresolution_aniso_mri_amd.evaluate.cardiac.resample_sax_to_lax",
                                 description="Reslice every frame of a short-axis volume onto the grid of a long-axis scan (on the GPU).")
    ap.add_argument("--sax", required=True, help="the short-axis volume, 3-D or 4-D (.nii, .nii.gz, .mha, .mhd)")
    ap.add_argument("--lax", required=True, help="the long-axis scan whose grid and header the output takes")
    ap.add_argument("--out", required=True, help="the file to write (.nii, .nii.gz, .mha, .mhd)")
    ap.add_argument("--interp", choices=list(_reslice.AFFINE_INTERPS), default="linear",
                    help="bspline: cubic B-spline; lanczos, cosine: windowed sincs (cosine is the reference's sitkCosineWindowedSinc)")
    ap.add_argument("--radius", type=int, choices=list(_reslice.RADII), default=5, help="radius of lanczos and cosine (default 5)")
    ap.add_argument("--clamp01", action="store_true", help="clamp the result of bspline, lanczos or cosine to [0, 1] (linear and nearest "
                                                            "cannot leave the range of the samples and ignore it)")
    return ap.parse_args(argv)


def main(argv=None):
    from ... import volume_io
    args = parse_args(argv)
    for flag in ("sax", "lax", "out"):
        if str(getattr(args, flag)).lower().endswith(".npy"):
            sys.exit("--%s %s: a .npy file has no geometry (spacing, origin, direction); give a NIfTI or MetaImage file" % (flag, getattr(args, flag)))
    sax, lax = volume_io.read_volume(args.sax), volume_io.read_volume(args.lax)
    res = _reslice.reslice_like(sax, lax, interp=args.interp, radius=args.radius, clamp01=args.clamp01)
    spacing = list(lax.spacing[:3])
    if res.ndim == 4:
        spacing.append(sax.spacing[3] if len(sax.spacing) > 3 else 1.0)
    volume_io.write_volume(args.out, lax, res, spacing)
    print("%s: %d frame(s) of %s on the %s grid of %s (%s)" % (args.out, sax.num_frames, args.sax, "x".join(str(s) for s in res.shape[-3:]), args.lax,
                                                             args.interp))
    return res


if __name__ == "__main__":
    main()
