"""Reslice a volume into the geometry of another scan on the device: the 3-D interpolating gather of csrc/reslice.hip
(include/aesr_hip_reslice.h) behind world-coordinate geometry.  This is what puts a (super-resolved) short-axis stack on the grid of the
patient's acquired long-axis scan (the reference's evaluate/cardiac/resample_sax_to_lax.py and kwatsch/create_nifti_from_dicom.py
``create_cross_section_3d``).

A ``Geometry`` is what SimpleITK calls spacing, origin and direction, in its (x, y, z) order and LPS convention: voxel index (i, j, k)
sits at ``origin + direction @ (spacing * (i, j, k))``, i.e. at ``T @ R @ S @ (i, j, k, 1)`` (``index_to_world``).  All matrix algebra is
float64 on the host; the kernel receives the 3x4 matrix that takes an OUTPUT voxel index to a SOURCE voxel index and evaluates it in fp64.
Interpolation is trilinear with zero padding (a corner outside the source contributes nothing) or nearest (halves to even), exactly
``torch.nn.functional.grid_sample(..., padding_mode='zeros', align_corners=True)`` on a 5-D input.

The affine path also takes three higher-order interpolators (csrc/reslice_taps.hip, include/aesr_hip_reslice_taps.h): ``bspline``, the cubic B-spline
over a separable 3-D pre-filter (``scipy.ndimage.map_coordinates(order=3, mode='mirror')``), and the windowed sincs ``lanczos`` and
``cosine`` of radius 3, 4 or 5 (ITK's WindowedSincInterpolateImageFunction; ``cosine`` is what the reference's
kwatsch/create_nifti_from_dicom.py reslices with).  They follow ITK's buffer rule: a voxel is computed only where
``-0.5 <= p < size - 0.5`` on every axis and is 0 elsewhere.  DESIGN.md section 2 has the definitions and what pins them."""
import numpy as np
import torch

from .. import _hip
from .._hip import check, lib, ptr, stream

INTERPS = {"nearest": _hip.RESLICE_NEAREST, "linear": _hip.RESLICE_LINEAR}
TAP_KERNELS = {"bspline": _hip.TAPS_BSPLINE3, "lanczos": _hip.TAPS_LANCZOS, "cosine": _hip.TAPS_COSINE}          # the affine path only
AFFINE_INTERPS = tuple(sorted(INTERPS)) + tuple(sorted(TAP_KERNELS))
RADII = tuple(range(_hip.TAPS_MIN_RADIUS, _hip.TAPS_MAX_RADIUS + 1))


class Geometry:
    """spacing_xyz [3] (mm), origin [3] (mm, (x, y, z)), direction [3, 3] (columns = axis cosines): all float64."""

    def __init__(self, spacing_xyz, origin=(0.0, 0.0, 0.0), direction=None):
        self.spacing = np.array(spacing_xyz, dtype=np.float64).reshape(-1)[:3].copy()
        self.origin = np.array(origin, dtype=np.float64).reshape(-1)[:3].copy()
        self.direction = np.eye(3) if direction is None else np.array(direction, dtype=np.float64).reshape(3, 3).copy()
        if self.spacing.shape != (3,) or self.origin.shape != (3,):
            raise ValueError("spacing and origin need 3 entries each (got %d, %d)" % (self.spacing.size, self.origin.size))
        if not (np.isfinite(self.spacing).all() and (self.spacing > 0).all()):
            raise ValueError("spacing %s must be positive" % (self.spacing.tolist(),))
        if not (np.isfinite(self.origin).all() and np.isfinite(self.direction).all()):
            raise ValueError("origin and direction must be finite")
        if abs(np.linalg.det(self.direction)) < 1e-6:
            raise ValueError("direction is singular: %s" % (self.direction.tolist(),))

    @classmethod
    def from_volume(cls, vol):
        """The geometry of a ``volume_io.Volume`` (the leading three spacings of a 4-D one)."""
        return cls(vol.spacing[:3], vol.origin, vol.direction)


def index_to_world(geom):
    """float64 [4, 4]: ``T @ R @ S``, voxel index (x, y, z, 1) -> world (x, y, z, 1) in mm."""
    S, R, T = np.eye(4), np.eye(4), np.eye(4)
    S[:3, :3] = np.diag(geom.spacing)
    R[:3, :3] = geom.direction
    T[:3, 3] = geom.origin
    return T @ R @ S


def affine_between(src_geom, ref_geom):
    """float64 [4, 4]: ``inv(T_s R_s S_s) @ (T_r R_r S_r)``, a voxel index of the reference grid -> the voxel index of the source."""
    return np.linalg.inv(index_to_world(src_geom)) @ index_to_world(ref_geom)


def _interp_code(interp):
    if interp not in INTERPS:
        raise ValueError("interp=%r: expected 'linear' or 'nearest'" % (interp,))
    return INTERPS[interp]


def _check_affine_interp(interp, radius):
    if interp not in AFFINE_INTERPS:
        raise ValueError("interp=%r: expected one of %s" % (interp, ", ".join(AFFINE_INTERPS)))
    if isinstance(radius, bool) or radius not in RADII:
        raise ValueError("radius=%r: the radius of a windowed sinc is one of %s" % (radius, RADII))
    return int(radius)


def bspline_coefficients_3d(x4):
    """CUDA float32 [N, Z, H, W] -> CUDA float64 coefficients of the same shape: ``scipy.ndimage.spline_filter(order=3, mode='mirror')`` of
    every frame (three launches, y and x in place)."""
    _hip.require_gpu_tensor(x4, "x4")
    N, Z, H, W = (int(s) for s in x4.shape)
    coef = torch.empty((N, Z, H, W), device=x4.device, dtype=torch.float64)
    with torch.cuda.device(x4.device):
        check(lib.aesr_bspline_prefilter_3d(ptr(x4), ptr(coef), N, Z, H, W, stream()), "aesr_bspline_prefilter_3d")
    return coef


def _to_device(src):
    """(CUDA float32 contiguous [N, Z, H, W], was 3-D, was numpy)"""
    is_np = not torch.is_tensor(src)
    t = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)) if is_np else src
    if t.dim() not in (3, 4):
        raise ValueError("expected [Z, Y, X] or [T, Z, Y, X], got %s" % (tuple(t.shape),))
    if min(t.shape) < 1:
        raise ValueError("nothing to reslice: shape %s" % (tuple(t.shape),))
    if is_np:
        if not torch.cuda.is_available():
            raise RuntimeError("reslicing runs on the GPU: the HIP path has no CPU fallback")
        t = t.cuda()                                            # the one upload
    elif not t.is_cuda:
        raise RuntimeError("src must live on the GPU (got %s): the HIP path has no CPU fallback; pass a numpy array to have it uploaded" % t.device)
    elif t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return (t if t.dim() == 4 else t.unsqueeze(0)), t.dim() == 3, is_np


def _out_shape(ref_shape):
    shape = tuple(int(s) for s in ref_shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("ref_shape=%r: expected a positive [z, y, x]" % (ref_shape,))
    return shape


def reslice_affine(src, matrix, ref_shape, interp="linear", radius=5, clamp01=False):
    """``matrix`` ([3, 4] or [4, 4], float64): source voxel (x, y, z) = matrix @ (xo, yo, zo, 1) for every voxel of the output grid
    ``ref_shape`` = [z, y, x].  ``src``: [Z, Y, X] or [T, Z, Y, X]; numpy in -> numpy out (one upload, one download), a CUDA tensor in -> a
    new CUDA tensor out.  All frames are one launch (``bspline``: the pre-filter's launches into a float64 buffer of the source's shape
    first); nothing is synchronised for device input.  ``interp``: one of AFFINE_INTERPS; ``radius`` (3, 4 or 5) is the radius of
    ``lanczos`` and ``cosine``, validated and otherwise ignored; ``clamp01`` clamps the fp32 result of those three to [0, 1] in the
    kernel; like ``radius`` it is ignored by ``linear`` and ``nearest``, which cannot leave the range of the samples."""
    radius = _check_affine_interp(interp, radius)
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64)[:3, :4])
    if m.shape != (3, 4) or not np.isfinite(m).all():
        raise ValueError("matrix must be a finite 3x4 or 4x4 (got shape %s)" % (np.shape(matrix),))
    Zo, Ho, Wo = _out_shape(ref_shape)
    x4, was3d, is_np = _to_device(src)
    N, Zs, Hs, Ws = (int(s) for s in x4.shape)
    out = torch.empty((N, Zo, Ho, Wo), device=x4.device, dtype=torch.float32)
    with torch.cuda.device(x4.device):
        if interp in INTERPS:
            check(lib.aesr_reslice_affine(ptr(x4), ptr(out), N, Zs, Hs, Ws, Zo, Ho, Wo, m.ctypes.data_as(_hip.DP), INTERPS[interp], stream()),
                  "aesr_reslice_affine")
        else:
            coef = bspline_coefficients_3d(x4) if interp == "bspline" else None
            check(lib.aesr_reslice_taps_affine(None if coef is not None else ptr(x4), ptr(coef), ptr(out), N, Zs, Hs, Ws, Zo, Ho, Wo,
                                               m.ctypes.data_as(_hip.DP), TAP_KERNELS[interp], radius, int(bool(clamp01)), stream()),
                  "aesr_reslice_taps_affine")
    out = out[0] if was3d else out
    return out.cpu().numpy() if is_np else out


def reslice_grid(src, grid, interp="linear"):
    """``grid``: [Zo, Yo, Xo, 3] = (x, y, z) normalised to [-1, 1] (``grid_sample`` with ``align_corners=True``), numpy or tensor, one grid
    for all frames.  Otherwise as ``reslice_affine``, with ``linear`` and ``nearest`` only: the higher-order interpolators are on the
    affine path."""
    if interp in TAP_KERNELS:
        raise ValueError("interp=%r is on the affine path only (reslice_affine, reslice, reslice_like); a grid takes 'linear' or 'nearest'" % (interp,))
    code = _interp_code(interp)
    x4, was3d, is_np = _to_device(src)
    g = grid if torch.is_tensor(grid) else torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float32))
    if g.dim() != 4 or g.shape[-1] != 3 or min(g.shape) < 1:
        raise ValueError("grid must be [Zo, Yo, Xo, 3], got %s" % (tuple(g.shape),))
    g = g.to(device=x4.device, dtype=torch.float32).contiguous()
    Zo, Ho, Wo = (int(s) for s in g.shape[:3])
    N, Zs, Hs, Ws = (int(s) for s in x4.shape)
    out = torch.empty((N, Zo, Ho, Wo), device=x4.device, dtype=torch.float32)
    with torch.cuda.device(x4.device):
        check(lib.aesr_reslice_grid(ptr(x4), ptr(g), ptr(out), N, Zs, Hs, Ws, Zo, Ho, Wo, code, stream()), "aesr_reslice_grid")
    out = out[0] if was3d else out
    return out.cpu().numpy() if is_np else out


def reslice(src, src_geom, ref_geom, ref_shape, interp="linear", radius=5, clamp01=False):
    """``src`` ([Z, Y, X] or [T, Z, Y, X]) with geometry ``src_geom`` on the grid ``ref_shape`` = [z, y, x] of geometry ``ref_geom``."""
    return reslice_affine(src, affine_between(src_geom, ref_geom), ref_shape, interp, radius=radius, clamp01=clamp01)


def reslice_like(src_volume, ref_volume, interp="linear", radius=5, clamp01=False):
    """A ``volume_io.Volume`` on the grid of another: every frame of ``src_volume`` on the [z, y, x] grid of ``ref_volume``; float32
    [z, y, x] or [T, z, y, x] with T the frame count of the SOURCE."""
    return reslice(src_volume.array, Geometry.from_volume(src_volume), Geometry.from_volume(ref_volume), ref_volume.array.shape[-3:], interp,
                   radius=radius, clamp01=clamp01)
