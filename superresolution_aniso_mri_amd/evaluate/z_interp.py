"""Conventional through-plane interpolation along z by an integer factor: nearest, linear, cubic B-spline and Lanczos-windowed sinc -- the
interpolators the reference hands to SimpleITK's ``ExpandImageFilter`` (evaluate/common.py:114-118) -- on the device (csrc/z_expand.hip,
include/aesr_hip_baselines.h).

All phase arithmetic is done HERE, in float64: the continuous input coordinate of each output phase ``p = o % factor``, the first tap
(``base``) and the weights (``phase_tables``).  They cross the C ABI as small host tables and the kernel only looks up: output slice
``o = q * factor + p`` is ``sum_k weights[p][k] * src[bound(q + base[p] + k)]``, summed in ascending k in double and rounded to fp32 once.

``align="itk"``: ``x(o) = (o + 0.5) / f - 0.5`` for ``o < Z f`` (ExpandImageFilter of ITK >= 4: the output grid is centred on the input's
extent, so no output slice coincides with an input slice).  ``align="grid"``: ``x(o) = o / f`` for ``o <= (Z - 1) f`` (every f-th output slice
is an input slice: the layout of the model's super-volume).  DESIGN.md section 2 has the definition of each method and what pins it."""
import numpy as np
import torch

from .. import _hip
from .._hip import check, lib, ptr, stream

METHODS = ("nearest", "linear", "bspline", "lanczos")
ALIGNS = {"itk": _hip.ZX_ALIGN_ITK, "grid": _hip.ZX_ALIGN_GRID}
LANCZOS_RADII = (3, 4, 5)
MAX_FACTOR = _hip.ZX_MAX_FACTOR


def check_method(interpol_filter):
    """None -> 'lanczos' (the reference's default, sitkLanczosWindowedSinc); anything outside METHODS is a ValueError."""
    if interpol_filter is None:
        return "lanczos"
    if interpol_filter not in METHODS:
        raise ValueError("interpol_filter=%r: expected one of %s (or None for lanczos)" % (interpol_filter, ", ".join(METHODS)))
    return interpol_filter


def _check(factor, align, radius):
    if int(factor) != factor or not 1 <= int(factor) <= MAX_FACTOR:
        raise ValueError("expand factor %r: expected an integer in 1..%d" % (factor, MAX_FACTOR))
    if align not in ALIGNS:
        raise ValueError("align=%r: expected 'itk' or 'grid'" % (align,))
    if radius not in LANCZOS_RADII:
        raise ValueError("radius=%r: the Lanczos radius is one of %s" % (radius, LANCZOS_RADII))


def phase_coordinates(factor, align="itk"):
    """float64 [factor]: the input coordinate of output slice o = p (q = 0); slice q * factor + p reads x[p] + q."""
    p = np.arange(int(factor), dtype=np.float64)
    return (p + 0.5) / factor - 0.5 if align == "itk" else p / factor


def _sinc(u):
    return np.sin(np.pi * u) / (np.pi * u)


def phase_tables(method, factor, align="itk", radius=5):
    """(base int32 [f], weights float64 [f, taps], boundary, needs_coefficients) of a method."""
    method = check_method(method)
    _check(factor, align, radius)
    x = phase_coordinates(factor, align)
    b = np.floor(x)
    t = x - b
    if method == "nearest":
        return np.floor(x + 0.5).astype(np.int32), np.ones((len(x), 1)), _hip.ZX_CLAMP, False
    if method == "linear":
        # x clamped to [0, Z - 1] then lerped == the lerp of index-clamped neighbours: outside the volume both neighbours are the edge slice
        return b.astype(np.int32), np.stack([1.0 - t, t], axis=1), _hip.ZX_CLAMP, False
    if method == "bspline":
        u = 1.0 - t
        w0 = u * u * u / 6.0
        w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
        w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
        return (b - 1).astype(np.int32), np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], axis=1), _hip.ZX_MIRROR, True
    R = int(radius)
    k = np.arange(-R + 1, R + 1, dtype=np.float64)
    w = np.empty((len(x), 2 * R))
    for p in range(len(x)):
        if t[p] == 0.0:
            w[p] = (k == 0).astype(np.float64)          # on a sample: exactly that sample
        else:
            d = t[p] - k
            w[p] = _sinc(d) * _sinc(d / R)          # not normalised: ITK's WindowedSincInterpolateImageFunction does not either
    return (b - R + 1).astype(np.int32), w, _hip.ZX_CLAMP, False


def out_slices(Z, factor, align="itk"):
    return int(lib.aesr_z_expand_out_slices(int(Z), int(factor), ALIGNS[align]))


def bspline_coefficients(x):
    """CUDA float32 [N, Z, H, W] -> CUDA float64 coefficients of the same shape (``spline_filter1d(order=3, mode='mirror')`` along z)."""
    _hip.require_gpu_tensor(x, "x")
    N, Z, H, W = (int(s) for s in x.shape)
    coef = torch.empty((N, Z, H, W), device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        check(lib.aesr_bspline_prefilter_z(ptr(x), ptr(coef), N, Z, H, W, stream()), "aesr_bspline_prefilter_z")
    return coef


def z_expand(x, factor, method="lanczos", align="itk", radius=5, clamp01=False):
    """x: CUDA float32 [Z, H, W] or [N, Z, H, W], contiguous -> new CUDA tensor with ``out_slices(Z, factor, align)`` slices per frame.
    One launch for all frames (two for ``bspline``: the pre-filter writes float64 coefficients first); no synchronisation; x is untouched."""
    _hip.require_gpu_tensor(x, "x")
    if x.dim() not in (3, 4):
        raise ValueError("expected [Z, H, W] or [N, Z, H, W], got %s" % (tuple(x.shape),))
    base, w, boundary, needs_coef = phase_tables(method, factor, align, radius)
    x4 = x if x.dim() == 4 else x.unsqueeze(0)
    N, Z, H, W = (int(s) for s in x4.shape)
    if min(N, Z, H, W) < 1:
        raise ValueError("nothing to expand: shape %s" % (tuple(x.shape),))
    Zo = out_slices(Z, factor, align)
    out = torch.empty((N, Zo, H, W), device=x.device, dtype=torch.float32)
    base = np.ascontiguousarray(base, np.int32)
    w = np.ascontiguousarray(w, np.float64)
    with torch.cuda.device(x.device):
        coef = bspline_coefficients(x4) if needs_coef else None
        check(lib.aesr_z_expand(None if needs_coef else ptr(x4), ptr(coef), ptr(out), N, Z, H, W, int(factor), Zo, w.shape[1],
                                base.ctypes.data_as(_hip.IP), w.ctypes.data_as(_hip.DP), boundary, int(bool(clamp01)), stream()), "aesr_z_expand")
    return out if x.dim() == 4 else out[0]


class ExpandedImage:
    """What the reference gets back from SimpleITK, as far as its callers use it: ``array`` ([z, y, x], numpy or a CUDA tensor),
    ``spacing`` and ``origin`` ([z, y, x], float64) and the two getters in SimpleITK's (x, y, z) order."""

    def __init__(self, array, spacing, origin):
        self.array = array
        self.spacing = np.asarray(spacing, dtype=np.float64)
        self.origin = np.asarray(origin, dtype=np.float64)

    def GetSpacing(self):
        return tuple(float(s) for s in self.spacing[::-1])

    def GetOrigin(self):
        return tuple(float(s) for s in self.origin[::-1])


def expanded_geometry(spacing, factor, align="itk"):
    """([z, y, x] spacing, [z, y, x] origin shift) of the expanded volume: z spacing s / f; the ITK grid starts half an input slice minus
    half an output slice before the first input slice (ExpandImageFilter keeps the physical extent), the ``grid`` alignment on it."""
    spacing = np.array(spacing, dtype=np.float64)
    origin = np.zeros_like(spacing)
    s = spacing[0]
    spacing[0] = s / factor
    if align == "itk":
        origin[0] = -0.5 * (s - s / factor)
    return spacing, origin
