"""The through-plane output grid at a target slice spacing: the ONE statement of where the output slices of a volume of ``Z`` slices,
``spacing_z`` mm apart, sit when ``target_spacing_z`` mm is asked for.  Pure host code, float64, no torch.

Output slice ``j`` sits at the input coordinate ``p_j = j * d / s`` (s = spacing_z, d = target_spacing_z); there are
``J = floor((Z - 1) * s / d + snap) + 1`` of them.  A ``p_j`` within ``snap`` of an integer IS that integer (10 mm at 10 / 3 mm: every
third slice is an input slice, however d / s rounds).  The first output slice is the first input slice, and the last one never lies
beyond the last input slice: nothing is extrapolated.  ``gap_j = min(floor(p_j), Z - 2)`` and ``alpha_j = p_j - gap_j`` is the weight of
slice ``gap_j + 1`` -- the convention of ``HipAE.decode_mixes``, ``alpha * z[i + 1] + (1 - alpha) * z[i]``.  ``alpha_j == 0`` is input
slice ``gap_j`` itself and ``alpha_j == 1`` (only the last slice can have it) input slice ``gap_j + 1``: both are ORIGINALS, passed
through and never synthesised.  With ``d = s / (n + 1)`` this is the integer grid of ``--num_interpolations n``; its alphas, cast to
fp32 as the kernels take them, are ``np.linspace(0, 1, n + 2)[1:-1]``'s."""
import math

import numpy as np

MAX_PER_GAP = 16          # aesr_lerp_multi takes 1..16 mixing coefficients per call


class ZGrid:
    """``J`` output slices; per output slice ``position`` (float64 input coordinate), ``gap`` (int64), ``alpha`` (float64),
    ``is_original`` (bool) and ``source`` (int64: the input slice an original IS, -1 for a synthesised one); per gap ``gap_alphas[i]``,
    the ascending list of the alphas of its synthesised slices (possibly empty)."""

    def __init__(self, Z, spacing_z, target_spacing_z, position, gap, alpha):
        self.Z, self.spacing_z, self.target_spacing_z = int(Z), float(spacing_z), float(target_spacing_z)
        self.position, self.gap, self.alpha = position, gap, alpha
        self.J = int(position.shape[0])
        self.is_original = (alpha == 0.0) | (alpha == 1.0)
        self.source = np.where(self.is_original, gap + (alpha == 1.0), -1).astype(np.int64)
        self.gap_alphas = [[float(a) for a in alpha[(gap == i) & ~self.is_original]] for i in range(max(self.Z - 1, 0))]

    @property
    def num_synthesised(self):
        return int((~self.is_original).sum())


def _spacing(value, name):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s=%r: a spacing in mm is expected" % (name, value))
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError("%s=%r must be positive and finite" % (name, value))
    return v


def target_grid(Z, spacing_z, target_spacing_z, snap=1e-6):
    """The grid of a volume of ``Z`` slices ``spacing_z`` mm apart at ``target_spacing_z`` mm (module docstring) as a ``ZGrid``."""
    if int(Z) != Z or Z < 1:
        raise ValueError("Z=%r: a volume has one slice or more" % (Z,))
    Z = int(Z)
    s, d = _spacing(spacing_z, "spacing_z"), _spacing(target_spacing_z, "target_spacing_z")
    if d > s:
        raise ValueError("target_spacing_z=%g is coarser than spacing_z=%g: that is a down-sampling, which slice synthesis does not do" % (d, s))
    J = int(math.floor((Z - 1) * s / d + snap)) + 1
    p = np.arange(J, dtype=np.float64) * d / s
    near = np.rint(p)
    p = np.where(np.abs(p - near) <= snap, near, p)
    p = np.minimum(p, float(Z - 1))
    gap = np.minimum(np.floor(p), max(Z - 2, 0)).astype(np.int64)
    alpha = p - gap
    grid = ZGrid(Z, s, d, p, gap, alpha)
    most = max([len(a) for a in grid.gap_alphas] + [0])
    if most > MAX_PER_GAP:
        raise ValueError("target_spacing_z=%g puts %d synthesised slices into one gap of spacing_z=%g (spacing_z / target_spacing_z = %.4g > %d): "
                         "at most %d per gap, the n <= %d of aesr_lerp_multi" % (d, most, s, s / d, MAX_PER_GAP + 1, MAX_PER_GAP, MAX_PER_GAP))
    return grid
