"""In-plane resampling to and from the training spacing on the device: the reference's ``datasets/common.py:157-206``
``apply_2d_zoom_3d`` / ``apply_2d_zoom_4d`` (per slice ``scipy.ndimage.gaussian_filter(slice, 0.25 / zoom)``, then
``scipy.ndimage.zoom(volume, (1, zoom_y, zoom_x), order=1)``) as ONE launch of ``aesr_inplane_resample`` (csrc/inplane.hip,
include/aesr_hip_preproc.h) over all slices.

Every coordinate decision is made here, on the host, in float64 the way scipy makes it, and handed to the kernel as tables:

- ``zoom = float64(spacing) / new_spacing`` (the last two entries of each), the output size per axis is ``int(round(n * zoom))`` with
  Python's round (halves to even);
- output index ``o`` reads input coordinate ``c = o * ((n - 1) / (n_out - 1))`` (0 when ``n_out == 1``), linear between ``floor(c)`` and
  ``floor(c) + 1``;
- **the edge quirk**: scipy's mode is ``constant`` with ``cval = 0``, so when rounding makes ``c > n - 1`` for the last index that whole last
  output row / column is exactly 0 (3 % of the (size, spacing) pairs: 229 -> 224 at 1.37 mm, 243 -> 217 at 1.25 mm, 222 -> 111 at 0.7 mm;
  never for 216 -> 193, 256 -> 286, 224 -> 224).  The reference's saved volumes and scores carry that black line, so it is mirrored by
  default; ``clamp_edges=True`` gives the last line the value at ``n - 1`` instead;
- the Gaussian weights are scipy's (``radius = int(4 sigma + 0.5)``, ``exp(-0.5 / sigma^2 * x^2)`` normalised, in double), the boundary is
  ``reflect``; each 1-D pass is accumulated in double and stored as float32, as scipy does for float32 input.

``order=0`` (how the reference resamples label maps: ``apply_2d_zoom_3d(labels, ..., order=0, do_blur=False, as_type=int)``) is host tables
only: the same launch with the nearest-sample index ``min(floor(c + 0.5), n - 1)`` and weight 0, so a value is copied and never mixed; the
dead lines are the same.  Equal to ``scipy.ndimage.zoom(order=0)`` on every case of tests/golden/inplane_labels.npz, exact .5 ties included.

The device path takes float32: anything else is cast to float32 first (the reference would let scipy truncate every filter pass of an
integer-typed array back to the integer type; that case is not reproduced).  There is no CPU fallback: a numpy
array goes to the device and comes back."""
import numpy as np
import torch

from .. import _hip
from .._hip import check, lib, ptr, stream

MAX_RADIUS = 8          # IP_MAXR of csrc/inplane.hip
LAUNCHES = 0            # aesr_inplane_resample calls made by this process (tests: a 4-D volume is one launch)


def zoom_factors(spacing, new_spacing):
    """(zoom_y, zoom_x) in float64 from the last two entries of each spacing (datasets/common.py:190-196)."""
    spacing, new_spacing = list(spacing), list(new_spacing)
    zoom = np.array(spacing[-2:], np.float64) / np.array(new_spacing[-2:], np.float64)
    if zoom.shape != (2,) or not np.all(np.isfinite(zoom)) or not np.all(zoom > 0):
        raise ValueError("spacing %r / new_spacing %r do not give two positive zoom factors" % (spacing, new_spacing))
    return zoom


def out_size(n, zoom):
    """``int(round(n * zoom))``: the size scipy.ndimage.zoom gives an axis of n samples."""
    return int(round(int(n) * float(zoom)))


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage's 1-D Gaussian kernel for ``sigma``: (weights [2 r + 1] float64, r)."""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi / phi.sum(), radius


def zoom_tables(n, n_out, clamp_edges=False, order=1):
    """(i0 [n_out] int32, t [n_out] float64): output index o is ``(1 - t[o]) * in[i0[o]] + t[o] * in[min(i0[o] + 1, n - 1)]``;
    ``i0[o] == -1`` marks a dead line (exactly 0).  With ``clamp_edges`` a dead line reads ``in[n - 1]`` instead.
    ``order=0`` (nearest, for label maps): ``i0[o] = min(floor(c + 0.5), n - 1)`` and ``t = 0`` -- scipy.ndimage.zoom(order=0) rounds an
    exact .5 up; the dead lines are the same."""
    n, n_out = int(n), int(n_out)
    if n < 1 or n_out < 1:
        raise ValueError("cannot resample %d samples to %d" % (n, n_out))
    step = np.float64(n - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(1.0)
    c = np.arange(n_out, dtype=np.float64) * step
    dead = c > np.float64(n - 1)
    if order == 0:
        i0 = np.minimum(np.floor(c + 0.5).astype(np.int64), n - 1)
        t = np.zeros(n_out, np.float64)
    else:
        fl = np.floor(c)
        i0 = fl.astype(np.int64)
        t = c - fl
    i0[dead], t[dead] = (n - 1, 0.0) if clamp_edges else (-1, 0.0)
    return i0.astype(np.int32), t.astype(np.float64)


def dead_lines(n, n_out):
    """Indices of the output lines scipy leaves at 0 for an axis resampled from n to n_out samples."""
    return np.nonzero(zoom_tables(n, n_out)[0] < 0)[0]


def inplane_resample(x, zoom, do_blur=True, clamp_edges=False, order=1):
    """x: CUDA float32 [N, H, W], contiguous -> new CUDA tensor [N, Ho, Wo].  One launch; x is not modified.  ``order=0``: the same launch
    with the nearest-sample tables of ``zoom_tables`` (weight 0: a value is copied, never mixed)."""
    global LAUNCHES
    _hip.require_gpu_tensor(x, "x")
    if x.dim() != 3:
        raise ValueError("expected [N, H, W], got %s" % (tuple(x.shape),))
    N, H, W = (int(s) for s in x.shape)
    zy, zx = float(zoom[0]), float(zoom[1])
    Ho, Wo = out_size(H, zy), out_size(W, zx)
    if N < 1 or Ho < 1 or Wo < 1:
        raise ValueError("resampling %s by (%g, %g) leaves nothing" % (tuple(x.shape), zy, zx))
    assert Ho == lib.aesr_inplane_out_size(H, zy) and Wo == lib.aesr_inplane_out_size(W, zx)
    wy, ry = gaussian_weights(0.25 / zy)
    wx, rx = gaussian_weights(0.25 / zx)
    iy, ty = zoom_tables(H, Ho, clamp_edges, order)
    ix, tx = zoom_tables(W, Wo, clamp_edges, order)
    out = torch.empty((N, Ho, Wo), device=x.device, dtype=torch.float32)
    ws = torch.empty(int(lib.aesr_inplane_workspace_bytes(Ho, Wo)) // 8, device=x.device, dtype=torch.float64)
    as_d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_hip.DP)        # noqa: E731
    as_i = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_hip.IP)          # noqa: E731
    with torch.cuda.device(x.device):
        check(lib.aesr_inplane_resample(ptr(x), ptr(out), ptr(ws), N, H, W, Ho, Wo, as_d(wy), ry, as_d(wx), rx, as_i(iy), as_d(ty), as_i(ix),
                                        as_d(tx), 1 if do_blur else 0, stream()), "aesr_inplane_resample")
    LAUNCHES += 1
    return out


def _is_integer_type(as_type):
    try:
        return np.issubdtype(np.dtype(as_type), np.integer)
    except TypeError:
        return False


def _apply(arr, spacing, new_spacing, order, do_blur, as_type, clamp_edges, ndim):
    if order not in (0, 1):
        raise NotImplementedError("order=%r: only order=1 (linear, the reference's default) and order=0 (nearest, its choice for label maps) "
                                  "are built" % (order,))
    if arr.ndim != ndim:
        raise ValueError("expected a %d-D array, got shape %s" % (ndim, tuple(arr.shape)))
    zoom = zoom_factors(spacing, new_spacing)
    on_device = torch.is_tensor(arr)
    if on_device:
        if not arr.is_cuda:
            raise RuntimeError("a tensor must live on the GPU (got %s); pass a numpy array for host data" % arr.device)
        x = arr
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("apply_2d_zoom needs the GPU: the HIP path has no CPU fallback")
        x = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).cuda()
    lead = tuple(x.shape[:-2])
    x = x.to(torch.float32).contiguous().reshape((-1,) + tuple(x.shape[-2:]))       # no copy for a contiguous float32 tensor
    out = inplane_resample(x, zoom, do_blur=do_blur, clamp_edges=clamp_edges, order=order)
    out = out.reshape(lead + tuple(out.shape[-2:]))
    if _is_integer_type(as_type):
        out = torch.round(out)                      # halves to even, like np.round
        if on_device:
            return out.to({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[np.dtype(as_type).itemsize])
        return out.cpu().numpy().astype(as_type)
    return out if on_device else out.cpu().numpy()


def apply_2d_zoom_3d(arr3d, spacing, new_spacing, order=1, do_blur=True, as_type=np.float32, clamp_edges=False):
    """The reference's ``apply_2d_zoom_3d`` (datasets/common.py:178-206) on the device.

    :param arr3d: [#slices, IH, IW]; a numpy array (-> numpy array) or a CUDA tensor (-> CUDA tensor, no host round trip)
    :param spacing: the array's spacing; only the last two entries (y, x) count
    :param new_spacing: the spacing to resample to; only the last two entries count
    :param order: 1 (linear) or 0 (nearest: label maps, with do_blur=False); anything else raises NotImplementedError
    :param do_blur: Gaussian blur with sigma = 0.25 / zoom before the interpolation
    :param as_type: an integer type marks labels (use with do_blur=False): the result is rounded and cast; otherwise float32
    :param clamp_edges: False mirrors scipy's all-zero last row / column where it occurs (module docstring); True repeats the edge

    The reference blurs INTO its caller's array; this does not: the input is left untouched."""
    return _apply(arr3d, spacing, new_spacing, order, do_blur, as_type, clamp_edges, 3)


def apply_2d_zoom_4d(arr4d, spacing, new_spacing, order=1, do_blur=True, as_type=np.float32, clamp_edges=False):
    """The reference's ``apply_2d_zoom_4d`` (datasets/common.py:157-175): [#timepoints, #slices, IH, IW], all T * Z slices in ONE
    launch (the reference loops over the frames).  Arguments as ``apply_2d_zoom_3d``; the input is left untouched."""
    return _apply(arr4d, spacing, new_spacing, order, do_blur, as_type, clamp_edges, 4)
