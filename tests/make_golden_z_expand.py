#!/usr/bin/env python
"""Generate tests/golden/z_expand.npz: scipy's own results for the conventional through-plane baselines, and the restatement's for the two
methods scipy has no counterpart of.  A script, not a test (pytest does not collect it).  It needs scipy and numpy only.

Per case ``<tag>`` of ``test_z_expand_golden.CASES`` (inputs uniform in [0, 1] from a seeded RandomState, quantised to multiples of 1/1024
so that they are exact in fp32, stored as uint16 counts):
  <tag>/in, <tag>/factor
  <tag>/coef                 scipy.ndimage.spline_filter1d(in, order=3, axis=z, mode='mirror', output=float64)
  <tag>/<align>/linear       scipy.ndimage.map_coordinates(column, [x], order=1, mode='nearest') of every (y, x) column, float32
  <tag>/<align>/bspline      map_coordinates(coef column, [x], order=3, mode='mirror', prefilter=False, output=float64): before any rounding
  <tag>/<align>/nearest, lanczos3, lanczos5     the numpy restatement of tests/test_z_expand_golden.py (scipy has no Lanczos; its order-0
                             rounding is not the round-half-up of the definition)
with ``x(o) = (o + 0.5) / f - 0.5`` for o < Z f (align ``itk``) or ``x(o) = o / f`` for o <= (Z - 1) f (``grid``), computed per OUTPUT SLICE.
Of the one large case only what ``test_z_expand_golden.BIG`` lists is stored.

Run:  python tests/make_golden_z_expand.py
"""
import os
import sys

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import test_z_expand_golden as tz  # noqa: E402

SEED = 20261


def scipy_columns(vol, coords, order, mode, dtype):
    """map_coordinates along z of every (y, x) column of vol [Z, H, W] (1-D calls: in-plane nothing is interpolated)"""
    Z, H, W = vol.shape
    out = np.empty((len(coords), H, W), dtype)
    for y in range(H):
        for x in range(W):
            out[:, y, x] = ndi.map_coordinates(vol[:, y, x], [coords], order=order, mode=mode, prefilter=False, output=dtype)
    return out


def frames(a, fn):
    return np.stack([fn(v) for v in a]) if a.ndim == 4 else fn(a)


def main():
    rs = np.random.RandomState(SEED)
    out = {"tags": np.array(list(tz.CASES))}
    for tag, (shape, f) in tz.CASES.items():
        counts = rs.randint(0, int(tz.Q) + 1, size=shape).astype(np.uint16)
        x = (counts / tz.Q).astype(np.float32)
        Z = shape[-3]
        out["%s/in" % tag], out["%s/factor" % tag] = counts, np.int32(f)
        coef = ndi.spline_filter1d(x, order=3, axis=x.ndim - 3, mode="mirror", output=np.float64)
        out["%s/coef" % tag] = coef
        for align, method in tz.stored(tag):
            c = tz.coordinates(Z, f, align)
            if method == "linear":
                y = frames(x, lambda v: scipy_columns(v, c, 1, "nearest", np.float32))
            elif method == "bspline":
                y = frames(coef, lambda v: scipy_columns(v, c, 3, "mirror", np.float64))
            else:
                y = tz.restate(x, f, method, align)
            out["%s/%s/%s" % (tag, align, method)] = y
    path = os.path.join(HERE, "golden", "z_expand.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
