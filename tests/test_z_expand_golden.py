"""not gpu: the conventional through-plane baselines (nearest, linear, cubic B-spline, Lanczos along z by an integer factor) against scipy's
own results (tests/golden/z_expand.npz, written by tests/make_golden_z_expand.py) and against a numpy restatement kept in this file.

- The restatement (``restate_*``; it shares no code with the package) works per OUTPUT SLICE: coordinate ``x(o)``, taps and weights in
  float64, the sum over the taps in ascending index order in double, one rounding to fp32.  Against the fixture: the spline coefficients and
  the spline (scipy's float64 output, before any rounding) within 1e-12 absolute (two independent implementations: 9e-16 measured), linear
  exactly; its own Lanczos and nearest results are stored in the fixture too and must stay what they were.
- The package's host tables (``evaluate.z_interp.phase_tables``: per PHASE, the form the kernel is given) applied by ``apply_tables`` -- the
  kernel's arithmetic in numpy -- reproduce the restatement within one fp32 rounding.
- Lanczos weights: sum in [0.998, 1] at the default radius 5 (LANCZOS_SUM has the ranges of radius 3 and 4), exactly {1, 0...} at the phase that sits on a sample; ``align='grid'`` with linear returns the
  originals bitwise at every f-th slot; the evaluation protocol returns as many slices as it was given.
- Every refusal of the two launch entry points and of the Python interface that is decided on the host; the CLI flags."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 1024.0          # the fixture's inputs are multiples of 1/1024 (exact in fp32), stored as uint16 counts
# tag -> (shape, factor); the last three axes are [Z, H, W]
CASES = {"z1f2": ((1, 3, 5), 2), "z2f3": ((2, 3, 5), 3), "z3f2": ((3, 3, 5), 2), "z5f4": ((5, 4, 8), 4), "z11f6": ((11, 4, 8), 6),
         "z40f3": ((40, 16, 12), 3), "w33": ((7, 2, 33), 2), "n2": ((2, 5, 4, 8), 3)}
ALIGNS = ("itk", "grid")
METHODS = ("nearest", "linear", "bspline", "lanczos3", "lanczos5")
SCIPY_METHODS = ("linear", "bspline")
# what the fixture holds of the one large case: scipy's results only (the restatement's are recomputed where they are needed)
BIG = {"z40f3": (("itk", "linear"), ("itk", "bspline"))}
TOL_SPLINE = 1e-12
TOL_ROUNDING = 1.2e-7          # one fp32 rounding of a value below 2: per-phase against per-slice coordinates can flip one
# The Lanczos kernel is no partition of unity and the weights are not normalised.  Range of sum_k sinc(t - k) sinc((t - k) / R) over t in
# [0, 1), from the closed form on a grid of 2000 t (the extreme is at t = 1/2, the other end at t = 0 where the sum is exactly 1):
# R = 5: 0.998746 .. 1, R = 3: 0.994299 .. 1, R = 4: 1 .. 1.002433.  The bound of the default radius 5 is [0.998, 1]; the other two radii
# get the same margin below / above their own extreme.
LANCZOS_SUM = {5: (0.998, 1.0), 3: (0.994, 1.0), 4: (1.0, 1.0025)}
_FX = {}


def fixture():
    if not _FX:
        _FX.update(np.load(os.path.join(HERE, "golden", "z_expand.npz")))
    return _FX


def case_input(tag):
    return (fixture()["%s/in" % tag] / Q).astype(np.float32)


def stored(tag):
    """[(align, method)] the fixture holds for a case"""
    return BIG.get(tag, tuple((a, m) for a in ALIGNS for m in METHODS))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def out_count(Z, f, align):
    return Z * f if align == "itk" else (Z - 1) * f + 1


def coordinates(Z, f, align):
    o = np.arange(out_count(Z, f, align), dtype=np.float64)
    return (o + 0.5) / f - 0.5 if align == "itk" else o / f


def mirror(i, Z):
    if Z == 1:
        return np.zeros_like(i)
    p = 2 * Z - 2
    m = np.mod(i, p)
    return np.where(m < Z, m, p - m)


def restate_coefficients(x):
    """float32 [Z, ...] -> float64 cubic B-spline coefficients along axis 0: gain 6, pole sqrt(3) - 2, whole-sample mirror, exact
    initialisation over the whole line with running powers of the pole."""
    Z = x.shape[0]
    c = x.astype(np.float64)
    if Z == 1:
        return c
    z1 = np.sqrt(3.0) - 2.0
    c = c * 6.0
    zn1 = 1.0
    for _ in range(Z - 1):
        zn1 *= z1
    c0 = c[0] + zn1 * c[Z - 1]
    zi = z1
    for i in range(1, Z - 1):
        c0 = c0 + zi * (c[i] + zn1 * c[Z - 1 - i])
        zi *= z1
    c[0] = c0 / (1.0 - zn1 * zn1)
    for i in range(1, Z):
        c[i] = c[i] + z1 * c[i - 1]
    c[Z - 1] = z1 / (z1 * z1 - 1.0) * (z1 * c[Z - 2] + c[Z - 1])
    for i in range(Z - 2, -1, -1):
        c[i] = z1 * (c[i + 1] - c[i])
    return c


def _sum_taps(src, idx, weights):
    """sum_k weights[k] * src[idx[k]] in ascending k, in double; idx[k]: int [Zo], weights[k]: float64 [Zo]"""
    tail = (1,) * (src.ndim - 1)
    acc = weights[0].reshape((-1,) + tail) * src[idx[0]]
    for k in range(1, len(idx)):
        acc = acc + weights[k].reshape((-1,) + tail) * src[idx[k]]
    return acc


def lanczos_weights(t, R):
    """float64 [2 R] for one t in [0, 1): taps k = -R + 1 .. R"""
    k = np.arange(-R + 1, R + 1, dtype=np.float64)
    if t == 0.0:
        return (k == 0).astype(np.float64)
    d = t - k
    return np.sin(np.pi * d) / (np.pi * d) * (np.sin(np.pi * d / R) / (np.pi * d / R))


def restate_spline64(x, f, align):
    """the cubic spline before its rounding to fp32: float64 [out_count, H, W]"""
    if x.ndim == 4:
        return np.stack([restate_spline64(v, f, align) for v in x])
    Z = x.shape[0]
    c = coordinates(Z, f, align)
    b = np.floor(c).astype(np.int64)
    t = c - b
    u = 1.0 - t
    w = [u * u * u / 6.0, (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0, (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0]
    w.append(1.0 - w[0] - w[1] - w[2])
    return _sum_taps(restate_coefficients(x), [mirror(b - 1 + k, Z) for k in range(4)], w)


def restate(x, f, method, align="itk"):
    """float32 [Z, H, W] -> float32 [out_count, H, W] (a 4-D input frame by frame); method: one of METHODS"""
    if x.ndim == 4:
        return np.stack([restate(v, f, method, align) for v in x])
    Z = x.shape[0]
    c = coordinates(Z, f, align)
    xd = x.astype(np.float64)
    if method == "nearest":
        return x[np.clip(np.floor(c + 0.5).astype(np.int64), 0, Z - 1)]
    if method == "linear":
        c = np.clip(c, 0, Z - 1)
        b = np.floor(c).astype(np.int64)
        t = c - b
        return _sum_taps(xd, [b, np.minimum(b + 1, Z - 1)], [1.0 - t, t]).astype(np.float32)
    if method == "bspline":
        return restate_spline64(x, f, align).astype(np.float32)
    b = np.floor(c).astype(np.int64)
    t = c - b
    R = int(method[len("lanczos"):])
    w = np.stack([lanczos_weights(ti, R) for ti in t], axis=1)
    return _sum_taps(xd, [np.clip(b - R + 1 + k, 0, Z - 1) for k in range(2 * R)], list(w)).astype(np.float32)


def apply_tables(src, f, Zo, base, w, boundary):
    """The kernel's arithmetic in numpy: out[q f + p] = sum_k w[p][k] * src[bound(q + base[p] + k)], ascending k, double, one rounding."""
    if src.ndim == 4:
        return np.stack([apply_tables(v, f, Zo, base, w, boundary) for v in src])
    Z = src.shape[0]
    o = np.arange(Zo)
    q, p = o // f, o % f
    idx = [q + base[p] + k for k in range(w.shape[1])]
    idx = [mirror(i, Z) if boundary == 1 else np.clip(i, 0, Z - 1) for i in idx]
    return _sum_taps(src.astype(np.float64), idx, [w[p, k] for k in range(w.shape[1])]).astype(np.float32)


def package_method(method):
    """restatement method name -> (package method, radius)"""
    return ("lanczos", int(method[len("lanczos"):])) if method.startswith("lanczos") else (method, 5)


# ---- fixture and restatement -----------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_issue_asked_for():
    fx = fixture()
    assert [str(t) for t in fx["tags"]] == list(CASES)
    for tag, (shape, f) in CASES.items():
        x = fx["%s/in" % tag]
        assert x.shape == shape and x.dtype == np.uint16 and int(x.max()) <= Q and int(fx["%s/factor" % tag]) == f
        assert fx["%s/coef" % tag].shape == shape and fx["%s/coef" % tag].dtype == np.float64
        for align, method in stored(tag):
            y = fx["%s/%s/%s" % (tag, align, method)]
            assert y.dtype == (np.float64 if method == "bspline" else np.float32) and y.shape == shape[:-3] + (out_count(shape[-3], f, align),) + shape[-2:], (tag, align, method)
    assert CASES["z40f3"][0][2] % 4 == 0 and CASES["z3f2"][0][2] % 4 != 0 and CASES["w33"][0][2] == 33 and len(CASES["n2"][0]) == 4
    size = os.path.getsize(os.path.join(HERE, "golden", "z_expand.npz"))
    assert size < 0.7 * os.path.getsize(os.path.join(HERE, "golden", "inplane.npz"))


def test_restatement_against_scipys_results():
    fx = fixture()
    for tag, (shape, f) in CASES.items():
        x = case_input(tag)
        coef = np.stack([restate_coefficients(v) for v in x]) if x.ndim == 4 else restate_coefficients(x)
        err = float(np.abs(coef - fx["%s/coef" % tag]).max())
        assert err <= TOL_SPLINE, (tag, "coef", err)
        for align, method in stored(tag):
            want, got = fx["%s/%s/%s" % (tag, align, method)], restate(x, f, method, align)
            assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == (np.float64 if method == "bspline" else np.float32)
            if method == "bspline":          # scipy's result in float64, before any rounding
                err = float(np.abs(restate_spline64(x, f, align) - want).max())
                assert err <= TOL_SPLINE, (tag, align, err)
                assert float(np.abs(got.astype(np.float64) - want).max()) <= TOL_ROUNDING / 2 + TOL_SPLINE
            else:
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (tag, align, method, float(np.abs(got - want).max()))


def test_restatement_edge_cases():
    x = case_input("z5f4")
    for align in ALIGNS:
        assert np.array_equal(restate(x, 1, "linear", align), x) and np.array_equal(restate(x, 1, "lanczos5", align), x)
        assert np.array_equal(restate(x, 1, "nearest", align), x)
        assert np.abs(restate(x, 1, "bspline", align) - x).max() <= TOL_ROUNDING              # the spline interpolates its samples
    one = case_input("z1f2")
    for method in METHODS:          # a single slice: every method repeats it (Lanczos up to its weight sum)
        got = restate(one, 2, method, "itk")
        defect = max(abs(1 - v) for v in LANCZOS_SUM[int(method[7:])]) if method.startswith("lanczos") else 0.0
        assert got.shape == (2, 3, 5) and np.abs(got - one[0]).max() <= defect + TOL_ROUNDING, method
    const = np.full((6, 2, 3), 0.75, np.float32)
    assert np.abs(restate(const, 3, "bspline", "itk") - 0.75).max() <= TOL_ROUNDING
    assert np.array_equal(restate(const, 3, "linear", "itk"), np.full((18, 2, 3), 0.75, np.float32))


# ---- the host tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(CASES))
def test_phase_tables_reproduce_the_restatement(tag):
    from superresolution_aniso_mri_amd.evaluate import z_interp
    shape, f = CASES[tag]
    x = case_input(tag)
    Z = shape[-3]
    for align in ALIGNS:
        assert z_interp.out_slices(Z, f, align) == out_count(Z, f, align)
        for method in METHODS:
            name, radius = package_method(method)
            base, w, boundary, needs_coef = z_interp.phase_tables(name, f, align, radius)
            assert base.dtype == np.int32 and base.shape == (f,) and w.dtype == np.float64 and w.shape[0] == f and w.shape[1] <= 10
            assert needs_coef == (method == "bspline") and boundary == (1 if method == "bspline" else 0)
            src = x
            if needs_coef:
                src = np.stack([restate_coefficients(v) for v in x]) if x.ndim == 4 else restate_coefficients(x)
            got, want = apply_tables(src, f, out_count(Z, f, align), base, w, boundary), restate(x, f, method, align)
            err = float(np.abs(got.astype(np.float64) - want).max())
            assert err <= (0 if method == "nearest" else TOL_ROUNDING), (tag, align, method, err)


def test_lanczos_weights():
    from superresolution_aniso_mri_amd.evaluate import z_interp
    for R in (3, 4, 5):
        for f in range(1, 17):
            for align in ALIGNS:
                base, w, _, _ = z_interp.phase_tables("lanczos", f, align, R)
                lo, hi = LANCZOS_SUM[R]
                assert w.shape == (f, 2 * R) and (lo <= w.sum(axis=1)).all() and (w.sum(axis=1) <= hi).all(), (R, f, align, w.sum(axis=1))
                x = z_interp.phase_coordinates(f, align)
                for p in range(f):
                    # two ways to write sinc(u / R) in float64: a few ulps of weights below 1
                    assert np.abs(w[p] - lanczos_weights(x[p] - np.floor(x[p]), R)).max() <= 1e-15 and base[p] == np.floor(x[p]) - R + 1
                on_sample = [p for p in range(f) if x[p] == np.floor(x[p])]
                assert on_sample == ([(f - 1) // 2] if f % 2 else []) if align == "itk" else on_sample == [0]
                for p in on_sample:          # exactly the sample: 1 at k = 0 (column R - 1), 0 elsewhere -- not sin(pi k) / (pi k)
                    assert w[p].tolist() == [1.0 if k == R - 1 else 0.0 for k in range(2 * R)] and base[p] + R - 1 == x[p]
    with pytest.raises(ValueError, match="radius"):
        z_interp.phase_tables("lanczos", 3, "itk", 6)
    with pytest.raises(ValueError, match="radius"):
        z_interp.phase_tables("lanczos", 3, "itk", 2)


def test_grid_alignment_passes_the_originals_through():
    from superresolution_aniso_mri_amd.evaluate import z_interp
    for tag, (shape, f) in CASES.items():
        x = case_input(tag)
        Z = shape[-3]
        for method in ("nearest", "linear", "lanczos3", "lanczos5"):
            name, radius = package_method(method)
            base, w, boundary, _ = z_interp.phase_tables(name, f, "grid", radius)
            for got in (restate(x, f, method, "grid"), apply_tables(x, f, out_count(Z, f, "grid"), base, w, boundary)):
                slots = got[..., ::f, :, :]
                assert slots.shape == x.shape and np.array_equal(slots.view(np.int32), x.view(np.int32)), (tag, method)
        # the ITK grid never sits on a sample for even f, and on one per f outputs for odd f
        lin = restate(x, f, "linear", "itk")
        if f % 2:
            assert np.array_equal(lin[..., (f - 1) // 2::f, :, :], x)


def test_protocol_slice_count_is_the_inputs():
    """keep [::f], expand, cut to the last kept slice, append the unpaired originals: Z slices again, with and without a remainder."""
    from evaluate.common import determine_last_slice
    from superresolution_aniso_mri_amd.evaluate import z_interp
    for Z in range(1, 27):
        for f in range(1, 9):
            kept = len(range(0, Z, f))
            last, remain = determine_last_slice(Z, f), (Z - 1) % f
            for align in ALIGNS:
                Zo = z_interp.out_slices(kept, f, align)
                assert Zo >= last + 1 and (align == "itk" or Zo == last + 1), (Z, f, align)
                assert min(Zo, last + 1) + remain == Z
    sp, org = z_interp.expanded_geometry([8.0, 1.4, 1.25], 4, "itk")
    assert sp.tolist() == [2.0, 1.4, 1.25] and org.tolist() == [-3.0, 0.0, 0.0]
    sp, org = z_interp.expanded_geometry([8.0, 1.4, 1.25], 4, "grid")
    assert sp.tolist() == [2.0, 1.4, 1.25] and org.tolist() == [0.0, 0.0, 0.0]
    img = z_interp.ExpandedImage(np.zeros((2, 3, 4), np.float32), sp, [-3.0, 0.0, 0.5])
    assert img.GetSpacing() == (1.25, 1.4, 2.0) and img.GetOrigin() == (0.5, 0.0, -3.0) and img.spacing.dtype == np.float64


# ---- the fifth header ------------------------------------------------------------------------------------------------------------
def test_host_queries():
    from superresolution_aniso_mri_amd import _hip
    f = _hip.lib.aesr_z_expand_out_slices
    for Z in (1, 2, 3, 30, 59, 4096):
        for k in (1, 2, 3, 7, 16, 100):
            assert f(Z, k, 0) == Z * k and f(Z, k, 1) == (Z - 1) * k + 1
    assert f(0, 2, 0) == 0 and f(-1, 2, 1) == 0 and f(5, 0, 0) == 0 and f(5, 2, 2) == 0 and f(5, 2, -1) == 0
    assert f(2 ** 30, 2, 0) == 0 and f(2 ** 30, 2, 1) == 2 ** 30 * 2 - 1            # Z f = 2^31 does not fit an int; (Z - 1) f + 1 does
    sb, P = _hip.lib.aesr_z_expand_store_bytes, ctypes.c_void_p
    assert sb(12, P(4096), P(8192)) == 16 and sb(10, P(4096), P(8192)) == 4 and sb(12, P(4100), P(8192)) == 4 and sb(12, P(4096), P(8200)) == 4
    assert sb(12, P(4104), P(8192)) == 4 and sb(0, P(4096), P(8192)) == 4 and sb(33, P(4096), P(8192)) == 4
    cb = _hip.lib.aesr_bspline_coef_bytes
    assert cb(2, 30, 224, 224) == 8 * 2 * 30 * 224 * 224 and cb(1, 1, 1, 1) == 8 and cb(0, 3, 4, 5) == 0 and cb(1, 3, -4, 5) == 0
    assert cb(30, 59, 1024, 1024) == 8 * 30 * 59 * 1024 * 1024                      # size_t arithmetic: 14.8e9


# ---- refusals decided on the host ------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the device pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    from superresolution_aniso_mri_amd.evaluate import z_interp
    fake, fake2 = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    base, w, boundary, _ = z_interp.phase_tables("lanczos", 3, "itk", 5)
    IA = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_hip.IP)          # noqa: E731
    DA = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_hip.DP)        # noqa: E731
    names = ["inp", "coef", "out", "N", "Z", "H", "W", "factor", "Zo", "taps", "base", "weights", "boundary", "clamp01", "stream"]
    ok = [fake, None, fake2, 1, 40, 16, 12, 3, 120, 10, IA(base), DA(w), boundary, 0, None]

    def rc(**over):
        args = list(ok)
        for k, v in over.items():
            args[names.index(k)] = v
        return _hip.lib.aesr_z_expand(*args)

    err = _hip.last_error
    assert rc(inp=None) == 1 and "neither" in err() and "in and coef" in err()
    assert rc(coef=fake) == 1 and "both" in err() and "in and coef" in err()
    assert rc(out=None) == 1 and "out is a null" in err()
    assert rc(base=None) == 1 and "base_host" in err() and rc(weights=None) == 1 and "weights_host" in err()
    assert rc(inp=ctypes.c_void_p(4098)) == 1 and "in is not 4-byte" in err()
    assert rc(out=ctypes.c_void_p(4097)) == 1 and "out is not 4-byte" in err()
    assert rc(inp=None, coef=ctypes.c_void_p(4100)) == 1 and "coef is not 8-byte" in err()
    for dim in ("N", "Z", "H", "W"):
        assert rc(**{dim: 0}) == 1 and "N, Z, H, W" in err() and rc(**{dim: -4}) == 1
    assert rc(factor=0) == 1 and "factor" in err() and rc(taps=0) == 1 and "taps" in err()
    assert rc(factor=17, Zo=40 * 17) == 3 and "factor=17" in err() and "16" in err()
    assert rc(taps=11) == 3 and "taps=11" in err() and "10" in err()
    assert rc(boundary=2) == 1 and "boundary" in err() and rc(clamp01=2) == 1 and "clamp01" in err()
    for bad in (119, 121, 0, -120, 117):
        assert rc(Zo=bad) == 1 and "Zo=%d" % bad in err() and "aesr_z_expand_out_slices" in err()
    assert rc(Z=2048, H=1024, W=1024, factor=1, Zo=2048) == 1 and "2^31" in err()
    big = base.copy()
    big[1] = 5000
    assert rc(base=IA(big)) == 1 and "base_host[1]" in err()
    wide = base.copy()
    wide[2] += 40
    assert rc(base=IA(wide)) == 3 and "base_host" in err() and "window" in err()
    nan = w.copy()
    nan[2, 3] = np.nan
    assert rc(weights=DA(nan)) == 1 and "weights_host[2][3]" in err()
    # the pre-filter
    pf = _hip.lib.aesr_bspline_prefilter_z
    assert pf(None, fake2, 1, 4, 4, 4, None) == 1 and "in is a null" in err()
    assert pf(fake, None, 1, 4, 4, 4, None) == 1 and "coef is a null" in err()
    assert pf(fake, ctypes.c_void_p(4100), 1, 4, 4, 4, None) == 1 and "coef is not 8-byte" in err()
    assert pf(ctypes.c_void_p(4098), fake2, 1, 4, 4, 4, None) == 1 and "in is not 4-byte" in err()
    for i in range(4):
        dims = [1, 4, 4, 4]
        dims[i] = 0
        assert pf(fake, fake2, *dims, None) == 1 and "N, Z, H, W" in err()
    assert pf(fake, fake2, 2, 1024, 1024, 1024, None) == 1 and "2^31" in err()


def test_python_interface_refusals():
    import torch
    from evaluate.common import create_simple_interpolation
    from superresolution_aniso_mri_amd.evaluate import common as ec
    from superresolution_aniso_mri_amd.evaluate import find_best_model as fbm
    from superresolution_aniso_mri_amd.evaluate import z_interp
    assert create_simple_interpolation is ec.create_simple_interpolation              # the root shim
    vol, sp = np.zeros((4, 3, 5), np.float32), np.array([8.0, 1.4, 1.4])
    with pytest.raises(ValueError, match="new_spacing_z or expand_factor"):
        create_simple_interpolation(vol, sp)
    with pytest.raises(ValueError, match="interpol_filter"):
        create_simple_interpolation(vol, sp, expand_factor=2, interpol_filter="cubic")
    with pytest.raises(ValueError, match="interpol_filter"):
        create_simple_interpolation(vol, sp, expand_factor=2, interpol_filter=3)
    with pytest.raises(ValueError, match="align"):
        create_simple_interpolation(vol, sp, expand_factor=2, align="center")
    with pytest.raises(ValueError, match="radius"):
        create_simple_interpolation(vol, sp, expand_factor=2, radius=7)
    with pytest.raises(ValueError, match="1..16"):
        create_simple_interpolation(vol, sp, expand_factor=17)
    with pytest.raises(ValueError, match="1..16"):
        create_simple_interpolation(vol, sp, new_spacing_z=0.25)                     # ceil(8 / 0.25) = 32
    with pytest.raises(ValueError, match="1..16"):
        create_simple_interpolation(vol, sp, expand_factor=0)
    with pytest.raises(ValueError, match=r"\[z, y, x\]"):
        create_simple_interpolation(vol[0], sp, expand_factor=2)
    with pytest.raises(ValueError, match="spacing"):
        create_simple_interpolation(vol, sp[:2], expand_factor=2)
    with pytest.raises(TypeError):
        create_simple_interpolation(vol, sp, None, 2, None, False, "grid")            # align and radius are keyword-only
    assert z_interp.check_method(None) == "lanczos" and [z_interp.check_method(m) for m in z_interp.METHODS] == list(z_interp.METHODS)
    with pytest.raises(RuntimeError, match="GPU"):
        z_interp.z_expand(torch.zeros(3, 4, 4), 2)                                   # a CPU tensor: no fallback
    with pytest.raises(ValueError, match="interpol_filter"):
        fbm.evaluate_interpolation_performance(None, {}, {}, downsample_steps=2, interpol_filter="spline")
    with pytest.raises(ValueError, match="trainer"):
        fbm.evaluate_interpolation_performance(None, {}, {}, downsample_steps=2)
    empty = fbm.evaluate_interpolation_performance(None, {}, {}, downsample_steps=2, interpol_filter="linear")
    assert empty["ssim"] == [] and set(empty) >= {"ssim", "psnr", "vif", "ssim_synth", "lpips"}


def test_cli_flags(tmp_path, capsys):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd.evaluate import compare_methods as cm
    np.save(str(tmp_path / "v.npy"), np.zeros((3, 4, 4), np.float32))
    with pytest.raises(SystemExit):
        ghv.main(["--method=linear", "--resample", "--spacing", "1.5", "1.5", "--data_input_dir=" + str(tmp_path), "--output_dir=" + str(tmp_path / "o")])
    assert "--resample belongs to --method ae" in capsys.readouterr().err and not (tmp_path / "o").exists()
    with pytest.raises(SystemExit):
        ghv.main(["--method=cubic", "--data_input_dir=" + str(tmp_path)])
    assert "--method" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ghv.main(["--method=lanczos", "--lanczos_radius=6", "--data_input_dir=" + str(tmp_path)])
    with pytest.raises(SystemExit):
        ghv.main(["--method=lanczos", "--align=centre", "--data_input_dir=" + str(tmp_path)])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        ghv.main(["--method=bspline", "--data_input_dir=" + str(tmp_path)])          # neither --exper_dir nor --output_dir: nowhere to write
    assert "--output_dir" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ghv.main(["--data_input_dir=" + str(tmp_path), "--output_dir=" + str(tmp_path / "o")])
    assert "--exper_dir" in capsys.readouterr().err
    a = cm.parse_args(["--exper_dir=E", "--volumes_dir=D", "--downsample_steps=3"])
    assert (a.exper_dir, a.volumes_dir, a.downsample_steps, a.eval_axis, a.align, a.model_nbr) == ("E", "D", 3, 0, "itk", None)
    a = cm.parse_args(["--exper_dir=E", "--volumes_dir=D", "--downsample_steps=2", "--eval_axis=2", "--align=grid", "--model_nbr=4"])
    assert (a.eval_axis, a.align, a.model_nbr) == (2, "grid", 4)
    with pytest.raises(SystemExit):
        cm.parse_args(["--exper_dir=E", "--volumes_dir=D"])
    with pytest.raises(SystemExit):
        cm.parse_args(["--exper_dir=E", "--volumes_dir=D", "--downsample_steps=2", "--eval_axis=3"])
    table = cm.format_table({"ae_combined": {"ssim": [0.5, 0.7], "psnr": [20.0, 22.0], "vif": [0.3, 0.5], "ssim_synth": [0.4], "psnr_synth": [19.0],
                                             "vif_synth": []}}, 3)
    assert "ae_combined" in table and "0.6000" in table and "21.0000" in table and "nan" in table
