"""not gpu: affine reslicing with a cubic B-spline or a windowed sinc (include/aesr_hip_reslice_taps.h) restated in numpy, against the fixture that
tests/make_golden_reslice_taps.py wrote with scipy (tests/golden/reslice_taps.npz); and the parts of the host layer that need no device.

The restatement is the contract itself, in the device's operation order and kept in this file (it shares no code with the package):
positions ((m0 xo + m1 yo) + m2 zo) + m3; ITK's buffer rule -0.5 <= p < size - 0.5 on every axis, 0 elsewhere; per axis b = floor(p),
t = p - b and taps k = -R + 1 ... R; acc += ((wz wy) wx) v for kz, ky, kx ascending in float64.  The pre-filter is the 1-D recursion (gain 6,
pole sqrt(3) - 2, causal start summed exactly over the whole line) along z, then y, then x.

What pins what.  ``bspline``: scipy -- the coefficients are ``spline_filter(order=3, mode='mirror')`` and the values
``map_coordinates(order=3, mode='mirror')`` under the inside rule, both within 1e-12 of the restatement.  ``lanczos`` and ``cosine``: their
closed form only (SimpleITK is not installed) -- the fixture's values are this restatement's, stored so that the GPU
test has one yardstick, and the tests here check the properties the closed form implies: a position on a sample returns the sample,
the weights of an axis sum to 1 within the window's ripple, the clamped border.
tests/test_gpu_reslice_taps.py holds the device to the fixture within 1e-6 (fp32 results on [0, 1] data, the bound of the sibling kernels)."""
import ctypes
import os

import numpy as np
import pytest

import abi_util as au

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reslice_taps.npz")
Q = 1024.0                  # the fixture's volumes are uint16 counts of 1/1024 (exact in fp32)
TOL = 1e-6                  # fp32 results on [0, 1] data: the bound of tests/test_reslice_golden.py and tests/test_gpu_z_expand.py
TOL_COEF = 1e-12            # fp64 coefficients
BAR = 1e-12                 # restatement against scipy, both float64
# name -> (frames, source [z, y, x], output [z, y, x], oblique: between 10 % and 60 % of the output voxels are outside)
CASES = {"oblique": (1, (5, 9, 11), (2, 7, 13), True), "oneslice": (1, (1, 3, 2), (2, 4, 5), True), "halfvoxel": (1, (2, 2, 2), (3, 3, 3), False),
         "frames": (3, (7, 12, 10), (3, 9, 66), True), "identity": (1, (4, 6, 7), (4, 6, 7), False), "flip": (1, (4, 6, 7), (7, 6, 4), False),
         "samegrid": (1, (4, 6, 7), (4, 6, 7), False), "halfgrid": (1, (4, 6, 7), (7, 11, 13), False)}
# the last two: an oblique geometry onto its own grid, and onto a grid of half the spacing with the same origin, their matrices composed as
# ``inv(T R S) @ (T R S)`` in float64: the identity (a scale of 1/2) with rounding noise, so positions whose exact value is a whole number
# come out some 1e-14 off it on either side, and as -1e-17 where it is 0 -- there p - floor(p) rounds to exactly 1.0
NOISY = ("samegrid", "halfgrid")
SINCS = (("lanczos", 3), ("lanczos", 5), ("cosine", 5))          # what the fixture stores, as "<kernel><radius>"
_CACHE = {}


def fixture():
    if "rec" not in _CACHE:
        _CACHE["rec"] = dict(np.load(GOLDEN))
    return _CACHE["rec"]


def case(name):
    """dict: vol float32 [N, Z, Y, X], matrix float64 [3, 4], out_shape, coef float64 [N, Z, Y, X] (scipy), bspline float64 [N, Zo, Yo, Xo]
    (scipy under the inside rule), lanczos3 / lanczos5 / cosine5 float64 [N, Zo, Yo, Xo]"""
    rec = fixture()
    c = {k: rec["%s/%s" % (name, k)] for k in ("matrix", "coef", "bspline") + tuple("%s%d" % s for s in SINCS)}
    c["vol"] = (rec["%s/vol" % name] / Q).astype(np.float32)
    c["out_shape"] = CASES[name][2]
    return c


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def positions(M, out_shape):
    """float64 [z, y, x, 3] = (x, y, z): ((m0 * xo + m1 * yo) + m2 * zo) + m3 per row of M, the operation order of the kernels"""
    zo, yo, xo = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in out_shape], indexing="ij")
    return np.stack([((M[a, 0] * xo + M[a, 1] * yo) + M[a, 2] * zo) + M[a, 3] for a in range(3)], axis=-1)


def inside(c, src_shape):
    """bool [...]: ITK's buffer rule on all three axes (false for a position that is not finite)"""
    size = np.array(src_shape[::-1], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ((c >= -0.5) & (c < size - 0.5)).all(axis=-1)


def mirror(i, n):
    """whole-sample mirror of period 2 n - 2; a line of one sample: index 0"""
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def axis_taps(p, n, kernel, radius):
    """p float64 [...] inside [-0.5, n - 0.5) -> (weights float64 [T, ...], indices int64 [T, ...]) of taps k = -R + 1 ... R"""
    b = np.floor(p)
    t = p - b
    ib = b.astype(np.int64)
    if kernel == "bspline":
        u = 1.0 - t
        w0 = u * u * u / 6.0
        w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
        w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
        return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2]), np.stack([mirror(ib + k, n) for k in (-1, 0, 1, 2)])
    R = int(radius)
    ws, idx = [], []
    for k in range(-R + 1, R + 1):
        with np.errstate(invalid="ignore", divide="ignore"):
            d = t - float(k)
            sinc = np.sin(np.pi * d) / (np.pi * d)
            window = np.sin(np.pi * (d / R)) / (np.pi * (d / R)) if kernel == "lanczos" else np.cos(np.pi * d / (2.0 * R))
        # on a sample: exactly that sample.  t == 1.0 (p - floor(p) rounds to it for p in (-2^-54, 0)) is the sample b + 1.  Never normalised
        ws.append(np.where(t == 0.0, 1.0 if k == 0 else 0.0, np.where(t == 1.0, 1.0 if k == 1 else 0.0, sinc * window)))
        idx.append(np.clip(ib + k, 0, n - 1))
    return np.stack(ws), np.stack(idx)


def gather(src64, c, kernel, radius=5):
    """src64 float64 [Z, Y, X] (samples, or coefficients for bspline), c float64 [..., 3] -> float64 [...]: the sum before its one rounding"""
    Z, Y, X = src64.shape
    ok = inside(c, src64.shape)
    safe = np.where(ok[..., None], c, 0.0)
    (wx, ix), (wy, iy), (wz, iz) = (axis_taps(safe[..., a], n, kernel, radius) for a, n in ((0, X), (1, Y), (2, Z)))
    acc = np.zeros(c.shape[:-1])
    for kz in range(len(wz)):
        for ky in range(len(wy)):
            for kx in range(len(wx)):
                acc = acc + ((wz[kz] * wy[ky]) * wx[kx]) * src64[iz[kz], iy[ky], ix[kx]]
    return np.where(ok, acc, 0.0)


def prefilter_line(x):
    """the 1-D filter along the LAST axis of float64 [..., L]"""
    L = x.shape[-1]
    if L == 1:
        return x.copy()
    z1, gain = np.sqrt(3.0) - 2.0, 6.0
    zn1 = z1 ** (L - 1)
    c = np.empty_like(x)
    c0 = x[..., 0] * gain + zn1 * (x[..., L - 1] * gain)
    for i in range(1, L - 1):
        c0 = c0 + z1 ** i * (x[..., i] * gain + zn1 * (x[..., L - 1 - i] * gain))
    c[..., 0] = c0 / (1.0 - zn1 * zn1)
    for i in range(1, L):
        c[..., i] = x[..., i] * gain + z1 * c[..., i - 1]
    c[..., L - 1] = z1 / (z1 * z1 - 1.0) * (z1 * c[..., L - 2] + c[..., L - 1])
    for i in range(L - 2, -1, -1):
        c[..., i] = z1 * (c[..., i + 1] - c[..., i])
    return c


def prefilter_3d(vol):
    """float [..., Z, Y, X] -> float64 coefficients: the line filter along z, then y, then x"""
    c = vol.astype(np.float64)
    for axis in (-3, -2, -1):
        c = np.moveaxis(prefilter_line(np.moveaxis(c, axis, -1)), -1, axis)
    return np.ascontiguousarray(c)


def flipped(vol):
    """what the ``flip`` case's matrix does to [N, Z, Y, X]: output (zo, yo, xo) is source (z, y, x) = (xo, Y - 1 - yo, zo)"""
    return np.flip(np.transpose(vol, (0, 3, 2, 1)), axis=2)


def restated(name, kernel, radius=5):
    """float64 [N, Zo, Yo, Xo] of the restatement on a fixture case; computed once per session and shared, read-only"""
    key = (name, kernel, radius)
    if key not in _CACHE:
        c = case(name)
        pos = positions(c["matrix"], c["out_shape"])
        src = prefilter_3d(c["vol"]) if kernel == "bspline" else c["vol"].astype(np.float64)
        out = np.stack([gather(f, pos, kernel, radius) for f in src])
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


# ---- restatement against the fixture --------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_cases_of_the_issue():
    rec = fixture()
    assert [str(n) for n in rec["names"]] == list(CASES)
    for name, (frames, src_shape, out_shape, oblique) in CASES.items():
        c = case(name)
        assert c["vol"].shape == (frames,) + src_shape and c["matrix"].shape == (3, 4) and c["coef"].shape == c["vol"].shape, name
        assert np.array_equal(c["vol"] * Q, np.round(c["vol"] * Q)) and c["vol"].min() >= 0 and c["vol"].max() <= 1
        for k in ("bspline",) + tuple("%s%d" % s for s in SINCS):
            assert c[k].shape == (frames,) + out_shape and c[k].dtype == np.float64, (name, k)
        out = 1.0 - inside(positions(c["matrix"], out_shape), src_shape).mean()
        assert (0.10 <= out <= 0.60) if oblique else out == 0.0, (name, out)
    # positions below the first sample, in [-0.5, 0): the mirror and the clamp are exercised on the low side
    pos = positions(case("halfvoxel")["matrix"], (3, 3, 3))
    assert (pos < 0).any() and inside(pos, (2, 2, 2)).all()
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("name", list(CASES))
def test_restated_coefficients_are_scipys(name):
    c = case(name)
    got = prefilter_3d(c["vol"])
    worst = float(np.abs(got - c["coef"]).max())
    print("%s: worst |restated coefficient - spline_filter| = %.3g, bar %.3g" % (name, worst, BAR))
    assert worst <= BAR


@pytest.mark.parametrize("name", list(CASES))
def test_restated_bspline_is_map_coordinates_under_the_inside_rule(name):
    c = case(name)
    got = restated(name, "bspline")
    worst = float(np.abs(got - c["bspline"]).max())
    ok = inside(positions(c["matrix"], c["out_shape"]), CASES[name][1])
    print("%s: worst |restatement - map_coordinates| = %.3g, bar %.3g; %.1f %% of the voxels outside" % (name, worst, BAR, 100 * (1 - ok.mean())))
    assert worst <= BAR
    assert not got[:, ~ok].any() and not c["bspline"][:, ~ok].any()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kernel,radius", SINCS)
def test_restated_sincs_are_the_fixtures(name, kernel, radius):
    c = case(name)
    got = restated(name, kernel, radius)
    worst = float(np.abs(got - c["%s%d" % (kernel, radius)]).max())
    print("%s %s r=%d: worst |restatement - fixture| = %.3g, bar %.3g" % (name, kernel, radius, worst, BAR))
    assert worst <= BAR and np.isfinite(got).all()


def test_sinc_properties_of_the_closed_form():
    # a position on a sample: exactly that sample, so identity and the integer flip reproduce the input bit for bit
    for kernel, radius in SINCS:
        assert np.array_equal(restated("identity", kernel, radius).astype(np.float32), case("identity")["vol"]), (kernel, radius)
        assert np.array_equal(restated("flip", kernel, radius).astype(np.float32), flipped(case("flip")["vol"])), (kernel, radius)
    t = np.linspace(0.0, 1.0, 257)[:-1]
    for kernel in ("lanczos", "cosine"):
        for radius in (3, 4, 5):
            w, idx = axis_taps(t + 20.0, 64, kernel, radius)
            assert w.shape == (2 * radius, 256) and np.array_equal(idx[:, 0], 20 + np.arange(-radius + 1, radius + 1))
            assert np.array_equal(w[:, 0], (np.arange(-radius + 1, radius + 1) == 0).astype(np.float64))
            ripple = float(np.abs(w.sum(axis=0) - 1.0).max())          # not normalised: the sum leaves 1 by the window's ripple
            print("%s r=%d: largest |sum of weights - 1| = %.3g" % (kernel, radius, ripple))
            assert 0.0 < ripple < 0.02
            # symmetric: the weights at 1 - t are those at t in reverse
            w2, _ = axis_taps(20.0 + (1.0 - t[1:]), 64, kernel, radius)
            assert np.abs(w2[::-1] - w[:, 1:]).max() < 1e-14
    # the two windows, written out at one point
    w, _ = axis_taps(np.array([7.25]), 32, "lanczos", 3)
    d = 0.25 - np.arange(-2, 4)
    assert np.abs(w[:, 0] - np.sinc(d) * np.sinc(d / 3)).max() < 1e-15
    w, _ = axis_taps(np.array([7.25]), 32, "cosine", 4)
    d = 0.25 - np.arange(-3, 5)
    assert np.abs(w[:, 0] - np.sinc(d) * np.cos(np.pi * d / 8)).max() < 1e-15
    # the border: indices clamp for the sincs, mirror for the B-spline, down to a position of -0.5 and a line of one sample
    assert axis_taps(np.array([-0.5]), 4, "cosine", 3)[1][:, 0].tolist() == [0, 0, 0, 0, 1, 2]
    assert axis_taps(np.array([3.25]), 4, "lanczos", 3)[1][:, 0].tolist() == [1, 2, 3, 3, 3, 3]
    assert axis_taps(np.array([-0.5]), 4, "bspline", 5)[1][:, 0].tolist() == [2, 1, 0, 1]
    assert axis_taps(np.array([3.25]), 4, "bspline", 5)[1][:, 0].tolist() == [2, 3, 2, 1]
    assert axis_taps(np.array([0.25]), 1, "bspline", 5)[1][:, 0].tolist() == [0, 0, 0, 0]
    # not finite, and just outside on either side: 0
    c = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -0.5000001], [10.5, 0, 0], [-0.5, 8.4999, 4.4999]])
    assert inside(c, (5, 9, 11)).tolist() == [False, False, False, False, True]


def noisy_expectation(name):
    """float32 [1, Zo, Yo, Xo] and bool mask: the samples a NOISY case must return (every voxel of ``samegrid``, every second one per axis of
    ``halfgrid``), the positions being whole numbers up to the rounding noise of the composed matrix"""
    vol = case(name)["vol"]
    if name == "samegrid":
        return vol, np.ones(vol.shape, bool)
    want = np.zeros((1,) + CASES[name][2], np.float32)
    mask = np.zeros(want.shape, bool)
    want[:, ::2, ::2, ::2], mask[:, ::2, ::2, ::2] = vol, True
    return want, mask


@pytest.mark.parametrize("name", NOISY)
def test_a_position_that_rounds_onto_the_next_sample_is_that_sample(name):
    """A composed affine leaves -1e-17 where the exact position is 0: b = -1 and t = p - b rounds to exactly 1.0, where sinc(t - 1) is 0 / 0.
    The contract makes it the sample b + 1; every interpolator returns finite values that equal the samples within TOL."""
    c = case(name)
    pos = positions(c["matrix"], c["out_shape"])
    t = pos - np.floor(pos)
    assert inside(pos, CASES[name][1]).all() and np.abs(pos - np.round(pos * 2) / 2).max() < 1e-12
    assert int((t == 1.0).sum()) >= 3 and (pos[t == 1.0] < 0).all() and (pos[t == 1.0] > -2.0 ** -54).all()
    assert ((t > 0.999) & (t < 1.0)).any()          # and the noise just below a sample that does not round onto it
    want, mask = noisy_expectation(name)
    for kernel, radius in (("bspline", 5),) + tuple((k, r) for k in ("lanczos", "cosine") for r in (3, 4, 5)):
        got = restated(name, kernel, radius)
        assert np.isfinite(got).all(), (name, kernel, radius)
        worst = float(np.abs(got - want)[mask].max())
        print("%s %s r=%d: worst |restatement - sample| = %.3g" % (name, kernel, radius, worst))
        assert worst <= TOL, (name, kernel, radius, worst)


# ---- the radius limits ---------------------------------------------------------------------------------------------------------------
def test_the_radius_limits_are_3_and_5():
    from superresolution_aniso_mri_amd import _hip
    assert (_hip.TAPS_MIN_RADIUS, _hip.TAPS_MAX_RADIUS) == (3, 5)          # tests/test_abi.py holds them to the header's #defines


# ---- refusals decided on the host -----------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the device pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    P = ctypes.c_void_p
    src, coef, out = P(1 << 20), P(1 << 22), P(1 << 24)
    m = np.ascontiguousarray(np.eye(4)[:3], np.float64)
    DA = lambda a: a.ctypes.data_as(_hip.DP)          # noqa: E731
    err = _hip.last_error
    names = ["src", "coef", "out", "N", "Zs", "Hs", "Ws", "Zo", "Ho", "Wo", "m_host", "kernel", "radius", "clamp01", "stream"]
    sinc_ok = [src, None, out, 2, 5, 9, 11, 2, 7, 13, DA(m), _hip.TAPS_COSINE, 5, 0, None]
    spline_ok = [None, coef, out, 2, 5, 9, 11, 2, 7, 13, DA(m), _hip.TAPS_BSPLINE3, 5, 1, None]

    def taps(ok, **over):
        args = list(ok)
        for k, v in over.items():
            args[names.index(k)] = v
        return _hip.lib.aesr_reslice_taps_affine(*args)

    fn = "aesr_reslice_taps_affine"
    for ok, source in ((sinc_ok, "src"), (spline_ok, "coef")):
        assert taps(ok, out=None) == 1 and "out is a null" in err() and fn in err()
        assert taps(ok, m_host=None) == 1 and "m_host is a null" in err()
        assert taps(ok, src=None, coef=None) == 1 and "exactly one of src and coef" in err() and "neither" in err()
        assert taps(ok, src=src, coef=coef) == 1 and "exactly one of src and coef" in err() and "both" in err()
        assert taps(ok, out=P((1 << 24) + 2)) == 1 and "out is not 4-byte" in err()
        assert taps(ok, N=0) == 1 and "N=0" in err() and taps(ok, N=-3) == 1
        for dim in ("Zs", "Hs", "Ws"):
            assert taps(ok, **{dim: 0}) == 1 and "Zs, Hs, Ws" in err() and taps(ok, **{dim: -4}) == 1
        for dim in ("Zo", "Ho", "Wo"):
            assert taps(ok, **{dim: 0}) == 1 and "Zo, Ho, Wo" in err() and taps(ok, **{dim: -4}) == 1
        for bad in (3, -1, 7):
            assert taps(ok, kernel=bad) == 1 and "kernel=%d" % bad in err()
        for bad in (2, 6, 0, -5):          # validated for the B-spline too, which ignores it
            assert taps(ok, radius=bad) == 1 and "radius=%d" % bad in err()
        for bad in (2, -1):
            assert taps(ok, clamp01=bad) == 1 and "clamp01=%d" % bad in err()
        for i, bad in ((0, np.nan), (7, np.inf), (11, -np.inf)):
            mm = m.copy()
            mm.reshape(-1)[i] = bad
            assert taps(ok, m_host=DA(mm)) == 1 and "m_host[%d]" % i in err()
        assert taps(ok, N=2, Zs=1024, Hs=1024, Ws=1024) == 1 and "2^31" in err() and "Zs" in err()
        assert taps(ok, N=2, Zo=1024, Ho=1024, Wo=1024) == 1 and "2^31" in err() and "Zo" in err()
        assert taps(ok, N=30, Zs=2048, Hs=2048, Ws=2048) == 1 and "2^31" in err()
        # out inside the source, the source inside out, out starting at the source's last element
        base, esize = (1 << 20, 4) if source == "src" else (1 << 22, 8)
        for at in (base + 4 * 100, base - 4 * 100, base + esize * (2 * 5 * 9 * 11) - 4):
            assert taps(ok, out=P(at)) == 3 and "out overlaps %s" % source in err()
    # the wrong source for the kernel
    assert taps(sinc_ok, kernel=_hip.TAPS_BSPLINE3) == 1 and "coef, not src" in err()
    assert taps(spline_ok, kernel=_hip.TAPS_LANCZOS) == 1 and "src, not coef" in err()
    assert taps(sinc_ok, src=P((1 << 20) + 2)) == 1 and "src is not 4-byte" in err()
    assert taps(spline_ok, coef=P((1 << 22) + 4)) == 1 and "coef is not 8-byte" in err()

    pnames = ["in", "coef", "N", "Z", "H", "W", "stream"]

    def prefilter(**over):
        args = [src, coef, 2, 5, 9, 11, None]
        for k, v in over.items():
            args[pnames.index(k)] = v
        return _hip.lib.aesr_bspline_prefilter_3d(*args)

    fn = "aesr_bspline_prefilter_3d"
    assert prefilter(**{"in": None}) == 1 and "in is a null" in err() and fn in err()
    assert prefilter(coef=None) == 1 and "coef is a null" in err()
    assert prefilter(**{"in": P((1 << 20) + 1)}) == 1 and "in is not 4-byte" in err()
    assert prefilter(coef=P((1 << 22) + 4)) == 1 and "coef is not 8-byte" in err()
    for dim in ("N", "Z", "H", "W"):
        assert prefilter(**{dim: 0}) == 1 and "N, Z, H, W" in err() and prefilter(**{dim: -2}) == 1
    assert prefilter(N=2, Z=1024, H=1024, W=1024) == 1 and "2^31" in err() and fn in err()
    assert prefilter(coef=P((1 << 20) + 8)) == 3 and "coef overlaps in" in err()
    assert prefilter(coef=P((1 << 20) - 8 * 2 * 5 * 9 * 11 + 8)) == 3 and "coef overlaps in" in err()
    # aesr_reslice_affine does not know the new kernels: its interp stays 0 or 1
    assert _hip.lib.aesr_reslice_affine(src, out, 2, 5, 9, 11, 2, 7, 13, DA(m), 2, None) == 1 and "interp=2" in err()


# ---- the Python interface -------------------------------------------------------------------------------------------------------------
def test_python_interface(capsys):
    import torch
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    from superresolution_aniso_mri_amd.evaluate.cardiac import resample_sax_to_lax as rs
    assert rl.AFFINE_INTERPS == ("linear", "nearest", "bspline", "cosine", "lanczos") and rl.RADII == (3, 4, 5)
    assert sorted(rl.INTERPS) == ["linear", "nearest"]
    g = rl.Geometry((1.0, 1.0, 1.0))
    vol = np.zeros((3, 4, 5), np.float32)
    for interp in ("bspline", "lanczos", "cosine"):
        for bad in (2, 6, 0, 3.5, "5", None, True):
            with pytest.raises(ValueError, match="radius"):
                rl.reslice_affine(vol, np.eye(4), (3, 4, 5), interp, radius=bad)
        with pytest.raises(ValueError, match="ref_shape"):
            rl.reslice(vol, g, g, (4, 5), interp=interp)
        with pytest.raises(ValueError, match="matrix"):
            rl.reslice_affine(vol, np.full((3, 4), np.nan), (3, 4, 5), interp)
        with pytest.raises(RuntimeError, match="GPU"):
            rl.reslice(torch.zeros(3, 4, 5), g, g, (3, 4, 5), interp=interp, radius=3)                  # a CPU tensor: no fallback
        with pytest.raises(ValueError, match="interp"):
            rl.reslice_grid(vol, np.zeros((2, 2, 2, 3), np.float32), interp)
        with pytest.raises(ValueError, match="interp"):
            rl.reslice_grid(torch.zeros(3, 4, 5), torch.zeros(2, 2, 2, 3), interp=interp)
        if not torch.cuda.is_available():          # accepted up to the point where the device is needed
            for call in (lambda: rl.reslice_affine(vol, np.eye(4), (3, 4, 5), interp, radius=4, clamp01=True),
                         lambda: rl.reslice(vol, g, g, (3, 4, 5), interp=interp), lambda: rl.reslice(vol[None], g, g, (3, 4, 5), interp, radius=3)):
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    call()
    for interp in ("linear", "nearest"):          # radius is validated there too; clamp01 is accepted and ignored
        with pytest.raises(ValueError, match="radius"):
            rl.reslice_affine(vol, np.eye(4), (3, 4, 5), interp, radius=7)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                rl.reslice_affine(vol, np.eye(4), (3, 4, 5), interp, radius=3, clamp01=True)
    with pytest.raises(ValueError, match="interp"):
        rl.reslice_affine(vol, np.eye(4), (3, 4, 5), "cubic")
    with pytest.raises(ValueError, match="interp"):
        rl.reslice_affine(vol, np.eye(4), (3, 4, 5), "sinc", radius=3)
    # the command line
    base = ["--sax", "s.nii", "--lax", "l.nii", "--out", "o.nii"]
    a = rs.parse_args(base)
    assert (a.interp, a.radius, a.clamp01) == ("linear", 5, False)
    for interp in ("bspline", "lanczos", "cosine"):
        a = rs.parse_args(base + ["--interp", interp, "--radius", "3", "--clamp01"])
        assert (a.interp, a.radius, a.clamp01) == (interp, 3, True)
        assert rs.parse_args(base + ["--interp", interp]).radius == 5
    for bad in (["--interp", "cubic"], ["--interp", "cosine", "--radius", "6"], ["--interp", "lanczos", "--radius", "2"], ["--radius", "x"],
                ["--interp", "sinc"]):
        with pytest.raises(SystemExit):
            rs.parse_args(base + bad)
    a = rs.parse_args(base + ["--clamp01", "--radius", "4"])          # accepted with the default linear, which ignores both
    assert (a.interp, a.radius, a.clamp01) == ("linear", 4, True)
    capsys.readouterr()
