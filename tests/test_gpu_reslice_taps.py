"""-m gpu: affine reslicing with a cubic B-spline or a windowed sinc on the device -- aesr_bspline_prefilter_3d and aesr_reslice_taps_affine
(csrc/reslice_taps.hip, csrc/bspline_prefilter.hip, include/aesr_hip_reslice_taps.h), ``evaluate.reslice`` and the command line of ``evaluate.cardiac.resample_sax_to_lax``.

- Every case of tests/golden/reslice_taps.npz and every kernel against the fixture (scipy for ``bspline``, the closed form for the sincs) and
  against the float64 restatement of tests/test_reslice_taps_golden.py: 1e-6 absolute, the bound of the sibling kernels for fp32 results on
  [0, 1] data; the coefficients within 1e-12.  Each test prints the error it measured.
- Exact: the identity and the integer flip with a sinc reproduce the input; N frames equal their single-frame calls; ``clamp01`` equals
  ``torch.clamp`` (with voxels that it changes); a device tensor in gives a device tensor out and the input is unchanged.
- Cross-checks: ``diag(1, 1, 1 / f)`` with a sinc against ``z_expand(align="grid", method="lanczos")``; ``bspline`` at the identity.
- The pre-filter at line lengths around the staged block (32 columns), the workgroup's rows (64) and one, against ``spline_filter1d`` thrice;
  its y pass bit for bit against ``aesr_bspline_prefilter_z`` on the same lines (one recursion, csrc/bspline_prefilter.h).
- Both launch entry points between the guard bands of tests/memguard.py: NaN and 3e38 poisons, pointers shifted by 4, 8 and 12 bytes
  (``coef`` by 8), output widths 47, 48, 131, 132; refusals write nothing.
- The command line on small NIfTI files."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

import memguard as mg
import test_reslice_taps_golden as tt

pytestmark = pytest.mark.gpu
# GUARDED_ENTRIES and EXEMPT partition ``_hip.SIGNATURES_RESLICE_TAPS`` (tests/test_abi.py checks that without a GPU)
GUARDED_ENTRIES = ("aesr_reslice_taps_affine", "aesr_bspline_prefilter_3d")
EXEMPT = {}

TOL, TOL_COEF = tt.TOL, tt.TOL_COEF
KERNELS = (("bspline", 5),) + tt.SINCS          # (interp, radius): what the fixture stores
ALL_SINCS = tuple((k, r) for k in ("lanczos", "cosine") for r in (3, 4, 5))


def fixture_key(interp, radius):
    return "bspline" if interp == "bspline" else "%s%d" % (interp, radius)


def frames_volume():
    return tt.case("frames")["vol"]          # [3, 7, 12, 10]


def scipy_coefficients(vol):
    """float [N, Z, Y, X] -> float64: ``spline_filter1d(order=3, mode='mirror')`` along z, then y, then x"""
    c = vol.astype(np.float64)
    for axis in (1, 2, 3):
        c = ndimage.spline_filter1d(c, order=3, axis=axis, mode="mirror", output=np.float64)
    return c


# ---- accuracy -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tt.CASES))
def test_every_kernel_vs_fixture_and_restatement(name):
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    c = tt.case(name)
    x = torch.from_numpy(c["vol"]).cuda()
    saved = mg.bits(x)
    coef = rl.bspline_coefficients_3d(x)
    assert coef.is_cuda and coef.dtype == torch.float64 and tuple(coef.shape) == c["vol"].shape
    err = float(np.abs(coef.cpu().numpy() - c["coef"]).max())
    print("%-10s coefficients: max |kernel - spline_filter| = %.3g (bound %.3g)" % (name, err, TOL_COEF))
    assert err <= TOL_COEF, (name, err)
    for interp, radius in KERNELS:
        got = rl.reslice_affine(x, c["matrix"], c["out_shape"], interp, radius=radius)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == c[fixture_key(interp, radius)].shape and got.data_ptr() != x.data_ptr()
        g = got.cpu().numpy()
        e_fix = float(np.abs(g.astype(np.float64) - c[fixture_key(interp, radius)]).max())
        want = tt.restated(name, interp, radius)
        e_res = float(np.abs(g.astype(np.float64) - want).max())
        same = float((g.view(np.int32) == want.astype(np.float32).view(np.int32)).mean())
        print("%-10s %-8s r=%d: max |kernel - fixture| = %.3g, max |kernel - restatement| = %.3g (bit-equal to its fp32 rounding: %.4f)"
              % (name, interp, radius, e_fix, e_res, same))
        assert e_fix <= TOL and e_res <= TOL, (name, interp, radius, e_fix, e_res)
        ok = tt.inside(tt.positions(c["matrix"], c["out_shape"]), tt.CASES[name][1])
        assert not g[:, ~ok].any() and g[:, ok].any()
        # numpy in -> numpy out, the same bits; a 3-D input gives a 3-D result
        host = rl.reslice_affine(c["vol"], c["matrix"], c["out_shape"], interp, radius=radius)
        assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host.view(np.int32), g.view(np.int32))
        one = rl.reslice_affine(x[0], c["matrix"], c["out_shape"], interp, radius=radius)
        assert one.dim() == 3 and torch.equal(one.view(torch.int32), got[0].view(torch.int32))
    mg.assert_unchanged(x, saved, "src")


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------------
def test_identity_and_integer_flip_with_a_sinc_are_exact():
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    ident, flip = tt.case("identity"), tt.case("flip")
    xi, xf = torch.from_numpy(ident["vol"]).cuda(), torch.from_numpy(flip["vol"]).cuda()
    for interp, radius in ALL_SINCS:
        same = rl.reslice_affine(xi, ident["matrix"], ident["out_shape"], interp, radius=radius)
        assert torch.equal(same.view(torch.int32), xi.view(torch.int32)), (interp, radius)
        turned = rl.reslice_affine(xf, flip["matrix"], flip["out_shape"], interp, radius=radius).cpu().numpy()
        assert np.array_equal(turned, tt.flipped(flip["vol"])), (interp, radius)
    # the B-spline goes through its coefficients: the input within the bound, not bit for bit
    back = rl.reslice_affine(xi, ident["matrix"], ident["out_shape"], "bspline")
    err = float((back - xi).abs().max())
    print("bspline at the identity: max |result - input| = %.3g" % err)
    assert err <= TOL


@pytest.mark.parametrize("name", tt.NOISY)
def test_a_position_that_rounds_onto_the_next_sample_is_that_sample(name):
    """An oblique geometry onto its own grid (and onto one of half the spacing), the matrix composed in float64: positions are whole numbers
    up to rounding noise, some of them -1e-17, where p - floor(p) rounds to 1.0 and sinc(t - 1) is 0 / 0.  Finite, and the samples within TOL."""
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    c = tt.case(name)
    x = torch.from_numpy(c["vol"]).cuda()
    want, mask = tt.noisy_expectation(name)
    for interp, radius in (("bspline", 5),) + ALL_SINCS:
        for clamp01 in (False, True):
            got = rl.reslice_affine(x, c["matrix"], c["out_shape"], interp, radius=radius, clamp01=clamp01).cpu().numpy()
            assert np.isfinite(got).all(), (name, interp, radius, clamp01, int((~np.isfinite(got)).sum()))
            err = float(np.abs(got.astype(np.float64) - want)[mask].max())
            assert err <= TOL, (name, interp, radius, clamp01, err)
        print("%s %s r=%d: max |kernel - sample| = %.3g" % (name, interp, radius, err))
    # linear and nearest ignore clamp01 and radius
    for interp in ("linear", "nearest"):
        assert torch.equal(rl.reslice_affine(x, c["matrix"], c["out_shape"], interp, radius=3, clamp01=True), rl.reslice_affine(x, c["matrix"], c["out_shape"], interp))


def test_frames_equal_their_single_frame_calls_bitwise():
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    c = tt.case("frames")
    x = torch.from_numpy(c["vol"]).cuda()
    for interp, radius in KERNELS + (("cosine", 3), ("lanczos", 4)):
        whole = rl.reslice_affine(x, c["matrix"], c["out_shape"], interp, radius=radius)
        assert tuple(whole.shape) == (3,) + c["out_shape"]
        for n in range(3):
            one = rl.reslice_affine(x[n].contiguous(), c["matrix"], c["out_shape"], interp, radius=radius)
            assert torch.equal(whole[n].view(torch.int32), one.view(torch.int32)), (interp, radius, n)
        assert not torch.equal(whole[0], whole[1])


def test_clamp01_equals_torch_clamp_bitwise():
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    c = tt.case("frames")
    x = torch.from_numpy(c["vol"]).cuda()
    for interp, radius in KERNELS:
        raw = rl.reslice_affine(x, c["matrix"], c["out_shape"], interp, radius=radius)
        cl = rl.reslice_affine(x, c["matrix"], c["out_shape"], interp, radius=radius, clamp01=True)
        changed = int((raw != cl).sum())
        print("%-8s r=%d: clamp01 changes %d of %d voxels (range of the raw result %.4f ... %.4f)" % (interp, radius, changed, raw.numel(), float(raw.min()),
                                                                                                 float(raw.max())))
        assert torch.equal(cl.view(torch.int32), torch.clamp(raw, 0.0, 1.0).view(torch.int32)), (interp, radius)
        assert changed >= 1 and float(raw.min()) < 0.0 and float(raw.max()) > 1.0, (interp, radius)


# ---- cross-checks ---------------------------------------------------------------------------------------------------------------------
def test_a_z_scale_with_a_sinc_agrees_with_z_expand():
    from superresolution_aniso_mri_amd.evaluate import reslice as rl, z_interp
    x = torch.from_numpy(tt.case("identity")["vol"]).cuda()          # [1, 4, 6, 7]
    for f in (2, 3):
        for radius in (3, 5):
            want = z_interp.z_expand(x, f, "lanczos", align="grid", radius=radius)
            Zo = int(want.shape[1])
            assert Zo == 3 * f + 1
            got = rl.reslice_affine(x, np.diag([1.0, 1.0, 1.0 / f, 1.0]), (Zo, 6, 7), "lanczos", radius=radius)
            err = float((got - want).abs().max())
            print("f=%d r=%d: max |reslice - z_expand| = %.3g" % (f, radius, err))
            assert err <= TOL, (f, radius, err)
            if f == 2:          # 0.5 * zo is exact: every second output slice is an input slice, bit for bit
                assert torch.equal(got[:, ::2].view(torch.int32), x.view(torch.int32))


# ---- the pre-filter -------------------------------------------------------------------------------------------------------------------
PREFILTER_SHAPES = ([(2, 2, 3, W) for W in (1, 2, 3, 31, 32, 33, 64, 65, 130)] + [(2, 3, H, 2) for H in (1, 2, 5, 67)] + [(2, Z, 2, 3) for Z in (1, 2, 5)]
                    + [(1, 3, 30, 70), (1, 1, 1, 1)])          # the last but one: two workgroups of rows, three staged blocks per row


@pytest.mark.parametrize("shape", PREFILTER_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_prefilter_shapes_vs_spline_filter1d_thrice(shape):
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    vol = (np.random.RandomState(sum(shape)).randint(0, 1025, size=shape) / tt.Q).astype(np.float32)
    x = torch.from_numpy(vol).cuda()
    saved = mg.bits(x)
    got = rl.bspline_coefficients_3d(x).cpu().numpy()
    want = scipy_coefficients(vol)
    err = float(np.abs(got - want).max())
    print("%s: max |kernel - spline_filter1d x 3| = %.3g (bound %.3g)" % (shape, err, TOL_COEF))
    assert got.shape == want.shape and err <= TOL_COEF, (shape, err)
    mg.assert_unchanged(x, saved, "in")


@pytest.mark.parametrize("H", (2, 3, 5, 67))
def test_the_y_pass_is_the_z_recursion_bit_for_bit(H):
    """On [N, 1, H, 1] only the y pass of aesr_bspline_prefilter_3d acts (z copies, x is skipped): its coefficients equal those of
    aesr_bspline_prefilter_z on the same data seen as [N, H, 1, 1], in every bit."""
    from superresolution_aniso_mri_amd import _hip as hip
    N = 2
    x = torch.from_numpy((np.random.RandomState(100 + H).randint(0, 1025, size=(N, H)) / tt.Q).astype(np.float32)).cuda()
    got, want = torch.full((N, H), float("nan"), dtype=torch.float64, device="cuda"), torch.full((N, H), float("nan"), dtype=torch.float64, device="cuda")
    hip.check(hip.lib.aesr_bspline_prefilter_3d(hip.ptr(x), hip.ptr(got), N, 1, H, 1, hip.stream()), "aesr_bspline_prefilter_3d")
    hip.check(hip.lib.aesr_bspline_prefilter_z(hip.ptr(x), hip.ptr(want), N, H, 1, 1, hip.stream()), "aesr_bspline_prefilter_z")
    torch.cuda.synchronize()
    assert not torch.isnan(want).any() and torch.equal(got.view(torch.int64), want.view(torch.int64)), H


# ---- the launch entry points between guard bands --------------------------------------------------------------------------------------
def _taps_call(x4, M, out_shape, interp, radius, poison, s_src, s_out, over=None):
    """x4 float32 [N, Z, H, W] (samples; for bspline the coefficients are made first, by the library); ``over``: arguments to replace.
    Returns (rc, guarded out, out)."""
    over = dict(over or {})
    from superresolution_aniso_mri_amd import _hip as hip
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    N, Zs, Hs, Ws = x4.shape
    Zo, Ho, Wo = out_shape
    m = np.ascontiguousarray(np.asarray(M, np.float64)[:3, :4])
    kept = m.copy()
    if interp == "bspline":
        coef = rl.bspline_coefficients_3d(torch.from_numpy(x4).cuda())
        gsrc = mg.guarded(x4.size, torch.float64, "cuda", coef.reshape(-1), s_src, "coef")
        assert gsrc.view.data_ptr() % 16 == 8 * s_src
    else:
        gsrc = mg.guarded(x4.size, torch.float32, "cuda", torch.from_numpy(x4).reshape(-1), s_src, "src")
        assert gsrc.view.data_ptr() % 16 == 4 * s_src
    gout = mg.guarded(N * Zo * Ho * Wo, torch.float32, "cuda", poison, s_out, "out")
    assert gout.view.data_ptr() % 16 == 4 * s_out
    saved = mg.bits(gsrc.view)
    args = dict(src=None if interp == "bspline" else hip.ptr(gsrc.view), coef=hip.ptr(gsrc.view) if interp == "bspline" else None, out=hip.ptr(gout.view),
                N=N, Zs=Zs, Hs=Hs, Ws=Ws, Zo=Zo, Ho=Ho, Wo=Wo, m_host=m.ctypes.data_as(hip.DP), kernel=rl.TAP_KERNELS[interp], radius=radius,
                clamp01=0, stream=hip.stream())
    if over.pop("out_in_source", False):
        args["out"] = ctypes.c_void_p(gsrc.view.data_ptr() + gsrc.view.element_size() * x4.size - 4)
    args.update(over)
    torch.cuda.synchronize()
    rc = hip.lib.aesr_reslice_taps_affine(*args.values())
    torch.cuda.synchronize()
    assert np.array_equal(m, kept)
    mg.assert_guards_intact([gsrc, gout])
    mg.assert_unchanged(gsrc.view, saved, gsrc.name)
    return rc, gout, gout.view.reshape(N, Zo, Ho, Wo)


# (poison, shift of the source, shift of out) in elements: 4-byte steps for src and out, 8-byte steps for coef (0 or 1 only)
LEGS = [(mg.POISON_NAN, 0, 0), (mg.POISON_FINITE, 0, 0), (mg.POISON_NAN, 1, 1), (mg.POISON_FINITE, 2, 2), (mg.POISON_NAN, 3, 3), (mg.POISON_FINITE, 1, 0),
        (mg.POISON_NAN, 0, 3)]
GUARD_SHAPES = [(2, 5, 47), (2, 5, 48), (1, 3, 131), (1, 3, 132)]          # Wo % 4 == 0 and not; one tile in x and three; two tiles in y
GUARD_KERNELS = (("bspline", 5), ("lanczos", 5), ("cosine", 3), ("lanczos", 4))


def _guard_matrix(out_shape):
    """the ``frames`` case's matrix with its x step shrunk so that the wider output row still crosses the volume and leaves it"""
    M = tt.case("frames")["matrix"].copy()
    M[:, 0] *= 66.0 / out_shape[2]
    return M


@pytest.mark.parametrize("out_shape", GUARD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("interp,radius", GUARD_KERNELS)
def test_taps_guard_bands_poisons_and_offset_pointers(out_shape, interp, radius):
    """Guards intact, the const source and m_host unchanged, every output element written, results bit-identical across the legs (the
    alignment of the source and of ``out`` changes nothing) and right."""
    x4 = frames_volume()[:2]
    M = _guard_matrix(out_shape)
    pos = tt.positions(M, out_shape)
    ok = tt.inside(pos, x4.shape[1:])
    assert 0.1 <= 1 - ok.mean() <= 0.6
    src64 = tt.prefilter_3d(x4) if interp == "bspline" else x4.astype(np.float64)
    want_np = np.stack([tt.gather(f, pos, interp, radius) for f in src64])
    want = None
    for poison, s_src, s_out in LEGS:
        s_src = s_src % 2 if interp == "bspline" else s_src          # coef moves by 8 bytes or not at all
        rc, gout, out = _taps_call(x4, M, out_shape, interp, radius, poison, s_src, s_out)
        assert rc == 0
        left = mg.poison_left(gout.view, poison)
        assert left.numel() == 0, "%d output element(s) never written, first %d" % (left.numel(), int(left[0]))
        bits = mg.bits(out)
        if want is None:
            want = bits
            got = out.cpu().numpy()
            err = float(np.abs(got.astype(np.float64) - want_np).max())
            print("%s r=%d %s: max |kernel - restatement| = %.3g" % (interp, radius, out_shape, err))
            assert err <= TOL and got.any() and not got[:, ~ok].any()
        else:
            assert torch.equal(bits, want), "%s %s [poison %s, shifts %d, %d]: differs from leg 1" % (interp, out_shape, poison, s_src, s_out)


def _prefilter_call(vol, poison, s_in, s_coef, **over):
    from superresolution_aniso_mri_amd import _hip as hip
    N, Z, H, W = vol.shape
    gin = mg.guarded(vol.size, torch.float32, "cuda", torch.from_numpy(vol).reshape(-1), s_in, "in")
    gcoef = mg.guarded(vol.size, torch.float64, "cuda", poison, s_coef, "coef")
    assert gin.view.data_ptr() % 16 == 4 * s_in and gcoef.view.data_ptr() % 16 == 8 * s_coef
    saved = mg.bits(gin.view)
    args = {"in": hip.ptr(gin.view), "coef": hip.ptr(gcoef.view), "N": N, "Z": Z, "H": H, "W": W, "stream": hip.stream()}
    if over.pop("coef_in_in", False):
        args["coef"] = ctypes.c_void_p(gin.view.data_ptr() + 8)
    args.update(over)
    torch.cuda.synchronize()
    rc = hip.lib.aesr_bspline_prefilter_3d(*args.values())
    torch.cuda.synchronize()
    mg.assert_guards_intact([gin, gcoef])
    mg.assert_unchanged(gin.view, saved, "in")
    return rc, gcoef


@pytest.mark.parametrize("shape", [(2, 3, 5, 33), (1, 2, 3, 131), (2, 2, 66, 3), (1, 1, 1, 1), (1, 4, 1, 1)], ids=lambda s: "x".join(str(v) for v in s))
def test_prefilter_guard_bands_poisons_and_offset_pointers(shape):
    vol = (np.random.RandomState(7 + sum(shape)).randint(0, 1025, size=shape) / tt.Q).astype(np.float32)
    want_np = scipy_coefficients(vol)
    want = None
    for poison, s_in, s_coef in ((mg.POISON_NAN, 0, 0), (mg.POISON_FINITE, 0, 0), (mg.POISON_NAN, 1, 1), (mg.POISON_FINITE, 2, 1), (mg.POISON_NAN, 3, 0)):
        rc, gcoef = _prefilter_call(vol, poison, s_in, s_coef)
        assert rc == 0
        assert mg.poison_left(gcoef.view, poison).numel() == 0
        bits = mg.bits(gcoef.view)
        if want is None:
            want = bits
            err = float(np.abs(gcoef.view.cpu().numpy().reshape(shape) - want_np).max())
            print("%s: max |kernel - spline_filter1d x 3| = %.3g" % (shape, err))
            assert err <= TOL_COEF
        else:
            assert torch.equal(bits, want), "%s [poison %s, shifts %d, %d]: differs from leg 1" % (shape, poison, s_in, s_coef)


def test_refusals_write_nothing():
    from superresolution_aniso_mri_amd import _hip as hip
    x4 = frames_volume()[:2]
    M = tt.case("frames")["matrix"]
    bad_m = np.ascontiguousarray(M.copy())
    bad_m[1, 2] = np.nan
    fn = "aesr_reslice_taps_affine"
    for interp, source in (("cosine", "src"), ("bspline", "coef")):
        other = ctypes.c_void_p(1 << 20)
        cases = ((dict(out=None), 1, "out is a null"), (dict(m_host=None), 1, "m_host is a null"), (dict(src=None, coef=None), 1, "neither"),
                 (dict(**{"coef" if source == "src" else "src": other}), 1, "both"), (dict(N=0), 1, "N=0"), (dict(Hs=0), 1, "Zs, Hs, Ws"),
                 (dict(Wo=-3), 1, "Zo, Ho, Wo"), (dict(kernel=3), 1, "kernel=3"), (dict(radius=6), 1, "radius=6"), (dict(radius=2), 1, "radius=2"),
                 (dict(clamp01=2), 1, "clamp01=2"), (dict(m_host=bad_m.ctypes.data_as(hip.DP)), 1, "m_host[6]"),
                 (dict(kernel=1 if source == "coef" else 0), 1, "not " + source), (dict(out_in_source=True), 3, "out overlaps " + source))
        for over, code, word in cases:
            rc, gout, _ = _taps_call(x4, M, (2, 5, 47), interp, 5, mg.POISON_NAN, 0, 0, over)
            assert rc == code and word in hip.last_error() and fn in hip.last_error(), (interp, sorted(over), rc, hip.last_error())
            assert mg.poison_left(gout.view, mg.POISON_NAN).numel() == gout.view.numel()
        rc, gout, _ = _taps_call(x4, M, (2, 5, 47), interp, 5, mg.POISON_FINITE, 0, 0, {source: ctypes.c_void_p(4097 if source == "src" else 4100)})
        assert rc == 1 and "%s is not %d-byte" % (source, 4 if source == "src" else 8) in hip.last_error()
        assert mg.poison_left(gout.view, mg.POISON_FINITE).numel() == gout.view.numel()
    vol = x4[:1, :2, :3, :5].copy()
    for over, code, word in ((dict(**{"in": None}), 1, "in is a null"), (dict(coef=None), 1, "coef is a null"), (dict(Z=0), 1, "N, Z, H, W"),
                             (dict(W=-1), 1, "N, Z, H, W"), (dict(coef_in_in=True), 3, "coef overlaps in")):
        rc, gcoef = _prefilter_call(vol, mg.POISON_NAN, 0, 0, **over)
        assert rc == code and word in hip.last_error() and "aesr_bspline_prefilter_3d" in hip.last_error(), (sorted(over), rc, hip.last_error())
        assert mg.poison_left(gcoef.view, mg.POISON_NAN).numel() == gcoef.view.numel()


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_command_line_with_each_new_interpolator(tmp_path, capsys):
    from superresolution_aniso_mri_amd import volume_io
    from superresolution_aniso_mri_amd.evaluate import reslice as rl
    from superresolution_aniso_mri_amd.evaluate.cardiac import resample_sax_to_lax as rs
    rng = np.random.RandomState(11)
    sax = volume_io.Volume((rng.randint(0, 1025, size=(2, 5, 9, 11)) / tt.Q).astype(np.float32), (1.4, 1.4, 2.5, 1.0), "npy", {})
    lax = volume_io.Volume(np.zeros((4, 7, 13), np.float32), (1.3, 1.9, 3.3), "npy", {})
    volume_io.write_volume(str(tmp_path / "sax.nii.gz"), sax, sax.array)
    volume_io.write_volume(str(tmp_path / "lax.nii.gz"), lax, lax.array)
    sax_f, lax_f = volume_io.read_volume(tmp_path / "sax.nii.gz"), volume_io.read_volume(tmp_path / "lax.nii.gz")
    assert np.array_equal(sax_f.array, sax.array) and np.allclose(lax_f.spacing[:3], lax.spacing)
    for interp, extra in (("bspline", []), ("lanczos", ["--radius", "3"]), ("cosine", []), ("cosine", ["--radius", "4", "--clamp01"])):
        out = tmp_path / ("out_%s%d.nii.gz" % (interp, len(extra)))
        res = rs.main(["--sax", str(tmp_path / "sax.nii.gz"), "--lax", str(tmp_path / "lax.nii.gz"), "--out", str(out), "--interp", interp] + extra)
        said = capsys.readouterr().out
        assert "2 frame(s)" in said and interp in said
        got = volume_io.read_volume(out)
        radius = int(extra[1]) if "--radius" in extra else 5
        want = rl.reslice_like(sax_f, lax_f, interp=interp, radius=radius, clamp01="--clamp01" in extra)
        assert got.array.shape == (2, 4, 7, 13) and got.array.dtype == np.float32 and np.array_equal(got.array, res)
        assert np.array_equal(got.array.view(np.int32), want.view(np.int32)) and want.any() and not want.all()
        if "--clamp01" in extra:
            assert want.min() == 0.0 and want.max() == 1.0
    # the radius matters, and the default interpolator is still linear
    a, b = (rl.reslice_like(sax_f, lax_f, interp="cosine", radius=r) for r in (3, 5))
    assert not np.array_equal(a, b)
    res = rs.main(["--sax", str(tmp_path / "sax.nii.gz"), "--lax", str(tmp_path / "lax.nii.gz"), "--out", str(tmp_path / "lin.nii.gz")])
    assert np.array_equal(res, rl.reslice_like(sax_f, lax_f, interp="linear"))
