"""-m gpu: the conventional through-plane baselines on the device -- aesr_z_expand and aesr_bspline_prefilter_z (csrc/z_expand.hip,
include/aesr_hip_baselines.h), ``evaluate.z_interp``, ``evaluate.common.create_simple_interpolation``, the ``interpol_filter`` keyword of
``evaluate_interpolation_performance``, ``generate_hr_volumes --method`` and ``evaluate.compare_methods``.

- The kernel against tests/golden/z_expand.npz (scipy) and the restatement of tests/test_z_expand_golden.py on every case, both alignments,
  all methods: within 1e-6 absolute on [0, 1] data, the bound of the sibling kernels.  The operation order and the single rounding are the
  restatement's, so 0 is expected up to the one fp32 rounding (1.2e-7) that per-phase against per-slice coordinates can flip; against
  ``apply_tables`` (the same tables, numpy) the result is expected bit-equal and each case prints the fraction.  Coefficients within 1e-12
  of ``spline_filter1d`` and of the restatement.
- Bitwise: the 4-D launch equals its frames; the 16-byte path equals the 4-byte path; ``clamp01`` equals ``torch.clamp``; device in ->
  device out.
- Both launch entry points between the guard bands of tests/memguard.py at the contractual sizes: NaN and 3e38 poisons, inputs unchanged,
  ``in`` / ``coef`` / ``out`` shifted by 4, 8 and 12 bytes (``coef`` by 8 only: it stays double-aligned); refusals write nothing and name the
  argument.
- The protocol and the tools on small volumes."""
import os
import struct

import numpy as np
import pytest
import torch

import memguard as mg
import test_z_expand_golden as tz

pytestmark = pytest.mark.gpu

TOL = 1e-6
TOL_COEF = 1e-12
GUARDED_ENTRIES = ("aesr_z_expand", "aesr_bspline_prefilter_z")
EXEMPT = {"aesr_z_expand_out_slices": "host query", "aesr_z_expand_store_bytes": "host query", "aesr_bspline_coef_bytes": "host query"}
_RESTATED = {}


def restated(tag, method, align):
    """the restatement's result of a case, computed once per session"""
    key = (tag, method, align)
    if key not in _RESTATED:
        _RESTATED[key] = tz.restate(tz.case_input(tag), tz.CASES[tag][1], method, align)
    return _RESTATED[key]


def _expand(x, f, method, align, **kw):
    from superresolution_aniso_mri_amd.evaluate import z_interp
    name, radius = tz.package_method(method)
    return z_interp.z_expand(x, f, name, align=align, radius=radius, **kw)


@pytest.mark.parametrize("tag", list(tz.CASES))
def test_kernel_vs_fixture_and_restatement(tag):
    from superresolution_aniso_mri_amd.evaluate import z_interp
    fx = tz.fixture()
    shape, f = tz.CASES[tag]
    x = tz.case_input(tag)
    xd = torch.from_numpy(x).cuda()
    saved = mg.bits(xd)
    for align in tz.ALIGNS:
        for method in tz.METHODS:
            dev = _expand(xd, f, method, align)
            assert dev.is_cuda and dev.dtype == torch.float32 and dev.data_ptr() != xd.data_ptr()
            got, want = dev.cpu().numpy(), restated(tag, method, align)
            assert got.shape == want.shape
            err = float(np.abs(got.astype(np.float64) - want).max())
            name, radius = tz.package_method(method)
            base, w, boundary, needs_coef = z_interp.phase_tables(name, f, align, radius)
            src = x
            if needs_coef:
                src = np.stack([tz.restate_coefficients(v) for v in x]) if x.ndim == 4 else tz.restate_coefficients(x)
            model = tz.apply_tables(src, f, want.shape[-3], base, w, boundary)
            err_fx = None
            if (align, method) in tz.stored(tag) and method in tz.SCIPY_METHODS:
                err_fx = float(np.abs(got.astype(np.float64) - fx["%s/%s/%s" % (tag, align, method)]).max())
            print("%-6s %-5s %-9s max |kernel - restatement| = %.3g, |kernel - scipy| = %s, bit-equal to the tables in numpy %.4f"
                  % (tag, align, method, err, "%.3g" % err_fx if err_fx is not None else "-", float((got.view(np.int32) == model.view(np.int32)).mean())))
            assert err <= TOL, (tag, align, method, err)
            assert err_fx is None or err_fx <= TOL, (tag, align, method, err_fx)
            if method == "nearest":
                assert np.array_equal(got.view(np.int32), want.view(np.int32))
    mg.assert_unchanged(xd, saved, "x")


@pytest.mark.parametrize("tag", list(tz.CASES))
def test_coefficients_vs_scipy_and_restatement(tag):
    from superresolution_aniso_mri_amd.evaluate import z_interp
    x = tz.case_input(tag)
    x4 = x if x.ndim == 4 else x[None]
    coef = z_interp.bspline_coefficients(torch.from_numpy(x4).cuda()).cpu().numpy()
    assert coef.dtype == np.float64 and coef.shape == x4.shape
    want = np.stack([tz.restate_coefficients(v) for v in x4])
    e_fx, e_rs = float(np.abs(coef.reshape(x.shape) - tz.fixture()["%s/coef" % tag]).max()), float(np.abs(coef - want).max())
    print("%-6s max |coef - spline_filter1d| = %.3g, |coef - restatement| = %.3g" % (tag, e_fx, e_rs))
    assert e_fx <= TOL_COEF and e_rs <= TOL_COEF, (tag, e_fx, e_rs)


def test_4d_launch_equals_its_frames_bitwise():
    x = torch.from_numpy(tz.case_input("n2")).cuda()
    f = tz.CASES["n2"][1]
    for align in tz.ALIGNS:
        for method in tz.METHODS:
            whole = _expand(x, f, method, align)
            assert tuple(whole.shape) == (2, tz.out_count(5, f, align), 4, 8)
            for n in range(2):
                one = _expand(x[n].contiguous(), f, method, align)
                assert torch.equal(whole[n].view(torch.int32), one.view(torch.int32)), (align, method, n)
    assert not torch.equal(whole[0], whole[1])


def test_clamp01_equals_torch_clamp_bitwise():
    x = torch.from_numpy(tz.case_input("z11f6")).cuda()
    seen = 0
    for method in ("bspline", "lanczos3", "lanczos5", "linear"):
        for align in tz.ALIGNS:
            plain, clamped = _expand(x, 6, method, align), _expand(x, 6, method, align, clamp01=True)
            assert torch.equal(clamped.view(torch.int32), plain.clamp(0, 1).view(torch.int32)), (method, align)
            seen += int(((plain < 0) | (plain > 1)).sum())
    assert seen > 0                    # the spline and the sinc overshoot on random data: the clamp had something to do


# ---- the launch entry points between guard bands -------------------------------------------------------------------------------------
def _expand_call(x_np, f, method, align, poison, shift_src, shift_out, clamp01=0, **over):
    """x_np [N, Z, H, W].  Returns (rc, guarded out, out as [N, Zo, H, W], vec)."""
    from superresolution_aniso_mri_amd import _hip as hip
    from superresolution_aniso_mri_amd.evaluate import z_interp
    N, Z, H, W = x_np.shape
    name, radius = tz.package_method(method)
    base, w, boundary, needs_coef = z_interp.phase_tables(name, f, align, radius)
    base, w = np.ascontiguousarray(base, np.int32), np.ascontiguousarray(w, np.float64)
    Zo = z_interp.out_slices(Z, f, align)
    if needs_coef:
        data = torch.from_numpy(np.stack([tz.restate_coefficients(v) for v in x_np])).reshape(-1)
        gsrc = mg.guarded(x_np.size, torch.float64, "cuda", data, shift_src, "coef")
        assert gsrc.view.data_ptr() % 16 == 8 * shift_src
    else:
        gsrc = mg.guarded(x_np.size, torch.float32, "cuda", torch.from_numpy(x_np).reshape(-1), shift_src, "in")
        assert gsrc.view.data_ptr() % 16 == 4 * shift_src
    gout = mg.guarded(N * Zo * H * W, torch.float32, "cuda", poison, shift_out, "out")
    saved, kept = mg.bits(gsrc.view), (base.copy(), w.copy())
    vec = hip.lib.aesr_z_expand_store_bytes(W, hip.ptr(gsrc.view), hip.ptr(gout.view)) == 16          # the launcher's own decision function
    args = dict(inp=None if needs_coef else hip.ptr(gsrc.view), coef=hip.ptr(gsrc.view) if needs_coef else None, out=hip.ptr(gout.view), N=N, Z=Z,
                H=H, W=W, factor=f, Zo=Zo, taps=w.shape[1], base=base.ctypes.data_as(hip.IP), weights=w.ctypes.data_as(hip.DP), boundary=boundary,
                clamp01=clamp01, stream=hip.stream())
    if over.pop("both", False):
        args["inp"] = args["coef"] = hip.ptr(gsrc.view)
    args.update(over)
    torch.cuda.synchronize()
    rc = hip.lib.aesr_z_expand(*args.values())
    torch.cuda.synchronize()
    assert np.array_equal(base, kept[0]) and np.array_equal(w, kept[1])
    mg.assert_guards_intact([gsrc, gout])
    mg.assert_unchanged(gsrc.view, saved, gsrc.name)
    return rc, gout, gout.view.reshape(N, Zo, H, W), vec


@pytest.mark.parametrize("tag,method,align", [("z40f3", "lanczos5", "itk"), ("z40f3", "bspline", "grid"), ("z40f3", "linear", "itk"),
                                              ("z11f6", "lanczos3", "grid"), ("z11f6", "bspline", "itk"), ("n2", "lanczos5", "itk"),
                                              ("n2", "bspline", "itk"), ("w33", "bspline", "itk"), ("z3f2", "lanczos5", "grid"),
                                              ("z1f2", "bspline", "itk"), ("z2f3", "nearest", "itk")])
def test_z_expand_guard_bands_poisons_and_offset_pointers(tag, method, align):
    """NaN poison, finite poison, source / ``out`` shifted by 4, 8 and 12 bytes (fp32 samples) or by 8 (fp64 coefficients, which must stay
    double-aligned): guards intact, the const source unchanged, every output element written, results bit-identical across the legs and
    right.  With W % 4 == 0 both paths must have been chosen: the choice is read from ``aesr_z_expand_store_bytes``, the function the
    launcher itself decides with; the results of both are compared bit for bit."""
    x = tz.case_input(tag)
    x4 = x if x.ndim == 4 else x[None]
    f = tz.CASES[tag][1]
    want, paths = None, set()
    if method == "bspline":
        legs = [(mg.POISON_NAN, 0, 0), (mg.POISON_FINITE, 0, 0), (mg.POISON_NAN, 1, 0), (mg.POISON_FINITE, 1, 2), (mg.POISON_NAN, 0, 1),
                (mg.POISON_FINITE, 0, 3)]
    else:
        legs = [(mg.POISON_NAN, 0, 0), (mg.POISON_FINITE, 0, 0), (mg.POISON_NAN, 1, 1), (mg.POISON_FINITE, 2, 2), (mg.POISON_NAN, 3, 3),
                (mg.POISON_FINITE, 1, 0), (mg.POISON_NAN, 0, 2)]
    for poison, s_src, s_out in legs:
        rc, gout, out, vec = _expand_call(x4, f, method, align, poison, s_src, s_out)
        assert rc == 0
        assert vec == (x4.shape[3] % 4 == 0 and s_src == 0 and s_out == 0)
        paths.add(vec)
        left = mg.poison_left(gout.view, poison)
        assert left.numel() == 0, "%s: %d output element(s) never written, first %d" % (tag, left.numel(), int(left[0]))
        bits = mg.bits(out)
        if want is None:
            want = bits
            got = out.cpu().numpy().reshape(restated(tag, method, align).shape)
            assert np.abs(got.astype(np.float64) - restated(tag, method, align)).max() <= TOL
        else:
            assert torch.equal(bits, want), "%s [poison %s, shifts %d, %d]: differs from leg 1" % (tag, poison, s_src, s_out)
    assert paths == ({True, False} if x4.shape[3] % 4 == 0 else {False})


@pytest.mark.parametrize("tag", ["z40f3", "n2", "w33", "z1f2", "z2f3"])
def test_prefilter_guard_bands_poisons_and_offset_pointers(tag):
    from superresolution_aniso_mri_amd import _hip as hip
    x = tz.case_input(tag)
    x4 = x if x.ndim == 4 else x[None]
    N, Z, H, W = x4.shape
    assert hip.lib.aesr_bspline_coef_bytes(N, Z, H, W) == 8 * x4.size
    want = None
    for poison, s_in, s_coef in ((mg.POISON_NAN, 0, 0), (mg.POISON_FINITE, 0, 0), (mg.POISON_NAN, 1, 1), (mg.POISON_FINITE, 2, 0),
                                 (mg.POISON_NAN, 3, 1)):
        gin = mg.guarded(x4.size, torch.float32, "cuda", torch.from_numpy(x4).reshape(-1), s_in, "in")
        gcoef = mg.guarded(x4.size, torch.float64, "cuda", poison, s_coef, "coef")
        assert gin.view.data_ptr() % 16 == 4 * s_in and gcoef.view.data_ptr() % 16 == 8 * s_coef
        saved = mg.bits(gin.view)
        torch.cuda.synchronize()
        rc = hip.lib.aesr_bspline_prefilter_z(hip.ptr(gin.view), hip.ptr(gcoef.view), N, Z, H, W, hip.stream())
        torch.cuda.synchronize()
        assert rc == 0, hip.last_error()
        mg.assert_guards_intact([gin, gcoef])
        mg.assert_unchanged(gin.view, saved, "in")
        assert mg.poison_left(gcoef.view, poison).numel() == 0
        bits = mg.bits(gcoef.view)
        if want is None:
            want = bits
            got = gcoef.view.cpu().numpy().reshape(x4.shape)
            assert np.abs(got - np.stack([tz.restate_coefficients(v) for v in x4])).max() <= TOL_COEF
        else:
            assert torch.equal(bits, want)
    # refusals: nothing written
    gcoef = mg.guarded(x4.size, torch.float64, "cuda", mg.POISON_NAN, 0, "coef")
    for args, word in (((hip.ptr(gin.view), hip.ptr(gcoef.view), N, 0, H, W), "N, Z, H, W"), ((None, hip.ptr(gcoef.view), N, Z, H, W), "in is a null"),
                       ((hip.ptr(gin.view), ctypes_ptr(gcoef.view.data_ptr() + 4), N, Z, H, W), "coef is not 8-byte")):
        assert hip.lib.aesr_bspline_prefilter_z(*args, hip.stream()) == 1 and word in hip.last_error()
        torch.cuda.synchronize()
        assert mg.poison_left(gcoef.view, mg.POISON_NAN).numel() == gcoef.view.numel()
        mg.assert_guards_intact([gcoef])


def ctypes_ptr(address):
    import ctypes
    return ctypes.c_void_p(address)


def test_z_expand_refusals_write_nothing():
    from superresolution_aniso_mri_amd import _hip as hip
    x4 = tz.case_input("z11f6")[None]
    wide = np.zeros((17, 2))
    cases = ((dict(factor=17, Zo=11 * 17, base=np.zeros(17, np.int32).ctypes.data_as(hip.IP), weights=wide.ctypes.data_as(hip.DP), taps=2), 3, "factor=17"),
             (dict(taps=11), 3, "taps=11"), (dict(both=True), 1, "both"), (dict(inp=None), 1, "neither"), (dict(Zo=65), 1, "Zo=65"),
             (dict(Zo=67), 1, "Zo=67"), (dict(Z=0), 1, "N, Z, H, W"), (dict(W=-8), 1, "N, Z, H, W"), (dict(N=0), 1, "N, Z, H, W"),
             (dict(boundary=3), 1, "boundary"), (dict(out=None), 1, "out is a null"))
    for over, code, word in cases:
        rc, gout, _, _ = _expand_call(x4, 6, "lanczos5", "itk", mg.POISON_NAN, 0, 0, **over)
        assert rc == code and word in hip.last_error(), (sorted(over), rc, hip.last_error())
        assert mg.poison_left(gout.view, mg.POISON_NAN).numel() == gout.view.numel()
    rc, gout, _, _ = _expand_call(x4, 6, "bspline", "itk", mg.POISON_FINITE, 0, 0, coef=None)
    assert rc == 1 and "neither" in hip.last_error() and mg.poison_left(gout.view, mg.POISON_FINITE).numel() == gout.view.numel()
    rc, gout, _, _ = _expand_call(x4, 6, "bspline", "itk", mg.POISON_FINITE, 0, 0, both=True)
    assert rc == 1 and "both" in hip.last_error() and mg.poison_left(gout.view, mg.POISON_FINITE).numel() == gout.view.numel()
    from superresolution_aniso_mri_amd.evaluate import z_interp
    with pytest.raises(ValueError, match="1..16"):
        z_interp.z_expand(torch.from_numpy(x4).cuda(), 17)
    with pytest.raises(ValueError, match="expected"):
        z_interp.z_expand(torch.zeros(4, 4, device="cuda"), 2)


# ---- protocol and tools ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z,f", [(13, 3), (12, 3), (9, 4)])
def test_create_simple_interpolation_protocol(Z, f):
    """generate_inbetween_slices=True equals the composition by hand for all four methods: with (12, 3) two originals are appended."""
    from evaluate.common import create_simple_interpolation, determine_last_slice
    from superresolution_aniso_mri_amd.evaluate import z_interp
    vol = np.random.RandomState(Z * f).rand(Z, 6, 8).astype(np.float32)
    sp = np.array([2.0, 1.4, 1.25])
    last, remain = determine_last_slice(Z, f), (Z - 1) % f
    for method in z_interp.METHODS:
        for align in tz.ALIGNS:
            res = create_simple_interpolation(vol, sp, expand_factor=f, interpol_filter=method, generate_inbetween_slices=True, align=align)
            assert isinstance(res.array, np.ndarray) and res.array.dtype == np.float32 and res.array.shape == vol.shape
            by_hand = z_interp.z_expand(torch.from_numpy(np.ascontiguousarray(vol[::f])).cuda(), f, method, align=align).cpu().numpy()[:last + 1]
            if remain:
                by_hand = np.concatenate([by_hand, vol[-remain:]])
            assert np.array_equal(res.array.view(np.int32), by_hand.view(np.int32)), (method, align)
            assert np.abs(res.array[:last + 1] - tz.restate(vol[::f], f, method if method != "lanczos" else "lanczos5", align)[:last + 1]).max() <= TOL
            assert res.spacing.tolist() == [2.0, 1.4, 1.25] and res.GetSpacing() == (1.25, 1.4, 2.0)          # f * 2.0 / f
            assert res.GetOrigin() == (0.0, 0.0, -0.5 * (2.0 * f - 2.0) if align == "itk" else 0.0)
    # without the protocol: Z * f slices at spacing / f; None is Lanczos; new_spacing_z gives the factor; a device tensor stays on the device
    full = create_simple_interpolation(vol, sp, new_spacing_z=2.0 / f + 1e-9)
    assert full.array.shape == (Z * f, 6, 8) and abs(full.spacing[0] - 2.0 / f) < 1e-12
    assert np.array_equal(full.array, create_simple_interpolation(vol, sp, expand_factor=f, interpol_filter="lanczos", radius=5).array)
    dev = create_simple_interpolation(torch.from_numpy(vol).cuda(), sp, expand_factor=f, interpol_filter="linear", align="grid")
    assert torch.is_tensor(dev.array) and dev.array.is_cuda and tuple(dev.array.shape) == ((Z - 1) * f + 1, 6, 8)
    assert torch.equal(dev.array[::f].cpu(), torch.from_numpy(vol))
    cpu_t = create_simple_interpolation(torch.from_numpy(vol), sp, expand_factor=f, interpol_filter="linear", align="grid")
    assert isinstance(cpu_t.array, np.ndarray) and np.array_equal(cpu_t.array, dev.array.cpu().numpy())
    over = create_simple_interpolation(vol, sp, expand_factor=f, interpol_filter="bspline").array
    assert over.min() < 0 or over.max() > 1          # nothing is clamped: the caller clips


def _volumes():
    g = np.random.RandomState(9)
    yy, xx = np.mgrid[0:40, 0:36] / 40.0
    vols = {}
    for p, z in enumerate((9, 8)):          # 8 slices with downsample_steps 3: one remainder slice that is not scored
        base = [np.exp(-((yy - 0.3 - 0.04 * k) ** 2 + (xx - 0.5) ** 2) / 0.03) for k in range(z)]
        vols[p] = {"image": (np.stack(base) * 0.8 + 0.05 * g.rand(z, 40, 36)).astype(np.float32), "patient_id": "p%d" % p,
                   "spacing": np.array([8.0, 1.4, 1.4])}
    return vols


def _tiny_experiment(tmp_path):
    from superresolution_aniso_mri_amd import train_aesr
    out = str(tmp_path / "expers")
    train_aesr.main(["--dataset=ACDC", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8",
                     "--width=32", "--depth=8", "--downsample_steps=3", "--epochs=1", "--lr=0.001", "--ex_loss_weight1=0.05", "--exper_id=c1",
                     "--output_dir=" + out, "--synthetic", "--iters_per_epoch=2", "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    return os.path.join(out, "c1")


def test_evaluate_interpolation_performance_and_compare_methods(tmp_path, capsys):
    from evaluate.common import create_simple_interpolation, determine_last_slice
    from evaluate.find_best_model import adjust_and_center_crop, compute_metrics, evaluate_interpolation_performance, get_transforms
    from superresolution_aniso_mri_amd.evaluate import compare_methods as cm
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    vols = _volumes()
    tf = get_transforms(32, to_tensor=False)
    r = evaluate_interpolation_performance(None, {}, vols, transform=tf, downsample_steps=3, interpol_filter="linear")
    for k in ("ssim", "psnr", "vif", "ssim_synth", "psnr_synth", "vif_synth", "ssim_recon", "psnr_recon", "vif_recon"):
        assert len(r[k]) == 2 and np.isfinite(r[k]).all(), k
    assert r["lpips"] == []
    img = adjust_and_center_crop(vols[1]["image"], 32)          # by hand: 8 slices, one appended original
    hand = create_simple_interpolation(img, vols[1]["spacing"], expand_factor=3, interpol_filter="linear", generate_inbetween_slices=True).array
    m = compute_metrics(img, np.clip(hand, 0, 1), 3)
    assert abs(m["ssim"] - r["ssim"][1]) < 1e-12 and abs(m["psnr_synth"] - r["psnr_synth"][1]) < 1e-12
    assert determine_last_slice(8, 3) == 6 and np.array_equal(hand[7], img[7])
    grid = evaluate_interpolation_performance(None, {}, vols, transform=tf, downsample_steps=3, interpol_filter="linear", align="grid")
    # the grid alignment passes the kept slices through; the ITK grid does not
    assert abs(grid["ssim_recon"][0] - 1.0) < 1e-9 and r["ssim_recon"][0] < 1.0 - 1e-4 and grid["ssim_synth"][0] < 1.0 - 1e-4
    axis1 = evaluate_interpolation_performance(None, {}, vols, transform=tf, downsample_steps=3, interpol_filter="lanczos", eval_axis=1)
    assert len(axis1["ssim"]) == 2 and axis1["ssim_synth"] == [] and np.isfinite(axis1["vif"]).all()
    # the model's path is what it was: the keyword's default changes nothing
    src = _tiny_experiment(tmp_path)
    ev, e_args = get_trainer_dynamic(src_path=src, model_nbr=1, eval_mode=True)
    a = evaluate_interpolation_performance(ev, e_args, vols, transform=tf, downsample_steps=3)
    b = evaluate_interpolation_performance(ev, e_args, vols, transform=tf, downsample_steps=3, interpol_filter=None, align="grid")
    assert a == b and len(a["ssim"]) == 2 and a["ssim"] != r["ssim"]
    # compare_methods on the same experiment directory: four result files and one table
    data = tmp_path / "vols"
    data.mkdir()
    for p, v in vols.items():
        np.save(str(data / ("p%d.npy" % p)), v["image"][:, :32, :32] * 700.0)
    capsys.readouterr()
    res = cm.main(["--exper_dir=" + src, "--volumes_dir=" + str(data), "--downsample_steps=3"])
    table = capsys.readouterr().out
    assert list(res) == ["ae_combined", "linear", "bspline", "lanczos"]
    for method in res:
        f = os.path.join(src, "results", "%s_3x.npz" % method)
        assert os.path.isfile(f) and method in table
        saved = np.load(f)
        assert saved["ssim"].shape == (2,) and np.array_equal(saved["ssim"], np.asarray(res[method]["ssim"])) and np.isfinite(saved["vif_synth"]).all()
    assert len({tuple(res[m]["ssim"]) for m in res}) == 4 and "ssim_synth" in table
    cm.main(["--exper_dir=" + src, "--volumes_dir=" + str(data), "--downsample_steps=3", "--eval_axis=2", "--align=grid", "--model_nbr=1"])
    assert os.path.isfile(os.path.join(src, "results", "lanczos_3x_axis2.npz")) and os.path.isfile(os.path.join(src, "results", "ae_combined_3x_axis2.npz"))


def test_generate_hr_volumes_method(tmp_path):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd import volume_io
    from superresolution_aniso_mri_amd.evaluate import z_interp
    g = np.random.RandomState(3)
    v3, v4 = (g.rand(5, 12, 16) * 900).astype(np.float32), (g.rand(2, 4, 6, 9) * 900).astype(np.float32)
    npy, nii = tmp_path / "npy", tmp_path / "nii"
    npy.mkdir()
    nii.mkdir()
    np.save(str(npy / "a.npy"), v3)
    np.save(str(npy / "b.npy"), v4)
    volume_io.write_volume(nii / "c.nii.gz", volume_io.Volume(v3, (1.25, 1.5, 8.0), "npy", {}), v3, (1.25, 1.5, 8.0))
    out = tmp_path / "out_npy"
    res = ghv.main(["--method=lanczos", "--num_interpolations=3", "--data_input_dir=" + str(npy), "--output_dir=" + str(out), "--save"])
    assert [os.path.basename(str(p)) for p, _ in res] == ["a.npy", "b.npy"]
    a, b = np.load(str(out / "a.npy")), np.load(str(out / "b.npy"))
    assert a.shape == (20, 12, 16) and b.shape == (2, 16, 6, 9) and a.dtype == np.float32
    want = z_interp.z_expand(torch.from_numpy(v3).cuda(), 4, "lanczos").cpu().numpy()
    assert np.array_equal(a, want) and np.abs(a - tz.restate(v3, 4, "lanczos5", "itk")).max() <= 900 * TOL          # intensities as they are
    assert np.array_equal(b[1], z_interp.z_expand(torch.from_numpy(v4[1]).cuda(), 4, "lanczos").cpu().numpy())
    out = tmp_path / "out_nii"
    ghv.main(["--method=lanczos", "--lanczos_radius=3", "--align=grid", "--num_interpolations=3", "--data_input_dir=" + str(nii),
              "--output_dir=" + str(out), "--save"])
    w = volume_io.read_volume(out / "c.nii.gz")
    hdr = w.meta["header"]
    assert struct.unpack("<8h", hdr[40:56])[:4] == (3, 16, 12, 17)                    # (5 - 1) * 4 + 1 slices
    assert struct.unpack("<8f", hdr[76:108])[1:4] == (1.25, 1.5, 2.0) and w.spacing == (1.25, 1.5, 2.0)
    assert np.array_equal(w.array[::4], v3) and np.array_equal(w.array, z_interp.z_expand(torch.from_numpy(v3).cuda(), 4, "lanczos", "grid", 3).cpu().numpy())
    out = tmp_path / "out_bs"
    ghv.main(["--method=bspline", "--num_interpolations=1", "--data_input_dir=" + str(nii), "--output_dir=" + str(out), "--save"])
    w = volume_io.read_volume(out / "c.nii.gz")
    assert w.array.shape == (10, 12, 16) and w.spacing == (1.25, 1.5, 4.0)
