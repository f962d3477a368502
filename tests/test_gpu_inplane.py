"""-m gpu: in-plane resampling on the device (aesr_inplane_resample, csrc/inplane.hip; datasets/common.py apply_2d_zoom_3d / _4d).

- The kernel against every case of tests/golden/inplane.npz (the reference's own function, tests/make_golden_inplane.py): shapes exactly,
  dead lines exactly 0, values within 1e-6 absolute on [0, 1] data (4 x the 2.4e-7 an all-float32 restatement measured on the CPU; room for
  summation order -- the kernel rounds where scipy does, so it lands near 1e-7), the label cases exactly.
- ``clamp_edges=True`` differs from the fixture only on the dead lines; device tensor in -> device tensor out with the input's bits
  unchanged; a 4-D input is one launch and equals the per-frame calls bitwise.
- The legs of tests/memguard.py on the C entry point at the contractual buffer sizes (GUARDED_ENTRIES / EXEMPT partition
  ``_hip.SIGNATURES_PREPROC``; tests/test_abi.py checks that without a GPU); the unsupported radius is refused with nothing written.
- ``generate_hr_volumes --resample`` end to end, the loaders of data_device.py and ``train_aesr --volumes_dir --resample``."""
import ctypes
import os

import numpy as np
import pytest
import torch

import memguard as mg
from test_inplane_golden import QUIRK, case_input, fixture, restate

pytestmark = pytest.mark.gpu

TOL = 1e-6
GUARDED_ENTRIES = ("aesr_inplane_resample",)          # subject of test_guard_bands_poisons_and_offset_pointers
EXEMPT = {"aesr_inplane_out_size": "host query", "aesr_inplane_workspace_bytes": "host query"}
_, TAGS = fixture()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("tag", TAGS)
def test_kernel_vs_reference(tag):
    from datasets.common import apply_2d_zoom_3d, apply_2d_zoom_4d
    fx, _ = fixture()
    x, want = case_input(fx, tag), fx[tag + "/out"]
    labels, do_blur = bool(fx[tag + "/labels"]), bool(fx[tag + "/do_blur"])
    fn = apply_2d_zoom_4d if x.ndim == 4 else apply_2d_zoom_3d
    kept = x.copy()
    got = fn(x, fx[tag + "/spacing"], fx[tag + "/new_spacing"], do_blur=do_blur, as_type=int if labels else np.float32)
    assert isinstance(got, np.ndarray) and got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(x, kept)                                  # the reference blurs into its argument; this does not
    dev = fn(torch.from_numpy(x).cuda(), fx[tag + "/spacing"], fx[tag + "/new_spacing"], do_blur=do_blur, as_type=int if labels else np.float32)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    if labels:
        assert got.dtype == want.dtype == np.int64 and dev.dtype == torch.int64
        assert np.array_equal(got, want), (tag, int((got != want).sum()))
        return
    assert got.dtype == np.float32
    row, col = QUIRK.get(tag, (False, False))
    flat = got.reshape((-1,) + got.shape[-2:])
    if row:
        assert (flat[:, -1, :].view(np.int32) == 0).all()           # exactly +0.0
    if col:
        assert (flat[:, :, -1].view(np.int32) == 0).all()
    assert bool((flat[:, -1, :] == 0).all()) == row and bool((flat[:, :, -1] == 0).all()) == col
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print("%-18s %s max |kernel - reference| = %.3g, bit-equal %.4f" % (tag, want.shape, err, float((got == want).mean())))
    assert err <= TOL, (tag, err)


@pytest.mark.parametrize("tag", ["d_quirk", "d_quirk224", "a_in_125"])
def test_clamp_edges_differs_only_on_the_dead_lines(tag):
    from datasets.common import apply_2d_zoom_3d
    fx, _ = fixture()
    x, want = case_input(fx, tag), fx[tag + "/out"]
    sp, ns = fx[tag + "/spacing"], fx[tag + "/new_spacing"]
    got = apply_2d_zoom_3d(x, sp, ns, clamp_edges=True)
    plain = apply_2d_zoom_3d(x, sp, ns)
    row, col = QUIRK.get(tag, (False, False))
    if not (row or col):
        assert np.array_equal(got.view(np.int32), plain.view(np.int32))
        return
    live = np.ones(got.shape, bool)
    live[:, -1, :] &= not row
    live[:, :, -1] &= not col
    assert np.array_equal(got[live].view(np.int32), plain[live].view(np.int32))
    assert np.abs(got[live].astype(np.float64) - want[live]).max() <= TOL
    # on the dead lines: the value at n - 1 (the restatement with the same opt-out), not 0
    ref = restate(x, sp, ns, clamp_edges=True)
    assert np.abs(got.astype(np.float64) - ref).max() <= TOL
    assert (plain[~live] == 0).all() and np.abs(got[~live]).max() > 0.01


def test_device_tensor_in_device_tensor_out_and_input_untouched():
    from datasets.common import apply_2d_zoom_3d
    from superresolution_aniso_mri_amd.datasets import common as dc
    g = torch.Generator().manual_seed(4)
    x = torch.rand(7, 45, 52, generator=g).cuda()
    saved = _bits(x).clone()
    n0 = dc.LAUNCHES
    y = apply_2d_zoom_3d(x, (8.0, 1.5625, 1.5625), (1.4, 1.4))
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (7, 50, 58) and y.data_ptr() != x.data_ptr()
    assert dc.LAUNCHES == n0 + 1
    assert torch.equal(_bits(x), saved)
    assert np.abs(y.cpu().numpy().astype(np.float64) - restate(x.cpu().numpy(), (1.5625, 1.5625), (1.4, 1.4))).max() <= TOL
    # a non-contiguous view and a float64 tensor are taken (copied / cast to float32), the result is the same
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not xt.is_contiguous() and torch.equal(_bits(apply_2d_zoom_3d(xt, (1.5625, 1.5625), (1.4, 1.4))), _bits(y))
    assert torch.equal(_bits(apply_2d_zoom_3d(x.double(), (1.5625, 1.5625), (1.4, 1.4))), _bits(y))


def test_4d_is_one_launch_and_equals_the_frames_bitwise():
    from datasets.common import apply_2d_zoom_3d, apply_2d_zoom_4d
    from superresolution_aniso_mri_amd.datasets import common as dc
    g = torch.Generator().manual_seed(5)
    x = torch.rand(5, 6, 44, 40, generator=g).cuda()
    for sp, ns in (((8.0, 1.5625, 1.5625), (1.4, 1.4)), ((1.4, 1.4), (8.0, 1.5625, 1.25))):
        n0 = dc.LAUNCHES
        y = apply_2d_zoom_4d(x, sp, ns)
        assert dc.LAUNCHES == n0 + 1
        frames = torch.stack([apply_2d_zoom_3d(f, sp, ns) for f in x])
        assert y.shape == frames.shape and y.shape[:2] == x.shape[:2] and torch.equal(_bits(y), _bits(frames))


# ---- the C entry point between guard bands -------------------------------------------------------------------------------------------
def _abi_call(x_np, zoom, do_blur, poison, shift, clamp_edges=False, radius_zoom=None):
    """One guarded call at the contractual sizes.  Returns (rc, in, out, workspace, saved input bits)."""
    from superresolution_aniso_mri_amd import _hip as hip
    from superresolution_aniso_mri_amd.datasets import common as dc
    N, H, W = x_np.shape
    Ho, Wo = dc.out_size(H, zoom[0]), dc.out_size(W, zoom[1])
    rz = zoom if radius_zoom is None else radius_zoom
    wy, ry = dc.gaussian_weights(0.25 / rz[0])
    wx, rx = dc.gaussian_weights(0.25 / rz[1])
    iy, ty = dc.zoom_tables(H, Ho, clamp_edges)
    ix, tx = dc.zoom_tables(W, Wo, clamp_edges)
    ws_bytes = int(hip.lib.aesr_inplane_workspace_bytes(Ho, Wo))
    assert ws_bytes % 8 == 0 and ws_bytes >= 8 * (Ho + Wo) + 4 * (Ho + Wo)
    gin = mg.guarded(x_np.size, torch.float32, "cuda", torch.from_numpy(x_np).reshape(-1), shift, "in")
    gout = mg.guarded(N * Ho * Wo, torch.float32, "cuda", poison, shift, "out")
    gws = mg.guarded(ws_bytes // 8, torch.float64, "cuda", poison, shift, "workspace")
    if shift:
        assert gin.view.data_ptr() % 16 == 4 and gout.view.data_ptr() % 16 == 4 and gws.view.data_ptr() % 16 == 8
    saved = mg.bits(gin.view)
    D = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(hip.DP)        # noqa: E731
    I = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(hip.IP)          # noqa: E731, E741
    host = [np.ascontiguousarray(a).copy() for a in (wy, wx, iy, ty, ix, tx)]
    torch.cuda.synchronize()
    rc = hip.lib.aesr_inplane_resample(hip.ptr(gin.view), hip.ptr(gout.view), hip.ptr(gws.view), N, H, W, Ho, Wo, D(wy), ry, D(wx), rx,
                                       I(iy), D(ty), I(ix), D(tx), 1 if do_blur else 0, hip.stream())
    torch.cuda.synchronize()
    for a, b in zip(host, (wy, wx, iy, ty, ix, tx)):
        assert np.array_equal(a, b)                               # the host arrays are const too
    mg.assert_guards_intact([gin, gout, gws])
    mg.assert_unchanged(gin.view, saved, "in")
    return rc, gin, gout.view.reshape(N, Ho, Wo), gws, gout


@pytest.mark.parametrize("tag,do_blur", [("a_back_15625", True), ("d_quirk", True), ("c_radius2", True), ("e_tiny_mixed", True),
                                         ("a_in_168", False)])
def test_guard_bands_poisons_and_offset_pointers(tag, do_blur):
    """Legs of tests/test_gpu_memguard.py for aesr_inplane_resample: NaN poison, finite poison, all device pointers offset from a 16-byte
    boundary (4 bytes for in / out -- the 16-byte store path must then not be taken -- and 8 for the workspace of doubles): guards
    intact, the const input unchanged, every output element written, results bit-identical across the legs and right."""
    fx, _ = fixture()
    x = case_input(fx, tag)
    zoom = np.array(fx[tag + "/spacing"][-2:]) / np.array(fx[tag + "/new_spacing"][-2:])
    want = None
    for poison, shift in ((mg.POISON_NAN, 0), (mg.POISON_FINITE, 0), (mg.POISON_NAN, 1), (mg.POISON_FINITE, 1)):
        rc, _, out, _, gout = _abi_call(x, zoom, do_blur, poison, shift)
        assert rc == 0
        left = mg.poison_left(gout.view, poison)
        assert left.numel() == 0, "%s: %d output element(s) never written, first %d" % (tag, left.numel(), int(left[0]))
        bits = mg.bits(out)
        if want is None:
            want = bits
            ref = restate(x, fx[tag + "/spacing"], fx[tag + "/new_spacing"], do_blur=do_blur)
            assert np.abs(out.cpu().numpy().astype(np.float64) - ref).max() <= TOL
            if do_blur:
                assert np.abs(out.cpu().numpy().astype(np.float64) - fx[tag + "/out"]).max() <= TOL
        else:
            assert torch.equal(bits, want), "%s [poison %s, shift %d]: differs from leg 1" % (tag, poison, shift)


def test_refusals_write_nothing():
    from superresolution_aniso_mri_amd import _hip as hip
    x = np.random.RandomState(2).rand(2, 40, 36).astype(np.float32)
    # radius 9 along y (the weights of zoom 0.11 with the tables of zoom 0.5): unsupported, the limit is named
    rc, _, _, gws, gout = _abi_call(x, (0.5, 0.5), True, mg.POISON_NAN, 0, radius_zoom=(0.11, 0.5))
    assert rc == 3 and "radius" in hip.last_error() and "8" in hip.last_error()
    assert mg.poison_left(gout.view, mg.POISON_NAN).numel() == gout.view.numel()
    assert mg.poison_left(gws.view, mg.POISON_NAN).numel() == gws.view.numel()
    # the Python interface raises with the library's message
    from datasets.common import apply_2d_zoom_3d
    with pytest.raises(RuntimeError, match="radius"):
        apply_2d_zoom_3d(torch.from_numpy(x).cuda(), (0.154, 1.4), (1.4, 1.4))          # zoom 0.11 along y
    # a workspace that is not 8-byte aligned is refused by name
    from superresolution_aniso_mri_amd.datasets import common as dc
    iy, ty = dc.zoom_tables(40, 20)
    ix, tx = dc.zoom_tables(36, 18)
    w, r = dc.gaussian_weights(0.5)
    xin, out = torch.from_numpy(x).cuda(), torch.full((2, 20, 18), 7.0, device="cuda")
    ws = torch.zeros(int(hip.lib.aesr_inplane_workspace_bytes(20, 18)) // 4 + 1, dtype=torch.float32, device="cuda")
    D = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(hip.DP)        # noqa: E731
    I = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(hip.IP)          # noqa: E731, E741
    odd = ctypes.c_void_p(ws.data_ptr() + 4)
    assert hip.lib.aesr_inplane_resample(hip.ptr(xin), hip.ptr(out), odd, 2, 40, 36, 20, 18, D(w), r, D(w), r, I(iy), D(ty), I(ix), D(tx), 1,
                                         hip.stream()) == 1
    assert "align" in hip.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0).all())


# ---- the users of the step -----------------------------------------------------------------------------------------------------------
def _tiny_model(tmp_path):
    from superresolution_aniso_mri_amd import train_aesr
    out = str(tmp_path / "expers")
    train_aesr.main(["--dataset=ACDC", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8",
                     "--width=32", "--depth=8", "--downsample_steps=2", "--epochs=1", "--lr=0.001", "--ex_loss_weight1=0.05", "--exper_id=r1",
                     "--output_dir=" + out, "--synthetic", "--iters_per_epoch=3", "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    return os.path.join(out, "r1")


def _volume(seed, shape, scale=900.0):
    z, h, w = shape
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    vol = np.stack([np.exp(-((yy - h * (0.4 + 0.03 * k)) ** 2 + (xx - w * 0.5) ** 2) / (0.05 * h * w)) for k in range(z)])
    return ((vol * 0.8 + 0.1 * g.rand(z, h, w)) * scale).astype(np.float32)


def test_generate_hr_volumes_resample_end_to_end(tmp_path):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd import volume_io
    from superresolution_aniso_mri_amd.datasets.common import apply_2d_zoom_3d
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    src = _tiny_model(tmp_path)
    vol = _volume(0, (5, 36, 72))                 # 36 x 72 at 1.5625 mm <-> 40 x 80 at 1.4 mm
    nii = tmp_path / "nii"
    nii.mkdir()
    sp = (1.5625, 1.5625, 8.0)                    # (x, y, z), as the header stores it
    volume_io.write_volume(nii / "vol0.nii.gz", volume_io.Volume(vol, sp, "npy", {}), vol, sp)
    common = ["--exper_dir=" + src, "--model_nbr=1", "--num_interpolations=3", "--data_input_dir=" + str(nii), "--save"]
    ghv.main(common + ["--output_dir=" + str(tmp_path / "hr_rs"), "--resample"])
    back = volume_io.read_volume(tmp_path / "hr_rs" / "vol0.nii.gz")
    assert back.array.shape == (17, 36, 72) and back.array.dtype == np.float32          # (Z - 1)(n + 1) + 1 slices, the input's in-plane shape
    assert back.spacing[:2] == (1.5625, 1.5625) and abs(back.spacing[2] - 2.0) < 1e-6
    assert back.array.min() >= 0 and back.array.max() <= 1 + 1e-6 and back.array.std() > 0.01
    # the composition by hand
    trainer, _ = get_trainer_dynamic(src_path=src, model_nbr=1, eval_mode=True)
    alphas = np.linspace(0, 1, 5)[1:-1]
    x = apply_2d_zoom_3d(torch.from_numpy(vol).cuda(), (1.5625, 1.5625), (1.4, 1.4))
    assert tuple(x.shape) == (5, 40, 80)
    x = ghv.normalize_on_device(x)
    assert float(x.min()) >= 0 and float(x.max()) <= 1
    lo, hi = np.percentile(apply_2d_zoom_3d(vol, (1.5625, 1.5625), (1.4, 1.4)), (1, 99))
    want_x = ((apply_2d_zoom_3d(vol, (1.5625, 1.5625), (1.4, 1.4)) - lo) / (hi - lo)).clip(0, 1)
    assert np.abs(x.cpu().numpy() - want_x).max() < 1e-5                                  # numpy's percentiles, the reference's order
    hr = ghv.create_super_volume(trainer, x.unsqueeze(1), alphas, use_original=True, to_cpu=False)["upsampled_image"]
    assert hr.is_cuda and tuple(hr.shape) == (17, 40, 80)
    want = apply_2d_zoom_3d(hr, (1.4, 1.4), (1.5625, 1.5625)).cpu().numpy()
    assert np.array_equal(back.array, want)
    # without the flag: what it was -- upsample_volume of the raw array, the z spacing divided by n + 1, the in-plane spacing kept
    ghv.main(common + ["--output_dir=" + str(tmp_path / "hr_plain")])
    plain = volume_io.read_volume(tmp_path / "hr_plain" / "vol0.nii.gz")
    assert np.array_equal(plain.array, ghv.upsample_volume(trainer, vol, 3)) and plain.array.shape == (17, 36, 72)
    assert plain.spacing[:2] == (1.5625, 1.5625) and abs(plain.spacing[2] - 2.0) < 1e-6
    assert not np.array_equal(plain.array, back.array)
    # a size whose resampled width (37 -> 41) is no multiple of the network's stride (4): padded for the synthesis, cropped, resampled back
    odd = _volume(2, (4, 36, 37))
    got = ghv.upsample_volume_resampled(trainer, odd, 3, (1.5625, 1.5625))
    xo = ghv.normalize_on_device(apply_2d_zoom_3d(torch.from_numpy(odd).cuda(), (1.5625, 1.5625), (1.4, 1.4)))
    assert tuple(xo.shape) == (4, 40, 41)
    xo = torch.nn.functional.pad(xo, (0, 3, 0, 0))
    ho = ghv.create_super_volume(trainer, xo.unsqueeze(1), alphas, use_original=True, to_cpu=False)["upsampled_image"][:, :, :41].contiguous()
    assert got.shape == (13, 36, 37) and np.array_equal(got, apply_2d_zoom_3d(ho, (1.4, 1.4), (1.5625, 1.5625)).cpu().numpy())
    # .npy with --spacing; a 4-D file goes through one resampling launch each way and equals its frames
    npy = tmp_path / "npy"
    npy.mkdir()
    np.save(str(npy / "vol0.npy"), vol)
    res = ghv.main(["--exper_dir=" + src, "--model_nbr=1", "--num_interpolations=3", "--data_input_dir=" + str(npy),
                    "--output_dir=" + str(tmp_path / "hr_npy"), "--resample", "--spacing", "1.5625", "1.5625"])
    assert np.array_equal(res[0][1], want)
    vol4 = np.stack([vol, _volume(1, (5, 36, 72))])
    got4 = ghv.upsample_volume_resampled(trainer, vol4, 3, (1.5625, 1.5625))
    assert got4.shape == (2, 17, 36, 72) and np.array_equal(got4[0], want)
    assert np.array_equal(got4[1], ghv.upsample_volume_resampled(trainer, vol4[1], 3, (1.5625, 1.5625), (1.4, 1.4)))


def test_loaders_and_training_resample(tmp_path):
    from superresolution_aniso_mri_amd import data_device, train_aesr, volume_io
    from superresolution_aniso_mri_amd.datasets.common import apply_2d_zoom_3d
    data = tmp_path / "vols"
    data.mkdir()
    v1, v2 = _volume(3, (9, 36, 40), 1200.0), np.stack([_volume(4, (8, 40, 36)), _volume(5, (8, 40, 36))])
    volume_io.write_volume(data / "p1.nii.gz", volume_io.Volume(v1, (1.5625, 1.5625, 8.0), "npy", {}), v1, (1.5625, 1.5625, 8.0))
    volume_io.write_volume(data / "p2.nii.gz", volume_io.Volume(v2, (1.25, 1.37, 10.0, 1.0), "npy", {}), v2, (1.25, 1.37, 10.0, 1.0))
    plain = data_device.load_volume_dir(str(data))
    vols = data_device.load_volumes(str(data), resample=True)
    assert [v.shape for v in plain] == [(9, 36, 40), (8, 40, 36), (8, 40, 36)]
    assert [v.dtype for v in vols] == [v.dtype for v in plain]
    assert [v.shape for v in vols] == [(9, 40, 45), (8, 39, 32), (8, 39, 32)]              # y at 1.37 mm, x at 1.25 mm -> 1.4 mm
    for v in vols:
        assert np.issubdtype(v.dtype, np.floating) and v.min() >= 0 and v.max() <= 1         # rescale_intensities' own dtype, as without the flag
    want = data_device.rescale_intensities(apply_2d_zoom_3d(v1, (8.0, 1.5625, 1.5625), (1.4, 1.4)))        # resample, then rescale
    assert np.array_equal(vols[0], want)
    d = data_device.load_image_dict(str(data), resample=True)
    assert sorted(d) == [1, 2] and d[1]["image"].shape == (1, 9, 40, 45) and d[2]["image"].shape == (2, 8, 39, 32)
    assert d[1]["spacing"].tolist() == [8.0, 1.4, 1.4] and d[1]["original_spacing"].tolist() == [8.0, 1.5625, 1.5625]
    assert d[2]["spacing"].tolist() == [10.0, 1.4, 1.4] and np.allclose(d[2]["original_spacing"], [10.0, 1.37, 1.25], atol=1e-6)
    assert "original_spacing" not in data_device.load_image_dict(str(data))[1]
    assert data_device.load_volumes(str(data), resample=True, new_spacing=(1.25, 1.25))[0].shape == (9, 45, 50)
    np.save(str(data / "p3.npy"), v1)
    with pytest.raises(ValueError, match="spacing"):
        data_device.load_volume_dir(str(data), resample=True)
    os.remove(str(data / "p3.npy"))
    out = str(tmp_path / "expers")
    tr = train_aesr.main(["--dataset=ACDC", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8",
                          "--width=32", "--depth=8", "--downsample_steps=2", "--epochs=1", "--lr=0.001", "--ex_loss_weight1=0.05",
                          "--exper_id=v1", "--output_dir=" + out, "--volumes_dir=" + str(data), "--resample", "--aug_patch_size=32",
                          "--iters_per_epoch=2", "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    assert tr.iters == 1 + 2 and np.isfinite(tr.mean_losses["loss_ae"][-1])
