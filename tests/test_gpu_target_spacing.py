"""-m gpu: slice synthesis at a target slice spacing (evaluate/z_grid.py, ``create_super_volume(..., grid=)``, ``HipAE.decode_mixes_at``,
``generate_hr_volumes --target_spacing_z / --isotropic``) on the small trainers of test_gpu_inference.py (32 x 32) and
test_gpu_multichannel.py (depth 8, latent 16, two scales; 40 x 36 and the 32 x 32 volume of tests/golden/supervolume_labels.npz).

Bounds.  A commensurate grid against the integer path: kept slots bit-identical, synthesised slots 1e-6 absolute on [0, 1] data (the
fp32 alphas are asserted equal first and the mixing arithmetic per element is the same; only the batch order of the rest of the decoder
differs -- whether the result is bit-equal is printed, not asserted).  A non-commensurate grid slice by slice against
``latent_space_interp``: rtol 1e-5 / atol 2e-6, what test_gpu_inference.py holds ``create_super_volume`` to against the per-alpha loop; the
fallback path within the same bound of the fused one.  Label maps: exact at the kept slots; in between equal to ``latent_space_interp``'s
wherever its two largest probabilities differ by >= 1e-4, of which at most 1 % of a map may fall short (test_gpu_multichannel.py's rule).
The linear baseline against a float64 numpy lerp rounded once: 1e-6 absolute, the bound of test_gpu_reslice.py; nearest away from
half-integer positions (> 1e-4): exact.  Files: 29 slices from 5 at 10 mm -> 1.4 mm, the z spacing written, origin and direction kept."""
import gzip
import os

import numpy as np
import pytest
import torch

import test_gpu_inference as ti
import test_gpu_multichannel as gm
import test_multichannel_golden as tm
from test_gpu_reslice import _nifti_bytes

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 2e-6          # test_gpu_inference.py::test_create_super_volume_vs_reference_loop
NON_COMMENSURATE = [(5, 10.0, 1.4), (3, 10.0, 1.5625)]
COMMENSURATE = [(10.0, 4), (8.0, 3)]


def _grid(Z, s, d):
    from superresolution_aniso_mri_amd.evaluate.z_grid import target_grid
    return target_grid(Z, s, d)


@pytest.fixture(scope="module")
def single():
    """(trainer, [5, 1, 32, 32] volume) of tests/golden/supervolume.npz"""
    rec = dict(np.load(os.path.join(ti.GOLDEN, "supervolume.npz")))
    tr = ti._trainer(dict(width=32, latent_width=8, depth=8, latent=16), {k[2:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p/")})
    return tr, torch.from_numpy(rec["vol"])


@pytest.fixture(scope="module")
def multi():
    """(trainer, {'32': (images, labels) of supervolume_labels.npz [5, 32, 32], '40x36': a random [4, 40, 36] pair})"""
    rec = tm.load("supervolume_labels.npz")
    tr = gm.make_trainer("ae_combined", "mse", {k[2:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p/")})
    tr.model.eval()
    g = torch.Generator().manual_seed(11)
    labels = torch.zeros(4, 40, 36)
    for k in range(4):
        labels[k, 8 + k:30, 6:28 - k] = 1.0
        labels[k, 12:24 + k, 10:22] = 2.0
        labels[k, 15:20, 13 + k:19 + k] = 3.0
    return tr, {"32": (torch.from_numpy(rec["Z5/images"]), torch.from_numpy(rec["Z5/labels"])), "40x36": (torch.rand(4, 40, 36, generator=g), labels)}


# ---- 1: a commensurate grid is the integer path ----------------------------------------------------------------------------------------
def _check_commensurate(tr, images, labels, s, n, use_original):
    from superresolution_aniso_mri_amd.generate_hr_volumes import create_super_volume
    Z = images.shape[0]
    alphas = np.linspace(0, 1, n + 2)[1:-1]
    grid = _grid(Z, s, s / (n + 1))
    for al in grid.gap_alphas:          # first: the kernels get the same fp32 alphas, so a difference cannot come from the grid
        assert np.array_equal(np.asarray(al, dtype=np.float64).astype(np.float32), alphas.astype(np.float32))
    want = create_super_volume(tr, images.clone(), alphas, use_original=use_original, labels=None if labels is None else labels.clone())
    got = create_super_volume(tr, images.clone(), None, use_original=use_original, labels=None if labels is None else labels.clone(), grid=grid)
    wi, gi = want["upsampled_image"], got["upsampled_image"]
    assert gi.shape == wi.shape == ((Z - 1) * (n + 1) + 1,) + tuple(images.shape[-2:]) and gi.dtype == wi.dtype and not gi.is_cuda
    assert torch.equal(gm.mg.bits(gi[::n + 1]), gm.mg.bits(wi[::n + 1]))
    synth = torch.ones(gi.shape[0], dtype=torch.bool)
    synth[::n + 1] = False
    err = float((gi[synth] - wi[synth]).abs().max())
    print("commensurate s=%g n=%d use_original=%s %s: synthesised max abs diff %.3e, bit-equal %s"
          % (s, n, use_original, tuple(images.shape), err, torch.equal(gm.mg.bits(gi), gm.mg.bits(wi))))
    assert err <= 1e-6
    if labels is None:
        assert got["upsampled_labels"] is None
    else:
        wl, gl = want["upsampled_labels"], got["upsampled_labels"]
        assert gl.shape == wl.shape and gl.dtype == wl.dtype == (torch.float32 if use_original else torch.int64)
        assert torch.equal(gl[::n + 1], wl[::n + 1])
        print("    labels: %d of %d synthesised pixels differ" % (int((gl[synth] != wl[synth]).sum()), int(gl[synth].numel())))


@pytest.mark.parametrize("use_original", [True, False])
@pytest.mark.parametrize("s,n", COMMENSURATE)
def test_commensurate_grid_equals_integer_path(single, s, n, use_original):
    tr, vol = single
    _check_commensurate(tr, vol, None, s, n, use_original)
    _check_commensurate(tr, vol[:4, 0], None, s, n, use_original)


@pytest.mark.parametrize("use_original", [True, False])
@pytest.mark.parametrize("s,n", COMMENSURATE)
def test_commensurate_grid_equals_integer_path_with_labels(multi, s, n, use_original):
    tr, vols = multi
    _check_commensurate(tr, vols["40x36"][0], vols["40x36"][1], s, n, use_original)


@pytest.mark.parametrize("shape", [(5, 5, 7), (4, 9, 3), (5, 8, 6), (2, 1, 1)])
def test_assembly_by_index_equals_interleave(shape):
    """odd H * W: the integer path's interleave takes its non-fused branch ((H * W) % 4 != 0); 8 x 6: the fused kernel"""
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    Z, n = shape[0], 3
    g = torch.Generator().manual_seed(sum(shape))
    kept = (torch.rand(shape, generator=g) * 1.4 - 0.2).cuda()
    synth = (torch.rand(((Z - 1) * n,) + shape[1:], generator=g) * 1.4 - 0.2).cuda()         # row k (Z - 1) + i, as lerp_multi orders them
    want = ghv._interleave(kept, synth, n, (0.0, 1.0))
    gap_major = synth.reshape(n, Z - 1, *shape[1:]).transpose(0, 1).reshape(synth.shape)     # ascending position
    got = ghv._assemble(kept, gap_major, _grid(Z, 8.0, 2.0), (0.0, 1.0))
    assert torch.equal(gm.mg.bits(got), gm.mg.bits(want)) and float(got.min()) >= 0 and float(got.max()) <= 1
    only = ghv._assemble(kept, None, _grid(Z, 8.0, 8.0), (0.0, 1.0))
    assert torch.equal(only, kept.clamp(0, 1))


# ---- 2, 3: a non-commensurate grid, slice by slice; the fallback ---------------------------------------------------------------------------
def _check_slices(tr, vol, grid, out, use_original):
    from superresolution_aniso_mri_amd.generate_hr_volumes import latent_space_interp
    assert tuple(out.shape) == (grid.J,) + tuple(vol.shape[-2:]) and not out.is_cuda
    with torch.no_grad():
        kept = vol[:, 0] if use_original else tr.decode(tr.encode(vol.cuda(), use_sr_model=True), use_sr_model=True)[:, 0].cpu()
    kept = kept.clamp(0, 1)          # the volume is clamped as a whole, as in the integer path: this fixture's input leaves [0, 1]
    worst = 0.0
    for j in range(grid.J):
        if grid.is_original[j]:
            assert torch.equal(gm.mg.bits(out[j]), gm.mg.bits(kept[grid.source[j]])), j
            continue
        i = int(grid.gap[j])
        want = latent_space_interp(float(grid.alpha[j]), tr, vol[i + 1:i + 2], vol[i:i + 1])["inter_image"][0, 0].clamp(0, 1)
        worst = max(worst, float((out[j] - want).abs().max()))
        np.testing.assert_allclose(out[j].numpy(), want.numpy(), rtol=RTOL, atol=ATOL, err_msg="slice %d" % j)
    return worst


@pytest.mark.parametrize("use_original", [True, False])
@pytest.mark.parametrize("Z,s,d", NON_COMMENSURATE)
def test_non_commensurate_grid_slice_by_slice_and_fallback(single, monkeypatch, Z, s, d, use_original):
    from superresolution_aniso_mri_amd.generate_hr_volumes import create_super_volume
    tr, vol = single
    vol, grid = vol[:Z], _grid(Z, s, d)
    model = tr._use_sr_model(True)
    calls = []
    fused_fn = type(model).decode_mixes_at
    monkeypatch.setattr(type(model), "decode_mixes_at", lambda self, z, ga: calls.append(len(ga)) or fused_fn(self, z, ga))
    res = create_super_volume(tr, vol.clone(), None, use_original=use_original, grid=grid)
    assert calls == [Z - 1] and res["upsampled_labels"] is None
    fused = res["upsampled_image"]
    worst = _check_slices(tr, vol, grid, fused, use_original)
    dev = create_super_volume(tr, vol.clone(), [], use_original=use_original, grid=grid, to_cpu=False)["upsampled_image"]
    assert dev.is_cuda and torch.equal(gm.mg.bits(dev.cpu()), gm.mg.bits(fused))
    # the fallback: a model whose decoder does not start as decode_mixes_at needs it
    monkeypatch.setattr(type(model), "decode_mixes_at", lambda self, z, ga: calls.append(None))
    plain = create_super_volume(tr, vol.clone(), None, use_original=use_original, grid=grid)["upsampled_image"]
    assert calls[-1] is None
    print("Z=%d s=%g d=%g use_original=%s: %d slices, worst abs diff to latent_space_interp %.3e, fallback to fused %.3e"
          % (Z, s, d, use_original, grid.J, worst, float((plain - fused).abs().max())))
    np.testing.assert_allclose(plain.numpy(), fused.numpy(), rtol=RTOL, atol=ATOL)
    orig = torch.from_numpy(np.flatnonzero(grid.is_original))
    assert torch.equal(gm.mg.bits(plain[orig]), gm.mg.bits(fused[orig]))
    _check_slices(tr, vol, grid, plain, use_original)


def test_decode_mixes_at_is_an_eval_path_with_one_list_per_gap(single):
    tr, vol = single
    model = tr._use_sr_model(True)
    model.eval()
    with torch.no_grad():
        lat = tr.encode(vol.cuda(), use_sr_model=True)
        with pytest.raises(ValueError, match="gap_alphas"):
            model.decode_mixes_at(lat, [[0.5]] * 3)
        with pytest.raises(ValueError, match="gap_alphas"):
            model.decode_mixes_at(lat, [[]] * 4)
        some = model.decode_mixes_at(lat, [[0.25, 0.5], [], [0.75], []])          # empty gaps, gap-major order
        want = model.decode_mixes(lat, [0.25, 0.5, 0.75])                           # row k * 4 + i
        assert tuple(some.shape) == (3, 1, 32, 32)
        assert float((some - want[[0, 4, 10]]).abs().max()) <= 1e-6
    model.train()
    try:
        with pytest.raises(RuntimeError, match="inference path"):
            model.decode_mixes_at(lat, [[0.5]] * 4)
    finally:
        model.eval()


# ---- 4: label maps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_original", [True, False])
@pytest.mark.parametrize("Z,s,d", NON_COMMENSURATE)
def test_label_maps_on_the_grid(multi, monkeypatch, Z, s, d, use_original):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd import ops
    tr, vols = multi
    images, labels = vols["32"][0][:Z], vols["32"][1][:Z]
    grid = _grid(Z, s, d)
    res = ghv.create_super_volume(tr, images.clone(), None, use_original=use_original, labels=labels.clone(), grid=grid)
    gi, gl = res["upsampled_image"], res["upsampled_labels"]
    assert tuple(gi.shape) == tuple(gl.shape) == (grid.J, 32, 32) and not gl.is_cuda
    assert gl.dtype == (torch.float32 if use_original else torch.int64)
    vol = torch.cat([images[:, None], labels[:, None]], dim=1)
    with torch.no_grad():
        rec = tr.decode(tr.encode(vol.cuda(), use_sr_model=True), use_sr_model=True)
    kept_i = (images if use_original else rec["image"][:, 0].cpu()).clamp(0, 1)
    kept_l = labels if use_original else rec["pred_labels"][:, 0].cpu()
    for j in range(grid.J):
        if grid.is_original[j]:
            assert torch.equal(gl[j], kept_l[grid.source[j]].to(gl.dtype)) and torch.equal(gm.mg.bits(gi[j]), gm.mg.bits(kept_i[grid.source[j]])), j
            continue
        i, a = int(grid.gap[j]), float(grid.alpha[j])
        r = ghv.latent_space_interp(a, tr, vol[i + 1:i + 2], vol[i:i + 1], with_labels=True)
        with torch.no_grad():          # the same call once more for its probabilities, which latent_space_interp does not return
            z = torch.cat([tr.encode(vol[i + 1:i + 2].cuda(), use_sr_model=True), tr.encode(vol[i:i + 1].cuda(), use_sr_model=True)], dim=0)
            inter = tr.decode(ops.lerp_mix(z, a, 1 - a), use_sr_model=True)
        assert torch.equal(inter["pred_labels"].cpu(), r["inter_label"])
        gm.labels_agree(gl[j][None, None].long(), r["inter_label"], inter["soft_probs"].cpu().numpy(), "slice %d" % j)
        np.testing.assert_allclose(gi[j].numpy(), r["inter_image"][0, 0].clamp(0, 1).numpy(), rtol=RTOL, atol=ATOL, err_msg="slice %d" % j)
    # the fallback gives the same maps under the same rule, and the errors of the integer path apply
    model = tr._use_sr_model(True)
    monkeypatch.setattr(type(model), "decode_mixes_at", lambda self, z, ga: None)
    plain = ghv.create_super_volume(tr, images.clone(), None, use_original=use_original, labels=labels.clone(), grid=grid)
    np.testing.assert_allclose(plain["upsampled_image"].numpy(), gi.numpy(), rtol=RTOL, atol=ATOL)
    assert plain["upsampled_labels"].dtype == gl.dtype
    print("Z=%d d=%g use_original=%s: fallback label maps differ from the fused ones at %d pixels"
          % (Z, d, use_original, int((plain["upsampled_labels"] != gl).sum())))
    monkeypatch.undo()
    with pytest.raises(ValueError, match="multi-channel"):
        ghv.create_super_volume(tr, vol.clone(), None, use_original=use_original, grid=grid)


def test_labels_without_a_label_head_are_refused(single):
    from superresolution_aniso_mri_amd.generate_hr_volumes import create_super_volume
    tr, vol = single
    for use_original in (True, False):          # a one-channel model refuses the two-channel volume: the same error on both grids
        errors = []
        for kw in (dict(alpha_range=[0.5]), dict(alpha_range=None, grid=_grid(3, 10, 1.5625))):
            with pytest.raises(RuntimeError, match="channel mismatch") as e:
                create_super_volume(tr, vol[:3].clone(), use_original=use_original, labels=torch.zeros(3, 1, 32, 32), **kw)
            errors.append(str(e.value))
        assert errors[0] == errors[1]

    class TwoChannelsNoHead:          # takes the two-channel volume, decodes images only
        args, decode, _use_sr_model = tr.args, staticmethod(tr.decode), staticmethod(tr._use_sr_model)

        @staticmethod
        def encode(x, **kw):
            return tr.encode(x[:, :1].contiguous(), **kw)
    for use_original in (True, False):
        for kw in (dict(alpha_range=[0.5]), dict(alpha_range=None, grid=_grid(3, 10, 1.5625))):
            with pytest.raises(ValueError, match="no label head"):
                create_super_volume(TwoChannelsNoHead, vol[:3].clone(), use_original=use_original, labels=torch.zeros(3, 1, 32, 32), **kw)
    with pytest.raises(ValueError, match="grid is for 4 slices"):
        create_super_volume(tr, vol[:3].clone(), None, grid=_grid(4, 10, 1.5625))


# ---- 7: nothing else moved -------------------------------------------------------------------------------------------------------------
def _parent_create_super_volume(trainer, images, alpha_range, use_original=False, labels=None, to_cpu=True):
    """The body of generate_hr_volumes.create_super_volume as it was before it took ``grid``."""
    from superresolution_aniso_mri_amd import _hip, ops
    from superresolution_aniso_mri_amd.generate_hr_volumes import _encode, _interleave, _no_label_model
    if images.dim() == 3:
        images = torch.unsqueeze(images, dim=1)
    with_labels = labels is not None
    if with_labels and labels.dim() == 3:
        labels = torch.unsqueeze(labels, dim=1)
    dev = trainer.args["device"]
    vol = images.float().to(dev)
    if with_labels:
        if tuple(labels.shape) != tuple(images.shape):
            raise ValueError("labels %s do not match the images %s" % (tuple(labels.shape), tuple(images.shape)))
        vol = torch.cat([vol, labels.float().to(dev)], dim=1)
    Z, _, H, W = vol.shape
    n = len(alpha_range)
    out_labels = None
    with torch.no_grad():
        lat = _encode(trainer, vol)
        recon = vol if use_original else trainer.decode(lat, use_sr_model=True)
        if with_labels and not use_original and not isinstance(recon, dict):
            raise ValueError("labels were given, but this model has no label head (MultiChannelAE is the one that has)")
        if not with_labels:
            _no_label_model(recon)
        dec = None
        if Z > 1 and n > 0:
            model = trainer._use_sr_model(True)
            model.eval()
            dec = model.decode_mixes(lat, [float(a) for a in alpha_range]) if hasattr(model, "decode_mixes") else None
            if dec is None:
                zpair = torch.cat([lat[1:], lat[:-1]], dim=0)
                mixes = torch.cat([ops.lerp_mix(zpair, float(a), float(1 - a)) for a in alpha_range], dim=0)
                dec = trainer.decode(mixes, use_sr_model=True)
            if with_labels and not isinstance(dec, dict):
                raise ValueError("labels were given, but this model has no label head (MultiChannelAE is the one that has)")
        if with_labels:
            kept = vol[:, 1] if use_original else recon["pred_labels"][:, 0].float()
            synth = None if dec is None else dec["pred_labels"][:, 0].float()
            out_labels = _interleave(kept, synth, n, (-3.0e38, 3.0e38))
            if not use_original:
                out_labels = out_labels.long()
            recon = vol[:, 0:1] if use_original else recon["image"]
            dec = None if dec is None else dec["image"]
        out = _interleave(recon[:, 0], dec, n, (0.0, 1.0))
    if to_cpu:
        out = out.cpu()
        out_labels = None if out_labels is None else out_labels.cpu()
        if vol.is_cuda:
            _hip.check_device_watchdogs("create_super_volume")
    return {"upsampled_image": out, "upsampled_labels": out_labels}


@pytest.mark.parametrize("use_original", [True, False])
def test_integer_path_is_what_it_was(single, multi, use_original):
    from superresolution_aniso_mri_amd.generate_hr_volumes import create_super_volume
    for n in (3, 6):
        alphas = np.linspace(0, 1, n + 2)[1:-1]
        tr, vol = single
        a = create_super_volume(tr, vol.clone(), alphas, use_original=use_original)
        b = _parent_create_super_volume(tr, vol.clone(), alphas, use_original=use_original)
        assert torch.equal(gm.mg.bits(a["upsampled_image"]), gm.mg.bits(b["upsampled_image"])) and a["upsampled_labels"] is None
        tr, vols = multi
        for images, labels in vols.values():
            a = create_super_volume(tr, images.clone(), alphas, use_original=use_original, labels=labels.clone())
            b = _parent_create_super_volume(tr, images.clone(), alphas, use_original=use_original, labels=labels.clone())
            assert torch.equal(gm.mg.bits(a["upsampled_image"]), gm.mg.bits(b["upsampled_image"]))
            assert a["upsampled_labels"].dtype == b["upsampled_labels"].dtype and torch.equal(a["upsampled_labels"], b["upsampled_labels"])


# ---- 6: the conventional baselines on the same grid ------------------------------------------------------------------------------------------
def _lerp_f64(vol, grid):
    p = grid.position
    i0 = np.minimum(np.floor(p).astype(np.int64), vol.shape[-3] - 1)
    i1 = np.minimum(i0 + 1, vol.shape[-3] - 1)
    t = (p - i0).reshape((-1, 1, 1))
    v = vol.astype(np.float64)
    return (np.take(v, i0, axis=-3) * (1.0 - t) + np.take(v, i1, axis=-3) * t).astype(np.float32)


@pytest.mark.parametrize("shape,s,d", [((5, 32, 32), 10.0, 1.4), ((3, 7, 9), 10.0, 1.5625), ((2, 4, 8, 6), 8.0, 1.25), ((4, 5, 5), 10.0, 10.0 / 3)])
def test_linear_and_nearest_baselines_on_the_grid(tmp_path, shape, s, d):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    vol = np.random.RandomState(len(shape) + shape[-1]).rand(*shape).astype(np.float32)
    grid = _grid(shape[-3], s, d)
    data = tmp_path / "in"
    data.mkdir()
    np.save(str(data / "vol0.npy"), vol)
    base = ["--data_input_dir=" + str(data), "--spacing_z=%r" % s, "--target_spacing_z=%r" % d]
    lin = ghv.main(base + ["--method=linear", "--output_dir=" + str(tmp_path / "lin"), "--save"])[0][1]
    want = _lerp_f64(vol, grid)
    assert lin.shape == want.shape == shape[:-3] + (grid.J,) + shape[-2:] and lin.dtype == np.float32
    print("linear %s s=%g d=%g: max abs diff to the float64 lerp %.3e" % (shape, s, d, float(np.abs(lin - want).max())))
    assert float(np.abs(lin - want).max()) <= 1e-6
    assert np.array_equal(np.load(str(tmp_path / "lin" / "vol0.npy")), lin)
    near = ghv.main(base + ["--method=nearest", "--output_dir=" + str(tmp_path / "near")])[0][1]
    clear = np.abs(grid.position - np.floor(grid.position) - 0.5) > 1e-4
    assert near.shape == want.shape and clear.sum() >= grid.J - 2
    assert np.array_equal(np.take(near, np.flatnonzero(clear), axis=-3), np.take(vol, np.rint(grid.position[clear]).astype(np.int64), axis=-3))


# ---- 5: the command line, end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def experiments(tmp_path_factory):
    """two tiny trained experiments on disk: (single-channel dir, multi-channel dir); model number 1"""
    from superresolution_aniso_mri_amd import train_aesr
    out = str(tmp_path_factory.mktemp("expers"))
    common = ["--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8", "--width=32", "--depth=8",
              "--downsample_steps=2", "--epochs=1", "--lr=0.001", "--ex_loss_weight1=0.05", "--output_dir=" + out, "--synthetic",
              "--iters_per_epoch=2", "--image_mix_loss_func=mse", "--epoch_threshold=0"]
    train_aesr.main(common + ["--dataset=ACDC", "--exper_id=s1"])
    train_aesr.main(common + ["--dataset=ACDCLBL", "--exper_id=m1"])
    return os.path.join(out, "s1"), os.path.join(out, "m1")


def test_cli_target_spacing_end_to_end(experiments, tmp_path, capsys):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd import volume_io
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    src = experiments[0]
    trainer, _ = get_trainer_dynamic(src_path=src, model_nbr=1, eval_mode=True)
    vol = ti_volume(0, (5, 36, 40))
    grid = _grid(5, 10.0, 1.4)
    assert grid.J == 29
    want = ghv.upsample_volume(trainer, vol, None, grid=grid)
    assert want.shape == (29, 36, 40) and np.array_equal(want[np.flatnonzero(grid.is_original)], ghv.array_to_torch(vol)[:, 0].numpy()[grid.source[grid.is_original]])
    # .npy with --spacing_z
    npy = tmp_path / "npy"
    npy.mkdir()
    np.save(str(npy / "vol0.npy"), vol)
    model = ["--exper_dir=" + src, "--model_nbr=1"]
    res = ghv.main(model + ["--data_input_dir=" + str(npy), "--output_dir=" + str(tmp_path / "hr_npy"), "--spacing_z=10", "--target_spacing_z=1.4", "--save"])
    assert np.array_equal(res[0][1], want) and np.array_equal(np.load(str(tmp_path / "hr_npy" / "vol0.npy")), want)
    # a NIfTI file with a geometry of its own: 29 slices, z spacing 1.4, origin and direction as they were
    nii = tmp_path / "nii"
    nii.mkdir()
    sp = (1.5625, 1.5625, 10.0)
    c, sn = np.cos(0.3), np.sin(0.3)
    origin, direction = np.array([-120.5, 33.25, 7.0]), np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
    with gzip.open(str(nii / "vol0.nii.gz"), "wb") as f:
        f.write(_nifti_bytes(vol, sp, origin, direction))
    first = volume_io.read_volume(nii / "vol0.nii.gz")
    assert np.abs(first.origin - origin).max() < 1e-4 and np.abs(first.direction - direction).max() < 1e-6
    ghv.main(model + ["--data_input_dir=" + str(nii), "--output_dir=" + str(tmp_path / "hr_nii"), "--target_spacing_z=1.4", "--save"])
    back = volume_io.read_volume(tmp_path / "hr_nii" / "vol0.nii.gz")
    assert back.array.shape == (29, 36, 40) and np.array_equal(back.array, want)
    assert back.spacing[:2] == first.spacing[:2] and abs(back.spacing[2] - 1.4) < 1e-6
    # the first slice coincides: the origin is the same number, the direction the same up to the fp32 header's rounding of the z column
    assert np.array_equal(back.origin, first.origin) and np.abs(back.direction - first.direction).max() < 1e-6
    # a 4-D file: one grid for the file, every frame what its own 3-D call gives
    nii4 = tmp_path / "nii4"
    nii4.mkdir()
    vol4 = np.stack([vol, ti_volume(1, (5, 36, 40))])
    sp4 = sp + (1.0,)
    volume_io.write_volume(nii4 / "vol0.nii.gz", volume_io.Volume(vol4, sp4, "npy", {}), vol4, sp4)
    ghv.main(model + ["--data_input_dir=" + str(nii4), "--output_dir=" + str(tmp_path / "hr_nii4"), "--target_spacing_z=1.4", "--save"])
    back4 = volume_io.read_volume(tmp_path / "hr_nii4" / "vol0.nii.gz")
    assert back4.array.shape == (2, 29, 36, 40) and abs(back4.spacing[2] - 1.4) < 1e-6
    assert np.array_equal(back4.array[0], want) and np.array_equal(back4.array[1], ghv.upsample_volume(trainer, vol4[1], None, grid=grid))
    # --isotropic --resample: the z spacing written is the in-plane spacing written, the file's own
    capsys.readouterr()
    ghv.main(model + ["--data_input_dir=" + str(nii), "--output_dir=" + str(tmp_path / "hr_iso"), "--isotropic", "--resample", "--save"])
    iso = volume_io.read_volume(tmp_path / "hr_iso" / "vol0.nii.gz")
    giso = _grid(5, 10.0, 1.5625)
    assert iso.spacing[:2] == first.spacing[:2] and abs(iso.spacing[2] - 1.5625) < 1e-6 and iso.array.shape == (giso.J, 36, 40) and giso.J == 26
    assert np.array_equal(iso.array, ghv.upsample_volume_resampled(trainer, vol, None, (1.5625, 1.5625), grid=giso))
    assert "not square" not in capsys.readouterr().out
    assert np.array_equal(iso.origin, first.origin) and np.abs(iso.direction - first.direction).max() < 1e-6
    # pixels that are not square: the smaller spacing, and stdout says so
    rect = tmp_path / "rect"
    rect.mkdir()
    spr = (1.25, 1.5625, 10.0)          # (x, y, z)
    volume_io.write_volume(rect / "vol0.nii.gz", volume_io.Volume(vol, spr, "npy", {}), vol, spr)
    ghv.main(model + ["--data_input_dir=" + str(rect), "--output_dir=" + str(tmp_path / "hr_rect"), "--isotropic", "--save"])
    assert "not square" in capsys.readouterr().out
    out = volume_io.read_volume(tmp_path / "hr_rect" / "vol0.nii.gz")
    assert abs(out.spacing[2] - 1.25) < 1e-6 and out.array.shape == (33, 36, 40)
    assert np.array_equal(out.array, ghv.upsample_volume(trainer, vol, None, grid=_grid(5, 10.0, 1.25)))


def test_cli_target_spacing_with_labels(experiments, tmp_path):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd.data_synth import synthetic_labelled_batch
    src = experiments[1]
    b = synthetic_labelled_batch(5, 32, 32, seed=3)["slice_between"]
    data, labs = tmp_path / "vols", tmp_path / "labels"
    data.mkdir()
    labs.mkdir()
    np.save(str(data / "vol0.npy"), b[:, 0].numpy())
    np.save(str(labs / "vol0.npy"), b[:, 1].numpy().astype(np.uint8))
    base = ["--exper_dir=" + src, "--model_nbr=1", "--data_input_dir=" + str(data), "--labels_input_dir=" + str(labs), "--spacing_z=10", "--save"]
    res = ghv.main(base + ["--target_spacing_z=1.4", "--output_dir=" + str(tmp_path / "hr")])
    hr, hl = np.load(str(tmp_path / "hr" / "vol0.npy")), np.load(str(tmp_path / "hr" / "vol0_labels.npy"))
    grid = _grid(5, 10.0, 1.4)
    assert len(res) == 2 and hr.shape == hl.shape == (29, 32, 32) and hr.dtype == np.float32 and hl.dtype == np.uint8
    assert hr.min() >= 0 and hr.max() <= 1 and hl.max() <= 3
    orig = np.flatnonzero(grid.is_original)
    assert np.array_equal(hl[orig], b[:, 1].numpy().astype(np.uint8)[grid.source[orig]])
    assert np.array_equal(hr[orig], b[:, 0].numpy()[grid.source[orig]])
    # the clean-up of the label volume works on the new grid as on the old one
    ghv.main(base + ["--target_spacing_z=1.4", "--output_dir=" + str(tmp_path / "hr_lc"), "--largest_component", "--min_component_size=4"])
    lc = np.load(str(tmp_path / "hr_lc" / "vol0_labels.npy"))
    assert lc.shape == hl.shape and lc.dtype == np.uint8 and np.array_equal(np.load(str(tmp_path / "hr_lc" / "vol0.npy")), hr)
    assert ((lc == hl) | (lc == 0)).all()
    with pytest.raises(SystemExit):          # a multi-channel model without its label volumes is refused as before
        ghv.main(["--exper_dir=" + src, "--model_nbr=1", "--data_input_dir=" + str(data), "--spacing_z=10", "--target_spacing_z=1.4",
                  "--output_dir=" + str(tmp_path / "hr2")])


def ti_volume(seed, shape, scale=900.0):
    """a smooth blob that moves from slice to slice plus noise, unnormalised intensities (as test_gpu_inplane.py's volumes)"""
    z, h, w = shape
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    vol = np.stack([np.exp(-((yy - h * (0.4 + 0.03 * k)) ** 2 + (xx - w * 0.5) ** 2) / (0.05 * h * w)) for k in range(z)])
    return ((vol * 0.8 + 0.1 * g.rand(z, h, w)) * scale).astype(np.float32)
