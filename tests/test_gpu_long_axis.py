"""-m gpu: evaluation in long-axis views (eval_axis 1 and 2).  The view kernel (aesr_long_axis_views, csrc/long_axis.hip) against
torch.swapaxes bit for bit; ``compute_{ssim,psnr,vif,lpips}_for_batch(eval_axis=k)`` against the reference's own results
(tests/golden/long_axis.npz, tests/make_golden_long_axis.py) with the tolerances tests/test_gpu_metrics.py uses for the same kernels at
axis 0 -- the swap is a copy and adds no rounding -- and the number of scored slices exactly; the error cases; model selection."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = {"ssim": 1e-9, "psnr": 1e-8, "vif": 1e-10}          # absolute; 1e-8 dB is what 1e-9 relative on the MSE allows
CASES = ["v6x40x48", "v10x33x47", "v30x64x56", "lowvif", "allblack"]


def _fixture():
    return dict(np.load(os.path.join(HERE, "golden", "long_axis.npz")))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pair(shape, seed):
    """Volume pair whose reference has zeroed bands (black slices in both views), a -0.0 row and one black slice per view broken by a
    single non-zero element."""
    z, h, w = shape
    g = torch.Generator().manual_seed(seed)
    ref, rec = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    ref[:, :min(3, h), :] = 0.0
    ref[:, :, w - min(4, w):] = 0.0
    ref[:, 0, :] = -0.0
    if h >= 2:
        ref[z - 1, 1, w - 1] = 1e-30              # slice h = 1 (axis 1) and slice w = W - 1 (axis 2) are not black: one element each
    return ref, rec


def _expected(v, axis):
    return torch.swapaxes(v, 0, axis).contiguous()


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("shape", [(6, 40, 48), (10, 33, 47), (30, 64, 56), (1, 7, 9), (3, 1, 5), (65, 17, 130), (30, 224, 224), (130, 20, 70),
                                   (40, 9, 260)])
def test_views_bitwise(shape, axis):
    from evaluate.metrics import long_axis_views
    ref, rec = _pair(shape, seed=shape[0] * 1000 + shape[1] * 10 + shape[2])
    ref, rec = ref.cuda(), rec.cuda()
    ref_view, rec_view, black = long_axis_views(ref, rec, axis)
    want_ref, want_rec = _expected(ref, axis), _expected(rec, axis)
    assert ref_view.is_cuda and ref_view.is_contiguous() and tuple(ref_view.shape) == tuple(want_ref.shape)
    assert torch.equal(_bits(ref_view), _bits(want_ref)) and torch.equal(_bits(rec_view), _bits(want_rec))
    want_black = (want_ref == 0).flatten(1).all(1).cpu().numpy()
    assert black.dtype == np.bool_ and np.array_equal(black, want_black), (black, want_black)
    if shape[1] >= 4 and shape[2] >= 5:
        assert want_black.sum() == ((3 - 1) if axis == 1 else (4 - 1))          # the bands minus the slice with the single element


def test_views_from_unaligned_storage():
    """W % 4 == 0 but the volumes start 4 bytes into their allocations: the 16-byte row path must not be taken."""
    from evaluate.metrics import long_axis_views
    shape = (5, 12, 16)
    n = shape[0] * shape[1] * shape[2]
    ref, rec = _pair(shape, seed=77)
    bufs = [torch.zeros(n + 1, device="cuda") for _ in range(2)]
    a, b = bufs[0][1:].view(shape), bufs[1][1:].view(shape)
    a.copy_(ref)
    b.copy_(rec)
    assert a.data_ptr() % 16 == 4 and a.is_contiguous()
    for axis in (1, 2):
        ref_view, rec_view, black = long_axis_views(a, b, axis)
        assert torch.equal(_bits(ref_view), _bits(_expected(a, axis))) and torch.equal(_bits(rec_view), _bits(_expected(b, axis)))
        assert np.array_equal(black, (_expected(a, axis) == 0).flatten(1).all(1).cpu().numpy())


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("tag", CASES)
def test_metrics_vs_reference(tag, axis):
    from evaluate.metrics import (compute_psnr_for_batch, compute_ssim_for_batch, compute_vif_for_batch, long_axis_slice_scores)
    fx = _fixture()
    ref, rec = fx[tag + "/ref"], fx[tag + "/rec"]
    fns = {"ssim": compute_ssim_for_batch, "psnr": compute_psnr_for_batch, "vif": compute_vif_for_batch}
    for steps in (0, 2):
        ds = None if steps == 0 else steps
        for name, fn in fns.items():
            key = "%s/axis%d/ds%d/%s" % (tag, axis, steps, name)
            want, count = float(fx[key]), int(fx[key + "_count"])
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)                  # the mean of nothing must not warn
                got = fn(ref, torch.from_numpy(rec), eval_axis=axis, downsample_steps=ds)
                scores, keep = long_axis_slice_scores(name, ref, rec, axis, downsample_steps=ds)
            print(key, got, want, int(keep.sum()), count)
            assert int(keep.sum()) == count, (key, int(keep.sum()), count)          # exactly: no passing by skipping more
            if count == 0:
                assert np.isnan(want) and np.isnan(got), key
            else:
                assert abs(got - want) <= TOL[name], (key, got, want)
                assert got == float(np.mean(scores[keep]))


@pytest.mark.parametrize("axis", [1, 2])
def test_per_slice_scores_equal_the_axis0_kernels_on_a_swapped_copy(axis):
    from evaluate.metrics import long_axis_slice_scores, slice_ssim_psnr, slice_vif
    fx = _fixture()
    for tag in ("v6x40x48", "v30x64x56"):
        ref, rec = torch.from_numpy(fx[tag + "/ref"]).cuda(), torch.from_numpy(fx[tag + "/rec"]).cuda()
        a, b = _expected(ref, axis), _expected(rec, axis)
        ssim, psnr, mse = slice_ssim_psnr(a, b)
        vif = slice_vif(a, b)
        per = long_axis_slice_scores(("ssim", "psnr", "vif"), ref, rec, axis)
        assert np.array_equal(per["ssim"][0], ssim) and np.array_equal(per["psnr"][0], psnr)
        assert np.array_equal(per["psnr"][0], 10.0 * np.log10(1.0 / mse))
        assert np.array_equal(per["vif"][0], vif, equal_nan=True)
        black = (a == 0).flatten(1).all(1).cpu().numpy()
        assert np.array_equal(per["ssim"][1], ~black) and np.array_equal(per["vif"][1], ~black & np.isfinite(vif))


def test_lpips_long_axis():
    from evaluate.metrics import compute_lpips_for_batch
    from superresolution_aniso_mri_amd.lpips.perceptual import PerceptualLoss
    fx = _fixture()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        crit = PerceptualLoss(model="net-lin", net="vgg", use_gpu=True, gpu_ids=[0], device="cuda", vgg_weights="synthetic-hash")
    ref, rec = torch.from_numpy(fx["v30x64x56/ref"]).cuda(), torch.from_numpy(fx["v30x64x56/rec"]).cuda()
    for axis in (0, 1, 2):
        got = compute_lpips_for_batch(ref, rec, eval_axis=axis, criterion=crit)
        if axis != 0:
            assert got == compute_lpips_for_batch(_expected(ref, axis), _expected(rec, axis), criterion=crit)
            ds = compute_lpips_for_batch(ref, rec, eval_axis=axis, downsample_steps=2, criterion=crit)
            assert np.isfinite(ds) and ds != got            # ids 0, 2, ..., 28, 29 (from Z = 30) leave the swapped slices
        want = float(fx["v30x64x56/axis%d/lpips" % axis])
        print("lpips axis", axis, got, want)
        np.testing.assert_allclose(got, want, rtol=2e-5)


def test_errors_and_degenerate_inputs():
    from evaluate.metrics import (compute_lpips_for_batch, compute_psnr_for_batch, compute_ssim_for_batch, compute_vif_for_batch,
                                  long_axis_views)
    from superresolution_aniso_mri_amd import _hip as hip
    g = torch.Generator().manual_seed(3)
    a = torch.rand(4, 40, 48, generator=g)
    b = (a + 0.05 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    with pytest.raises(ValueError, match="4, 48"):
        compute_ssim_for_batch(a, b, eval_axis=1)                 # slices 4 x 48: below the smallest SSIM window the reference uses
    assert np.isfinite(compute_psnr_for_batch(a, b, eval_axis=1)) and np.isfinite(compute_vif_for_batch(a, b, eval_axis=1))
    a6 = torch.rand(6, 40, 48, generator=g)
    with pytest.raises(ValueError, match="16"):
        compute_lpips_for_batch(a6, a6, eval_axis=1, criterion=lambda *args, **kw: pytest.fail("criterion must not be reached"))
    for fn in (compute_ssim_for_batch, compute_psnr_for_batch, compute_vif_for_batch, compute_lpips_for_batch):
        with pytest.raises(ValueError, match="eval_axis"):
            fn(a6, a6, eval_axis=3)
    with pytest.raises(ValueError):
        long_axis_views(a6, a6, 0)
    # the C entry point: argument status, nothing launched (the outputs keep their contents)
    v = a6.cuda()
    out = torch.full((2, v.numel()), 7.0, device="cuda")
    black = torch.full((48,), 9, device="cuda", dtype=torch.uint8)
    call = hip.lib.aesr_long_axis_views
    assert call(hip.ptr(v), hip.ptr(v), hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(black), 6, 40, 48, 0, hip.stream()) == 1
    assert "axis" in hip.last_error()
    assert call(hip.ptr(v), hip.ptr(v), hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(black), 6, 0, 48, 1, hip.stream()) == 1
    assert call(hip.ptr(v), hip.ptr(v), hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(black), 6, 40, 48, 3, hip.stream()) == 1
    assert call(hip.ptr(v), None, hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(black), 6, 40, 48, 1, hip.stream()) == 1
    assert call(hip.ptr(v), hip.ptr(v), hip.ptr(out[0]), hip.ptr(out[1]), hip.ptr(black), 1024, 1024, 1024, 2, hip.stream()) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((black == 9).all())
    # an all-black reference: nothing is scored -> nan, and no warning about the mean of nothing
    zeros = torch.zeros(6, 40, 48)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for fn in (compute_ssim_for_batch, compute_psnr_for_batch, compute_vif_for_batch):
            for axis in (1, 2):
                assert np.isnan(fn(zeros, a6, eval_axis=axis))
    # a 2-D image (also as [1,1,H,W]) ignores eval_axis
    for fn in (compute_ssim_for_batch, compute_psnr_for_batch, compute_vif_for_batch):
        assert fn(a[0], b[0], eval_axis=1) == fn(a[0], b[0], eval_axis=0) == fn(a[0][None, None], b[0][None, None], eval_axis=2)


def test_find_best_val_model_long_axis(tmp_path, capsys):
    """In the manner of test_gpu_model_selection.py::test_find_best_val_model: own tiny checkpoints, every epoch scored in the long-axis
    views.  The all-slices file holds finite rows equal to ``compute_*_for_batch(eval_axis=k)`` of the same synthesised volumes; the
    synthesis file holds NaN rows (the reference's lists stay empty there); axis 0 on the same data is what it was."""
    from evaluate.common import create_super_volume, determine_last_slice
    from evaluate.find_best_model import adjust_and_center_crop, compute_metrics, find_best_val_model
    from evaluate.metrics import compute_psnr_for_batch, compute_ssim_for_batch, compute_vif_for_batch
    from superresolution_aniso_mri_amd import train_aesr
    from superresolution_aniso_mri_amd.data_synth import synthetic_batch
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    out = str(tmp_path / "expers")
    tr = train_aesr.main(["--dataset=ACDC", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16",
                          "--latent_width=8", "--width=32", "--depth=8", "--downsample_steps=2", "--epochs=1", "--lr=0.001",
                          "--ex_loss_weight1=0.05", "--exper_id=m1", "--output_dir=" + out, "--synthetic", "--iters_per_epoch=3",
                          "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    src = os.path.join(out, "m1")
    for it in range(4):
        tr.train(synthetic_batch(4, 32, 32, seed=520 + it), keep_predictions=False)
    tr.save_models(os.path.join(src, "models", "2.models"), 2)
    g = np.random.RandomState(9)
    yy, xx = np.mgrid[0:40, 0:36] / 40.0
    vols = {}
    for p, z in enumerate((9, 8)):
        base = [np.exp(-((yy - 0.3 - 0.04 * k) ** 2 + (xx - 0.5) ** 2) / 0.03) for k in range(z)]
        vols[p] = {"image": (np.stack(base) * 0.8 + 0.05 * g.rand(z, 40, 36)).astype(np.float32), "patient_id": "p%d" % p,
                   "spacing": np.array([8.0, 1.4, 1.4])}
    ev, _ = get_trainer_dynamic(src_path=src, model_nbr=2, eval_mode=True)
    pairs = []
    for v in vols.values():
        img = adjust_and_center_crop(v["image"], 32)
        hr = create_super_volume(ev, torch.from_numpy(img), alpha_range=np.linspace(0, 1, 4)[1:-1], use_original=False, downsample_steps=3,
                                 generate_inbetween_slices=True)["upsampled_image"].numpy()
        last = determine_last_slice(img.shape[0], 3) + 1
        pairs.append((img[:last], hr[:last]))
    fns = (compute_ssim_for_batch, compute_psnr_for_batch, compute_vif_for_batch)
    for axis in (1, 2):
        scores = find_best_val_model(vols, src, epoch_range=[1, 2], ps_evaluate=32, downsample_steps=3, eval_axis=axis)
        assert "Top synthesis" in capsys.readouterr().out
        assert list(scores.keys()) == ["1", "2"] and all(np.isfinite(v).all() for v in scores.values())
        main = np.load(os.path.join(src, "model_perf_1_to_2_axis%d.npz" % axis))
        synth = np.load(os.path.join(src, "model_perf_synth_1_to_2_axis%d.npz" % axis))
        assert sorted(main.files) == ["1", "2"] and sorted(synth.files) == ["1", "2"]
        assert all(synth[e].shape == (3,) and np.isnan(synth[e]).all() for e in synth.files)
        want = [np.mean([fn(a, b, eval_axis=axis) for a, b in pairs]) for fn in fns]
        assert np.array_equal(main["2"], scores["2"]) and np.allclose(main["2"], want, rtol=0, atol=1e-12), (main["2"], want)
        m = compute_metrics(pairs[0][0], pairs[0][1], 3, eval_axis=axis)
        assert sorted(m.keys()) == ["psnr", "ssim", "vif"]
    # axis 0 keeps its path and its numbers
    scores0 = find_best_val_model(vols, src, epoch_range=[1, 2], ps_evaluate=32, downsample_steps=3, eval_axis=0)
    want0 = [np.mean([fn(a, b) for a, b in pairs]) for fn in fns]
    assert np.allclose(scores0["2"], want0, rtol=0, atol=1e-12), (scores0["2"], want0)
    synth0 = np.load(os.path.join(src, "model_perf_synth_1_to_2_axis0.npz"))
    assert np.isfinite(synth0["2"]).all()
    assert "ssim_synth" in compute_metrics(pairs[0][0], pairs[0][1], 3)
