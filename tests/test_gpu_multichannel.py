"""-m gpu: the multi-channel (image + label map) auto-encoder on the device.

Kernel level -- aesr_softmax_dice_fwd / _bwd (csrc/seg_head.hip, include/aesr_hip_seg.h) against the float64 restatement
``test_multichannel_golden.softmax_dice_f64``:
    probabilities 1e-6 abs (a few fp32 roundings on [0, 1]); sums and loss 2e-6 rel (fp32 partials of <= 2^16 non-negative terms, fp64
    combine); d(logits) rel-L2 1e-5 (the project's bound for elementwise chains); arg-max exact for the same probabilities, ties to the
    lowest class; two runs bit-identical; guard bands, NaN / 3e38 poisons and pointers shifted by 4, 8 and 12 bytes.
Model and trainers against the reference's own modules (tests/make_golden_multichannel.py), with tests/test_gpu_acai.py's bounds: first-step
losses 2e-5 rel, later steps 5e-3; image / soft_probs / z rel-L2 1e-5; first-step gradients rel-L2 2e-4; final parameters and running
statistics by the two-part rule of test_gpu_acai.py; num_batches_tracked and the model's train / eval flag after ``train()`` exact;
predicted labels equal at every pixel whose reference gap between the two largest probabilities is >= 1e-4, of which at most 1 % may
fall short.  Then both ``create_super_volume(labels=...)``, the checkpoint round trip and the command lines."""
import os
import types

import numpy as np
import pytest
import torch

import memguard as mg
import test_multichannel_golden as tm

pytestmark = pytest.mark.gpu
GOLDEN = tm.GOLDEN
GUARDED_ENTRIES = ("aesr_softmax_dice_fwd", "aesr_softmax_dice_bwd")
EXEMPT = {"aesr_softmax_dice_workspace_floats": "host arithmetic on four integers: returns a size, touches no memory"}
MIN_GAP, MAX_EXCLUDED = 1e-4, 0.01
G_UP = 0.37          # upstream gradient of the loss in the kernel tests


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def close_rel(got, want, tol):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return bool(((got - want).abs() <= tol * want.abs()).all())


# ---- kernel level --------------------------------------------------------------------------------------------------------------------
def make_case(K, N, H, W):
    g = torch.Generator().manual_seed(1000 * K + 100 * N + H + W)
    logits = torch.randn(N, H, W, K, generator=g) * 2.0
    labels = torch.randint(0, K, (N, H, W), generator=g).float()
    if H * W > 1:
        labels[0][labels[0] == K - 1] = 0.0          # sample 0 lacks the last class ...
        labels[0, 0, 0] = float(K)                    # ... and has one label outside [0, K)
        if N > 1:
            labels[N - 1] = 1.0                        # the last sample is one class only
    return logits, labels


def lowest_argmax(probs_nhwc):
    p = probs_nhwc.cpu()
    K = p.shape[-1]
    return torch.where(p == p.max(-1, keepdim=True).values, torch.arange(K), K).min(-1).values.int()


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (28, 28), (40, 36), (64, 65)])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [3, 4, 8])
def test_softmax_dice_kernels_vs_float64(K, N, H, W):
    from superresolution_aniso_mri_amd import _hip, ops
    logits, labels = make_case(K, N, H, W)
    ref = tm.softmax_dice_f64(logits.permute(0, 3, 1, 2), labels, g=G_UP)
    want_sums = torch.stack([ref["I"], ref["R"], ref["P"]], dim=1)
    assert _hip.lib.aesr_softmax_dice_workspace_floats(N, H, W, K) == N * ((H * W + 1023) // 1024) * 3 * K
    first = None
    for layout in ("contiguous", "channel 1 of an NCHW batch", "again"):
        if layout == "contiguous" or layout == "again":
            lab = labels.cuda()
        else:
            x = torch.full((N, 2, H, W), float("nan")).cuda()
            x[:, 1] = labels.cuda()
            lab = x[:, 1]
            view, stride = ops._label_view(lab, N, H, W)
            assert view.data_ptr() == x.data_ptr() + 4 * H * W and stride == (2 * H * W if N > 1 else H * W)      # read in place
        lg = logits.cuda().requires_grad_(True)
        saved = mg.bits(lg)
        loss, probs, amax, sums = ops.softmax_dice(lg, lab, want_argmax=True, return_sums=True)
        (loss * G_UP).backward()
        torch.cuda.synchronize()
        mg.assert_unchanged(lg, saved, "logits")
        got = (mg.bits(probs), mg.bits(amax), mg.bits(sums), mg.bits(loss), mg.bits(lg.grad))
        if first is not None:
            assert all(torch.equal(a, b) for a, b in zip(got, first)), "%s: not bit-identical to the first run" % layout
            continue
        first = got
        e_p = float((probs.double().cpu() - ref["probs"].permute(0, 2, 3, 1)).abs().max())
        e_g = rel_l2(lg.grad, ref["dlogits"].permute(0, 2, 3, 1))
        print("K=%d N=%d %dx%d: probs %.2e abs, loss %.2e rel, dlogits %.2e rel-L2" %
              (K, N, H, W, e_p, abs(float(loss) - float(ref["loss"])) / abs(float(ref["loss"])), e_g))
        assert e_p <= 1e-6
        assert close_rel(sums, want_sums, 2e-6) and torch.equal(sums[:, 1].cpu(), ref["R"])          # counts are exact
        assert close_rel(loss, ref["loss"], 2e-6)
        assert e_g <= 1e-5
        assert torch.equal(amax.cpu(), lowest_argmax(probs))
        top2 = ref["probs"].topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) >= MIN_GAP
        assert torch.equal(amax.cpu().long()[clear], ref["probs"].argmax(1)[clear])
        if H * W > 1:
            assert float(sums[0, 1, K - 1]) == 0 and float(sums[:, 1].sum()) == N * H * W - 1
            if N > 1:
                assert float(sums[N - 1, 1, 1]) == H * W
        # inference: no labels, the same probabilities and arg-max
        p2, a2 = ops.softmax_argmax(lg.detach())
        assert torch.equal(mg.bits(p2), got[0]) and torch.equal(mg.bits(a2), got[1])


def test_argmax_ties_go_to_the_lowest_class():
    from superresolution_aniso_mri_amd import ops
    for K in (3, 4, 8):
        z = torch.zeros(2, 5, 7, K).cuda()
        p, a = ops.softmax_argmax(z)
        assert not a.any() and torch.equal(p, torch.full_like(p, 1.0 / K))
        z[..., 1], z[..., 2] = 3.0, 3.0
        assert bool((ops.softmax_argmax(z)[1] == 1).all())
        z[..., K - 1] = 3.0
        z[..., 1] = 0.0
        assert bool((ops.softmax_argmax(z)[1] == 2).all())
    # large logits: the row maximum is subtracted
    big = torch.tensor([[[[1e4, 1e4 - 1.0, -1e4, 0.0]]]]).cuda()
    p, a = ops.softmax_argmax(big)
    assert bool(torch.isfinite(p).all()) and int(a) == 0 and abs(float(p[0, 0, 0, 0]) - 1 / (1 + np.exp(-1.0))) < 1e-6


LEGS = [(mg.POISON_NAN, 0, 0, 0), (mg.POISON_FINITE, 1, 2, 3), (mg.POISON_NAN, 2, 3, 1), (mg.POISON_FINITE, 3, 1, 2)]


@pytest.mark.parametrize("K,N,H,W", [(4, 3, 9, 7), (3, 2, 9, 7), (8, 2, 5, 5), (4, 2, 40, 36)])
def test_guard_bands_poisons_and_offset_pointers(K, N, H, W):
    """Both entry points between guard bands: NaN and 3e38 poisons in every output, every pointer shifted by 4, 8 and 12 bytes (``sums``
    by 8: it holds doubles).  Guards intact, inputs unchanged, every output element written, and the same bits in every leg: the alignment
    of a pointer (16-byte accesses or 4-byte ones) changes nothing."""
    from superresolution_aniso_mri_amd import _hip
    lib, ptr = _hip.lib, _hip.ptr
    logits, labels = make_case(K, N, H, W)
    ref = tm.softmax_dice_f64(logits.permute(0, 3, 1, 2), labels, g=G_UP)
    n, HW = N * H * W * K, H * W
    nws = lib.aesr_softmax_dice_workspace_floats(N, H, W, K)
    f32, dev = torch.float32, "cuda"
    want = None
    for poison, s1, s2, s3 in LEGS:
        g_logits = mg.guarded(n, f32, dev, logits.reshape(-1), s1, "logits")
        g_labels = mg.guarded(N * HW, f32, dev, labels.reshape(-1), s2, "labels")
        g_probs = mg.guarded(n, f32, dev, poison, s3, "probs")
        g_amax = mg.guarded(N * HW, torch.int32, dev, poison, s1, "argmax")
        g_part = mg.guarded(nws, f32, dev, poison, s2, "partial")
        g_sums = mg.guarded(N * 3 * K, torch.float64, dev, poison, s1 % 2, "sums")
        g_loss = mg.guarded(1, f32, dev, poison, s3, "loss")
        g_up = mg.guarded(1, f32, dev, torch.tensor([G_UP]), s1, "gloss")
        g_dl = mg.guarded(n, f32, dev, poison, s2, "dlogits")
        ins = [(g, mg.bits(g.view)) for g in (g_logits, g_labels, g_up)]
        rc = lib.aesr_softmax_dice_fwd(ptr(g_logits.view), ptr(g_labels.view), HW, ptr(g_probs.view), ptr(g_amax.view), ptr(g_part.view),
                                       ptr(g_sums.view), ptr(g_loss.view), N, H, W, K, None)
        assert rc == 0, _hip.last_error()
        mid = [(g, mg.bits(g.view)) for g in (g_probs, g_sums)]
        rc = lib.aesr_softmax_dice_bwd(ptr(g_probs.view), ptr(g_labels.view), HW, ptr(g_sums.view), ptr(g_up.view), ptr(g_dl.view),
                                       N, H, W, K, None)
        assert rc == 0, _hip.last_error()
        torch.cuda.synchronize()
        everything = [g_logits, g_labels, g_probs, g_amax, g_part, g_sums, g_loss, g_up, g_dl]
        mg.assert_guards_intact(everything)
        for g, saved in ins + mid:
            mg.assert_unchanged(g.view, saved, g.name)
        for g in (g_probs, g_amax, g_part, g_sums, g_loss, g_dl):
            left = mg.poison_left(g.view, poison)
            assert left.numel() == 0, "%s: %d element(s) never written, first %d" % (g.name, left.numel(), int(left[0]))
        got = tuple(mg.bits(g.view) for g in (g_probs, g_amax, g_sums, g_loss, g_dl))
        if want is None:
            want = got
            assert float((g_probs.view.double().cpu().reshape(N, H, W, K) - ref["probs"].permute(0, 2, 3, 1)).abs().max()) <= 1e-6
            assert close_rel(g_loss.view, ref["loss"].reshape(1), 2e-6)
            assert rel_l2(g_dl.view.reshape(N, H, W, K), ref["dlogits"].permute(0, 2, 3, 1)) <= 1e-5
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, want)), "K=%d [poison %s, shifts %d %d %d]: differs from leg 1" % (K, poison, s1, s2, s3)
    # inference form: NULL labels touch neither the workspace nor the sums nor the loss
    g_probs = mg.guarded(n, f32, dev, mg.POISON_NAN, 1, "probs")
    g_logits = mg.guarded(n, f32, dev, logits.reshape(-1), 3, "logits")
    assert lib.aesr_softmax_dice_fwd(ptr(g_logits.view), None, 0, ptr(g_probs.view), None, None, None, None, N, H, W, K, None) == 0
    torch.cuda.synchronize()
    mg.assert_guards_intact([g_probs, g_logits])
    assert torch.equal(mg.bits(g_probs.view), want[0])


# ---- the network against the reference's MultiChannelAE ----------------------------------------------------------------------------
def cuda_model(size, rec, prefix="p0/"):
    from superresolution_aniso_mri_amd.networks.acai_multi_channel import MultiChannelAE
    model = MultiChannelAE(tm.small_args(size, device="cuda")).cuda()
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in rec.items() if k.startswith(prefix)})
    return model


@pytest.mark.parametrize("size", tm.SMALL)
def test_model_forward_backward_vs_reference(size):
    from superresolution_aniso_mri_amd import engine, ops
    rec = tm.load("mc_ae_small_%s.npz" % size)
    model = cuda_model(size, rec)
    model.train()
    x = torch.from_numpy(rec["x"]).cuda()
    z = model.encode(x)
    out = model.decode_logits(z)
    loss_ae = ops.mse_loss(out["image"], x[:, 0:1])
    dice, probs, amax = ops.softmax_dice(out["logits"], x[:, 1], want_argmax=True)
    (loss_ae + float(rec["label_weight"]) * dice).backward()
    soft_probs = engine.to_nchw_view(probs)
    errs = dict(z=rel_l2(z, rec["z"]), image=rel_l2(out["image"], rec["image"]), soft_probs=rel_l2(soft_probs, rec["soft_probs"]),
                logits=rel_l2(engine.to_nchw_view(out["logits"]), rec["logits"]))
    print(size, errs, float(loss_ae), float(dice))
    assert tuple(out["image"].shape) == rec["image"].shape and tuple(soft_probs.shape) == rec["soft_probs"].shape
    assert max(errs.values()) < 1e-5, errs
    assert abs(float(loss_ae) - float(rec["loss_ae"])) <= 2e-5 * abs(float(rec["loss_ae"]))
    assert abs(float(dice) - float(rec["loss_label"])) <= 2e-5 * abs(float(rec["loss_label"]))
    for k, p in model.named_parameters():
        assert p.grad is not None and rel_l2(p.grad, rec["grad/" + k]) < 2e-4, k
    sd = model.state_dict()
    for k, v in rec.items():
        if k.startswith("p1/"):
            if "num_batches" in k:
                assert int(sd[k[3:]]) == int(v) == 1, k
            else:
                assert rel_l2(sd[k[3:]], v) < 1e-5, k
    assert torch.equal(amax.cpu(), lowest_argmax(probs))
    # decode(): the reference's interface, soft probabilities that carry a gradient of their own -- the same gradients through DiceLoss
    from superresolution_aniso_mri_amd.kwatsch.dice_loss import DiceLoss
    model2 = cuda_model(size, rec)
    model2.train()
    o2 = model2(x)
    assert sorted(o2) == ["image", "soft_probs"] and torch.equal(mg.bits(o2["soft_probs"]), mg.bits(soft_probs))
    (ops.mse_loss(o2["image"], x[:, 0:1]) + float(rec["label_weight"]) * DiceLoss(4)(o2["soft_probs"], x[:, 1])).backward()
    for (k, p), q in zip(model.named_parameters(), model2.parameters()):
        assert rel_l2(q.grad, p.grad) < 1e-4, k
    # eval mode: labels with the probabilities, int64 [N, 1, H, W]
    model.eval()
    d = model.decode_labels(model.encode(x))
    assert d["pred_labels"].dtype == torch.int64 and tuple(d["pred_labels"].shape) == (x.shape[0], 1) + tuple(x.shape[2:])
    assert torch.equal(d["pred_labels"][:, 0].cpu().int(), lowest_argmax(d["soft_probs"].permute(0, 2, 3, 1)))


# ---- the trainers against the reference's own train() --------------------------------------------------------------------------------
def trainer_args(model, mix, **over):
    from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig
    args = dict(model=model, dataset="ACDCLBL", device="cuda", lr=1e-3, weight_decay=0.0, epochs=10, width=32, latent_width=8, depth=8,
                latent=16, ex_loss_weight1=0.05, use_percept_loss=False, get_masks=False, use_loss_annealing=False,
                use_extra_latent_loss=False, epoch_threshold=100, ae_class="MultiChannelAE", image_mix_loss_func=mix,
                vgg_weights="synthetic-hash")
    args.update(over)
    for k, v in NetworkConfig(model, dataset="ACDCLBL", ae_class="MultiChannelAE").architecture.items():
        args.setdefault(k, v)
    return args


def make_trainer(model, mix, state, **over):
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    tr = get_trainer_dynamic(trainer_args(model, mix, **over))
    tr.model.load_state_dict(state)
    return tr


def labels_agree(got, want, ref_probs, what):
    """equal at every pixel whose reference top-two gap is >= MIN_GAP; at most MAX_EXCLUDED of the pixels may fall short of it"""
    top2 = torch.from_numpy(ref_probs).topk(2, dim=1).values
    keep = ((top2[:, 0] - top2[:, 1]) >= MIN_GAP)[:, None]
    got, want = torch.as_tensor(got).cpu().long(), torch.as_tensor(want).long()
    excluded, differ = 1 - float(keep.float().mean()), int((got != want)[keep].sum())
    print("%s: %.4f of the pixels excluded, %d of the others differ (%d anywhere)" % (what, excluded, differ, int((got != want).sum())))
    assert got.shape == want.shape and got.dtype == torch.int64
    assert excluded <= MAX_EXCLUDED and differ == 0, what


@pytest.mark.parametrize("tag", ["plain", "caisr_mse", "caisr_lpips"])
def test_trainer_steps_vs_reference_trainers(tag):
    rec = tm.load("step_k3_mc_%s.npz" % tag)
    cls = str(rec["trainer_class"])
    tr = make_trainer("ae" if tag == "plain" else "ae_combined", "perceptual" if tag.endswith("lpips") else "mse",
                      {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")})
    assert type(tr).__name__ == cls == ("MultiChannelTrainer" if tag == "plain" else "MultiChannelCAISRTrainer")
    keys = [str(k) for k in rec["loss_keys"]]
    want_keys = ["loss_ae", "loss_ae_dist", "loss_label", "loss_latent_1"] + ([] if tag == "plain" else ["loss_ae_extra", "loss_ae_dist_extra", "loss_ae_dist_labels"])
    assert sorted(keys) == sorted(want_keys)
    n = len(rec["losses"])
    for step in range(n):
        batch = {"image": torch.from_numpy(rec["image_%d" % step]), "slice_between": torch.from_numpy(rec["between_%d" % step])}
        tr.train(batch, keep_predictions=(step == 0))
        tol = 2e-5 if step == 0 else 5e-3
        assert sorted(tr.losses.keys()) == sorted(keys)
        for i, k in enumerate(keys):
            got, want = tr.losses[k][-1], float(rec["losses"][step][i])
            print("%s step %d %-20s got %+.9e want %+.9e rel %.2e" % (tag, step, k, got, want, abs(got - want) / abs(want)))
        for i, k in enumerate(keys):
            assert len(tr.losses[k]) == step + 1
            assert abs(tr.losses[k][-1] - float(rec["losses"][step][i])) <= tol * abs(float(rec["losses"][step][i])), (step, k)
        assert tr.model.training == bool(rec["training_after"]) == (tag != "plain")
        if step == 0:
            pr = tr.train_predictions
            assert rel_l2(pr["reconstruction"], rec["out_0"]) < 1e-5
            assert rel_l2(pr["slice_inbetween_mix"], rec["s_mix_0"]) < 1e-5
            assert rel_l2(pr["z_mix"], rec["z_mix_0"]) < 1e-5
            labels_agree(pr["pred_labels"], rec["pred_labels_0"], rec["soft_probs_0"], "pred_labels")
            labels_agree(pr["label_inbetween_mix"], rec["label_mix_0"], rec["soft_probs_mix_0"], "label_inbetween_mix")
            for k, p in tr.model.named_parameters():
                assert rel_l2(p.grad, rec["grad0/" + k]) < 2e-4, k
    assert tr.iters == int(rec["iters"])
    sd = tr.model.state_dict()
    prefix = "p%d/" % n
    assert {k[len(prefix):] for k in rec if k.startswith(prefix)} == set(sd.keys())
    for k, v in rec.items():
        if not k.startswith(prefix):
            continue
        a, b = sd[k[len(prefix):]].double().cpu().numpy(), v.astype(np.float64)
        if "num_batches" in k:
            assert int(a) == int(b), k          # encoder layers n, decoder and head layers n (plain) or 2 n (CAISR)
            continue
        diff = np.abs(a - b)
        assert diff.max() <= n * 2 * 1e-3 + 1e-6, k
        assert (diff > 2e-4 + 1e-3 * np.abs(b)).mean() <= 0.03, k
    nbt = {k: int(v) for k, v in sd.items() if "num_batches" in k}
    assert nbt["enc.5.num_batches_tracked"] == n and nbt["decoder_head2.2.num_batches_tracked"] == (n if tag == "plain" else 2 * n)


@pytest.mark.parametrize("tag", ["plain", "caisr_lpips"])
def test_first_optimizer_step_is_adam(tag):
    """The first optimizer step, element by element, against -lr * g / (|g| + eps) on the fixture's ``grad0/*`` (tests/adam_util.py:
    first_step_check; as tests/test_gpu_step.py::test_first_optimizer_step_is_adam): every trainable tensor, >= 75 % of each."""
    import adam_util as au
    rec = tm.load("step_k3_mc_%s.npz" % tag)
    tr = make_trainer("ae" if tag == "plain" else "ae_combined", "perceptual" if tag.endswith("lpips") else "mse",
                      {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")})
    group = tr.opt_ae.param_groups[0]
    assert group["lr"] == 1e-3 and float(tr.opt_ae.dev_state[0]) == 0.0
    p0 = {k: p.detach().cpu().numpy().copy() for k, p in tr.model.named_parameters() if p.requires_grad}
    tr.train({"image": torch.from_numpy(rec["image_0"]), "slice_between": torch.from_numpy(rec["between_0"])}, keep_predictions=False)
    assert float(tr.opt_ae.dev_state[0]) == 1.0                                       # one optimizer step per train()
    p1 = {k: p.detach().cpu().numpy().copy() for k, p in tr.model.named_parameters() if p.requires_grad}
    share, where, worst = au.first_step_check(p0, p1, {k[6:]: v for k, v in rec.items() if k.startswith("grad0/")}, group["lr"], group["eps"],
                                              group["weight_decay"])
    print("mc %s: first step within %.4f lr of -lr g / (|g| + eps); smallest share compared %.3f (%s)" % (tag, worst, share, where))


def test_trainers_are_single_process_and_eval_steps_do_not_move_parameters():
    rec = tm.load("step_k3_mc_caisr_mse.npz")
    tr = make_trainer("ae_combined", "mse", {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")})
    batch = {"image": torch.from_numpy(rec["image_0"]), "slice_between": torch.from_numpy(rec["between_0"])}
    before = {k: mg.bits(v) for k, v in tr.model.state_dict().items()}
    tr.train(batch, keep_predictions=False, eval_mode=True)
    assert all(torch.equal(mg.bits(v), before[k]) for k, v in tr.model.state_dict().items())
    tr.dp = types.SimpleNamespace(active=True)
    with pytest.raises(NotImplementedError, match="single-process"):
        tr.train(batch)
    with pytest.raises(NotImplementedError, match="single-process"):
        tr.validate(batch)


def test_validate_logs_and_checkpoint_round_trip(tmp_path):
    from superresolution_aniso_mri_amd.kwatsch.common import saveExperimentSettings
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    rec = tm.load("step_k3_mc_caisr_mse.npz")
    src = tmp_path / "exp"
    (src / "models").mkdir(parents=True)
    tr = make_trainer("ae_combined", "mse", {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")},
                      dir_models=str(src / "models"), dir_images=str(src), output_dir=str(src))
    batch = {"image": torch.from_numpy(rec["image_0"]), "slice_between": torch.from_numpy(rec["between_0"])}
    tr.train(batch)
    res = tr.validate(batch)
    assert sorted(res) == ["img_grid_recons", "loss_ae", "pred_label_grid"] and res["pred_label_grid"].shape == res["img_grid_recons"].shape
    assert sorted(tr.losses_test.keys()) == ["loss_ae", "loss_ae_dist", "loss_ae_dist_extra", "loss_ae_dist_labels", "loss_ae_extra", "loss_label",
                                             "loss_latent_1"]
    assert all(len(v) == 1 and np.isfinite(v[-1]) for v in tr.losses_test.values()) and not tr.model.training
    assert tr.test_predictions["pred_labels"].dtype == torch.int64
    # 17 images: the chunked path gives the same reconstruction
    big = {"image": torch.cat([batch["image"]] * 5)[:18], "slice_between": torch.cat([batch["slice_between"]] * 5)[:9]}
    tr.validate(big, generate_images=False)
    assert rel_l2(tr.test_predictions["img_recons"][:4], tr.predict(batch["image"])["image"]) < 1e-6
    saveExperimentSettings(dict(tr.args), str(src / "settings.yaml"))
    tr.save_models(str(src / "models" / "3.models"), 3)
    ck = torch.load(str(src / "models" / "3.models"), map_location="cpu")
    assert list(ck["model_dict_ae"].keys()) == list(tr.model.state_dict().keys()) and ck["epoch"] == 3
    assert len(ck["optimizer_dict_ae"]["state"]) == len(list(tr.model.parameters()))
    ev, args = get_trainer_dynamic(src_path=str(src), model_nbr=3, eval_mode=True)
    assert type(ev).__name__ == "MultiChannelCAISRTrainer" and args["ae_class"] == "MultiChannelAE" and args["nclasses"] == 4
    a, b = tr.predict(batch["image"]), ev.predict(batch["image"])
    assert sorted(a) == sorted(b) == ["image", "pred_labels", "soft_probs"]
    for k in a:
        assert torch.equal(mg.bits(a[k]), mg.bits(b[k])), k


# ---- volumes -----------------------------------------------------------------------------------------------------------------------
def reference_image_slices(vol, tag, kept, n, remain):
    """The fixture's image volume as the reference meant it.  With ``use_original=True`` the reference takes the kept slots from its
    two-channel input (``recon_volume = images`` after the label maps were concatenated to it, evaluate/common.py:176,192), so every kept
    image slice is followed by its own label map in 'upsampled_image': (kept - 1) blocks of [image, label map, n in-between slices], then
    [image, label map], then the remainder slices.  Those label-map slices are dropped here; every other slice is compared as it is."""
    if tag != "eval_orig":
        return vol
    body = (kept - 1) * (n + 2) + 2
    assert vol.shape[0] == body + remain
    return vol[[i for i in range(body) if i % (n + 2) != 1] + list(range(body, body + remain))]


def test_super_volumes_with_labels_vs_reference():
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd.evaluate import common as ec
    from superresolution_aniso_mri_amd.kwatsch import img_interpolation as ii
    rec = tm.load("supervolume_labels.npz")
    assert float(rec["min_gap"]) >= MIN_GAP          # no pixel of this fixture is excluded: every label must agree
    tr = make_trainer("ae_combined", "mse", {k[2:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p/")})
    tr.model.eval()
    alphas, steps = rec["alpha_range"], int(rec["downsample_steps"])
    n = len(alphas)
    for Z in (5, 6):
        images, labels = torch.from_numpy(rec["Z%d/images" % Z]), torch.from_numpy(rec["Z%d/labels" % Z])
        outs = {"hr": ghv.create_super_volume(tr, images.clone(), alphas, labels=labels.clone())}
        for tag, uo in (("eval_orig", True), ("eval_recon", False)):
            outs[tag] = ec.create_super_volume(tr, images.clone(), alpha_range=alphas, labels=labels.clone(), downsample_steps=steps,
                                               use_original=uo, generate_inbetween_slices=True)
        for tag, out in outs.items():
            want_i, want_l = rec["Z%d/%s/image" % (Z, tag)], rec["Z%d/%s/labels" % (Z, tag)]
            want_i = reference_image_slices(want_i, tag, len(range(0, Z - (Z - 1) % steps, steps)), n, (Z - 1) % steps)
            got_i, got_l = out["upsampled_image"], out["upsampled_labels"]
            assert tuple(got_i.shape) == want_i.shape and tuple(got_l.shape) == want_l.shape, (Z, tag)
            assert not got_i.is_cuda and not got_l.is_cuda
            err = rel_l2(got_i, want_i)
            print("Z=%d %-10s %d slices, image rel-L2 %.2e, labels differing %d" % (Z, tag, got_i.shape[0], err, int((got_l.double().numpy() != want_l).sum())))
            assert err < 1e-5
            assert np.array_equal(got_l.double().numpy(), want_l.astype(np.float64)), (Z, tag)
        # slot order and remainder slices
        kept = labels[:Z - (Z - 1) % steps:steps]
        lo = outs["eval_orig"]["upsampled_labels"]
        remain = (Z - 1) % steps
        body = lo[:lo.shape[0] - remain]
        assert body.shape[0] == (kept.shape[0] - 1) * (n + 1) + 1 and torch.equal(body[::n + 1], kept)
        assert remain == (1 if Z == 6 else 0) and (remain == 0 or torch.equal(lo[-remain:], labels[-remain:]))
        assert outs["eval_recon"]["upsampled_labels"].dtype == (torch.float32 if remain else torch.int64)
        assert outs["hr"]["upsampled_labels"].dtype == torch.int64 and outs["hr"]["upsampled_labels"].shape[0] == (Z - 1) * (n + 1) + 1
        # one alpha at a time: the same in-between slices and label maps
        vol = torch.cat([images[:, None], labels[:, None]], dim=1)
        for fn in (ghv.latent_space_interp, ii.latent_space_interp):
            r = fn(float(alphas[1]), tr, vol[1:], vol[:-1], with_labels=True)
            assert torch.equal(r["inter_label"][:, 0], outs["hr"]["upsampled_labels"][2::n + 1])
            assert rel_l2(r["inter_image"][:, 0].clamp(0, 1), outs["hr"]["upsampled_image"][2::n + 1]) < 1e-5
    with pytest.raises(ValueError, match="multi-channel"):
        ghv.create_super_volume(tr, torch.rand(3, 2, 32, 32), alphas)


# ---- command lines -----------------------------------------------------------------------------------------------------------------
def test_train_then_generate_with_labels(tmp_path):
    from superresolution_aniso_mri_amd import generate_hr_volumes, train_aesr
    from superresolution_aniso_mri_amd.data_synth import synthetic_labelled_batch
    out = str(tmp_path / "expers")
    tr = train_aesr.main(["--dataset=ACDCLBL", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16",
                          "--latent_width=8", "--width=32", "--depth=8", "--downsample_steps=2", "--epochs=2", "--lr=0.001",
                          "--ex_loss_weight1=0.05", "--exper_id=m1", "--output_dir=" + out, "--synthetic", "--iters_per_epoch=3",
                          "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    src = os.path.join(out, "m1")
    assert type(tr).__name__ == "MultiChannelCAISRTrainer" and type(tr.model).__name__ == "MultiChannelAE"
    assert os.path.isfile(os.path.join(src, "settings.yaml")) and os.path.isfile(os.path.join(src, "models", "2.models"))
    assert tr.iters == 1 + 6 and np.isfinite(tr.mean_losses["loss_label"][-1]) and np.isfinite(tr.mean_losses_test["loss_ae_dist_labels"][-1])
    b = synthetic_labelled_batch(5, 32, 32, seed=3)["slice_between"]
    data, labs = tmp_path / "vols", tmp_path / "labels"
    data.mkdir()
    labs.mkdir()
    np.save(str(data / "vol0.npy"), b[:, 0].numpy())
    np.save(str(labs / "vol0.npy"), b[:, 1].numpy().astype(np.uint8))
    res = generate_hr_volumes.main(["--exper_dir=" + src, "--model_nbr=2", "--num_interpolations=3", "--data_input_dir=" + str(data),
                                    "--labels_input_dir=" + str(labs), "--output_dir=" + str(tmp_path / "hr"), "--save"])
    hr, hl = np.load(str(tmp_path / "hr" / "vol0.npy")), np.load(str(tmp_path / "hr" / "vol0_labels.npy"))
    assert len(res) == 2 and hr.shape == hl.shape == (17, 32, 32) and hr.dtype == np.float32 and hl.dtype == np.uint8
    assert hr.min() >= 0 and hr.max() <= 1 and hl.max() <= 3 and np.array_equal(hl[::4], b[:, 1].numpy().astype(np.uint8))
    with pytest.raises(SystemExit):          # a multi-channel model without its label volumes is refused
        generate_hr_volumes.main(["--exper_dir=" + src, "--model_nbr=2", "--num_interpolations=3", "--data_input_dir=" + str(data),
                                  "--output_dir=" + str(tmp_path / "hr2")])
    with pytest.raises(NotImplementedError, match="label-aware"):
        train_aesr.main(["--dataset=ACDCLBL", "--model=ae", "--downsample_steps=2", "--exper_id=m2", "--output_dir=" + out,
                         "--volumes_dir=" + str(data)])
