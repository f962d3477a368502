"""-m gpu: the training step and the inference paths AWAY from the freshly initialised state.

Every other trainer-level comparison starts from the reference's initialisation (all biases and BatchNorm betas exactly zero, running
statistics (0, 1), ``num_batches_tracked`` 0) or one optimizer step behind it, and checks gradients against fp64 at the first step only.
Here the same flip-aware check (oracle/routing.py, tests/routing_util.py, as test_gpu_step.test_three_train_steps at step 0) runs

  a. at a randomised state (tests/state_util.randomise_state: biases, betas, running statistics and gammas of a size that shows; negative
     gammas) -- the stem fold with its bias, beta in the pooled-once BatchNorm forms, the running statistics' momentum update;
  b. behind two eager optimizer steps, c. behind three steps of which two are replays of the captured step graph -- HipAdam and a replayed
     graph rewrite the parameters through raw pointers, so the packed forward operand, the transposed data-gradient operand, the Winograd U,
     the folded stem and the flipped cout1 filter are fresh only because ``on_step`` / the replay hook bump ``weights_epoch``.  A stale
     data-gradient operand changes no loss and nothing any other test reads; it changes the gradients checked here by O(1)
     (tests/test_trained_state_reference.py::test_state_one_step_old_is_far_outside_the_bound is that statement on the CPU);
  d. through the eval paths at the randomised state: eval-mode BatchNorm scale / shift fold, the aesr_conv2d_wino_fwd_bn epilogue and the
     linearity argument of aesr_lerp_multi ("the bias is included because the weights add up to 1") with biases that are not zero.

The bounds are the project's own (3e-5 on every parameter gradient, 6e-5 with LPIPS as the reconstruction loss; forward 2e-5 / 1e-5); that
the reference's arithmetic keeps a margin of 3x inside them at exactly these states, batches and seeds is
tests/test_trained_state_reference.py.  Measured values: profiles/trained_state_parity.txt."""
import numpy as np
import pytest
import torch

import state_util as su

pytestmark = pytest.mark.gpu


def build_trainer(case, eval_mode=False):
    """As test_gpu_step.make_trainer builds it, without a fixture: the model's own initialisation under ``torch.manual_seed(case["init"])``."""
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig
    args = dict(model="ae_combined", dataset="ACDC", device="cuda", lr=su.LR, weight_decay=0.0, epochs=10, width=32,
                latent_width=8, depth=8, latent=16, ex_loss_weight1=0.05, use_percept_loss=False, get_masks=False,
                use_loss_annealing=False, use_extra_latent_loss=False, epoch_threshold=100, ae_class="VanillaACAI",
                vgg_weights="synthetic-hash")
    args.update(case["trainer"])
    for k, v in NetworkConfig(args["model"], dataset=args["dataset"]).architecture.items():
        args.setdefault(k, v)
    torch.manual_seed(case["init"])
    return get_trainer_dynamic(args, eval_mode=eval_mode)


def snapshot(trainer):
    return {k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()}


def check_step(trainer, batch, make_oracle_step, percept, record_property=None, passes=2, bound=None):
    """One host-launched step of ``trainer`` on ``batch`` against the oracle.  ``make_oracle_step()`` -> a fresh fp32 OracleStep on a CPU
    snapshot of the trainer's state taken BEFORE this call.  Asserts

      * losses within 2e-5 of the fp64 oracle's, reconstruction and synthesised slice within 1e-5 rel-L2 (the forward bounds of
        test_gpu_step.test_ragged_batch_shapes_vs_oracle);
      * at most 8 of the HIP path's non-smooth decisions differ from the fp64 oracle's own, each a tie (fp64 margin <= 2e-5 of the layer's rms);
      * every parameter gradient within 3e-5 rel-L2 (6e-5 with LPIPS as the reconstruction loss, ``percept``) of the fp64 oracle evaluated
        with the HIP path's decisions;
      * the BatchNorm running statistics behind the step against the oracle's: variances 1e-5 rel-L2, means within 1e-4 of a standard
        deviation, ``num_batches_tracked`` advanced by ``passes`` (the bounds of test_gpu_baseline_parity.test_baseline_configuration_vs_oracle).

    Records the worst gradient error, the number of differing decisions and the fp32 oracle's own error against fp64 (same measure, its
    own decisions).  Returns them as a dict."""
    import routing_util as ru
    from oracle import routing
    before = make_oracle_step().ae.state_dict()
    dec = ru.hip_step_decisions(trainer, batch)
    g_hip = {k: p.grad.detach().clone() for k, p in trainer.model.named_parameters()}
    r_own, g_own, res = ru.oracle64_step(make_oracle_step, batch)
    figures = {}
    for key in ("loss_ae", "loss_ae_dist_extra", "loss_latent_1"):
        got = trainer.losses[key][-1]
        figures[key] = abs(got - res[key]) / abs(res[key])
        print("  %-20s hip %.9g fp64 %.9g rel %.2e" % (key, got, res[key], figures[key]))
    figures["reconstruction"] = su.rel_l2(trainer.train_predictions["reconstruction"], res["out"])
    figures["slice_inbetween_mix"] = su.rel_l2(trainer.train_predictions["slice_inbetween_mix"], res["s_mix"])
    print("  reconstruction rel-L2 %.2e, synthesised slice rel-L2 %.2e" % (figures["reconstruction"], figures["slice_inbetween_mix"]))
    for key in ("loss_ae", "loss_ae_dist_extra", "loss_latent_1"):
        assert figures[key] <= 2e-5, (key, figures[key])
    assert figures["reconstruction"] < 1e-5 and figures["slice_inbetween_mix"] < 1e-5, figures
    # decisions, then gradients under the HIP path's decisions
    diffs = routing.differing_decisions(r_own, dec)
    print("  decisions differing from the fp64 oracle's own: %d\n%s" % (len(diffs), ru.describe(diffs)))
    assert len(diffs) <= 8 and all(d["rel"] <= 2e-5 for d in diffs), "decisions that are not ties:\n" + ru.describe(diffs)
    g_ref = ru.oracle64_step(make_oracle_step, batch, forced=dec)[1] if diffs else g_own
    errs = sorted(((su.rel_l2(g_hip[k], g_ref[k]), k) for k in g_ref), reverse=True)
    print("  gradients vs fp64 under the same decisions, worst: " + ", ".join("%s %.2e" % (k, e) for e, k in errs[:4]))
    # the fp32 CPU oracle's step: the running statistics to compare with, and its own gradient error beside the HIP path's
    r32 = routing.Routing()
    o32 = make_oracle_step()
    o32.train(*su.train_batch(batch), route=r32)
    dec32 = {name: seen[2] for name, seen in r32.seen.items()}
    g_ref32 = ru.oracle64_step(make_oracle_step, batch, forced=dec32)[1] if routing.differing_decisions(r_own, dec32) else g_own
    worst32 = max((su.rel_l2(p.grad, g_ref32[k]), k) for k, p in o32.ae.params.items())
    print("  the fp32 CPU oracle's own worst: %s %.2e" % (worst32[1], worst32[0]))
    figures.update(worst_gradient=errs[0][0], worst_gradient_name=errs[0][1], decisions_differing=len(diffs), fp32_oracle_worst=worst32[0])
    if record_property is not None:
        record_property("worst_gradient_rel_l2_vs_fp64_same_decisions", errs[0][0])
        record_property("decisions_differing_from_fp64", len(diffs))
        record_property("fp32_oracle_worst_gradient_rel_l2_vs_fp64", worst32[0])
    if bound is None:          # (an explicit bound: the control run through the direct fp32 kernels, test_gpu_step.DIRECT_CONTROL)
        bound = su.GRAD_BOUND_PERCEPT if percept else su.GRAD_BOUND
    assert errs[0][0] < bound, errs[:4]
    # running statistics behind the step
    sd = trainer.model.state_dict()
    for k, v in o32.ae.buffers.items():
        if k.endswith("running_var"):
            e = su.rel_l2(sd[k], v)
            assert e < 1e-5, (k, e)
        elif k.endswith("running_mean"):
            std = o32.ae.buffers[k.replace("running_mean", "running_var")].sqrt()
            e = float(((sd[k].cpu() - v).abs() / std).max())
            assert e < 1e-4, (k, e)
        elif "num_batches" in k:
            assert int(sd[k]) == int(v) == int(before[k]) + passes, (k, int(sd[k]), int(v), int(before[k]))
    return figures


@pytest.mark.parametrize("name", sorted(su.CASES))
def test_step_at_a_randomised_state(name, record_property):
    """One step from ``randomise_state``: MSE at 4 triplets of 32x32 and at 3 of 44x28 (partial tiles), the LPIPS synthesis loss, LPIPS as the
    reconstruction loss, three pooling stages, a brain-style batch with per-sample alpha_from / alpha_to.  Measured on the product path
    (profiles/trained_state_parity.txt)."""
    case = su.CASES[name]
    trainer = build_trainer(case)
    state = su.randomise_state(trainer.model.state_dict(), case["state"])
    trainer.model.load_state_dict(state)
    snap = snapshot(trainer)
    for k, v in state.items():
        assert torch.equal(snap[k], v), k
    check_step(trainer, su.case_batch(case), su.oracle_step_maker(case, snap), bool(case.get("percept")), record_property)


@pytest.mark.parametrize("loss", sorted(su.STEPPED))
def test_gradients_after_eager_steps(loss, record_property):
    """Two eager optimizer steps (lr 1e-3, distinct batches) from the model's own initialisation, then the flip-aware check of a third step
    against the oracle built from a snapshot of the state the two steps left: every operand derived from the parameters -- the backward ones
    too -- must be the one of THAT state."""
    case = su.STEPPED[loss]
    trainer = build_trainer(case)
    for s in case["batch_seeds"][:2]:
        trainer.train(su.case_batch(case, seed=s))
    snap = snapshot(trainer)
    check_step(trainer, su.case_batch(case, seed=case["batch_seeds"][2]), su.oracle_step_maker(case, snap), False, record_property)


@pytest.mark.parametrize("loss", sorted(su.STEPPED))
def test_gradients_after_replayed_steps(loss, record_property):
    """One eager step, the capture step and one replay of the captured step graph, then the flip-aware check of a host-launched fourth step
    (``keep_predictions=True`` takes the eager path) against the oracle built from a snapshot of the state the replays left; then one more
    replay: the parameters must equal, bit for bit, those of a twin trainer that ran the same five steps without a graph -- the eager step
    in the middle must not disturb what the captured graph owns."""
    case = su.STEPPED[loss]
    batches = [su.case_batch(case, seed=s) for s in case["batch_seeds"]]
    trainer = build_trainer(case)
    trainer.enable_step_graph(eager_steps=1)
    for b in batches[:3]:
        trainer.train(b, keep_predictions=False)
    assert len(trainer._graphs) == 1
    assert float(trainer.opt_ae.dev_state[0]) == 3.0
    snap = snapshot(trainer)
    check_step(trainer, batches[3], su.oracle_step_maker(case, snap), False, record_property)
    trainer.train(batches[4], keep_predictions=False)
    assert len(trainer._graphs) == 1 and float(trainer.opt_ae.dev_state[0]) == 5.0
    twin = build_trainer(case)
    for i, b in enumerate(batches):
        twin.train(b, keep_predictions=(i == 3))
    assert not hasattr(twin, "_graphs")
    for (k, a), (_, b) in zip(trainer.model.state_dict().items(), twin.model.state_dict().items()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("name", sorted(su.EVAL_CASES))
def test_eval_paths_at_a_randomised_state(name, monkeypatch):
    """An eval-mode trainer with the randomised state: ``create_super_volume`` on a 5-slice 32x32 volume with three alphas, and the eval-mode
    reconstruction of a batch, against the oracle in fp64 with ``train=False`` (rtol 1e-5, atol 2e-6: the bounds of
    test_gpu_inference.test_create_super_volume_vs_reference_loop) -- once with the fused lerp + decode path and once with lerp on the
    latents + a full decoder pass.  ``small``: every eval-mode BatchNorm in the stand-alone scale / shift form; ``wide``: the encoder's in the
    epilogue of aesr_conv2d_wino_fwd_bn (counted)."""
    import routing_util as ru
    from oracle import ae_oracle
    from superresolution_aniso_mri_amd import engine
    from superresolution_aniso_mri_amd.generate_hr_volumes import create_super_volume
    from superresolution_aniso_mri_amd.networks.acai_vanilla import HipAE
    case = su.EVAL_CASES[name]
    trainer = build_trainer(case, eval_mode=True)
    state = su.randomise_state(trainer.model.state_dict(), case["state"])
    trainer.model.load_state_dict(state)
    ae = ru.as_fp64(ae_oracle.OracleAE(su.case_cfg(case), init=False).load_state_dict(state))
    batch = su.case_batch(case, seed=case["batch_seed"])
    vol = torch.cat([batch["image"][:3], batch["slice_between"][:2]], dim=0)          # 5 slices
    alphas = [0.25, 0.5, 0.8]
    epilogues = []
    real_fwd_bn = engine.lib.aesr_conv2d_wino_fwd_bn
    monkeypatch.setattr(engine.lib, "aesr_conv2d_wino_fwd_bn", lambda *a: epilogues.append(1) or real_fwd_bn(*a))
    want = su.oracle_super_volume(ae, vol.double(), alphas).numpy()
    with torch.no_grad():
        want_rec = ae.forward(batch["image"].double(), train=False).numpy()
    fused = create_super_volume(trainer, vol, alphas, use_original=True)["upsampled_image"]
    assert fused.shape == want.shape == (4 * 4 + 1, 32, 32)
    called = []
    orig = HipAE.decode_mixes
    monkeypatch.setattr(HipAE, "decode_mixes", lambda self, z, a: called.append(1) or None)          # -> lerp on latents + full decode
    plain = create_super_volume(trainer, vol, alphas, use_original=True)["upsampled_image"]
    monkeypatch.setattr(HipAE, "decode_mixes", orig)
    assert called
    rec = trainer.predict(batch["image"]).cpu()
    assert bool(epilogues) == bool(case.get("epilogue")), len(epilogues)
    for name, got, ref in (("fused", fused, want), ("plain", plain, want), ("reconstruction", rec, want_rec)):
        d = np.abs(got.double().numpy() - ref)
        print("  %-14s max |diff| %.2e, max |diff| / (2e-6 + 1e-5 |ref|) %.2f" % (name, d.max(), (d / (2e-6 + 1e-5 * np.abs(ref))).max()))
    np.testing.assert_allclose(fused.numpy(), want, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(plain.numpy(), want, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(rec.numpy(), want_rec, rtol=1e-5, atol=2e-6)
    # the synthesised slices are not the clamp's constants and not copies of the originals
    assert float(fused[1].min()) < float(fused[1].max()) and not torch.equal(fused[1], fused[0])
