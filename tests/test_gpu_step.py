"""-m gpu: the full training step (trainer classes on the HIP engine) against vectors made by the reference's OWN trainer classes
(tests/golden/step_k3_*.npz, step_k4_cardiac_anneal.npz, step_probe_c*.npz: oracle/make_golden.py runs AETrainerEndToEnd /
AETrainerExtension1Brain / AEBaseTrainer on the CPU): losses of step 0 (pure forward, rel 2e-5), latents / synthesised slices
(rel-L2 1e-5), first-step gradients (rel-L2 2e-4), parameters and BatchNorm statistics after 3 Adam steps; the BASELINE
configurations at their own size (12 triplets of 160x160, MSE and LPIPS, scales 2 and 3) against the probes and the oracle."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


DIRECT_CONTROL = os.environ.get("AESR_WINO") == "0" and os.environ.get("AESR_WGRAD_WINO") == "0"


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# fixture tag -> (args overrides, lr); every step_k3_* fixture is the reference's OWN trainer class run on the CPU (oracle/make_golden.py)
STEP_CASES = {
    "cardiac_mse": (dict(image_mix_loss_func="mse"), 1e-3),
    "cardiac_lpips": (dict(image_mix_loss_func="perceptual"), 1e-3),
    "brain_lpips": (dict(image_mix_loss_func="perceptual", dataset="OASIS"), 1e-3),
    "cardiac_percept": (dict(use_percept_loss=True), 1e-3),                      # --use_percept_loss: LPIPS reconstruction loss too
    "ae_plain": (dict(model="ae", image_mix_loss_func="mse"), 1e-3),            # plain `ae`: kwatsch/trainer_ae.py:71-109
    "cardiac_mse_s3": (dict(image_mix_loss_func="mse", latent_width=4), 1e-3),  # three pooling stages
    "cardiac_mse_lr1e-5": (dict(image_mix_loss_func="mse"), 1e-5),              # the reference's default learning rate
}


def make_trainer(tag, rec, lr=None, **over):
    from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    kw, lr0 = STEP_CASES.get(tag, (dict(image_mix_loss_func="mse" if tag.endswith("mse") else "perceptual"), 1e-3))
    args = dict(model="ae_combined", dataset="ACDC", device="cuda", lr=lr0 if lr is None else lr, weight_decay=0.0, epochs=10, width=32,
                latent_width=8, depth=8, latent=16, ex_loss_weight1=0.05, use_percept_loss=False, get_masks=False,
                use_loss_annealing=False, use_extra_latent_loss=False, epoch_threshold=100, ae_class="VanillaACAI",
                vgg_weights="synthetic-hash")
    args.update(kw)
    args.update(over)
    for k, v in NetworkConfig(args["model"], dataset=args["dataset"]).architecture.items():
        args.setdefault(k, v)
    trainer = get_trainer_dynamic(args)
    trainer.model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")})
    return trainer


def _batch(rec, step):
    batch = {"image": torch.from_numpy(rec["image_%d" % step]), "slice_between": torch.from_numpy(rec["between_%d" % step])}
    if "alpha_from" in rec:
        batch["alpha_from"], batch["alpha_to"] = torch.from_numpy(rec["alpha_from"]), torch.from_numpy(rec["alpha_to"])
    return batch


def _oracle_step(tag, rec, state=None):
    """The CPU oracle's trainer for a fixture, from the fixture's initial parameters (fp32, Adam at the fixture's learning rate) or from
    ``state`` (a CPU snapshot of a model's state_dict)."""
    import test_oracle_golden as tog
    from oracle import ae_oracle, step_oracle
    kw, lr, _ = tog.STEP_CASES[tag]
    if state is None:
        state = {k[3:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p0/")}
    ae = ae_oracle.OracleAE(tog.small_cfg(tag), init=False).load_state_dict(state)
    return step_oracle.OracleStep(ae, lr=lr, ex_loss_weight1=0.05, vgg_sd=tog.lpips_oracle.hash_vgg16_state(), lin_w=tog._lin_w(), **kw)


def _other_side(a, b):
    """Names and counts of the decisions on which two decision tables (same names, same shapes) disagree."""
    out = {}
    for name, t in a.items():
        n = int((t.to(torch.int64) != b[name].to(torch.int64)).sum())
        if n:
            out[name] = n
    return out


@pytest.mark.parametrize("tag", sorted(STEP_CASES))
def test_three_train_steps(tag, record_property):
    """Three optimisation steps of the HIP trainer classes against three steps of the reference's own trainer classes, at the fixture's EXACT
    input, deterministically.

    The step is piecewise smooth: a LeakyReLU / ReLU input (or two max-pool candidates) within fp32 rounding of a tie may be decided either way
    by two correct evaluations, and the derivative of that one element then differs by O(1).  So the gradient check has two parts
    (oracle/routing.py, tests/routing_util.py):

      * the HIP path's non-smooth decisions are recorded and compared with the oracle's in fp64: at most a handful may differ, each a PROVEN tie
        (fp64 margin below 2e-5 of the layer's rms), and against the fp64 oracle evaluated WITH the HIP path's decisions the first-step gradients
        must agree to 3e-5 (6e-5 with LPIPS as the reconstruction loss) -- a second flip or a real regression cannot hide behind that;
      * against the reference's fixture the bound stays 2e-4 whenever the fixture took the same decisions as the HIP path.  Where it did not
        (``cardiac_percept``: the REFERENCE's fp32 run sits on the far side of one VGG relu1_1 tie, 1.7e-7 from zero in fp64, which moves every
        parameter gradient by ~1e-3; the HIP path decides as fp64 does -- profiles/r06_routing_report.txt), the fixture's gradients are checked against
        the fp64 oracle under the FIXTURE's decisions instead, and the later steps against the oracle's trajectory under the HIP path's decisions:
        the same arithmetic, the same bounds, the other branch of a tie.

    Steps 1 and 2 of every ae_combined fixture that stays on the reference's branch get the same flip-aware check as step 0, against the
    oracle built from a snapshot of the state in front of the step (test_gpu_trained_state.check_step: forward 2e-5 / 1e-5, at most 8
    proven ties, gradients 3e-5, running statistics)."""
    import routing_util as ru
    import test_gpu_trained_state as tgs
    from oracle import routing
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_%s.npz" % tag)))
    lr = STEP_CASES[tag][1]
    plain = tag == "ae_plain"            # plain ``ae``: one pass pair, no synthesis branch; its decisions are not named by the routing oracle
    trainer = make_trainer(tag, rec)
    assert type(trainer).__name__ == str(rec["trainer_class"])
    keys = [str(k) for k in rec["loss_keys"]]
    percept = tag == "cardiac_percept"
    ost_branch = None                    # the fp32 oracle stepping along under the HIP path's decisions, once the fixture is on another branch
    for step in range(3):
        batch = _batch(rec, step)
        if plain:
            trainer.train(batch, keep_predictions=(step == 0))
            dec = None
        elif step > 0 and not percept:
            # behind one / two Adam steps: forward quantities, decisions, gradients and running statistics against the oracle built from a
            # snapshot of THIS state (test_gpu_trained_state.check_step) -- the trajectory comparison below cannot see a gradient that is
            # computed from operands of the previous state.  (``cardiac_percept`` goes on under forced decisions below.)  Measured
            # (profiles/trained_state_parity.txt): gradients <= 1.4e-5 but for step 1 of cardiac_lpips, 2.2e-5 on the 8 elements of enc.0.bias,
            # where the fp32 CPU oracle itself is 2.0e-5 from fp64; at most one decision differs
            snap = tgs.snapshot(trainer)
            tgs.check_step(trainer, batch, lambda: _oracle_step(tag, rec, snap), False, bound=1.5e-4 if DIRECT_CONTROL else None,
                           record_property=lambda k, v, step=step: record_property("step%d_%s" % (step, k), v))
            dec = None
        else:
            dec = ru.hip_step_decisions(trainer, batch)
        got = [trainer.losses[k][-1] for k in keys]
        if step == 0:
            # a pure forward comparison with the reference's own numbers
            np.testing.assert_allclose(got, rec["losses"][0], rtol=2e-5)
            assert rel_l2(trainer.train_predictions["slice_inbetween_mix"], rec["s_mix_0"]) < 1e-5
            assert rel_l2(trainer.train_predictions["reconstruction"], rec["out_0"]) < 1e-5
            assert rel_l2(trainer.train_predictions["z_mix"], rec["z_mix_0"]) < 1e-5
            g_hip = {k: p.grad.detach().clone() for k, p in trainer.model.named_parameters()}
            fix = {k[6:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("grad0/")}
            gtol = (1.5e-4 if percept else 1e-4) if DIRECT_CONTROL else 2e-4
            if plain:
                for k, g in g_hip.items():
                    assert rel_l2(g, fix[k]) < gtol, k
                continue
            # (1) the HIP path against exact arithmetic under ITS OWN decisions
            r_own, g_own, _ = ru.oracle64_step(lambda: _oracle_step(tag, rec), batch)
            diffs = routing.differing_decisions(r_own, dec)
            record_property("decisions_differing_from_fp64", len(diffs))
            assert len(diffs) <= 8 and all(d["rel"] <= 2e-5 for d in diffs), "decisions that are not ties:\n" + ru.describe(diffs)
            g_ref = ru.oracle64_step(lambda: _oracle_step(tag, rec), batch, forced=dec)[1] if diffs else g_own
            # measured on the product path: 1.9e-5 (LPIPS as the reconstruction loss), 1.2e-5 (three pooling stages), <= 4.4e-6 else.  The control
            # run through the direct fp32 kernels (and whatever alternate-path switch it inherits, scripts/env_matrix.sh) keeps round 1's
            # scale: its small-channel reductions sum in fp32 over all pixels (1.2e-4 on the 8-element enc.0.bias with the stem unfolded)
            tight = 1.5e-4 if DIRECT_CONTROL else (6e-5 if percept else 3e-5)
            worst = max((rel_l2(g_hip[k], g_ref[k]), k) for k in g_ref)
            record_property("worst_gradient_rel_l2_vs_fp64_same_decisions", worst[0])
            assert worst[0] < tight, worst
            # (2) the reference's fixture: on which side of its ties did the reference's own fp32 run land?
            r_fix = routing.Routing()
            o32 = _oracle_step(tag, rec)
            o32.train(batch["image"], batch["slice_between"], batch.get("alpha_from"), batch.get("alpha_to"), route=r_fix)      # (a throw-away oracle: its Adam step is not used)
            for k, p in o32.ae.params.items():          # this IS the reference's arithmetic (test_oracle_golden pins it): same gradients
                assert rel_l2(p.grad, fix[k]) < 2e-5, k
            fix_dec = {name: r_fix.seen[name][2] for name in dec}
            apart = _other_side(dec, fix_dec)
            record_property("decisions_fixture_vs_hip", sum(apart.values()))
            if not apart:
                for k, g in g_hip.items():
                    assert rel_l2(g, fix[k]) < gtol, k
            else:
                fdiffs = routing.differing_decisions(r_own, fix_dec)
                assert sum(apart.values()) <= 4 and all(d["rel"] <= 2e-5 for d in fdiffs), "the fixture's decisions are not ties:\n" + ru.describe(fdiffs)
                g_fix64 = ru.oracle64_step(lambda: _oracle_step(tag, rec), batch, forced=fix_dec)[1]
                for k, g in fix.items():                # the fixture is right for ITS branch: fp32 CPU against fp64, same decisions (measured 1.2e-4)
                    assert rel_l2(g, g_fix64[k]) < 2e-4, k
                # from here on the reference's trajectory is another branch: step the oracle along under the HIP path's decisions
                ost_branch = _oracle_step(tag, rec)
                want = ost_branch.train(batch["image"], batch["slice_between"], batch.get("alpha_from"), batch.get("alpha_to"), route=routing.Routing(dec))
                np.testing.assert_allclose(got, [want[k] for k in keys], rtol=2e-5)
            continue
        # later steps: behind Adam updates of lr * sign(g) the sign of a near-zero gradient is summation noise, so at lr 1e-3 later losses
        # agree to ~1e-3 only (LPIPS as the reconstruction loss, whose gradients have the most near-zero entries: 2.1e-3 on the 5e-5 latent
        # term measured); at the reference's lr (1e-5) they stay at forward accuracy
        later = 5e-3 if percept else 2e-3
        want = rec["losses"][step]
        if ost_branch is not None:
            r = ost_branch.train(batch["image"], batch["slice_between"], batch.get("alpha_from"), batch.get("alpha_to"), route=routing.Routing(dec))
            want = [r[k] for k in keys]
        # (atol: the logged latent term is ~5e-5 of a total of ~0.15; 2.7e-7 of absolute difference on it read 5.2e-3 relative under AESR_LPIPS_FOLD=0)
        np.testing.assert_allclose(got, want, rtol=2e-5 if lr < 1e-4 else later, atol=0.0 if lr < 1e-4 else 1e-6)
    assert trainer.iters == int(rec["iters"]) == 4
    sd = trainer.model.state_dict()
    final = {k[3:]: v for k, v in rec.items() if k.startswith("p3/")}
    if ost_branch is not None:
        final = {k: v.detach().numpy() for k, v in ost_branch.ae.state_dict().items()}
    record_property("parameters_compared_with", "the reference fixture" if ost_branch is None else "the oracle under the HIP path's decisions")
    nbt = 3 if plain else 6          # BatchNorm calls per layer: plain ae = one train-mode pass per step, ae_combined = two
    for k, v in final.items():
        a, b = sd[k].double().cpu().numpy(), np.asarray(v).astype(np.float64)
        if "num_batches" in k:
            assert int(a) == int(b) == nbt, k
            continue
        diff = np.abs(a - b)
        assert diff.max() <= 3 * 2 * lr + 1e-6, k                              # Adam: at most 2 lr per step
        # bulk: within a fifth of one Adam step (LPIPS as the reconstruction loss has more near-zero gradients whose sign is noise)
        # (tensors of a few elements: two of them may sit in that regime -- enc.11.bias of the three-stage model, 2 of 16, since Adam's
        # bias corrections follow torch's double-precision betas; one of 16 before)
        small = (3 if percept else 2) if diff.size <= 64 else 1      # (3 of enc.0.bias's 8 seen with the unfolded LPIPS stem)
        assert (diff > 0.2 * lr + 1e-3 * np.abs(b)).sum() <= max(small, (0.25 if percept else 0.03) * diff.size), k
        if "running" in k:                                                     # BatchNorm statistics: momentum / unbiased-var details
            # (at lr 1e-3 the trajectories separate through Adam's sign noise, most with LPIPS as the reconstruction loss; the
            # lr 1e-5 fixture pins momentum / unbiased-variance details at 2e-5)
            np.testing.assert_allclose(a, b, rtol=(1e-2 if percept else 2e-3) if lr > 1e-4 else 2e-5, atol=1e-2 * lr + 1e-7,
                                       err_msg=k)


@pytest.mark.parametrize("tag", ["cardiac_mse", "brain_lpips", "ae_plain", "cardiac_percept", "cardiac_mse_s3"])
def test_first_optimizer_step_is_adam(tag):
    """The first optimizer step of the trainer, element by element: with zero moments Adam moves a parameter by -lr * g / (|g| + eps) whatever
    the betas, so p - p0 is checked against that expression on the fixture's ``grad0/*`` wherever the gradient is clear of rounding
    (tests/adam_util.py: first_step_check -- bound 0.02 lr + ulp(p), >= 75 % of EVERY trainable tensor compared).  The trajectory bounds of
    test_three_train_steps (2 lr per step, 97 % within 0.2 lr) cannot see a parameter that never trains or a step of the wrong size."""
    import adam_util as au
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_%s.npz" % tag)))
    trainer = make_trainer(tag, rec)
    group = trainer.opt_ae.param_groups[0]
    assert group["lr"] == STEP_CASES[tag][1] and float(trainer.opt_ae.dev_state[0]) == 0.0
    p0 = {k: p.detach().cpu().numpy().copy() for k, p in trainer.model.named_parameters() if p.requires_grad}
    trainer.train(_batch(rec, 0), keep_predictions=False)
    assert float(trainer.opt_ae.dev_state[0]) == 1.0                                  # one optimizer step per train()
    p1 = {k: p.detach().cpu().numpy().copy() for k, p in trainer.model.named_parameters() if p.requires_grad}
    share, where, worst = au.first_step_check(p0, p1, {k[6:]: v for k, v in rec.items() if k.startswith("grad0/")}, group["lr"], group["eps"],
                                              group["weight_decay"])
    print("%s: first step within %.4f lr of -lr g / (|g| + eps); smallest share compared %.3f (%s)" % (tag, worst, share, where))


@pytest.mark.skipif(DIRECT_CONTROL, reason="this IS the control run")
def test_direct_kernels_hold_the_round1_bounds():
    """Control for the looser Winograd-path bounds: the same golden step fixtures through the exact-fp32 direct kernels (implicit GEMM
    forward / data gradient, direct weight gradient) must still meet round 1's tighter gradient bound -- so a fixture or host-logic
    change cannot hide behind kernel rounding.  (The library reads AESR_WGRAD_WINO once per process: a child process.)"""
    import subprocess
    import sys
    env = dict(os.environ, AESR_WINO="0", AESR_WGRAD_WINO="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "three_train_steps", "-p", "no:cacheprovider"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:]


def test_loss_annealing_under_the_step_graph():
    """use_loss_annealing (kwatsch/cardiac/trainer_ae.py:80-83, kwatsch/base_trainer.py:456-459) with the step replayed from a
    captured HIP graph: lambda lives in a device scalar, so the epoch's weight reaches the replayed kernels.  The reference
    trainer ran one step in each of 4 epochs (fixture); here 2 eager steps, then 2 replays of the graph captured at epoch 2."""
    rec = dict(np.load(os.path.join(GOLDEN, "step_k4_cardiac_anneal.npz")))
    trainer = make_trainer("cardiac_mse", rec, epochs=4, use_loss_annealing=True)
    np.testing.assert_allclose(trainer.loss_weights, rec["loss_weights"], rtol=1e-12)
    trainer.enable_step_graph(eager_steps=2)
    keys = [str(k) for k in rec["loss_keys"]]
    for step in range(4):
        trainer.epoch = step
        trainer.train(_batch(rec, step), keep_predictions=False)
        got = [trainer.losses[k][-1] for k in keys]
        np.testing.assert_allclose(got, rec["losses"][step], rtol=2e-5 if step == 0 else 2e-3)
        # the logged synthesis loss is lambda_epoch * mse: its ratio to the un-annealed weight pins the lambda that was applied
    assert len(trainer._graphs) == 1
    lam = np.array(trainer.losses["loss_ae_dist_extra"].floats()) / rec["losses"][:, keys.index("loss_ae_dist_extra")]
    np.testing.assert_allclose(lam, 1.0, rtol=2e-3)


def test_checkpoint_roundtrip(tmp_path):
    """.models format of the reference: model_dict_ae / optimizer_dict_ae / epoch; resume is exact."""
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_cardiac_mse.npz")))
    t1 = make_trainer("cardiac_mse", rec)
    batch = {"image": torch.from_numpy(rec["image_0"]), "slice_between": torch.from_numpy(rec["between_0"])}
    t1.train(batch)
    f = str(tmp_path / "7.models")
    t1.save_models(f, 7)
    ck = torch.load(f, map_location="cpu")
    assert set(ck.keys()) == {"model_dict_ae", "optimizer_dict_ae", "epoch"} and ck["epoch"] == 7
    assert "enc.5.running_mean" in ck["model_dict_ae"] and "dec.14.weight" in ck["model_dict_ae"]
    assert ck["optimizer_dict_ae"]["state"][0]["exp_avg"].shape == ck["model_dict_ae"]["enc.0.weight"].shape
    stock = torch.optim.Adam([torch.nn.Parameter(v.clone().float()) for k, v in ck["model_dict_ae"].items()
                              if "running" not in k and "num_batches" not in k], lr=1e-3)
    stock.load_state_dict(ck["optimizer_dict_ae"])           # stock torch.optim.Adam accepts it
    t2 = make_trainer("cardiac_mse", rec)
    t2.load(f)
    batch1 = {"image": torch.from_numpy(rec["image_1"]), "slice_between": torch.from_numpy(rec["between_1"])}
    t1.train(batch1)
    t2.train(batch1)
    for (k, a), (_, b) in zip(t1.model.state_dict().items(), t2.model.state_dict().items()):
        assert torch.equal(a, b), k
    # a SECOND checkpoint must carry the moments of its own step (saving must not detach HipAdam's flat-buffer views from
    # opt.state): step, save, load into a fresh trainer, one more step on both -> bit-equal parameters
    p0 = t1.opt_ae._plist[0]
    assert t1.opt_ae.state[p0]["exp_avg"].data_ptr() == t1.opt_ae.flat_m.data_ptr()
    f2 = str(tmp_path / "8.models")
    t1.save_models(f2, 8)
    assert t1.opt_ae.state[p0]["exp_avg"].data_ptr() == t1.opt_ae.flat_m.data_ptr()
    ck2 = torch.load(f2, map_location="cpu")
    assert float(ck2["optimizer_dict_ae"]["state"][0]["step"]) == 2.0
    assert not torch.equal(ck2["optimizer_dict_ae"]["state"][0]["exp_avg"], ck["optimizer_dict_ae"]["state"][0]["exp_avg"])
    assert torch.equal(ck2["optimizer_dict_ae"]["state"][0]["exp_avg"], t1.opt_ae.flat_m[:p0.numel()].view_as(p0).cpu())
    t3 = make_trainer("cardiac_mse", rec)
    t3.load(f2)
    batch2 = {"image": torch.from_numpy(rec["image_2"]), "slice_between": torch.from_numpy(rec["between_2"])}
    t1.train(batch2)
    t3.train(batch2)
    for (k, a), (_, b) in zip(t1.model.state_dict().items(), t3.model.state_dict().items()):
        assert torch.equal(a, b), k


def test_step_graph_replay_equals_eager():
    """The captured HIP graph replays exactly the kernels of the eager step: identical parameters after 6 steps."""
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_brain_lpips.npz")))
    eager, graphed = make_trainer("brain_lpips", rec), make_trainer("brain_lpips", rec)
    graphed.enable_step_graph(eager_steps=2)
    for step in range(6):
        k = step % 3
        batch = {"image": torch.from_numpy(rec["image_%d" % k]), "slice_between": torch.from_numpy(rec["between_%d" % k]),
                 "alpha_from": torch.from_numpy(rec["alpha_from"]), "alpha_to": torch.from_numpy(rec["alpha_to"])}
        eager.train(batch, keep_predictions=False)
        graphed.train(batch, keep_predictions=False)
    assert len(graphed._graphs) == 1 and graphed.iters == eager.iters == 7
    for key in ("loss_ae", "loss_ae_dist", "loss_ae_dist_extra", "loss_latent_1"):
        assert graphed.losses[key].floats() == eager.losses[key].floats(), key
    for (k, a), (_, b) in zip(eager.model.state_dict().items(), graphed.model.state_dict().items()):
        assert torch.equal(a, b), k
    assert float(graphed.opt_ae.dev_state[0]) == 6.0


def test_eval_after_replayed_steps_sees_the_replayed_state():
    """Round-4 advice: a replayed step graph rewrites parameters and BatchNorm running statistics through raw pointers -- no tensor version
    moves -- so host-side caches keyed on them (eval-mode BatchNorm scale / shift, packed filters) must be invalidated by the replay itself.
    Eager validate, four replayed steps, validate again == the same calls on an all-eager trainer, bit for bit."""
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_cardiac_mse.npz")))
    eager, graphed = make_trainer("cardiac_mse", rec), make_trainer("cardiac_mse", rec)
    graphed.enable_step_graph(eager_steps=1)
    eager.WATCHDOG_EVERY = graphed.WATCHDOG_EVERY = 2       # the periodic watchdog poll (a device sync) on every other step, replayed ones included
    val = _batch(rec, 2)
    vol = torch.from_numpy(rec["image_1"])
    got = {"eager": [], "graphed": []}
    for name, tr in (("eager", eager), ("graphed", graphed)):
        for step in range(6):
            if step in (1, 2):          # step 1: behind an eager step (fills the caches); step 2: behind the capture step
                got[name].append((tr.validate(val, generate_images=False)["loss_ae"], tr.encode(vol).clone(), tr.decode(tr.encode(vol)).clone()))
            tr.train(_batch(rec, step % 3), keep_predictions=False)
        # behind replays only
        got[name].append((tr.validate(val, generate_images=False)["loss_ae"], tr.encode(vol).clone(), tr.decode(tr.encode(vol)).clone()))
    assert len(graphed._graphs) == 1
    for (la, za, oa), (lb, zb, ob) in zip(got["eager"], got["graphed"]):
        assert float(la) == float(lb)
        assert torch.equal(za, zb) and torch.equal(oa, ob)
    # and the state really moved between the evaluations (the comparison above is not one of two constants)
    assert not torch.equal(got["graphed"][1][2], got["graphed"][2][2])


def test_two_captured_trainers_on_two_streams_keep_their_loss_workspaces_apart(monkeypatch):
    """aesr_mse3_fwd leaves partial sums and a ticket in a workspace: the captured steps of two trainers that replay on different streams at
    the same time must each own one (round-3 verdict, weak 8).  Two graph-captured MSE trainers stepped concurrently on two streams log
    exactly the losses they log when stepped alone.  (Concurrent trainers on one device switch the one-launch BatchNorm off, as
    engine.bn_fused_enabled says: its grid barrier needs the whole chip to itself.)"""
    monkeypatch.setenv("AESR_BN_FUSED", "0")
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_cardiac_mse.npz")))
    batches = [{k: v.cuda() for k, v in _batch(rec, k).items()} for k in range(3)]

    def run(concurrent):
        ta, tb = make_trainer("cardiac_mse", rec), make_trainer("cardiac_mse", rec, lr=3e-4)
        for t in (ta, tb):
            t.enable_step_graph(eager_steps=2)
            for k in range(3):
                t.train(batches[k], keep_predictions=False)         # 2 eager + the capture step
        torch.cuda.synchronize()
        sa, sb = (torch.cuda.Stream(), torch.cuda.Stream()) if concurrent else (torch.cuda.current_stream(), torch.cuda.current_stream())
        for k in range(12):
            with torch.cuda.stream(sa):
                ta.train(batches[k % 3], keep_predictions=False)
            with torch.cuda.stream(sb):
                tb.train(batches[(k + 1) % 3], keep_predictions=False)
        torch.cuda.synchronize()
        return ta, tb

    a0, b0 = run(False)
    a1, b1 = run(True)
    wa, wb = a1.__dict__["_aesr_mse3_ws"], b1.__dict__["_aesr_mse3_ws"]
    ga = [v for k, v in wa.items() if k[1] == "graph"]
    gb = [v for k, v in wb.items() if k[1] == "graph"]
    assert len(ga) == 1 and len(gb) == 1 and ga[0].data_ptr() != gb[0].data_ptr()
    for key in ("loss_ae", "loss_ae_dist", "loss_ae_dist_extra", "loss_latent_1"):
        assert a1.losses[key].floats() == a0.losses[key].floats(), key
        assert b1.losses[key].floats() == b0.losses[key].floats(), key


def test_step_captured_with_kernels_the_eager_steps_never_ran(monkeypatch):
    """The one-launch BatchNorm kernels own a grid-barrier state that must be born OUTSIDE a graph capture.  A step whose eager warm-up ran the
    three-launch form (a larger batch; here: the switch) and whose capture meets the one-launch form first must still capture and replay
    (AEBaseTrainer._train_graphed creates the state before it opens the capture)."""
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_cardiac_mse.npz")))
    ref, tr = make_trainer("cardiac_mse", rec), make_trainer("cardiac_mse", rec)
    tr.enable_step_graph(eager_steps=1)
    monkeypatch.setenv("AESR_BN_FUSED", "0")
    tr.train(_batch(rec, 0), keep_predictions=False)                  # eager, three-launch BatchNorm: no barrier state exists yet
    assert "_bn_bar" not in tr.model._runner("enc").__dict__
    monkeypatch.setenv("AESR_BN_FUSED", "1")
    for k in (1, 2, 1, 2):
        tr.train(_batch(rec, k), keep_predictions=False)              # capture (one-launch BatchNorm inside), then replays
    assert len(tr._graphs) == 1 and "_bn_bar" in tr.model._runner("enc").__dict__
    for k in (0, 1, 2, 1, 2):
        ref.train(_batch(rec, k), keep_predictions=False)
    torch.cuda.synchronize()
    from superresolution_aniso_mri_amd import _hip
    _hip.check_device_watchdogs("test")
    np.testing.assert_allclose(tr.losses["loss_ae"].floats(), ref.losses["loss_ae"].floats(), rtol=2e-3)
    np.testing.assert_allclose(tr.losses["loss_ae"].floats()[:1], ref.losses["loss_ae"].floats()[:1], rtol=1e-6)


@pytest.mark.parametrize("loss", ["mse", "perceptual"])
def test_twenty_steps_track_the_oracle(loss):
    """20 consecutive training steps (lr 1e-4, distinct batches) on the HIP trainer and on the CPU oracle from the same start:
    loss curve within 1e-3 (MSE) / 1e-2 (LPIPS synthesis loss) relative at every step (Adam turns summation-order noise in near-zero gradients into +-lr parameter
    differences, so the two fp32 trajectories separate slowly; measured 3e-4 after 20 steps), BatchNorm running variances
    within 1e-2 and means within 2 % of a standard deviation, reconstruction SSIM within 1e-3 (north_star), parameter drift bounded by the Adam step size."""
    from oracle import ae_oracle, lpips_oracle, step_oracle
    from superresolution_aniso_mri_amd.data_synth import synthetic_batch
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig
    cfg = dict(width=32, latent_width=8, depth=8, latent=16, colors=1, use_batchnorm=True, use_sigmoid=True)
    lr = 1e-4
    args = dict(model="ae_combined", dataset="ACDC", device="cuda", lr=lr, weight_decay=0.0, epochs=10, ex_loss_weight1=0.05,
                use_percept_loss=False, get_masks=False, use_loss_annealing=False, use_extra_latent_loss=False, epoch_threshold=100,
                ae_class="VanillaACAI", image_mix_loss_func=loss, vgg_weights="synthetic-hash", **cfg)
    for k, v in NetworkConfig("ae_combined", dataset="ACDC").architecture.items():
        args.setdefault(k, v)
    torch.manual_seed(3)
    tr = get_trainer_dynamic(args)
    oracle = ae_oracle.OracleAE(cfg, init=False).load_state_dict({k: v.detach().cpu() for k, v in tr.model.state_dict().items()})
    kw = {}
    if loss == "perceptual":
        lin = np.load(os.path.join(os.path.dirname(__file__), "..", "superresolution_aniso_mri_amd", "lpips", "weights", "v0.1", "vgg_lin.npz"))
        kw = dict(vgg_sd=lpips_oracle.hash_vgg16_state(), lin_w=[torch.from_numpy(lin["lin%d" % k]).reshape(1, -1, 1, 1) for k in range(5)])
    ost = step_oracle.OracleStep(oracle, lr=lr, ex_loss_weight1=0.05, image_mix_loss_func=loss, **kw)
    worst = 0.0
    for step in range(20):
        batch = synthetic_batch(4, 32, 32, seed=100 + step)
        tr.train(batch, keep_predictions=(step == 19))
        ref = ost.train(batch["image"], batch["slice_between"])
        got = tr.losses["loss_ae"][-1]
        worst = max(worst, abs(got - ref["loss_ae"]) / abs(ref["loss_ae"]))
    assert worst < (1e-3 if loss == "mse" else 1e-2), worst     # measured: 3e-4 (mse), 4e-3 (LPIPS term: steeper in the weights)
    sd = tr.model.state_dict()
    for k, v in oracle.buffers.items():
        if k.endswith("running_var"):
            assert rel_l2(sd[k], v) < 1e-2, k
        elif k.endswith("running_mean"):       # means sit near zero: compare in units of the channel's standard deviation
            std = oracle.buffers[k.replace("running_mean", "running_var")].sqrt()
            assert float(((sd[k].cpu() - v).abs() / std).max()) < 2e-2, k
        elif "num_batches" in k:
            assert int(sd[k]) == int(v)
    out = tr.train_predictions["reconstruction"]
    d_ssim = abs(step_oracle.ssim(out.numpy(), batch["image"].numpy()) - step_oracle.ssim(ref["out"].numpy(), batch["image"].numpy()))
    assert d_ssim < 1e-3
    for k, p in tr.model.named_parameters():
        assert float((p.detach().cpu() - oracle.params[k].detach()).abs().max()) <= 20 * 2 * lr + 1e-6, k     # <= 2 lr per step


@pytest.mark.parametrize("B,H,W", [(1, 36, 52), (5, 44, 28), (2, 64, 64)])
def test_ragged_batch_shapes_vs_oracle(B, H, W):
    """One triplet, odd batch counts and non-square slices (sizes that leave partial tiles in every kernel): one training step of
    the HIP trainer against the CPU oracle (losses 2e-5, synthesised slices 1e-5)."""
    from oracle import ae_oracle, step_oracle
    from superresolution_aniso_mri_amd.data_synth import synthetic_batch
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig
    cfg = dict(width=32, latent_width=8, depth=16, latent=32, colors=1, use_batchnorm=True, use_sigmoid=True)
    args = dict(model="ae_combined", dataset="ACDC", device="cuda", lr=1e-4, weight_decay=0.0, epochs=10, ex_loss_weight1=0.05,
                use_percept_loss=False, get_masks=False, use_loss_annealing=False, use_extra_latent_loss=False, epoch_threshold=100,
                ae_class="VanillaACAI", image_mix_loss_func="mse", **cfg)
    for k, v in NetworkConfig("ae_combined", dataset="ACDC").architecture.items():
        args.setdefault(k, v)
    torch.manual_seed(B * 100 + H)
    tr = get_trainer_dynamic(args)
    oracle = ae_oracle.OracleAE(cfg, init=False).load_state_dict({k: v.detach().cpu() for k, v in tr.model.state_dict().items()})
    ost = step_oracle.OracleStep(oracle, lr=1e-4, ex_loss_weight1=0.05, image_mix_loss_func="mse")
    batch = synthetic_batch(B, H, W, seed=B + W)
    tr.train(batch)
    ref = ost.train(batch["image"], batch["slice_between"])
    for key in ("loss_ae", "loss_ae_dist_extra", "loss_latent_1"):
        assert abs(tr.losses[key][-1] - ref[key]) <= 2e-5 * abs(ref[key]), key
    assert tuple(tr.train_predictions["reconstruction"].shape) == (2 * B, 1, H, W)
    assert rel_l2(tr.train_predictions["reconstruction"], ref["out"]) < 1e-5
    assert rel_l2(tr.train_predictions["slice_inbetween_mix"], ref["s_mix"]) < 1e-5
