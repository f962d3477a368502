"""not-gpu: what keeps the bounds of tests/test_gpu_trained_state.py honest without a GPU.

  * ``state_util.randomise_state`` obeys its rules on every model state it is used on (and on one it could be used on next);
  * at the state, batch and seed of every GPU case the REFERENCE's own arithmetic -- the fp32 CPU oracle -- agrees with the fp64 oracle,
    under the same decisions, to a third of the bound the GPU case asserts on every parameter gradient (3e-5; 6e-5 with LPIPS as the
    reconstruction loss), and at most 2 of its non-smooth decisions differ from the fp64 oracle's own, each a tie (<= 2e-5 of the layer's
    rms): the bound is not one the reference itself would miss;
  * a state that is ONE optimizer step old moves every parameter gradient by more than 100 times the bound: a stale operand cannot pass.

Measured here (worst parameter tensor, rel-L2 against fp64 under the same decisions; in brackets the decisions that differ from the fp64
oracle's own), on ONE thread -- the fp32 oracle's sums depend on how many threads share them, so the tests of this file pin the count and
the figures are the same on every machine:

    randomised state   mse 5.5e-6 (0)   mse_44x28 3.4e-6 (0)   lpips 2.8e-6 (0)   percept 6.1e-6 (1, 6.6e-7 of the rms)   mse_s3 3.0e-6 (0)
                       brain_mse 4.2e-6 (0)
    after 2 steps      mse 5.8e-6 (0)   lpips 6.6e-6 (0)
    after 3 steps      mse 2.3e-6 (0)   lpips 5.6e-6 (0)
    eval paths         small 0.020, wide 0.014 of the bound (max |diff| / (2e-6 + 1e-5 |ref|))
    one step old       mse 0.022 ... 3.3, lpips 0.042 ... 2.4 (smallest: the single element of dec.14.bias) against 100 x 3e-5 = 3e-3

With 2, 4 and 8 threads the gradient figures stay below 9.0e-6 (1.0e-5 is the third of the bound) and 8.5e-6 (percept, 2.0e-5); the number of
differing decisions stays at 0 or 1 except behind two steps with the LPIPS synthesis loss on 4 threads, where 3 proven ties were seen (the
state behind the steps is itself a product of the sums' order).

The seeds are CHOSEN: about half of the seeds tried keep the fp32 oracle inside a third of the bound.  The others do not because of one kind of
tensor, the bias of a convolution whose LeakyReLU feeds a BatchNorm (enc.3.bias, dec.2.bias, ...): with biases of N(0, 0.3^2) on top of
pre-activations of the initialised filters' size, some channels are positive (or negative) at every pixel, the LeakyReLU is linear there, the
BatchNorm behind it removes the bias, and the bias gradient of that channel is a sum over all pixels that cancels to zero exactly.  Where most
channels of such a tensor are in that state its fp64 gradient is a few ulps of its own summands and a relative error measures nothing (up
to 1e+8 seen); the seeds kept are those where this does not happen, not ones where the HIP path happens to do well."""
import functools
import os

import numpy as np
import pytest
import torch

import state_util as su

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def one_thread():
    """The fp32 oracle's summation order, and with it every figure below, is a function of the thread count: pinned, and put back."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- randomise_state -------------------------------------------------------------------------------------------------------------
def _states():
    from superresolution_aniso_mri_amd.networks.acai_vanilla import VanillaACAI
    torch.manual_seed(5)
    yield "VanillaACAI", VanillaACAI(dict(su.SMALL, device="cpu")).state_dict()
    import test_oracle_golden as tog
    torch.manual_seed(6)
    yield "three stages", VanillaACAI(dict(tog.small_cfg("cardiac_mse_s3"), device="cpu")).state_dict()
    rec = np.load(os.path.join(GOLDEN, "mc_ae_small_28x28.npz"))
    yield "MultiChannelAE", {k[3:]: torch.from_numpy(rec[k]) for k in rec.files if k.startswith("p0/")}
    yield "OracleAE", su.initial_state(su.CASES["mse"])


@pytest.mark.parametrize("which", ["VanillaACAI", "three stages", "MultiChannelAE", "OracleAE"])
def test_randomise_state_rules(which):
    sd = dict(_states())[which]
    # the gap this closes: the initial state has no bias that is not exactly zero, no statistics other than (0, 1)
    assert all(not bool(v.any()) for k, v in sd.items() if k.endswith(".bias"))
    assert all(int(v) == 0 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    new = su.randomise_state(sd, 3)
    assert list(new.keys()) == list(sd.keys())
    again = su.randomise_state({k: sd[k].double() if sd[k].is_floating_point() else sd[k] for k in reversed(list(sd.keys()))}, 3)
    other = su.randomise_state(sd, 4)
    nbias = 0
    for k, v in new.items():
        old = sd[k]
        assert v.device.type == "cpu" and tuple(v.shape) == tuple(old.shape), k
        assert torch.equal(v, again[k]), k                     # deterministic; key order and input dtype do not matter
        if k.endswith("num_batches_tracked"):
            assert v.dtype == torch.int64 and int(v) == 7, k
            continue
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), k
        assert not torch.equal(v, old.float()), k
        assert not torch.equal(v, other[k]), k                 # the seed matters
        if k.endswith(".bias"):
            nbias += 1
            assert bool((v != 0).all()), k
            assert float(v.abs().max()) < 1.5, k                # N(0, 0.3^2): within 5 sigma ...
            assert v.numel() < 8 or float(v.abs().max()) > 0.05, k      # ... and of a size that shows (8 draws all below sigma / 6: p < 1e-7)
        elif k.endswith("running_mean"):
            assert float(v.abs().max()) < 1.5, k
        elif k.endswith("running_var"):
            assert 0.3 <= float(v.min()) and float(v.max()) <= 2.3, k
        elif v.dim() == 1:                                      # BatchNorm gamma
            assert 0.5 <= float(v.abs().min()) and float(v.abs().max()) <= 1.5, k
        else:                                                   # filters: one factor per output channel
            f = (v.flatten(1) * old.float().flatten(1)).sum(1) / old.float().flatten(1).pow(2).sum(1)
            assert 0.7 <= float(f.min()) and float(f.max()) <= 1.3 and bool((f != 1).all()), k
            assert torch.allclose(v, old.float() * f.reshape((-1,) + (1,) * (v.dim() - 1)), rtol=1e-5, atol=0), k
    assert nbias >= 17
    gammas = torch.cat([v for k, v in new.items() if k.endswith(".weight") and v.dim() == 1])
    assert bool((gammas < 0).any()) and float((gammas < 0).float().mean()) < 0.4          # negative with probability 0.15


# ---- the reference's own error at the states of the GPU cases --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _states_behind_oracle_steps(loss):
    """The fp32 oracle's states behind 1, 2 and 3 optimizer steps from the initialisation test_gradients_after_*_steps start from, on the same
    batches.  (The HIP trainer's state behind the same steps differs from these by Adam's sign noise in near-zero gradients, at most 2 lr
    per step and element: the same neighbourhood of the parameter space, which is what the margin is a statement about.)"""
    case = su.STEPPED[loss]
    ost = su.oracle_step_maker(case, su.initial_state(case))()
    out = []
    for s in case["batch_seeds"][:3]:
        ost.train(*su.train_batch(su.case_batch(case, seed=s)))
        out.append({k: v.clone() for k, v in ost.ae.state_dict().items()})
    return out


def _gpu_cases():
    for name in sorted(su.CASES):
        yield "randomised-" + name
    for loss in sorted(su.STEPPED):
        yield "eager-" + loss
        yield "replayed-" + loss


@pytest.mark.parametrize("which", list(_gpu_cases()))
def test_fp32_oracle_keeps_a_third_of_the_gpu_bound(which, record_property):
    kind, name = which.split("-")
    if kind == "randomised":
        case = su.CASES[name]
        state = su.randomise_state(su.initial_state(case), case["state"])
        batch = su.case_batch(case)
    else:
        case = su.STEPPED[name]
        nsteps = 2 if kind == "eager" else 3
        state = _states_behind_oracle_steps(name)[nsteps - 1]
        batch = su.case_batch(case, seed=case["batch_seeds"][nsteps])
    worst, tensor, diffs = su.fp32_oracle_vs_fp64(su.oracle_step_maker(case, state), batch)
    record_property("fp32_oracle_worst_gradient_rel_l2_vs_fp64", worst)
    record_property("decisions_differing_from_fp64", len(diffs))
    print("%s: worst %.2e (%s), %d decisions differ" % (which, worst, tensor, len(diffs)))
    assert worst <= su.grad_bound(case) / 3, (worst, tensor)
    assert len(diffs) <= 2 and all(d["rel"] <= 2e-5 for d in diffs), diffs


@pytest.mark.parametrize("name", sorted(su.EVAL_CASES))
def test_fp32_oracle_keeps_a_third_of_the_eval_bound(name):
    """The eval paths: the fp32 oracle's super-resolved volume and reconstruction against the fp64 oracle's, at a third of rtol 1e-5 / atol 2e-6."""
    import routing_util as ru
    from oracle import ae_oracle, step_oracle
    case = su.EVAL_CASES[name]
    state = su.randomise_state(su.initial_state(case), case["state"])
    ae32 = ae_oracle.OracleAE(su.case_cfg(case), init=False).load_state_dict(state)
    ae64 = ru.as_fp64(ae_oracle.OracleAE(su.case_cfg(case), init=False).load_state_dict(state))
    batch = su.case_batch(case, seed=case["batch_seed"])
    vol = torch.cat([batch["image"][:3], batch["slice_between"][:2]], dim=0)
    alphas = [0.25, 0.5, 0.8]
    with torch.no_grad():
        pairs = [(step_oracle.create_super_volume(ae32, vol, alphas), su.oracle_super_volume(ae64, vol.double(), alphas)),
                 (ae32.forward(batch["image"], train=False), ae64.forward(batch["image"].double(), train=False))]
    for got, ref in pairs:
        frac = float(((got.double() - ref).abs() / (2e-6 + 1e-5 * ref.abs())).max())
        print("%s: %.3f of the bound" % (name, frac))
        assert frac <= 1 / 3, frac
        assert float(ref.min()) < float(ref.max())


@pytest.mark.parametrize("loss", sorted(su.STEPPED))
def test_state_one_step_old_is_far_outside_the_bound(loss):
    """The permanent form of "a deliberately stale state is caught": the fp64 gradients of one batch at the states behind one and behind two
    optimizer steps (lr 1e-3) differ by more than 100 times the GPU bound on EVERY parameter tensor -- an operand, a statistic or a
    parameter that is one step old cannot pass test_gradients_after_eager_steps / test_gradients_after_replayed_steps."""
    import routing_util as ru
    case = su.STEPPED[loss]
    states = _states_behind_oracle_steps(loss)
    batch = su.case_batch(case, seed=case["batch_seeds"][2])
    g_old = ru.oracle64_step(su.oracle_step_maker(case, states[0]), batch)[1]
    g_new = ru.oracle64_step(su.oracle_step_maker(case, states[1]), batch)[1]
    apart = {k: su.rel_l2(g_old[k], g_new[k]) for k in g_new}
    print("%s: %.3g (%s) ... %.3g" % (loss, min(apart.values()), min(apart, key=apart.get), max(apart.values())))
    assert min(apart.values()) > 100 * su.GRAD_BOUND, min(apart, key=apart.get)
