"""Test infrastructure (no GPU): model states AWAY from the reference's initialisation, and the table of cases that
tests/test_trained_state_reference.py (CPU: is the bound honest?) and tests/test_gpu_trained_state.py (GPU: does the HIP path meet it?) share.

The reference's Initializer (networks/acai_vanilla.py:26-28, ae_standard.py:19-20) zeroes every bias -- convolution biases and BatchNorm
betas -- and a fresh BatchNorm carries running statistics (0, 1) and ``num_batches_tracked`` 0.  A wiring error that multiplies a bias by
the wrong factor, drops a beta, or reads a running mean where a batch mean belongs is invisible in that state.  ``randomise_state`` makes
a state in which every such term has a size that shows at the bounds the parity tests use."""
import zlib

import torch

SMALL = dict(width=32, latent_width=8, depth=8, latent=16, colors=1, use_batchnorm=True, use_sigmoid=True)


def randomise_state(state_dict, seed):
    """{key: tensor of any device} -> {key: CPU tensor} (float32 but for ``num_batches_tracked``), deterministic in (key, shape, seed) --
    every key draws from a generator of its own, so the order of the keys and the device of the tensors do not matter.  By key and shape:

      * 1-D ``*.weight`` (BatchNorm gamma): magnitude U(0.5, 1.5), negative with probability 0.15 (the reference draws gammas from a
        normal distribution, so negative ones are ordinary);
      * ``*.bias`` (BatchNorm beta, convolution bias) and ``running_mean``: N(0, 0.3^2);
      * ``running_var``: U(0.3, 2.3);
      * ``num_batches_tracked``: 7;
      * every other ``*.weight`` (convolution filters): the given tensor times a per-output-channel factor U(0.7, 1.3).

    No floating tensor comes back equal to its input and no bias holds an exact zero."""
    out = type(state_dict)() if isinstance(state_dict, dict) else {}
    for key, t in state_dict.items():
        t = torch.as_tensor(t).detach().cpu()
        g = torch.Generator().manual_seed((zlib.crc32(key.encode()) + 1000003 * int(seed)) % (1 << 63))
        shape = tuple(t.shape)
        if key.endswith("num_batches_tracked"):
            out[key] = torch.full(shape, 7, dtype=torch.int64)
            continue
        if not t.is_floating_point():
            raise ValueError("randomise_state: no rule for the integer tensor %s" % key)
        t = t.float()
        if key.endswith("running_var"):
            new = 0.3 + 2.0 * torch.rand(shape, generator=g)
        elif key.endswith(".bias") or key.endswith("running_mean"):
            new = 0.3 * torch.randn(shape, generator=g)
            new = torch.where(new == 0, torch.full_like(new, 0.3), new)
        elif key.endswith(".weight") and t.dim() == 1:
            mag = 0.5 + torch.rand(shape, generator=g)
            new = torch.where(torch.rand(shape, generator=g) < 0.15, -mag, mag)
        elif key.endswith(".weight") and t.dim() >= 2:
            f = 0.7 + 0.6 * torch.rand(shape[:1], generator=g)
            f = torch.where(f == 1, torch.full_like(f, 1.25), f)
            new = t * f.reshape((-1,) + (1,) * (t.dim() - 1))
        else:
            raise ValueError("randomise_state: no rule for %s of shape %s" % (key, shape))
        out[key] = new.float().contiguous()
    return out


# ---- the cases of tests/test_gpu_trained_state.py ------------------------------------------------------------------------------------
# name -> trainer: overrides of test_gpu_step.make_trainer's arguments; oracle: OracleStep keywords; batch: synthetic_batch(B, H, W, seed);
# init: torch.manual_seed before the model is built; state: randomise_state's seed.  ``percept`` = LPIPS is the reconstruction loss (the
# gradient bound is 6e-5 instead of 3e-5, as in test_gpu_step.test_three_train_steps).
CASES = {
    "mse": dict(trainer=dict(image_mix_loss_func="mse"), oracle=dict(image_mix_loss_func="mse"), batch=(4, 32, 32, 11), init=21, state=131),
    "mse_44x28": dict(trainer=dict(image_mix_loss_func="mse"), oracle=dict(image_mix_loss_func="mse"), batch=(3, 44, 28, 12), init=22, state=432),
    "lpips": dict(trainer=dict(image_mix_loss_func="perceptual"), oracle=dict(image_mix_loss_func="perceptual"), batch=(4, 32, 32, 13),
                  init=23, state=1433),
    "percept": dict(trainer=dict(use_percept_loss=True), oracle=dict(image_mix_loss_func="perceptual", recon_loss="perceptual"),
                    batch=(4, 32, 32, 14), init=24, state=5934, percept=True),
    "mse_s3": dict(trainer=dict(image_mix_loss_func="mse", latent_width=4), oracle=dict(image_mix_loss_func="mse"), batch=(4, 32, 32, 15),
                   init=25, state=35, cfg=dict(latent_width=4)),
    "brain_mse": dict(trainer=dict(image_mix_loss_func="mse", dataset="OASIS"), oracle=dict(image_mix_loss_func="mse"), batch=(4, 32, 32, 16),
                      init=26, state=436, brain=True),
}
# after-steps cases (b, c): the model's own initialisation, then optimizer steps at lr 1e-3 on distinct batches, then the checked step
STEPPED = {
    "mse": dict(trainer=dict(image_mix_loss_func="mse"), oracle=dict(image_mix_loss_func="mse"), init=341, batch_seeds=(50, 51, 52, 53, 54)),
    "lpips": dict(trainer=dict(image_mix_loss_func="perceptual"), oracle=dict(image_mix_loss_func="perceptual"), init=142,
                  batch_seeds=(60, 61, 62, 63, 64)),
}
# eval-path cases (d): "small" is the SMALL config -- no layer of it qualifies for the folded BatchNorm epilogue (the encoder's layers in front
# of a BatchNorm are narrower than the Winograd kernels take, the decoder's BatchNorms carry the upsampling), so every eval-mode BatchNorm runs
# in the stand-alone scale / shift form; "wide" (depth 32: every 3x3 layer on the Winograd kernels) takes the epilogue, with the pooling inside
# it, in front of every encoder BatchNorm
EVAL_CASES = {
    "small": dict(trainer=dict(image_mix_loss_func="mse"), init=21, state=131, batch_seed=71),
    "wide": dict(trainer=dict(image_mix_loss_func="mse", depth=32, latent=32), cfg=dict(depth=32, latent=32), init=27, state=37, batch_seed=72,
                 epilogue=True),
}
LR = 1e-3
GRAD_BOUND, GRAD_BOUND_PERCEPT = 3e-5, 6e-5


def grad_bound(case):
    return GRAD_BOUND_PERCEPT if case.get("percept") else GRAD_BOUND


def case_cfg(case):
    return dict(SMALL, **case.get("cfg", {}))


def case_batch(case, seed=None, shape=(4, 32, 32)):
    """The case's batch as a CPU dict (image, slice_between and, brain-style, alpha_from / alpha_to)."""
    from superresolution_aniso_mri_amd.data_synth import synthetic_batch
    B, H, W, s = case["batch"] if "batch" in case else shape + (seed,)
    b = synthetic_batch(B, H, W, seed=s if seed is None else seed, brain=bool(case.get("brain")))
    b.pop("loss_mask")
    return b


def lpips_kw():
    import os

    import numpy as np
    from oracle import lpips_oracle
    lin = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "superresolution_aniso_mri_amd", "lpips", "weights", "v0.1", "vgg_lin.npz"))
    return dict(vgg_sd=lpips_oracle.hash_vgg16_state(), lin_w=[torch.from_numpy(lin["lin%d" % k]).reshape(1, -1, 1, 1) for k in range(5)])


def oracle_step_maker(case, state, lr=LR):
    """() -> a fresh fp32 OracleStep on a copy of ``state`` (CPU tensors)."""
    from oracle import ae_oracle, step_oracle
    kw = dict(case["oracle"])
    if "perceptual" in kw.values():
        kw.update(lpips_kw())

    def make():
        ae = ae_oracle.OracleAE(case_cfg(case), init=False).load_state_dict(state)
        return step_oracle.OracleStep(ae, lr=lr, ex_loss_weight1=0.05, **kw)
    return make


def initial_state(case):
    """The state ``VanillaACAI`` is born with under ``torch.manual_seed(case["init"])``: the oracle's construction draws the same numbers in
    the same order as the HIP model's (oracle/ae_oracle.py), so the CPU tests start where the GPU tests start."""
    from oracle import ae_oracle
    torch.manual_seed(case["init"])
    return ae_oracle.OracleAE(case_cfg(case), init=True).state_dict()


def train_batch(batch):
    return (batch["image"], batch["slice_between"], batch.get("alpha_from"), batch.get("alpha_to"))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def fp32_oracle_vs_fp64(make_oracle_step, batch):
    """The fp32 CPU oracle's step with its decisions recorded, against the fp64 oracle under those decisions and against the fp64 oracle's
    own: (worst per-tensor gradient rel-L2, its name, decisions that differ from the fp64 oracle's own)."""
    import routing_util as ru
    from oracle import routing
    r32 = routing.Routing()
    o32 = make_oracle_step()
    o32.train(*train_batch(batch), update=True, route=r32)
    dec = {name: seen[2] for name, seen in r32.seen.items()}
    r_own, _, _ = ru.oracle64_step(make_oracle_step, batch)
    diffs = routing.differing_decisions(r_own, dec)
    g64 = ru.oracle64_step(make_oracle_step, batch, forced=dec)[1]
    worst = max((rel_l2(p.grad, g64[k]), k) for k, p in o32.ae.params.items())
    return worst[0], worst[1], diffs


def oracle_super_volume(ae, vol, alphas):
    """generate_hr_volumes.create_super_volume on the fp64 oracle in eval mode: encode, lerp (the later slice weighted alpha), decode,
    interleave behind the original slices, clamp."""
    with torch.no_grad():
        lat = ae.encode(vol, train=False)
        mixes = [ae.decode(float(a) * lat[1:] + (1 - float(a)) * lat[:-1], train=False)[:, 0] for a in alphas]
        Z, n = vol.shape[0], len(alphas)
        out = torch.empty((Z - 1) * (n + 1) + 1, *vol.shape[-2:], dtype=vol.dtype)
        out[::n + 1] = vol[:, 0]
        for k in range(n):
            out[k + 1::n + 1] = mixes[k]
        return out.clamp(0, 1)
