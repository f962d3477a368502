#!/usr/bin/env python
"""Generate the multi-channel (image + label map) fixtures under tests/golden/ from the REFERENCE's own modules on the CPU:
networks/acai_multi_channel.py (``MultiChannelAE``), kwatsch/dice_loss.py (``DiceLoss``), kwatsch/sr_multi_channel/trainer_ae.py
(``MultiChannelTrainer`` / ``MultiChannelCAISRTrainer``, their real ``train()``), generate_hr_volumes.py and evaluate/common.py
(``create_super_volume(labels=...)``).  A script, not a test (pytest does not collect it); it needs the reference checkout
(``AESR_REFERENCE``, see oracle/make_golden.py), which the GPU box does not have.  Only data is written.

Shims, all of them:
  - the import stand-ins of ``oracle.make_golden.import_reference_trainers()`` (absent third-party packages the step never calls, the fake
    VGG16 with the synthetic backbone, ``torch.cuda.FloatTensor`` makes a CPU tensor) and, for further ModuleNotFoundErrors of the
    multi-channel modules' import chain, the same empty stand-in modules;
  - ONE more behavioural shim: ``Tensor.to`` / ``Module.to`` map a ``"cuda..."`` device string to the CPU (the multi-channel trainers put
    their Dice loss on ``"cuda:0"``, kwatsch/sr_multi_channel/trainer_ae.py:76, and the volume functions send slices ``.to('cuda')``);
  - ``latent_space_interp``'s default device of both volume modules is bound to 'cpu' (as oracle.make_golden.gen_supervolume_eval does);
  - forward hooks on ``enc``, ``decoder_head2[3]`` (logits) and ``decoder_head2`` RECORD tensors of the first step; they change nothing.
Nothing of a step, a loss or a volume function is replaced.

Sizes: depth 8, latent 16, scales 2 (width 32 / latent_width 8), nclasses 4, B = 2 pairs, lr 1e-3.  Inputs are smooth blobs, labels
``floor(3.999 * blob)`` of other blobs: all four classes occur and at least one sample lacks a class (asserted).  
Ties.  The tests compare predicted labels at every pixel where the reference's gap between its two largest class probabilities is
>= 1e-4 (ten times the bound on a probability) and allow at most 1 % of the pixels of a prediction to fall below that.  A gap of 1e-4 at
EVERY pixel is not to be had by choosing a seed: three steps after initialisation the class probabilities of a train-mode pass are
smooth fields around 1/4 that cross each other along curves, and with some thousand pixels per prediction the smallest gap is 1e-7 to
1e-5 for each of the 37 seeds tried (it is >= 1e-4 only in eval-mode passes, where the young running statistics leave the fields flat).
So the script ASSERTS what the tests rely on instead: in every stored label prediction fewer than 1 % of the pixels have a gap below
1e-4 -- the data seed is the first one of SEEDS for which that and the label census hold -- and records the smallest gap (``min_gap``)
and the largest such fraction (``max_frac_below``).  mc_ae_small stores no label prediction; only probabilities, losses and gradients
are compared there.

  mc_ae_small_{40x36,28x28}.npz   one train-mode forward + backward of MultiChannelAE with MSE(x[:, :1], image) + 0.1 DiceLoss(soft_probs,
                                  x[:, 1]); plus ``ref64/*``: the reference's nn.Softmax(dim=1) and DiceLoss on the stored logits in
                                  float64 with the gradients w.r.t. soft_probs and logits (what a float64 restatement must reproduce)
  step_k3_mc_{plain,caisr_mse,caisr_lpips}.npz   three steps of the real ``train()``
  supervolume_labels.npz          both ``create_super_volume`` functions with ``labels=``

Run:  python tests/make_golden_multichannel.py
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "golden")
SEEDS = range(3, 40)
MIN_GAP = 1e-4
MAX_FRAC_BELOW = 0.01
NCLASSES = 4


def import_reference_multichannel():
    mg.import_reference_trainers()
    t_to, m_to = torch.Tensor.to, torch.nn.Module.to

    def cpu_for_cuda(a):
        return tuple(("cpu" if (isinstance(v, str) and v.startswith("cuda")) else v) for v in a)

    torch.Tensor.to = lambda self, *a, **k: t_to(self, *cpu_for_cuda(a), **k)
    torch.nn.Module.to = lambda self, *a, **k: m_to(self, *cpu_for_cuda(a), **k)
    for _ in range(64):
        try:
            import kwatsch.sr_multi_channel.trainer_ae as mta
            import networks.acai_multi_channel as amc
            import kwatsch.dice_loss as dl
            break
        except ModuleNotFoundError as e:
            mg._any_stub(e.name)
    else:
        raise RuntimeError("could not import the reference's multi-channel modules")
    ref = os.path.realpath(mg.REF)
    for m in (mta, amc, dl):
        assert os.path.realpath(m.__file__).startswith(ref + os.sep), "%s came from %s, not from the reference" % (m.__name__, m.__file__)
    return mta, amc, dl


def blobs(n, H, W, g):
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    out = torch.zeros(n, H, W)
    for i in range(n):
        for _ in range(4):
            cy, cx = torch.rand(1, generator=g) * H, torch.rand(1, generator=g) * W
            s, a = 3 + torch.rand(1, generator=g) * 6, torch.rand(1, generator=g)
            out[i] += a * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return out.clamp(0, 1)


def two_channel(n, H, W, g):
    img = blobs(n, H, W, g)[:, None]
    lab = torch.floor(blobs(n, H, W, g) * 3.999)[:, None]
    return torch.cat([img, lab], 1)


def label_census(x):
    """(all classes occur, some sample lacks a class)"""
    per = torch.stack([torch.bincount(s.long().flatten(), minlength=NCLASSES) for s in x[:, 1]])
    return bool((per.sum(0) > 0).all()), bool((per == 0).any())


def min_gap(soft_probs):
    """(smallest top-two gap, fraction of pixels whose gap is below MIN_GAP)"""
    top2 = soft_probs.detach().topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    return float(gap.min()), float((gap < MIN_GAP).float().mean())


def worst(gaps):
    return min(g for g, _ in gaps), max(f for _, f in gaps)


def mc_args(mix="mse", H=32, **over):
    a = mg.trainer_args(mix=mix, lr=1e-3)
    a.update(colors=2, nclasses=NCLASSES, device="cpu", width=28 if H == 28 else 32, latent_width=7 if H == 28 else 8)
    a.update(over)
    return a


# ---- mc_ae_small ------------------------------------------------------------------------------------------------------------------
def ae_small(amc, dl, H, W, seed):
    args = mc_args(H=H)
    torch.manual_seed(1000 + H)
    model = amc.MultiChannelAE(args)
    model.train()
    rec = {"p0/" + k: v for k, v in mg.np_state(model.state_dict()).items()}
    rec["param_names"] = np.array([k for k, _ in model.named_parameters()])
    rec["state_keys"] = np.array(list(model.state_dict().keys()))
    x = two_channel(4, H, W, torch.Generator().manual_seed(seed))
    seen = {}
    h1 = model.decoder_head2[3].register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o))
    z = model.encode(x)
    out = model.decode(z)
    h1.remove()
    out["soft_probs"].retain_grad()
    seen["logits"].retain_grad()
    loss_ae = F.mse_loss(x[:, 0, None], out["image"])
    loss_label = dl.DiceLoss(NCLASSES)(out["soft_probs"], x[:, 1].to(torch.int64))
    (loss_ae + 0.1 * loss_label).backward()
    assert tuple(out["image"].shape) == (4, 1, H, W) and tuple(out["soft_probs"].shape) == (4, NCLASSES, H, W)
    rec.update(x=x.numpy(), z=z.detach().numpy(), image=out["image"].detach().numpy(), soft_probs=out["soft_probs"].detach().numpy(),
               logits=seen["logits"].detach().numpy(), loss_ae=np.float64(loss_ae.item()), loss_label=np.float64(loss_label.item()),
               dsoft_probs=out["soft_probs"].grad.numpy(), dlogits=seen["logits"].grad.numpy(), label_weight=np.float64(0.1))
    rec.update({"grad/" + k: p.grad.numpy() for k, p in model.named_parameters()})
    rec.update({"p1/" + k: v for k, v in mg.np_state(model.state_dict()).items() if "running" in k or "num_b" in k})
    # the reference's softmax and Dice loss in float64 on the stored logits: loss, d/d soft_probs, d/d logits
    lg = seen["logits"].detach().double().requires_grad_(True)
    sp = torch.nn.Softmax(dim=1)(lg)
    sp.retain_grad()
    l64 = dl.DiceLoss(NCLASSES)(sp, x[:, 1].to(torch.int64))
    l64.backward()
    rec.update({"ref64/soft_probs": sp.detach().numpy(), "ref64/loss_label": np.float64(l64.item()), "ref64/dsoft_probs": sp.grad.numpy(),
                "ref64/dlogits": lg.grad.numpy()})
    gap = min_gap(out["soft_probs"])
    rec["min_gap"], rec["max_frac_below"] = np.float64(gap[0]), np.float64(gap[1])
    return rec, gap, label_census(x)


# ---- step_k3_mc_* -------------------------------------------------------------------------------------------------------------------
def run_steps(mta, amc, cls, args, seed, nsteps=3, B=2, H=32, W=32):
    torch.manual_seed(4242)
    model = amc.MultiChannelAE(args)
    rec = {"p0/" + k: v for k, v in mg.np_state(model.state_dict()).items()}
    trainer = cls(args, model)
    z_seen, sp_seen = [], []
    hooks = [model.enc.register_forward_hook(lambda m, i, o: z_seen.append(o.detach().clone())),
             model.decoder_head2.register_forward_hook(lambda m, i, o: sp_seen.append(o.detach().clone()))]
    rows, keys, gaps, census = [], None, [], []
    for step in range(nsteps):
        g = torch.Generator().manual_seed(seed * 100 + step)
        batch = {"image": two_channel(2 * B, H, W, g), "slice_between": two_channel(B, H, W, g)}
        census.append(label_census(torch.cat([batch["image"], batch["slice_between"]])))
        n0 = {k: len(v) for k, v in trainer.losses.items()}
        z_seen.clear()
        sp_seen.clear()
        trainer.train(dict(batch), keep_predictions=True)
        if keys is None:
            keys = sorted(trainer.losses.keys())
        for k in trainer.losses:
            assert len(trainer.losses[k]) == n0.get(k, 0) + 1, "one value per key per step expected (%s)" % k
        rows.append([trainer.losses[k][-1] for k in keys])
        rec["image_%d" % step], rec["between_%d" % step] = batch["image"].numpy(), batch["slice_between"].numpy()
        gaps += [min_gap(sp) for sp in sp_seen]
        if step == 0:
            pr = trainer.train_predictions
            assert len(sp_seen) == 2          # dec(z), then the decoded mix
            rec["z_0"] = z_seen[0].numpy()
            rec["soft_probs_0"], rec["soft_probs_mix_0"] = sp_seen[0].numpy(), sp_seen[1].numpy()
            rec["out_0"], rec["pred_labels_0"] = pr["reconstruction"].numpy(), pr["pred_labels"].numpy()
            rec["s_mix_0"], rec["label_mix_0"], rec["z_mix_0"] = pr["slice_inbetween_mix"].numpy(), pr["label_inbetween_mix"].numpy(), pr["z_mix"].numpy()
            assert np.array_equal(rec["pred_labels_0"], sp_seen[0].argmax(1, keepdim=True).numpy())
            assert np.array_equal(rec["label_mix_0"], sp_seen[1].argmax(1, keepdim=True).numpy())
            rec.update({"grad0/" + k: p.grad.numpy().copy() for k, p in model.named_parameters()})
    for h in hooks:
        h.remove()
    rec["losses"], rec["loss_keys"] = np.array(rows, dtype=np.float64), np.array(keys)
    rec["iters"] = np.array(trainer.iters)
    rec["training_after"] = np.array(bool(model.training))
    rec["trainer_class"] = np.array(cls.__name__)
    rec.update({"p%d/" % nsteps + k: v for k, v in mg.np_state(model.state_dict()).items()})
    rec["min_gap"], rec["max_frac_below"] = (np.float64(v) for v in worst(gaps))
    return rec, worst(gaps), census


# ---- supervolume_labels -----------------------------------------------------------------------------------------------------------
def supervolumes(mta, amc, seed):
    """Both reference ``create_super_volume`` functions with ``labels=`` around the reference trainer's own encode / decode / predict."""
    for name in ("SimpleITK", "imageio"):
        if name not in sys.modules:
            mg._stub(name, sitkLanczosWindowedSinc=0, Image=object, imsave=None)
    for _ in range(64):
        try:
            import evaluate.common as ec
            import generate_hr_volumes as ghv
            break
        except ModuleNotFoundError as e:
            mg._any_stub(e.name)
    ref = os.path.realpath(mg.REF)
    for m in (ec, ghv):
        assert os.path.realpath(m.__file__).startswith(ref + os.sep)
    ec.latent_space_interp = functools.partial(ec.latent_space_interp, device="cpu")
    ghv.latent_space_interp = functools.partial(ghv.latent_space_interp, device="cpu")
    args = mc_args()
    torch.manual_seed(79)
    model = amc.MultiChannelAE(args)
    trainer = mta.MultiChannelCAISRTrainer(args, model)
    g = torch.Generator().manual_seed(seed * 100 + 50)
    for _ in range(2):          # running statistics away from their initial values
        trainer.train({"image": two_channel(4, 32, 32, g), "slice_between": two_channel(2, 32, 32, g)})
    model.eval()
    rec = {"p/" + k: v for k, v in mg.np_state(model.state_dict()).items()}
    gaps = []
    hook = model.decoder_head2.register_forward_hook(lambda m, i, o: gaps.append(min_gap(o)))
    alphas3 = np.linspace(0, 1, 5)[1:-1]
    tags = []
    for Z in (5, 6):
        vol = two_channel(Z, 32, 32, torch.Generator().manual_seed(seed * 100 + 60 + Z))
        images, labels = vol[:, 0].clone(), vol[:, 1].clone()
        rec["Z%d/images" % Z], rec["Z%d/labels" % Z] = images.numpy(), labels.numpy()
        out = ghv.create_super_volume(trainer, images.clone(), alpha_range=alphas3, labels=labels.clone())
        tag = "Z%d/hr" % Z
        rec[tag + "/image"], rec[tag + "/labels"] = np.asarray(out["upsampled_image"]), np.asarray(out["upsampled_labels"])
        tags.append(tag)
        for use_original in (True, False):
            out = ec.create_super_volume(trainer, images.clone(), alpha_range=alphas3, labels=labels.clone(), downsample_steps=2,
                                         use_original=use_original, generate_inbetween_slices=True)
            tag = "Z%d/eval_%s" % (Z, "orig" if use_original else "recon")
            rec[tag + "/image"], rec[tag + "/labels"] = np.asarray(out["upsampled_image"]), np.asarray(out["upsampled_labels"])
            tags.append(tag)
    hook.remove()
    rec["alpha_range"] = np.asarray(alphas3, np.float64)
    rec["downsample_steps"] = np.array(2)
    rec["tags"] = np.array(tags)
    rec["min_gap"], rec["max_frac_below"] = (np.float64(v) for v in worst(gaps))
    return rec, worst(gaps)


def save(name, rec):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print("%-32s %7d bytes, %3d arrays, min gap %.2e, at most %.3f %% of a prediction's pixels below %g" %
          (name, size, len(rec), float(rec["min_gap"]), 100 * float(rec["max_frac_below"]), MIN_GAP))
    assert size < 1 << 20


def first_good(make, what, need_gap=True):
    for seed in SEEDS:
        rec, gap, ok = make(seed)
        if (gap[1] < MAX_FRAC_BELOW or not need_gap) and ok:
            rec["data_seed"] = np.array(seed)
            return rec
        print("  %s: seed %d rejected (min gap %.2e, %.3f %% below, label census %s)" % (what, seed, gap[0], 100 * gap[1], ok))
    raise RuntimeError("no seed of %s keeps %s's pixels with a top-two gap below %g under %g" % (list(SEEDS), what, MIN_GAP, MAX_FRAC_BELOW))


def main():
    mta, amc, dl = import_reference_multichannel()
    only = set(sys.argv[1:])
    if not only or "ae" in only:
        for H, W in ((40, 36), (28, 28)):
            def make(seed, H=H, W=W):
                rec, gap, (all_occur, one_lacks) = ae_small(amc, dl, H, W, seed)
                return rec, gap, all_occur and one_lacks
            save("mc_ae_small_%dx%d.npz" % (H, W), first_good(make, "mc_ae_small_%dx%d" % (H, W), need_gap=False))
    if not only or "steps" in only:
        cases = [("plain", mta.MultiChannelTrainer, mc_args("mse", model="ae")), ("caisr_mse", mta.MultiChannelCAISRTrainer, mc_args("mse")),
                 ("caisr_lpips", mta.MultiChannelCAISRTrainer, mc_args("perceptual"))]
        for tag, cls, args in cases:
            def make(seed, cls=cls, args=args):
                rec, gap, census = run_steps(mta, amc, cls, dict(args), seed)
                return rec, gap, all(a for a, _ in census) and any(b for _, b in census)
            rec = first_good(make, "step_k3_mc_" + tag)
            save("step_k3_mc_%s.npz" % tag, rec)
            print("    %s keys %s\n    losses[0] %s training_after %s" % (cls.__name__, list(rec["loss_keys"]), rec["losses"][0], rec["training_after"]))
    if not only or "vol" in only:
        def make(seed):
            rec, gap = supervolumes(mta, amc, seed)
            return rec, gap, True
        save("supervolume_labels.npz", first_good(make, "supervolume_labels"))


if __name__ == "__main__":
    main()
