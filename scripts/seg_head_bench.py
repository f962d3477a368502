#!/usr/bin/env python
"""Times the label head of the multi-channel auto-encoder (aesr_softmax_dice_fwd / aesr_softmax_dice_bwd, csrc/seg_head.hip) at the sizes
of a training step: logits [24, 160, 160, 4] (the reconstructed pairs of B = 12) and [12, 160, 160, 4] (the synthesised slices), labels
read in place from channel 1 of an NCHW batch.  Needs the GPU; prints a table and writes it to ``--out`` (kept in profiles/seg_head.txt).

- kernel: HIP events around ``--batch`` back-to-back calls of the C entry point, divided by ``--batch``; median / min / max of ``--reps``
          such batches after ``--warmup`` of them.  Call i works on buffer set i % ``--sets``: with 16 sets the working set (350 MB at
          N = 24) is larger than the 256 MB last-level cache, so a call does not find its inputs left there by the one before.  The forward
          figure covers both of its launches (the pass over the logits and the one-workgroup finish).
- bytes:  algorithmic: forward = logits read + probabilities written + labels read + arg-max written; backward = probabilities read +
          labels read + d(logits) written.  The share of the 8 TB/s HBM peak is those bytes over the kernel time.
- torch:  the same computation composed of torch operations on the same device (softmax, comparison one-hot, three sums, the loss,
          argmax; backward through autograd), timed the same way on one buffer set.
- step:   ``MultiChannelCAISRTrainer.train`` at B = 12, 160 x 160, depth 32, latent 128, MSE synthesis loss: host clock around ``--steps``
          steps that end in a device synchronise."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import _hip  # noqa: E402

HBM_PEAK = 8.0e12
H = W = 160
K = 4


def event_times(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def torch_forward(logits, labels):
    p = torch.softmax(logits, dim=-1)
    onehot = (labels.unsqueeze(-1) == torch.arange(K, device=logits.device, dtype=torch.float32)).float()
    i, r, s = (onehot * p).sum(dim=(1, 2)), onehot.sum(dim=(1, 2)), p.sum(dim=(1, 2))
    return -(2 * i / (r + s + 1e-6)).mean(), p.argmax(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sets", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "seg_head.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seg_head_bench.py measures on the GPU; there is no CPU fallback"
    lib, ptr = _hip.lib, _hip.ptr
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("device: %s; %d warm-up batches, %d samples; kernel = %d back-to-back calls over %d buffer sets / %d" %
        (torch.cuda.get_device_name(0), args.warmup, args.reps, args.batch, args.sets, args.batch))
    say("%-18s %-34s | %-29s | %8s %8s | %s" % ("logits", "path", "med/min/max [us]", "GB/s", "of 8TB/s", "MB moved"))
    g = torch.Generator().manual_seed(1)
    for N in (24, 12):
        n = N * H * W * K
        sets = []
        for _ in range(args.sets):
            x = torch.rand(N, 2, H, W, generator=g)
            x[:, 1] = torch.randint(0, K, (N, H, W), generator=g).float()
            sets.append(dict(logits=(torch.randn(N, H, W, K, generator=g) * 2).cuda(), x=x.cuda(), probs=torch.empty(N, H, W, K, device="cuda"),
                             amax=torch.empty(N, H, W, dtype=torch.int32, device="cuda"), d=torch.empty(N, H, W, K, device="cuda"),
                             part=torch.empty(lib.aesr_softmax_dice_workspace_floats(N, H, W, K), device="cuda"),
                             sums=torch.empty(N, 3, K, dtype=torch.float64, device="cuda"), loss=torch.empty(1, device="cuda")))
        gl = torch.full((1,), 0.1, device="cuda")

        def fwd():
            for i in range(args.batch):
                s = sets[i % args.sets]
                _hip.check(lib.aesr_softmax_dice_fwd(ptr(s["logits"]), ptr(s["x"][:, 1]), 2 * H * W, ptr(s["probs"]), ptr(s["amax"]), ptr(s["part"]),
                                                     ptr(s["sums"]), ptr(s["loss"]), N, H, W, K, _hip.stream()), "fwd")

        def bwd():
            for i in range(args.batch):
                s = sets[i % args.sets]
                _hip.check(lib.aesr_softmax_dice_bwd(ptr(s["probs"]), ptr(s["x"][:, 1]), 2 * H * W, ptr(s["sums"]), ptr(gl), ptr(s["d"]),
                                                     N, H, W, K, _hip.stream()), "bwd")

        s0 = sets[0]
        lab0 = s0["x"][:, 1]

        def t_fwd():
            for _ in range(args.batch):
                torch_forward(s0["logits"], lab0)

        lg = s0["logits"].clone().requires_grad_(True)

        def t_fwd_bwd():
            for _ in range(args.batch):
                lg.grad = None
                torch_forward(lg, lab0)[0].backward()

        name = "%dx%dx%dx%d" % (N, H, W, K)
        rows = [("aesr_softmax_dice_fwd (2 launches)", fwd, 4.0 * (2 * n + 2 * N * H * W)), ("aesr_softmax_dice_bwd", bwd, 4.0 * (2 * n + N * H * W)),
                ("torch ops, forward", t_fwd, None), ("torch ops, forward + backward", t_fwd_bwd, None)]
        for label, fn, nbytes in rows:
            t = [v / args.batch for v in event_times(fn, args.warmup, args.reps)]
            med = statistics.median(t)
            rate = "%8.1f %7.1f%% | %.1f" % (nbytes / med / 1e9, 100 * nbytes / med / HBM_PEAK, nbytes / 1e6) if nbytes else "%8s %8s | -" % ("-", "-")
            say("%-18s %-34s | %9.1f %9.1f %9.1f | %s" % (name, label, med * 1e6, min(t) * 1e6, max(t) * 1e6, rate))
        # the two agree
        fwd()
        loss_t, amax_t = torch_forward(s0["logits"], lab0)
        torch.cuda.synchronize()
        say("%-18s kernel loss %.8f, torch loss %.8f, arg-max maps differ at %d of %d pixels" %
            (name, float(s0["loss"]), float(loss_t), int((s0["amax"].long() != amax_t).sum()), N * H * W))
        del sets, s0, lg
        torch.cuda.empty_cache()

    # the training step
    from superresolution_aniso_mri_amd.data_synth import synthetic_labelled_batch
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig
    a = dict(model="ae_combined", dataset="ACDCLBL", device="cuda", lr=1e-5, weight_decay=0.0, epochs=10, width=128, latent_width=32, depth=32,
             latent=128, ex_loss_weight1=0.001, use_percept_loss=False, get_masks=False, use_loss_annealing=False, use_extra_latent_loss=False,
             epoch_threshold=100, ae_class="MultiChannelAE", image_mix_loss_func="mse")
    for k, v in NetworkConfig("ae_combined", dataset="ACDCLBL", ae_class="MultiChannelAE").architecture.items():
        a.setdefault(k, v)
    torch.manual_seed(0)
    tr = get_trainer_dynamic(a)
    batch = {k: v.cuda() for k, v in synthetic_labelled_batch(12, H, W, seed=1).items()}
    for _ in range(5):
        tr.train(batch, keep_predictions=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.train(batch, keep_predictions=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    say("MultiChannelCAISRTrainer.train, B = 12 triplets of %dx%d, depth 32, latent 128, MSE synthesis loss, eager: %.2f ms per step "
        "(mean of %d steps, host clock, device synchronised); loss_ae %.5f, loss_label %.5f" %
        (H, W, dt * 1e3, args.steps, tr.losses["loss_ae"][-1], tr.losses["loss_label"][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
