#!/usr/bin/env python
"""Inference throughput of the slice-synthesis loop (generate_hr_volumes.create_super_volume): synthesised slices per second on a
synthetic volume, random-init weights.  bench_infer.py [Z H num_interpolations] [--target_spacing] [--reps R]

``--target_spacing`` also times the grid path (``create_super_volume(..., grid=)``, evaluate/z_grid.py) at the commensurate spacing
8 mm / (num_interpolations + 1), which gives the same slices as the integer path, and prints its ratio to it."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import generate_hr_volumes as ghv  # noqa: E402
from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic  # noqa: E402
from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig  # noqa: E402

argv = sys.argv[1:]
with_grid = "--target_spacing" in argv
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--reps")]
Z, H, n = (int(v) for v in (pos[:3] + ["30", "160", "6"][len(pos):]))
args = dict(model="ae_combined", dataset="ACDC", device="cuda", lr=1e-5, weight_decay=0.0, epochs=1, width=128, latent_width=32, depth=32,
            latent=128, ex_loss_weight1=0.05, use_percept_loss=False, get_masks=False, use_loss_annealing=False,
            use_extra_latent_loss=False, epoch_threshold=0, ae_class="VanillaACAI", image_mix_loss_func="mse")
for k, v in NetworkConfig("ae_combined", dataset="ACDC").architecture.items():
    args.setdefault(k, v)
torch.manual_seed(0)
tr = get_trainer_dynamic(args, eval_mode=True)
vol = torch.rand(Z, H, H)
alphas = np.linspace(0, 1, n + 2, endpoint=True)[1:-1]


def timed(fn):
    """(mean, min, max) seconds per call over ``reps`` calls, each synchronised, after one warm-up call; and the last result"""
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.mean(times)), min(times), max(times), out


dt, lo, hi, out = timed(lambda: ghv.create_super_volume(tr, vol, alphas, use_original=True)["upsampled_image"])
synth = (Z - 1) * n
print("volume %dx%dx%d, %d interpolations: %d synthesised slices in %.1f ms = %.0f slices/s (incl. the device-to-host copy of %d slices)"
      % (Z, H, H, n, synth, dt * 1e3, synth / dt, out.shape[0]))
print("    per call over %d calls: mean %.3f ms, min %.3f ms, max %.3f ms" % (reps, dt * 1e3, lo * 1e3, hi * 1e3))
if with_grid:
    from superresolution_aniso_mri_amd.evaluate.z_grid import target_grid
    grid = target_grid(Z, 8.0, 8.0 / (n + 1))
    gdt, glo, ghi, gout = timed(lambda: ghv.create_super_volume(tr, vol, None, use_original=True, grid=grid)["upsampled_image"])
    assert gout.shape == out.shape
    print("grid path at 8 mm -> %.6g mm (%d slices, %d mixing launches): mean %.3f ms, min %.3f ms, max %.3f ms; ratio to the integer path %.3f "
          "(of the means), %.3f (of the minima); max abs difference %.3e, bit-equal %s"
          % (8.0 / (n + 1), grid.J, sum(1 for a in grid.gap_alphas if a), gdt * 1e3, glo * 1e3, ghi * 1e3, gdt / dt, glo / lo,
             float((gout - out).abs().max()), bool(torch.equal(gout, out))))
