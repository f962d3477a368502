#!/usr/bin/env python
"""Times the in-plane resampling step (aesr_inplane_resample, csrc/inplane.hip) on one 4-D cardiac volume, 30 frames x 10 slices x
216 x 256 at 1.5625 mm -> 241 x 286 at 1.4 mm and back, and ``generate_hr_volumes`` with and without ``--resample``.  Needs the GPU;
prints a table (kept in profiles/inplane_resample.txt).

- call:   HIP events around ``apply_2d_zoom_4d`` on a device tensor, after a warm-up, median / min / max of ``--reps`` calls.  The call
          builds the host tables, copies them (a few KB), WAITS for that copy and launches one kernel, so this figure holds the
          host turn-around between copy and launch as well as the kernel.
- kernel: run this script under ``rocprofv3 --kernel-trace --stats -- python scripts/inplane_bench.py --reps 20 --no-cpu --no-e2e``
          for the kernel's own duration (the stats table names inplane_kernel<true> / <false>).
- bytes:  algorithmic, (N H W + N Ho Wo) x 4 B; the share of the 8 TB/s HBM peak is those bytes over the time.
- cpu:    if scipy is importable, the two scipy calls the reference makes per frame (gaussian_filter per slice, zoom per frame) on
          the same volume, on this machine's host threads, once.  Otherwise no CPU figure is printed.
- e2e:    ``upsample_volume`` (no resampling) against ``upsample_volume_resampled`` on one 10 x 216 x 256 frame with the intensities
          of a real scan (0..~1500), random-init ACDC network, wall clock incl. both PCIe copies, median of ``--e2e-reps``."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd.datasets import common as dc  # noqa: E402

HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "inplane_bench.py measures on the GPU; there is no CPU fallback"
    print("device: %s" % torch.cuda.get_device_name(0))
    T, Z, H, W = 30, 10, 216, 256
    fine, coarse = (1.4, 1.4), (1.5625, 1.5625)
    g = torch.Generator().manual_seed(1)
    vol = torch.rand(T, Z, H, W, generator=g).cuda()
    up = dc.apply_2d_zoom_4d(vol, coarse, fine)
    print("%-34s | %9s %9s %9s | %9s %8s" % ("call (HIP events, one launch)", "med [us]", "min [us]", "max [us]", "GB/s", "of 8TB/s"))
    for name, x, sp, ns in (("in  300x216x256 -> 300x241x286", vol, coarse, fine), ("out 300x241x286 -> 300x216x256", up, fine, coarse)):
        y = dc.apply_2d_zoom_4d(x, sp, ns)
        nbytes = 4.0 * (x.numel() + y.numel())
        t = event_times(lambda: dc.apply_2d_zoom_4d(x, sp, ns), args.warmup, args.reps)
        med = statistics.median(t)
        print("%-34s | %9.1f %9.1f %9.1f | %9.1f %7.1f%%   (%.1f MB moved, output %s)" % (
            name, med * 1e6, min(t) * 1e6, max(t) * 1e6, nbytes / med / 1e9, 100 * nbytes / med / HBM_PEAK, nbytes / 1e6, tuple(y.shape)))
    if not args.no_cpu:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            ndi = None
        if ndi is None:
            print("cpu: scipy is not importable here; no CPU figure")
        else:
            host = vol.cpu().numpy()
            zoom = dc.zoom_factors(coarse, fine)
            t0 = time.perf_counter()
            outs = []
            for f in host:
                f = f.copy()
                for z in range(f.shape[0]):
                    f[z] = ndi.gaussian_filter(f[z], 0.25 / zoom)
                outs.append(ndi.zoom(f, (1,) + tuple(zoom), order=1))
            dt = time.perf_counter() - t0
            err = float(np.abs(np.stack(outs).astype(np.float64) - up.cpu().numpy()).max())
            print("cpu: scipy %s on this host, the same volume, one pass: %.2f s  (max |device - scipy| = %.3g)" % (
                __import__("scipy").__version__, dt, err))
    if not args.no_e2e:
        from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
        from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
        from superresolution_aniso_mri_amd.networks.net_config import NetworkConfig
        a = dict(model="ae_combined", dataset="ACDC", device="cuda", lr=1e-5, weight_decay=0.0, epochs=1, width=128, latent_width=32, depth=32,
                 latent=128, ex_loss_weight1=0.05, use_percept_loss=False, get_masks=False, use_loss_annealing=False,
                 use_extra_latent_loss=False, epoch_threshold=0, ae_class="VanillaACAI", image_mix_loss_func="mse")
        for k, v in NetworkConfig("ae_combined", dataset="ACDC").architecture.items():
            a.setdefault(k, v)
        torch.manual_seed(0)
        tr = get_trainer_dynamic(a, eval_mode=True)
        frame = (torch.rand(Z, H, W, generator=g) * 1500.0).numpy()
        n = 6

        def wall(fn):
            fn()
            ts = []
            for _ in range(args.e2e_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts), min(ts), max(ts)
        plain = wall(lambda: ghv.upsample_volume(tr, frame, n))
        rs = wall(lambda: ghv.upsample_volume_resampled(tr, frame, n, coarse, fine))
        print("e2e one 10x216x256 frame, %d interpolations (64 slices out), wall incl. PCIe: no resampling %.2f ms (min %.2f, max %.2f); "
              "--resample (241x286 padded to 244x288 for the network) %.2f ms (min %.2f, max %.2f)" % (
                  n, plain[0] * 1e3, plain[1] * 1e3, plain[2] * 1e3, rs[0] * 1e3, rs[1] * 1e3, rs[2] * 1e3))
        x, hr = torch.from_numpy(frame).cuda(), torch.rand(64, 241, 286, generator=g).cuda()
        t_in = statistics.median(event_times(lambda: dc.apply_2d_zoom_3d(x, coarse, fine), 5, 50))
        t_out = statistics.median(event_times(lambda: dc.apply_2d_zoom_3d(hr, fine, coarse), 5, 50))
        print("     of which the two resampling calls (HIP events): 10 slices in %.1f us + 64 slices back %.1f us" % (t_in * 1e6, t_out * 1e6))


if __name__ == "__main__":
    main()
