#!/usr/bin/env python
"""Generate tests/golden/long_axis.npz: the REFERENCE's own ``evaluate.metrics.compute_{ssim,psnr,vif,lpips}_for_batch`` with
``eval_axis`` 1 and 2 (long-axis views), run on the CPU.  A script, not a test (pytest does not collect it); it needs the reference
checkout (``AESR_REFERENCE``, see oracle/make_golden.py), which the GPU box does not have.  Only data is written.

skimage is absent here, so the module's ``ssim_metric`` / ``psnr_metric`` are answered by ``oracle.step_oracle.ssim`` / ``psnr`` (the fp64
restatement of the skimage definitions the device kernels are tested against) behind skimage's signature, incl. its ``ValueError``
for a window larger than the image; everything else -- the squeeze, the swap, the black-slice test, the original-slice ids taken from
the shape before the swap, the window rule, the dropping of non-finite scores, the mean -- is the reference's code.  The stand-ins
also record how many slices each call scored and with which window.  LPIPS: ``criterion`` does what ``PerceptualLoss.forward(pred,
target, normalize=True)`` does around the reference's ``PNetLin`` with the hashed stand-in backbone (oracle.make_golden.build_pnetlin).

Run:  python tests/make_golden_long_axis.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402
from oracle import step_oracle  # noqa: E402

SHAPES = [(6, 40, 48), (10, 33, 47), (30, 64, 56)]      # SSIM window 5 on the first (Z < 8), 7 on the others
Q = 1024.0                                              # intensities are multiples of 1/1024: exact in fp32, and the file stays small


def import_reference_metrics():
    nb = mg.import_reference()[3]
    tv = sys.modules["torchvision"]
    for sub in ("datasets", "transforms", "utils"):
        setattr(tv, sub, mg._any_stub("torchvision." + sub))
    for _ in range(64):
        try:
            import evaluate.metrics as em
            return em, nb
        except ModuleNotFoundError as e:
            mg._any_stub(e.name)
    raise RuntimeError("could not import the reference's evaluate.metrics")


def volume_pair(rs, z, h, w, noise):
    """MRI-like volume in [0, 1] that changes smoothly along z, and a degraded copy; rows [:, :5, :] and columns [:, :, -7:] of the
    reference are exactly 0 (5 black slices in the axis-1 view, 7 in the axis-2 view), the copy is not black there."""
    zz, yy, xx = np.mgrid[0:z, 0:h, 0:w].astype(np.float64)
    vol = np.zeros((z, h, w))
    for _ in range(7):
        cz, cy, cx = rs.uniform(0, z), rs.uniform(0.2 * h, 0.8 * h), rs.uniform(0.2 * w, 0.8 * w)
        sz, sg, amp = rs.uniform(0.3, 0.9) * z, rs.uniform(0.08, 0.25) * min(h, w), rs.uniform(0.2, 0.8)
        vol += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg) - (zz - cz) ** 2 / (2 * sz * sz))
    vol = np.clip(vol + 0.03 * rs.randn(z, h, w), 0, 1)
    rec = np.clip(0.9 * vol + noise * rs.randn(z, h, w) + 0.03, 0, 1)
    vol[:, :5, :] = 0.0
    vol[:, :, -7:] = 0.0
    return (np.round(vol * Q) / Q).astype(np.float32), (np.round(rec * Q) / Q).astype(np.float32)


def main():
    em, nb = import_reference_metrics()
    log = {}

    def ssim_metric(a, b, win_size=None, **kw):
        win = 7 if win_size is None else win_size
        if min(a.shape) < win:
            raise ValueError("win_size exceeds image extent.")         # skimage's check
        log["n"] += 1
        log["win"].add(win)
        return step_oracle.ssim(a, b, win=win)

    def psnr_metric(a, b, **kw):
        v = step_oracle.psnr(a, b)
        log["n"] += int(np.isfinite(v))
        return v

    ref_vif = em.vifp_mscale

    def vifp_mscale(a, b, **kw):
        v = ref_vif(a, b, **kw)
        log["n"] += int(np.isfinite(v))
        return v
    em.ssim_metric, em.psnr_metric, em.vifp_mscale = ssim_metric, psnr_metric, vifp_mscale

    rs = np.random.RandomState(20240607)
    rec = {}
    cases = [("v%dx%dx%d" % s, s, 0.04) for s in SHAPES]
    vols = {tag: volume_pair(rs, *s, noise) for tag, s, noise in cases}
    # a slice that is black for VIF's uint8 image (all values below 1/255) but not for SSIM / PSNR, in either view
    a, b = volume_pair(rs, 6, 40, 48, 0.05)
    a[:, 10, :] = 2.0 / Q
    a[:, :, 20] = 2.0 / Q
    a[:, :5, :] = 0.0
    a[:, :, -7:] = 0.0
    vols["lowvif"] = (a, b)
    # every long-axis slice black: nothing is scored, the result is nan
    vols["allblack"] = (np.zeros((6, 40, 48), np.float32), volume_pair(rs, 6, 40, 48, 0.05)[1])
    fns = {"ssim": em.compute_ssim_for_batch, "psnr": em.compute_psnr_for_batch, "vif": em.compute_vif_for_batch}
    for tag, (a, b) in vols.items():
        rec[tag + "/ref"], rec[tag + "/rec"] = a, b
        for axis in (1, 2):
            for ds in (None, 2):
                for name, fn in fns.items():
                    log.update(n=0, win=set())
                    with np.errstate(all="ignore"):
                        import warnings
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            val = fn(a, b, eval_axis=axis, normalize=False, downsample_steps=ds)
                    key = "%s/axis%d/ds%d/%s" % (tag, axis, 0 if ds is None else ds, name)
                    rec[key] = np.array(val, dtype=np.float64)
                    rec[key + "_count"] = np.array(log["n"], dtype=np.int64)
                    if name == "ssim":
                        assert len(log["win"]) <= 1
                        rec[key + "_win"] = np.array(log["win"].pop() if log["win"] else 0, dtype=np.int64)
    # LPIPS of the largest volume in all three orientations (black slices included: the reference does not skip them there)
    net, _ = mg.build_pnetlin(nb)

    def criterion(pred, target, normalize=False):
        if normalize:
            target, pred = 2 * target - 1, 2 * pred - 1
        with torch.no_grad():
            return net.forward(target, pred)
    a, b = vols["v30x64x56"]
    for axis in (0, 1, 2):
        rec["v30x64x56/axis%d/lpips" % axis] = np.array(em.compute_lpips_for_batch(a, b, eval_axis=axis, criterion=criterion), dtype=np.float64)
    out = os.path.join(HERE, "golden", "long_axis.npz")
    np.savez_compressed(out, **rec)
    print("long_axis.npz: %d bytes" % os.path.getsize(out))
    for k in sorted(rec):
        if rec[k].size == 1:
            print("  %-40s %r" % (k, rec[k].tolist()))


if __name__ == "__main__":
    main()
