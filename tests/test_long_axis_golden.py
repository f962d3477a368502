"""No GPU: tests/golden/long_axis.npz (the reference's ``compute_{ssim,psnr,vif}_for_batch`` with ``eval_axis`` 1 and 2, written by
tests/make_golden_long_axis.py) against the long-axis rules written out here with numpy and the oracle's per-slice functions -- the
fixture and the stated rules check each other -- and the declaration of the view entry point."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ["v6x40x48", "v10x33x47", "v30x64x56", "lowvif", "allblack"]


def _fixture():
    return dict(np.load(os.path.join(HERE, "golden", "long_axis.npz")))


def original_slice_ids(n, steps):
    """evaluate/metrics.py:29-45 with conv_interpol=False."""
    ids = np.arange(n)
    keep = None
    if (n - 1) % steps != 0:
        rem = (n - 1) % steps
        keep, ids = ids[-rem:], ids[:-rem]
    ids = ids[::steps]
    return ids if keep is None else np.concatenate((ids, keep))


def long_axis_by_the_rules(name, ref, rec, axis, steps):
    """(mean, number of slices scored, SSIM window) of one metric, rules 1 - 6 of the long-axis evaluation:
    uint8 conversion (VIF) before the swap; original-slice ids from the shape BEFORE the swap, used on the swapped slices; swapaxes(0, axis);
    slices with np.sum(reference) == 0 skipped; window 5 when a slice side is below 8; non-finite PSNR / VIF dropped; mean (nan of nothing)."""
    from oracle import step_oracle, vif_oracle
    if name == "vif":
        ref, rec = vif_oracle.to_uint8(ref), vif_oracle.to_uint8(rec)
    skip = set(original_slice_ids(ref.shape[0], steps).tolist()) if steps else set()
    ref, rec = np.swapaxes(ref, 0, axis), np.swapaxes(rec, 0, axis)
    win = 5 if min(ref.shape[1:]) < 8 else 7
    scores = []
    for s in range(ref.shape[0]):
        if s in skip or np.sum(ref[s]) == 0:
            continue
        if name == "ssim":
            scores.append(step_oracle.ssim(np.ascontiguousarray(ref[s]), np.ascontiguousarray(rec[s]), win=win))
        elif name == "psnr":
            v = step_oracle.psnr(np.ascontiguousarray(ref[s]), np.ascontiguousarray(rec[s]))
            if np.isfinite(v):
                scores.append(v)
        else:
            with np.errstate(all="ignore"):
                v = vif_oracle.vifp_mscale(ref[s], rec[s])
            if np.isfinite(v):
                scores.append(v)
    return (float(np.mean(scores)) if scores else float("nan")), len(scores), win


def test_fixture_follows_the_long_axis_rules():
    fx = _fixture()
    checked = 0
    for tag in CASES:
        ref, rec = fx[tag + "/ref"], fx[tag + "/rec"]
        assert ref.dtype == np.float32 and rec.dtype == np.float32 and ref.shape == rec.shape
        for axis in (1, 2):
            for steps in (0, 2):
                for name, tol in (("ssim", 1e-12), ("psnr", 1e-12), ("vif", 1e-12)):
                    key = "%s/axis%d/ds%d/%s" % (tag, axis, steps, name)
                    want, count = float(fx[key]), int(fx[key + "_count"])
                    got, n, win = long_axis_by_the_rules(name, ref, rec, axis, steps)
                    assert n == count, (key, n, count)
                    if count == 0:
                        assert np.isnan(want) and np.isnan(got), key
                    else:
                        assert abs(got - want) <= tol, (key, got, want)
                        if name == "ssim":
                            assert int(fx[key + "_win"]) == win, key
                    checked += 1
    assert checked == len(CASES) * 2 * 2 * 3


def test_fixture_covers_what_it_claims():
    fx = _fixture()
    # 5 rows / 7 columns of the reference are black by construction: exactly that many slices are not scored
    for tag, (z, h, w) in (("v6x40x48", (6, 40, 48)), ("v10x33x47", (10, 33, 47)), ("v30x64x56", (30, 64, 56))):
        assert fx[tag + "/ref"].shape == (z, h, w)
        for name in ("ssim", "psnr", "vif"):
            assert int(fx["%s/axis1/ds0/%s_count" % (tag, name)]) == h - 5 and int(fx["%s/axis2/ds0/%s_count" % (tag, name)]) == w - 7
        # the original-slice ids (from Z, applied to the swapped slices) change the result
        assert float(fx[tag + "/axis1/ds0/ssim"]) != float(fx[tag + "/axis1/ds2/ssim"])
    assert int(fx["v6x40x48/axis1/ds0/ssim_win"]) == 5 and int(fx["v10x33x47/axis1/ds0/ssim_win"]) == 7
    # a slice below 1/255 everywhere: scored by SSIM / PSNR, black for VIF's uint8 image
    for axis in (1, 2):
        assert int(fx["lowvif/axis%d/ds0/vif_count" % axis]) == int(fx["lowvif/axis%d/ds0/ssim_count" % axis]) - 1
        assert int(fx["lowvif/axis%d/ds0/psnr_count" % axis]) == int(fx["lowvif/axis%d/ds0/ssim_count" % axis])
    low = fx["lowvif/ref"]
    assert 0 < low[:, 10, :].max() < 1.0 / 255.0 and 0 < low[:, 5:, 20].max() < 1.0 / 255.0
    assert not fx["allblack/ref"].any() and all(np.isnan(fx["allblack/axis%d/ds0/%s" % (a, m)]) for a in (1, 2) for m in ("ssim", "psnr", "vif"))
    for axis in (0, 1, 2):
        assert 0 < float(fx["v30x64x56/axis%d/lpips" % axis]) < 1
    assert os.path.getsize(os.path.join(HERE, "golden", "long_axis.npz")) < 1024 * 1024


def test_view_entry_point_is_declared():
    from superresolution_aniso_mri_amd import _hip
    with open(os.path.join(ROOT, "include", "aesr_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+aesr_long_axis_views\s*\(", header), "aesr_long_axis_views is not declared in include/aesr_hip.h"
    assert "aesr_long_axis_views" in _hip.SIGNATURES
    # argument validation runs on the host before any launch: callable without a GPU
    assert _hip.lib.aesr_long_axis_views(None, None, None, None, None, 2, 2, 2, 1, None) == 1 and "aesr_long_axis_views" in _hip.last_error()
