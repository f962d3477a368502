#!/usr/bin/env python
"""Generate tests/golden/brain_data.npz: the REFERENCE's own brain data path (datasets/common_brains.py, datasets/OASIS/dataset.py,
datasets/dHCP/dataset.py, datasets/shared_transforms.py; scipy and numpy on the CPU).  A script, not a test (pytest does not collect it);
it needs the reference checkout (``AESR_REFERENCE``, see oracle/make_golden.py), which the GPU box does not have.  Only data is written.

The reference is imported the way tests/make_golden_inplane.py imports it: its checkout AHEAD of the repository root on ``sys.path`` and
``__file__`` of every module used asserted to lie under it.  Packages its modules import at their top and this path never calls
(SimpleITK, pandas, tqdm, torchvision.datasets, ...) are answered with empty stand-ins.  Behavioural shims, all of them: ``np.int = int``
and ``np.float = float`` (names numpy 2 no longer has; ``GenericToTensor`` tests ``isinstance(v, np.float)``), and
``torchvision.transforms.Compose`` is the five-line class below (call the transforms in order).

Part (a), ``thick/<tag>/...``: ``simulate_thick_slices(in, thickness)`` on eight cases (``in`` as uint16 counts of 1/1024 -- ``const`` is
float32 0.7) and ``process_img(out, None, True, steps, True)`` of it (``[::steps]`` then ``rescale_intensities(percs=(0, 100))``).

Part (b), ``<set>/<leg>/...``: ``BrainOASIS(images=..., slice_selection='adjacent_plus', downsample_steps=3)`` and
``BrainDHCP(images=..., downsample_steps=5)`` on in-memory volumes, ``__getitem__`` of 12 given indices under
``get_transforms_brain`` in the crop branch, in the no-crop branch and under the test transform; the dataset's RandomState and the
transforms' RandomState are two objects with two seeds.  Per sample: slice ids, alphas, what the transforms drew (``top`` / ``left`` are -1
when no crop was drawn); per leg the batch after ``default_collate`` + ``prepare_batch_pairs``.
  - OASIS: volumes of 9 x 20 x 16 and 8 x 30 x 26.  The reference pads to its constant 220 and crops ``patch_size`` when that is smaller:
    crop leg ``patch_size = 200``, no-crop and test legs ``patch_size = 220``.  (A small crop of a 220 x 220 canvas would mostly show padding;
    batches of larger volumes at 220 x 220 would not fit the fixture's size limit.  Padded batches compress well.)
  - dHCP: the reference's dHCP transforms never pad, so volumes of unequal size can only be collated after a crop: the crop leg
    (``patch_size = 24 < 256``) has volumes of 12 x 40 x 36 and 11 x 30 x 28, the no-crop (``patch_size = 256``) and test legs have two
    28 x 28 volumes.  Every volume has at least 2 x slice step slices: below that the reference's neighbour rule produces index -1.

Run:  python tests/make_golden_brain.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

Q = 1024.0          # intensities are multiples of 1/1024: exact in fp32, stored as uint16 counts
DATASET_SEED, TRANSFORM_SEED = 4711, 815
INDICES = [0, 3, 5, 8, 9, 11, 12, 14, 16, 2, 7, 15]         # rows of the datasets' index table (volume, slice)

# tag, (Z, H, W), slice thickness, downsample_steps
THICK_CASES = [("oasis3", (40, 16, 12), 3, 3), ("oasis6", (40, 16, 12), 6, 6), ("dhcp5", (37, 8, 10), 2.5, 5), ("odd", (41, 7, 5), 4, 4),
               ("short", (3, 4, 4), 6, 6), ("two", (2, 5, 3), 5, 5), ("one", (1, 4, 8), 3, 3), ("const", (9, 4, 4), 3, 3)]


class Compose:
    """Stand-in for torchvision.transforms.Compose."""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


def import_reference_brains():
    np.int, np.float = int, float
    mg.import_reference()
    tv = sys.modules["torchvision"]
    for sub in ("datasets", "transforms", "utils"):
        setattr(tv, sub, mg._any_stub("torchvision." + sub))
    tv.transforms.Compose = Compose
    for _ in range(64):
        try:
            import datasets.common_brains as cb
            import datasets.OASIS.dataset as oasis
            import datasets.dHCP.dataset as dhcp
            break
        except ModuleNotFoundError as e:
            mg._any_stub(e.name)
    else:
        raise RuntimeError("could not import the reference's brain datasets")
    ref = os.path.realpath(mg.REF)
    for m in (cb, oasis, dhcp, sys.modules["datasets.shared_transforms"], sys.modules["datasets.common"]):
        assert os.path.realpath(m.__file__).startswith(ref + os.sep), "%s came from %s, not from the reference" % (m.__name__, m.__file__)
    import scipy.ndimage
    assert cb.gaussian_filter1d is scipy.ndimage.gaussian_filter1d
    return cb, oasis, dhcp


def volume(rs, shape):
    """MRI-like slices in [0, 1] that change smoothly along z: a few drifting blobs plus noise, as uint16 counts of 1/1024."""
    z, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros(shape)
    for _ in range(4):
        cy, cx = rs.uniform(0.2 * h, 0.8 * h), rs.uniform(0.2 * w, 0.8 * w)
        dy, dx = rs.uniform(-0.2, 0.2, 2)
        sg, amp = rs.uniform(0.1, 0.3) * min(h, w) + 0.7, rs.uniform(0.2, 0.7)
        for s in range(z):
            out[s] += amp * np.exp(-((yy - cy - dy * s) ** 2 + (xx - cx - dx * s) ** 2) / (2 * sg * sg))
    out += 0.04 * rs.randn(*shape)
    return np.round(np.clip(out, 0, 1) * Q).astype(np.uint16)


class RecordingState:
    """The transforms' RandomState with a log of what was drawn (the draws themselves are the RandomState's)."""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def randint(self, *a, **k):
        v = self.rs.randint(*a, **k)
        self.log.append(("randint", v))
        return v

    def uniform(self, *a, **k):
        v = self.rs.uniform(*a, **k)
        self.log.append(("uniform", v))
        return v


def run_leg(rec, key, cb, make_dataset, counts, transform_of):
    """One dataset object per leg (fresh dataset seed), its transform from ``transform_of(recording state)``."""
    import torch
    from torch.utils.data import default_collate
    images = {pid: {"image": (c / Q).astype(np.float32), "num_slices": c.shape[0]} for pid, c in enumerate(counts)}
    trs = RecordingState(TRANSFORM_SEED)
    ds = make_dataset(images, np.random.RandomState(DATASET_SEED), transform_of(trs))
    assert len(ds) == sum(c.shape[0] for c in counts) > max(INDICES)
    samples, draws = [], []
    for idx in INDICES:
        n0 = len(trs.log)
        s = ds[idx]
        log = trs.log[n0:]
        ints = [v for name, v in log if name == "randint"]
        unis = [v for name, v in log if name == "uniform"]
        assert len(ints) in (0, 1, 3) and len(unis) in (0, 2) and [n for n, _ in log] == ["randint"] * len(ints) + ["uniform"] * len(unis)
        top, left = (ints[0], ints[1]) if len(ints) == 3 else (-1, -1)
        draws.append((top, left, ints[-1] if ints else 0, unis[0] if unis else 0.0, unis[1] if unis else 0.0))
        samples.append(s)
    for i, name in enumerate(("top", "left", "k")):
        rec[key + "/" + name] = np.array([d[i] for d in draws], np.int64)
    rec[key + "/gain"], rec[key + "/cutoff"] = np.array([d[3] for d in draws], np.float64), np.array([d[4] for d in draws], np.float64)
    rec[key + "/vol"] = np.array([int(ds._idcs[i][0]) for i in INDICES], np.int64)
    rec[key + "/slice_id"] = np.array([int(ds._idcs[i][1]) for i in INDICES], np.int64)
    for name in ("slice_idx_from", "slice_idx_to", "inbetween_slice_id"):
        rec[key + "/" + name] = np.array([int(s[name]) for s in samples], np.int64)
        assert rec[key + "/" + name].min() >= 0
    batch = cb.prepare_batch_pairs(default_collate(samples))
    assert batch["image"].dtype == torch.float32 and batch["alpha_from"].dtype == torch.float32
    rec[key + "/alpha_from"], rec[key + "/alpha_to"] = batch["alpha_from"].numpy(), batch["alpha_to"].numpy()
    rec[key + "/image"], rec[key + "/slice_between"] = batch["image"].numpy(), batch["slice_between"].numpy()
    return batch


def main():
    cb, oasis, dhcp = import_reference_brains()
    rs = np.random.RandomState(20241017)
    rec, tags = {}, []
    # ---- part (a) ----
    for tag, shape, thickness, steps in THICK_CASES:
        if tag == "const":
            x = np.full(shape, 0.7, np.float32)
            rec["thick/%s/in" % tag] = x
        else:
            counts = volume(rs, shape)
            rec["thick/%s/in" % tag] = counts
            x = (counts / Q).astype(np.float32)
        kept = x.copy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = cb.simulate_thick_slices(x, thickness)
            proc = cb.process_img(out, None, True, steps, True)
        assert out.dtype == np.float32 and out.shape == x.shape and np.array_equal(x, kept)
        rec["thick/%s/out" % tag], rec["thick/%s/proc" % tag] = out, proc
        rec["thick/%s/thickness" % tag], rec["thick/%s/steps" % tag] = np.float64(thickness), np.int64(steps)
        tags.append(tag)
    rec["thick/tags"] = np.array(tags)
    # ---- part (b) ----
    def make_oasis(images, drs, transform):
        return oasis.BrainOASIS("training", images=images, transform=transform, rs=drs, slice_selection="adjacent_plus", downsample=True,
                                downsample_steps=3)

    def make_dhcp(images, drs, transform):
        return dhcp.BrainDHCP("training", images=images, transform=transform, rs=drs, slice_selection="adjacent_plus", downsample=True,
                              downsample_steps=5)

    sets = {"oasis": (make_oasis, "OASIS", {"crop": 200, "nocrop": 220, "test": 220},
                      {leg: [volume(rs, (9, 20, 16)), volume(rs, (8, 30, 26))] for leg in ("all",)}),
            "dhcp": (make_dhcp, "dHCP", {"crop": 24, "nocrop": 256, "test": 256},
                     {"crop": [volume(rs, (12, 40, 36)), volume(rs, (11, 30, 28))], "all": [volume(rs, (10, 28, 28)), volume(rs, (11, 28, 28))]})}
    for name, (make, dataset, patch, vols) in sets.items():
        for leg in ("crop", "nocrop", "test"):
            counts = vols.get(leg, vols["all"])
            key = "%s/%s" % (name, leg)
            for i, c in enumerate(counts):
                rec["%s/vol%d" % (key, i)] = c
            rec[key + "/patch_size"] = np.int64(patch[leg])
            batch = run_leg(rec, key, cb, make, counts,
                            lambda trs, d=dataset, p=patch[leg], t=(leg == "test"): cb.get_transforms_brain(d, rs=trs, patch_size=p)[1 if t else 0])
            print("%-14s image %s between %s alpha_from %s" % (key, tuple(batch["image"].shape), tuple(batch["slice_between"].shape),
                                                               np.round(rec[key + "/alpha_from"].ravel(), 2).tolist()))
            crop_drawn = bool((rec[key + "/top"] >= 0).all())
            assert crop_drawn == (leg == "crop") and (leg == "crop" or (rec[key + "/top"] == -1).all())
            assert (rec[key + "/gain"] > 0).all() == (leg != "test")
    rec["indices"] = np.array(INDICES, np.int64)
    rec["seeds"] = np.array([DATASET_SEED, TRANSFORM_SEED], np.int64)
    # recorded values of the two small helpers
    rec["suffix/args"] = np.array(["OASIS|t88_gfc.nii.gz|3", "OASIS|t88_gfc.nii.gz|6", "dHCP|_t2w.nii.gz|5", "dHCP|_t2w.nii.gz|4", "ADNI|.nii|3",
                                   "MNIST3D|.npy|2"])
    rec["suffix/out"] = np.array([cb.get_file_suffix_blurred(a.split("|")[0], a.split("|")[1], int(a.split("|")[2])) for a in rec["suffix/args"]])
    trip = [(0, 5, 1), (0, 5, 4), (5, 0, 3), (7, 9, 8), (9, 7, 8), (10, 4, 9), (3, 6, 4)]
    rec["coef/args"] = np.array(trip, np.int64)
    rec["coef/out"] = np.array([cb.determine_interpol_coefficients(*t) for t in trip], np.float64)
    path = os.path.join(HERE, "golden", "brain_data.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print("brain_data.npz: %d bytes, %d arrays" % (size, len(rec)))
    assert size < 1 << 20


if __name__ == "__main__":
    main()
