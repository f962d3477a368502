#!/usr/bin/env python
"""Generate tests/golden/labelled_batches.npz: the REFERENCE's own labelled cardiac data path -- ``ACDCDatasetEDESPairs(images4d=...)``
(datasets/ACDC/data_with_labels.py) under the transforms of train_cardiac_aesr.py:83-105 (datasets/shared_transforms.py) and
``prepare_batch_pairs`` (datasets/ACDC/data4d_simple.py), numpy on the CPU.  A script, not a test (pytest does not collect it); it needs the
reference checkout (``AESR_REFERENCE``, see oracle/make_golden.py), which the GPU box does not have.  Only data is written.

The reference is imported the way tests/make_golden_brain.py imports it: its checkout AHEAD of the repository root on ``sys.path`` and
``__file__`` of every module used asserted to lie under it; packages its modules import at their top and this path never calls (SimpleITK,
nibabel, cv2, tqdm, batchgenerators, ...) are answered with empty stand-ins; ``np.int = int`` and ``np.float = float`` (names
numpy 2 no longer has); ``torchvision.transforms.Compose`` is the five-line class below.

In-memory patients of two frames each (what ``get_4d_edes_image_array`` returns: 'image' and 'labels' [2, Z, H, W]); intensities are multiples
of 1/1024 stored as uint16 counts, labels uint8 in 0 .. 3 with every class present.  A (patient, frame) pair is volume ``2 * patient + frame``.

Legs (``<leg>/<one|two>/...``; 'one': ONE RandomState serves the dataset and the transforms, as in the training script; 'two': two objects
with two seeds):
  a_crop    adjacent_plus, volumes 7 x 20 x 18 and 6 x 13 x 24, aug_patch_size 12, width 8: one side smaller than the canvas, one larger
  b_nocrop  adjacent_plus, aug_patch_size = width = 16 on two patients of 5 x 11 x 9: padding on both sides, odd sizes, no crop drawn
  c_mix     mix on the volumes of a_crop: both steps and is_inbetween = 0 occur
  d_adj     adjacent on the volumes of a_crop
  e_test128 the test transform for width <= 128 (CenterCrop(aug_patch_size) only): 6 x 20 x 18 and 5 x 15 x 24, aug_patch_size 12
  e_testpad the test transform otherwise (AdjustToPatchSize(width) + CenterCrop(width)): 5 x 11 x 9 and 4 x 20 x 13 at width 16 (the script
            switches on ``width <= 128``; here the branch is named, the two Compose lists are train_cardiac_aesr.py:99-104's)
Per sample: vol, slice_id, id_from / id_to / id_between (slice ids), step, is_inbetween, and every number the transforms drew (top / left -1 for
"no crop drawn"; k, gain, cutoff 0 in the test legs).  Per leg: image [2B, 2, W, W], slice_between [B, 2, W, W], is_inbetween and loss_mask
after ``default_collate`` + ``prepare_batch_pairs``.

Run:  python tests/make_golden_labelled.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

Q = 1024.0
SEED_ONE, DATASET_SEED, TRANSFORM_SEED = 892372, 4711, 815
N_SAMPLES = 12


class Compose:
    """Stand-in for torchvision.transforms.Compose."""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


def import_reference_labelled():
    np.int, np.float = int, float
    mg.import_reference()
    tv = sys.modules["torchvision"]
    for sub in ("datasets", "transforms", "utils"):
        setattr(tv, sub, mg._any_stub("torchvision." + sub))
    tv.transforms.Compose = Compose
    for _ in range(64):
        try:
            import datasets.ACDC.data_with_labels as dwl
            import datasets.ACDC.data4d_simple as d4
            import datasets.shared_transforms as st
            break
        except ModuleNotFoundError as e:
            mg._any_stub(e.name)
    else:
        raise RuntimeError("could not import the reference's labelled ACDC dataset")
    ref = os.path.realpath(mg.REF)
    for m in (dwl, d4, st, sys.modules["datasets.common"]):
        assert os.path.realpath(m.__file__).startswith(ref + os.sep), "%s came from %s, not from the reference" % (m.__name__, m.__file__)
    assert dwl.get_random_adjacent_slice is sys.modules["datasets.common"].get_random_adjacent_slice
    return dwl, d4, st


def volume(rs, shape):
    """MRI-like slices in [0, 1] that change smoothly along z, as uint16 counts of 1/1024, and a label map 0 .. 3 of nested discs that drift
    the same way (every class present in every volume)."""
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
    lab = np.zeros(shape, np.uint8)
    cy, cx = rs.uniform(0.4 * h, 0.6 * h), rs.uniform(0.4 * w, 0.6 * w)
    dy, dx = rs.uniform(-0.3, 0.3, 2)
    for s in range(z):
        d2 = (yy - cy - dy * s) ** 2 + (xx - cx - dx * s) ** 2
        for v, r in ((1, 0.45), (2, 0.3), (3, 0.15)):
            lab[s][d2 < (r * min(h, w)) ** 2] = v
    assert set(np.unique(lab)) == {0, 1, 2, 3}
    return np.round(np.clip(out, 0, 1) * Q).astype(np.uint16), lab


class RecordingState:
    """A RandomState with a log of what was drawn (the draws themselves are the RandomState's)."""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def _logged(self, name, v):
        self.log.append((name, v))
        return v

    def randint(self, *a, **k):
        return self._logged("randint", self.rs.randint(*a, **k))

    def uniform(self, *a, **k):
        return self._logged("uniform", self.rs.uniform(*a, **k))

    def choice(self, *a, **k):
        return self._logged("choice", self.rs.choice(*a, **k))


def transforms_of(st, rs, width, aug, test, pad_branch):
    """train_cardiac_aesr.py:83-105 for dataset ACDCLBL and a model that is no vae.  The script takes the padding branch of its test
    transform for ``width > 128``; the fixture's widths are small, so the branch is named by ``pad_branch`` and the Compose list is the script's."""
    if not test:
        slice_mask = np.array([1, 0, 1, 0, 1, 0]).astype(np.bool)
        return Compose([st.AdjustToPatchSize(tuple((aug, aug))), st.CenterCrop(tuple((aug, aug))), st.RandomCrop(width, rs=rs),
                        st.RandomIntensity(rs=rs, slice_mask=slice_mask), st.RandomRotation(rs), st.GenericToTensor()])
    if not pad_branch:
        return Compose([st.CenterCrop(tuple((aug, aug))), st.GenericToTensor()])
    return Compose([st.AdjustToPatchSize(tuple((width, width))), st.CenterCrop(width), st.GenericToTensor()])


def run_leg(rec, key, dwl, d4, st, vols, slice_selection, width, aug, test, indices, two, pad_branch=False):
    from torch.utils.data import default_collate
    images4d = {}
    for pid in range(len(vols) // 2):
        (c0, l0), (c1, l1) = vols[2 * pid], vols[2 * pid + 1]
        images4d[pid] = {"image": np.stack([(c0 / Q).astype(np.float32), (c1 / Q).astype(np.float32)]), "labels": np.stack([l0, l1]),
                         "num_frames": 2, "num_slices": c0.shape[0], "spacing": np.array([10.0, 1.4, 1.4]), "orig_num_frames": 2,
                         "original_spacing": np.array([10.0, 1.5, 1.5]), "patient_id": "patient%03d" % pid}
    if two:
        drs, trs = RecordingState(DATASET_SEED), RecordingState(TRANSFORM_SEED)
    else:
        drs = trs = RecordingState(SEED_ONE)
    tf = transforms_of(st, trs, width, aug, test, pad_branch)
    ds = dwl.ACDCDatasetEDESPairs("training", images4d=images4d, transform=tf, slice_selection=slice_selection, rs=drs)
    assert len(ds) == sum(c.shape[0] for c, _ in vols) > max(indices)
    kept = {p: (d["image"].copy(), d["labels"].copy()) for p, d in images4d.items()}
    samples, rows = [], []
    for idx in indices:
        n0d, n0t = len(drs.log), len(trs.log)
        s = ds[idx]
        if two:
            dlog, tlog = drs.log[n0d:], trs.log[n0t:]
        else:           # one stream: the dataset draws first (step, neighbour, order), then the transforms
            log = drs.log[n0d:]
            nd = sum(1 for name, _ in log if name == "choice")
            dlog, tlog = log[:nd], log[nd:]
            assert all(name == "choice" for name, _ in dlog) and all(name != "choice" for name, _ in tlog)
        ints = [int(v) for name, v in tlog if name == "randint"]
        unis = [float(v) for name, v in tlog if name == "uniform"]
        if test:
            assert not tlog
            top = left = -1
            k, gain, cutoff = 0, 0.0, 0.0
        else:
            assert [n for n, _ in tlog] == ["randint"] * (len(ints) - 1) + ["uniform", "uniform", "randint"] and len(ints) in (1, 3)
            top, left = (ints[0], ints[1]) if len(ints) == 3 else (-1, -1)
            k, gain, cutoff = ints[-1], unis[0], unis[1]
        pid, frame, sid, Z = (int(v) for v in ds._idcs[idx])
        zf, zt = int(s["slice_id_from"][0]), int(s["slice_id_to"][0])
        step = abs(zf - zt)
        other = zt if zf == sid else zf
        zb, inb = dwl.ACDCDatasetEDESPairs._get_inbetween_sliceid(sid, other)
        assert float(s["is_inbetween"][0]) == inb and sid in (zf, zt) and step in (1, 2)
        interior = not (sid + step > Z - 1 or sid == 0 or sid - step < 0)          # only then is the neighbour drawn
        assert len(dlog) == (1 if slice_selection == "mix" else 0) + (1 if interior else 0) + 1, (key, idx, dlog)
        rows.append((2 * pid + frame, sid, zf, zt, zb, step, inb, top, left, k, gain, cutoff))
        samples.append(s)
    for p, d in images4d.items():
        assert np.array_equal(d["image"], kept[p][0]) and np.array_equal(d["labels"], kept[p][1]), "the reference changed its input"
    names = ("vol", "slice_id", "id_from", "id_to", "id_between", "step", "is_inbetween", "top", "left", "k")
    for i, name in enumerate(names):
        rec["%s/%s" % (key, name)] = np.array([r[i] for r in rows], np.int64)
    rec[key + "/gain"], rec[key + "/cutoff"] = np.array([r[10] for r in rows], np.float64), np.array([r[11] for r in rows], np.float64)
    batch = d4.prepare_batch_pairs(default_collate(samples))
    B = len(indices)
    img, btw = batch["image"].numpy(), batch["slice_between"].numpy()
    assert img.dtype == np.float32 and img.shape[:2] == (2 * B, 2) and btw.shape[:2] == (B, 2) and img.shape[2] == img.shape[3] == btw.shape[3]
    rec[key + "/image"], rec[key + "/slice_between"] = img, btw
    rec[key + "/batch_is_inbetween"], rec[key + "/batch_loss_mask"] = batch["is_inbetween"].numpy(), batch["loss_mask"].numpy()
    return rows, img


def main():
    dwl, d4, st = import_reference_labelled()
    rs = np.random.RandomState(20241020)
    crop_vols = [volume(rs, (7, 20, 18)), volume(rs, (7, 20, 18)), volume(rs, (6, 13, 24)), volume(rs, (6, 13, 24))]
    pad_vols = [volume(rs, (5, 11, 9)) for _ in range(4)]
    t128_vols = [volume(rs, (6, 20, 18)), volume(rs, (6, 20, 18)), volume(rs, (5, 15, 24)), volume(rs, (5, 15, 24))]
    tpad_vols = [volume(rs, (5, 11, 9)), volume(rs, (5, 11, 9)), volume(rs, (4, 20, 13)), volume(rs, (4, 20, 13))]
    # leg: volumes, slice_selection, width, aug_patch_size, test transform, the padding branch of the test transform
    legs = {"a_crop": (crop_vols, "adjacent_plus", 8, 12, False, False), "b_nocrop": (pad_vols, "adjacent_plus", 16, 16, False, False),
            "c_mix": (crop_vols, "mix", 8, 12, False, False), "d_adj": (crop_vols, "adjacent", 8, 12, False, False),
            "e_test128": (t128_vols, "adjacent_plus", 8, 12, True, False), "e_testpad": (tpad_vols, "adjacent_plus", 16, 16, True, True)}
    rec = {}
    pick = np.random.RandomState(7)
    for leg, (vols, sel, width, aug, test, pad_branch) in legs.items():
        n = sum(c.shape[0] for c, _ in vols)
        for i, (c, l) in enumerate(vols):
            rec["%s/vol%d" % (leg, i)], rec["%s/lab%d" % (leg, i)] = c, l
        rec[leg + "/width"], rec[leg + "/aug_patch_size"] = np.int64(width), np.int64(aug)
        rec[leg + "/slice_selection"], rec[leg + "/test"], rec[leg + "/pad_branch"] = np.array(sel), np.array(test), np.array(pad_branch)
        # given indices: the first and the last row of the table (slice 0 and Z - 1 of a volume) and a spread of the rest
        indices = [0, n - 1] + sorted(int(v) for v in pick.choice(np.arange(1, n - 1), N_SAMPLES - 2, replace=False))
        rec[leg + "/indices"] = np.array(indices, np.int64)
        for two in (False, True):
            key = "%s/%s" % (leg, "two" if two else "one")
            rows, img = run_leg(rec, key, dwl, d4, st, vols, sel, width, aug, test, indices, two, pad_branch)
            assert len(rows) >= 12, (leg, len(rows))
            ks, steps, inb = {r[9] for r in rows}, {r[5] for r in rows}, {r[6] for r in rows}
            if not test:
                assert ks == {0, 1, 2, 3}, (key, ks)
            crop_drawn = {r[7] >= 0 for r in rows}
            assert crop_drawn == ({True} if leg in ("a_crop", "c_mix", "d_adj") else {False}), (key, crop_drawn)
            if sel == "mix":
                assert steps == {1, 2} and inb == {0, 1}, (key, steps, inb)
            elif sel == "adjacent":
                assert steps == {1} and inb == {0}
            else:
                assert steps == {2} and inb == {1}
            labs = img[:, 1]
            assert set(np.unique(labs)) <= {0.0, 1.0, 2.0, 3.0} and labs.max() == 3.0
            print("%-16s image %s steps %s is_inbetween %s k %s" % (key, img.shape, sorted(steps), sorted(inb), sorted(ks)))
    rec["seeds"] = np.array([SEED_ONE, DATASET_SEED, TRANSFORM_SEED], np.int64)
    rec["legs"] = np.array(list(legs))
    path = os.path.join(HERE, "golden", "labelled_batches.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print("labelled_batches.npz: %d bytes, %d arrays" % (size, len(rec)))
    assert size < 1 << 20


if __name__ == "__main__":
    main()
