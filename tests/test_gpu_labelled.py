"""-m gpu: labelled triplet batches on the device (include/aesr_hip_labelprep.h, csrc/augment_labelled.hip; data_device.LabelledTripletAugmenter,
load_labelled_volume_dir; datasets.common order=0; train_aesr --labels_dir).

- The kernel against every leg of tests/golden/labelled_batches.npz (the reference's own batches; tests/test_labelled_golden.py holds the
  restatement and the draws without a GPU): labels exactly, images within 2e-6, the test-transform legs bitwise.
- Channel 0 equals ``aesr_triplet_assemble`` (raw: ``aesr_triplet_assemble_raw``) BITWISE for the same image cache and descriptors: the new
  kernel is held to the arithmetic the step already trains on.
- B = 1; B = 65 at W = 4 (two launches and the scatter) equals 65 single-sample calls bitwise; the shards of a batch equal the batch of one
  process bitwise; ``reuse_output`` returns the same storage and marks the batch ``_persistent``.
- Both entry points between the guard bands of tests/memguard.py at their contractual sizes, outputs poisoned (NaN pattern, 3e38), both caches
  compared bit for bit after the call; ``images`` / ``image`` / ``between`` shifted by 4, 8 and 12 bytes, ``labels`` by 1, 2 and 3 bytes.
  Refusals return their status and leave the poison: argument checks that return before a launch -- nothing here makes the device read or
  write out of range.
- ``apply_2d_zoom_3d`` / ``_4d(order=0)`` equal tests/golden/inplane_labels.npz exactly; device in, device out; a 4-D array is one launch.
- ``load_labelled_volume_dir`` on .npy and NIfTI pairs with ``resample``.
- End to end: train both multi-channel trainers from a directory of volumes and one of label maps, generate, score.

GUARDED_ENTRIES and EXEMPT partition ``_hip.SIGNATURES_LABELPREP`` (tests/test_abi.py checks that without a GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import memguard as mg
import test_labelled_golden as tl

pytestmark = pytest.mark.gpu

GUARDED_ENTRIES = ("aesr_labelled_triplet_assemble", "aesr_labelled_triplet_assemble_raw")
EXEMPT = {}
HERE = os.path.dirname(os.path.abspath(__file__))


def _descs(hip, aug, samples, transforms):
    d = (hip.TripletDesc * len(samples))()
    for i, ((vid, zf, zt, zb), (oy, ox, gain, cutoff, k)) in enumerate(zip(samples, transforms)):
        _, H, W = aug.shapes[vid]
        d[i] = hip.TripletDesc(aug.offsets[vid], H, W, zf, zt, zb, oy, ox, k, gain, cutoff)
    return d


def _plain_triplets(hip, aug, samples, transforms, W, raw):
    """aesr_triplet_assemble / _raw on the image cache alone -> (image [2B,1,W,W], between [B,1,W,W])"""
    B = len(samples)
    image = torch.full((2 * B, 1, W, W), float("nan"), device="cuda")
    between = torch.full((B, 1, W, W), float("nan"), device="cuda")
    fn = hip.lib.aesr_triplet_assemble_raw if raw else hip.lib.aesr_triplet_assemble
    hip.check(fn(hip.ptr(aug.cache), _descs(hip, aug, samples, transforms), B, W, hip.ptr(image), hip.ptr(between), hip.stream()), "aesr_triplet_assemble")
    torch.cuda.synchronize()
    return image, between


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ["one", "two"])
@pytest.mark.parametrize("leg", tl.LEG_IDS)
def test_kernel_against_the_reference_and_the_existing_kernel(leg, arrangement):
    from superresolution_aniso_mri_amd import _hip as hip
    fx, _ = tl.fixture()
    key = "%s/%s" % (leg, arrangement)
    test = tl.leg_settings(fx, leg)[3]
    aug = tl.make_augmenter(fx, leg, arrangement, "cuda")
    samples, inb, transforms, size = tl.draw_leg(fx, leg, arrangement, aug)
    out = aug.assemble(samples, transforms, raw=test, size=size)
    torch.cuda.synchronize()
    image, between = out["image"], out["slice_between"]
    err = max(float(np.abs(image[:, 0].cpu().numpy().astype(np.float64) - fx[key + "/image"][:, 0]).max()),
              float(np.abs(between[:, 0].cpu().numpy().astype(np.float64) - fx[key + "/slice_between"][:, 0]).max()))
    print("%s: images max |kernel - reference| %.3g (bound %.1g%s)" % (key, err, tl.TOL, ", bitwise asked" if test else ""))
    tl.assert_batch(image.cpu().numpy(), between.cpu().numpy(), fx, key, exact_images=test)
    assert np.array_equal(out["is_inbetween"].cpu().numpy(), fx[key + "/batch_is_inbetween"])
    assert np.array_equal(out["loss_mask"].cpu().numpy(), fx[key + "/batch_loss_mask"])
    B = len(samples)
    assert out["alpha_from"].shape == (B, 1) and bool((out["alpha_from"] == 0.5).all()) and bool((out["alpha_to"] == 0.5).all())
    assert "_persistent" not in out
    # channel 0 is the existing kernel's, bit for bit
    W = image.shape[-1]
    img1, btw1 = _plain_triplets(hip, aug, samples, transforms, W, raw=test)
    assert torch.equal(mg.bits(image[:, 0]), mg.bits(img1[:, 0])), "%s: image channel 0 differs from aesr_triplet_assemble%s" % (key, "_raw" if test else "")
    assert torch.equal(mg.bits(between[:, 0]), mg.bits(btw1[:, 0]))
    # the training legs through the raw entry point too: the samples unchanged, rotated and cropped the same way
    if not test:
        img2, btw2 = torch.empty_like(image), torch.empty_like(between)
        hip.check(hip.lib.aesr_labelled_triplet_assemble_raw(hip.ptr(aug.cache), hip.ptr(aug.label_cache), _descs(hip, aug, samples, transforms), B, W,
                                                             hip.ptr(img2), hip.ptr(btw2), hip.stream()), "aesr_labelled_triplet_assemble_raw")
        img3, btw3 = _plain_triplets(hip, aug, samples, transforms, W, raw=True)
        assert torch.equal(img2[:, 1], image[:, 1]) and torch.equal(btw2[:, 1], between[:, 1])
        assert torch.equal(mg.bits(img2[:, 0]), mg.bits(img3[:, 0])) and torch.equal(mg.bits(btw2[:, 0]), mg.bits(btw3[:, 0]))
        vals = torch.unique(torch.cat([torch.from_numpy(v).reshape(-1) for v in tl.leg_volumes(fx, leg)[0]] + [torch.zeros(1)]))
        assert bool(torch.isin(img2[:, 0].cpu().reshape(-1), vals).all())          # copied, never mixed


# ---- batch sizes, shards, persistent output ---------------------------------------------------------------------------------------------
def _small_augmenter(seed, width=4, aug=6, sel="mix"):
    from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter
    rs = np.random.RandomState(99)
    shapes = [(5, 7, 9), (4, 6, 5), (6, 3, 8)]
    vols = [rs.rand(*s).astype(np.float32) for s in shapes]
    labs = [rs.randint(0, 256, s).astype(np.uint8) for s in shapes]          # any byte value is copied as it is
    return LabelledTripletAugmenter(vols, labs, width, aug, slice_selection=sel, rs=np.random.RandomState(seed), device="cuda"), vols, labs


def _draw(aug, B, raw=False):
    samples, transforms = [], []
    for _ in range(B):
        vid = int(aug.rs.randint(0, len(aug.shapes)))
        s, _, t = aug.draw_sample(vid, int(aug.rs.randint(0, aug.shapes[vid][0])), raw=raw)
        samples.append(s)
        transforms.append(t)
    return samples, transforms


@pytest.mark.parametrize("raw", [False, True], ids=["curve", "raw"])
def test_one_sample_and_65_samples_equal_single_calls(raw):
    aug, vols, labs = _small_augmenter(5)
    samples, transforms = _draw(aug, 65, raw)
    W = aug.test_size() if raw else aug.width
    assert W == (6 if raw else 4)
    singles = [aug.assemble([s], [t], raw=raw) for s, t in zip(samples, transforms)]
    assert singles[0]["image"].shape == (2, 2, W, W) and singles[0]["slice_between"].shape == (1, 2, W, W)
    want_img, want_btw = tl.gather_by_descriptor(vols, labs, samples, transforms, W, raw)
    one = singles[0]
    assert np.array_equal(one["image"][:, 1].cpu().numpy(), want_img[[0, 65], 1]) and np.array_equal(one["slice_between"][:, 1].cpu().numpy(), want_btw[:1, 1])
    big = aug.assemble(samples, transforms, raw=raw)
    torch.cuda.synchronize()
    assert big["image"].shape == (130, 2, W, W) and big["slice_between"].shape == (65, 2, W, W) and big["is_inbetween"].shape == (130, 1)
    for b, s in enumerate(singles):
        assert torch.equal(mg.bits(big["image"][b]), mg.bits(s["image"][0])), b
        assert torch.equal(mg.bits(big["image"][65 + b]), mg.bits(s["image"][1])), b
        assert torch.equal(mg.bits(big["slice_between"][b]), mg.bits(s["slice_between"][0])), b
        assert float(big["is_inbetween"][b]) == float(s["is_inbetween"][0]) == float(big["is_inbetween"][65 + b])
    assert np.array_equal(big["image"][:, 1].cpu().numpy(), want_img[:, 1]) and np.array_equal(big["slice_between"][:, 1].cpu().numpy(), want_btw[:, 1])
    assert float(np.abs(big["image"][:, 0].cpu().numpy() - want_img[:, 0]).max()) <= (0 if raw else tl.TOL)
    assert len(set(np.unique(want_img[:, 1]))) > 100          # bytes above any class count went through


@pytest.mark.parametrize("raw", [False, True], ids=["curve", "raw"])
def test_shards_equal_the_single_process_batch(raw):
    full = _small_augmenter(17)[0].next_batch(7, raw=raw)
    for world in (2, 3, 7):
        parts = []
        for rank in range(world):
            aug = _small_augmenter(17)[0]
            parts.append(aug.next_batch(7, shard=(rank, world), raw=raw))
            assert aug.rs.randint(0, 1 << 30) == _after_full(raw)          # every rank leaves the stream where one process leaves it
        n = [p["slice_between"].shape[0] for p in parts]
        assert sum(n) == 7 and all(p["image"].shape[0] == 2 * k for p, k in zip(parts, n))
        image = torch.cat([p["image"][:k] for p, k in zip(parts, n)] + [p["image"][k:] for p, k in zip(parts, n)])
        assert torch.equal(mg.bits(image), mg.bits(full["image"])), world
        assert torch.equal(mg.bits(torch.cat([p["slice_between"] for p in parts])), mg.bits(full["slice_between"]))
        inb = torch.cat([p["is_inbetween"][:k] for p, k in zip(parts, n)] * 2)
        assert torch.equal(inb, full["is_inbetween"])


def _after_full(raw):
    aug = _small_augmenter(17)[0]
    aug.next_batch(7, raw=raw)
    return aug.rs.randint(0, 1 << 30)


def test_reuse_output_is_persistent():
    aug, _, _ = _small_augmenter(3, sel="adjacent_plus")
    ref, _, _ = _small_augmenter(3, sel="adjacent_plus")
    a = aug.next_batch(5, reuse_output=True)
    first = a["image"].clone(), a["slice_between"].clone()
    b = aug.next_batch(5, reuse_output=True)
    assert a["_persistent"] is True and b["_persistent"] is True
    assert b["image"].data_ptr() == a["image"].data_ptr() and b["slice_between"].data_ptr() == a["slice_between"].data_ptr()
    assert b["slice_between"].data_ptr() == a["image"].data_ptr() + 10 * 2 * 16 * 4          # one [3B, 2, W, W] buffer
    assert b["image"].shape == (10, 2, 4, 4) and b["slice_between"].shape == (5, 2, 4, 4) and b["image"].is_contiguous()
    r1, r2 = ref.next_batch(5), ref.next_batch(5)
    assert "_persistent" not in r1 and r1["image"].data_ptr() != r2["image"].data_ptr()
    assert torch.equal(first[0], r1["image"]) and torch.equal(first[1], r1["slice_between"])
    assert torch.equal(b["image"], r2["image"]) and torch.equal(b["slice_between"], r2["slice_between"]) and torch.equal(b["is_inbetween"], r2["is_inbetween"])
    assert aug.next_batch(3, reuse_output=True)["image"].data_ptr() != a["image"].data_ptr()          # another batch size, another buffer


# ---- between guard bands ----------------------------------------------------------------------------------------------------------------
class _ByteGuarded:
    """A uint8 payload at ANY byte offset between two guard regions (tests/memguard.py moves byte buffers by 4): the whole allocation outside
    the payload is compared with a copy taken before the call."""

    def __init__(self, data, shift_bytes, name):
        n, g = data.numel(), mg.GUARD_ELEMS * 4
        self.name, self.backing = name, torch.empty((g + 16 + n + 16 + g + 3) // 4 * 4, dtype=torch.uint8, device="cuda")
        self.backing.view(torch.int32).fill_(mg.GUARD_WORD)
        self.off = g + (-(self.backing.data_ptr() + g)) % 16 + shift_bytes
        self.view = self.backing[self.off:self.off + n]
        self.view.copy_(data.reshape(-1))
        assert self.view.data_ptr() % 16 == shift_bytes
        self.before = self.backing.cpu().clone()

    def assert_intact(self):
        assert torch.equal(self.backing.cpu(), self.before), "%s: the label cache or its surroundings were modified" % self.name


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _guarded_call(hip, entry, aug, samples, transforms, W, poison, shift, refuse=None):
    """One entry point, every device buffer between guard bands at its contractual size.  shift: elements (4 bytes) the float buffers start past
    a 16-byte boundary, and BYTES the label cache does.  refuse: (argument, value) -> the call must be refused and leave the poison."""
    B = len(samples)
    images = mg.guarded(aug.cache.numel(), torch.float32, "cuda", aug.cache, shift, "images")
    labels = _ByteGuarded(aug.label_cache, shift, "labels")
    image = mg.guarded(2 * B * 2 * W * W, torch.float32, "cuda", poison, shift, "image")
    between = mg.guarded(B * 2 * W * W, torch.float32, "cuda", poison, shift, "between")
    for g in (images, image, between):
        assert g.view.data_ptr() % 16 == 4 * shift
    saved = mg.bits(images.view)
    names = ["images", "labels", "desc", "B", "W", "image", "between", "stream"]
    args = [_p(images.view), _p(labels.view), _descs(hip, aug, samples, transforms), B, W, _p(image.view), _p(between.view), hip.stream()]
    if refuse is not None:
        args[names.index(refuse[0])] = refuse[1]
    torch.cuda.synchronize()
    rc = getattr(hip.lib, entry)(*args)
    torch.cuda.synchronize()
    mg.assert_guards_intact([images, image, between])
    mg.assert_unchanged(images.view, saved, "images")
    labels.assert_intact()
    if refuse is not None:
        assert rc == 1 and (entry + ":") in hip.last_error(), (entry, refuse, rc, hip.last_error())
        for g in (image, between):
            assert mg.poison_left(g.view, poison).numel() == g.view.numel(), "%s %s: refused, yet %s was written" % (entry, refuse, g.name)
        return None
    assert rc == 0, hip.last_error()
    for g in (image, between):
        left = mg.poison_left(g.view, poison)
        assert left.numel() == 0, "%s: %d element(s) never written, first %d [poison %s, shift %d]" % (g.name, left.numel(), int(left[0]), poison, shift)
    return image.view.reshape(2 * B, 2, W, W), between.view.reshape(B, 2, W, W)


@pytest.mark.parametrize("entry", GUARDED_ENTRIES)
def test_guard_bands_poisons_and_offset_pointers(entry):
    """NaN poison and finite poison; float pointers 0, 4, 8 and 12 bytes past a 16-byte boundary, the label cache 0, 1, 2 and 3 bytes: guards
    intact, both caches unchanged, every output element written, the results bit-identical across the legs and equal to the plain call."""
    from superresolution_aniso_mri_amd import _hip as hip
    raw = entry.endswith("_raw")
    for width, aug_size in ((4, 6), (10, 10)):          # a crop inside the canvas; no crop, a canvas larger than every slice, more than one wave
        aug, _, _ = _small_augmenter(23, width, aug_size)
        samples, transforms = _draw(aug, 5)          # the training transforms for both entry points: rotations and crops
        plain = aug.assemble(samples, transforms, raw=False)
        if raw:
            img = torch.empty_like(plain["image"])
            btw = torch.empty_like(plain["slice_between"])
            hip.check(hip.lib.aesr_labelled_triplet_assemble_raw(hip.ptr(aug.cache), hip.ptr(aug.label_cache), _descs(hip, aug, samples, transforms), 5,
                                                                 width, hip.ptr(img), hip.ptr(btw), hip.stream()), entry)
            plain = {"image": img, "slice_between": btw}
        for poison, shift in ((mg.POISON_NAN, 0), (mg.POISON_FINITE, 0), (mg.POISON_NAN, 1), (mg.POISON_FINITE, 2), (mg.POISON_NAN, 3)):
            image, between = _guarded_call(hip, entry, aug, samples, transforms, width, poison, shift)
            assert torch.equal(mg.bits(image), mg.bits(plain["image"])), (entry, width, poison, shift)
            assert torch.equal(mg.bits(between), mg.bits(plain["slice_between"])), (entry, width, poison, shift)


def test_refusals_write_nothing():
    from superresolution_aniso_mri_amd import _hip as hip
    aug, _, _ = _small_augmenter(23)
    samples, transforms = _draw(aug, 3)

    def bad_desc(**over):
        d = _descs(hip, aug, samples, transforms)
        for k, v in over.items():
            setattr(d[2], k, v)
        return d

    cases = [("images", None), ("labels", None), ("desc", None), ("image", None), ("between", None), ("B", 0), ("B", 65), ("B", -3), ("W", 0),
             ("W", -4), ("W", 32768), ("desc", bad_desc(k=4)), ("desc", bad_desc(k=-1)), ("desc", bad_desc(H=0)), ("desc", bad_desc(W=0)),
             ("desc", bad_desc(vol_off=-1)), ("desc", bad_desc(z_between=-1))]
    for n, case in enumerate(cases):
        for entry in GUARDED_ENTRIES:
            poison = (mg.POISON_NAN, mg.POISON_FINITE)[(n + entry.endswith("_raw")) % 2]          # each entry point sees both
            assert _guarded_call(hip, entry, aug, samples, transforms, 4, poison, 0, refuse=case) is None
    # the host layer checks slice indices against Z, which a descriptor does not carry, before any launch
    with pytest.raises(ValueError, match="slice index outside"):
        aug.assemble([(1, 0, 4, 2)], transforms=[(0, 0, 3.0, 0.5, 0)])


# ---- order=0 in-plane resampling on the device ------------------------------------------------------------------------------------------
def test_apply_2d_zoom_order0_equals_the_reference_exactly():
    from superresolution_aniso_mri_amd.datasets import common as dc
    fx = np.load(os.path.join(HERE, "golden", "inplane_labels.npz"))
    for tag in [str(t) for t in fx["tags"]]:
        a, want = fx[tag + "/in"], fx[tag + "/out"]
        sp, nsp = tuple(fx[tag + "/spacing"]), tuple(fx[tag + "/new_spacing"])
        fn = dc.apply_2d_zoom_4d if a.ndim == 4 else dc.apply_2d_zoom_3d
        n0 = dc.LAUNCHES
        got = fn(a.astype(np.float32), sp, nsp, order=0, do_blur=False, as_type=int)
        assert dc.LAUNCHES == n0 + 1, "%s: %d launches" % (tag, dc.LAUNCHES - n0)          # a 4-D array is one launch
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), tag
        x = torch.from_numpy(a.astype(np.float32)).cuda()
        kept = x.clone()
        dev = fn(x, sp, nsp, order=0, do_blur=False)          # device in, device out; float: the samples themselves
        assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.float32 and torch.equal(x, kept)
        assert torch.equal(dev.cpu(), torch.from_numpy(want.astype(np.float32))), tag
        assert fn(x, sp, nsp, order=0, do_blur=False, as_type=int).dtype == torch.int64
    # order=1 on the same labels mixes class ids at borders; order=0 never does
    a = fx["a_in_125/in"].astype(np.float32)
    lin = dc.apply_2d_zoom_3d(a, tuple(fx["a_in_125/spacing"]), tuple(fx["a_in_125/new_spacing"]), do_blur=False)
    assert (lin != np.round(lin)).any()
    with pytest.raises(NotImplementedError, match="order"):
        dc.apply_2d_zoom_3d(a, (1.25, 1.25), (1.4, 1.4), order=3)


def test_load_labelled_volume_dir_resamples_images_and_labels(tmp_path):
    from superresolution_aniso_mri_amd import volume_io
    from superresolution_aniso_mri_amd.data_device import load_labelled_volume_dir
    from superresolution_aniso_mri_amd.datasets import common as dc
    rs = np.random.RandomState(8)
    data, labs = tmp_path / "vols", tmp_path / "labels"
    data.mkdir()
    labs.mkdir()
    ids = np.array([0, 2, 5, 200], np.uint8)
    img3, lab3 = rs.rand(4, 40, 36).astype(np.float32), ids[rs.randint(0, 4, (4, 10, 9))].repeat(4, 1).repeat(4, 2)
    img4, lab4 = (500 * rs.rand(2, 3, 30, 44)).astype(np.float32), ids[rs.randint(0, 4, (2, 3, 6, 11))].repeat(5, 2).repeat(4, 3)
    sp3, sp4 = (1.5625, 1.5625, 8.0), (1.25, 1.1, 10.0, 1.0)          # (x, y, z[, t])
    volume_io.write_volume(str(data / "p1.nii.gz"), volume_io.Volume(img3, sp3, "npy", {}), img3, sp3)
    volume_io.write_volume(str(labs / "p1.nii"), volume_io.Volume(lab3, sp3, "npy", {}), lab3, sp3)          # another extension, the same stem
    volume_io.write_volume(str(data / "p2.nii.gz"), volume_io.Volume(img4, sp4, "npy", {}), img4, sp4)
    np.save(str(labs / "p2.npy"), lab4)          # a label file without a header: the image file's spacing serves both
    vols, labels = load_labelled_volume_dir(str(data), str(labs), resample=True)
    assert len(vols) == len(labels) == 3
    want3 = dc.apply_2d_zoom_3d(img3.copy(), (8.0, 1.5625, 1.5625), (1.4, 1.4))
    assert vols[0].shape == labels[0].shape == want3.shape == (4, 45, 40) and np.array_equal(vols[0], want3)
    assert vols[1].shape == labels[1].shape == vols[2].shape == labels[2].shape == (3, dc.out_size(30, 1.1 / 1.4), dc.out_size(44, 1.25 / 1.4))
    for v, l in zip(vols, labels):
        assert l.dtype == np.uint8 and set(np.unique(l)) <= set(ids.tolist()) and len(np.unique(l)) == 4 and 0 <= v.min() and v.max() <= 1
    plain_v, plain_l = load_labelled_volume_dir(str(data), str(labs), new_spacing=(1.0, 1.0))          # without resample nothing moves
    assert np.array_equal(plain_l[0], lab3) and np.array_equal(plain_l[2], lab4[1]) and np.array_equal(plain_v[0], img3)
    finer = load_labelled_volume_dir(str(data), str(labs), resample=True, new_spacing=(1.25, 1.25))
    assert finer[0][0].shape == finer[1][0].shape == (4, 50, 45)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_train_generate_and_score_from_volume_and_label_directories(tmp_path):
    from superresolution_aniso_mri_amd import generate_hr_volumes, train_aesr
    from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    data, labs = tmp_path / "vols", tmp_path / "labels"
    data.mkdir()
    labs.mkdir()
    ids = [0, 1, 2, 3]
    zz, yy, xx = np.meshgrid(np.arange(8.0), np.arange(40.0), np.arange(36.0), indexing="ij")
    written = []
    for n, (cy, cx) in enumerate(((19.0, 17.0), (21.0, 18.5))):
        field = np.exp(-((yy - cy - 0.5 * zz) ** 2 + (xx - cx + 0.4 * zz) ** 2) / (2 * 8.0 ** 2))
        lab = np.floor(4 * 0.999 * field).astype(np.uint8)
        assert set(np.unique(lab)) == set(ids)
        np.save(str(data / ("vol%d.npy" % n)), field.astype(np.float32))
        np.save(str(labs / ("vol%d.npy" % n)), lab)
        written.append((field.astype(np.float32), lab))
    seen = []
    keep = LabelledTripletAugmenter.next_batch

    def spy(self, *a, **k):
        out = keep(self, *a, **k)
        seen.append((k.get("raw", False), out["image"], out["slice_between"]))
        return out

    LabelledTripletAugmenter.next_batch = spy
    try:
        trainers = {}
        for model in ("ae_combined", "ae"):
            out = str(tmp_path / "expers")
            trainers[model] = train_aesr.main(
                ["--dataset=ACDCLBL", "--model=" + model, "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8", "--width=32",
                 "--depth=8", "--downsample_steps=2", "--epochs=2", "--lr=0.001", "--ex_loss_weight1=0.05", "--exper_id=" + model,
                 "--output_dir=" + out, "--volumes_dir=" + str(data), "--labels_dir=" + str(labs), "--aug_patch_size=36", "--iters_per_epoch=3",
                 "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    finally:
        LabelledTripletAugmenter.next_batch = keep
    assert type(trainers["ae_combined"]).__name__ == "MultiChannelCAISRTrainer" and type(trainers["ae"]).__name__ == "MultiChannelTrainer"
    for model, tr in trainers.items():
        src = os.path.join(str(tmp_path / "expers"), model)
        assert type(tr.model).__name__ == "MultiChannelAE" and tr.iters == 1 + 6
        assert os.path.isfile(os.path.join(src, "settings.yaml")) and os.path.isfile(os.path.join(src, "models", "2.models"))
        assert np.isfinite(tr.mean_losses["loss_label"][-1]) and np.isfinite(tr.mean_losses_test["loss_label"][-1]), model
        if model == "ae_combined":          # the loss on the synthesised slice in between belongs to the combined trainer alone
            assert np.isfinite(tr.mean_losses["loss_ae_dist_labels"][-1]) and np.isfinite(tr.mean_losses_test["loss_ae_dist_labels"][-1])
    # per run one validation batch (the test transform: a 36 x 36 centre crop, the intensities unchanged) and six training batches
    assert [raw for raw, _, _ in seen] == ([True] + [False] * 6) * 2
    values = torch.unique(torch.cat([torch.from_numpy(f).reshape(-1) for f, _ in written]))
    for raw, image, between in seen:
        W = 36 if raw else 32
        assert image.shape == (8, 2, W, W) and between.shape == (4, 2, W, W)
        for t in (image, between):
            assert set(torch.unique(t[:, 1]).tolist()) <= set(float(i) for i in ids), "label channels hold only the written ids"
            assert bool(torch.isfinite(t).all()) and float(t[:, 0].min()) >= 0 and float(t[:, 0].max()) <= 1
        if raw:
            assert bool(torch.isin(image[:, 0].cpu().reshape(-1), values).all())
    src = os.path.join(str(tmp_path / "expers"), "ae_combined")
    res = generate_hr_volumes.main(["--exper_dir=" + src, "--model_nbr=2", "--num_interpolations=3", "--data_input_dir=" + str(data),
                                    "--labels_input_dir=" + str(labs), "--output_dir=" + str(tmp_path / "hr"), "--save"])
    hr, hl = np.load(str(tmp_path / "hr" / "vol0.npy")), np.load(str(tmp_path / "hr" / "vol0_labels.npy"))
    assert len(res) == 2 * 2 and hr.shape == hl.shape == (29, 40, 36) and hr.dtype == np.float32 and hl.dtype == np.uint8
    assert hl.max() <= 3 and np.array_equal(hl[::4], written[0][1])
    for model, tr in trainers.items():
        tr.model.eval()
        field, lab = written[0]
        got = seg_metrics.score_label_supervolume(tr, torch.from_numpy(field[:7]), torch.from_numpy(lab[:7].astype(np.float32)), 2, (10.0, 1.4, 1.4),
                                                  classes=[1, 2, 3])
        assert sorted(got) == ["model", "nearest"]
        for k in seg_metrics.SCORE_KEYS:
            assert got["nearest"][k].shape == (1, 3) and np.isfinite(got["nearest"][k]).all(), (model, k)
            assert got["model"][k].shape == (1, 3)
        # the labels hold every class, so the overlap scores exist; a class the barely trained model never predicts has no surface to measure
        assert np.isfinite(got["model"]["dice"]).all(), model
