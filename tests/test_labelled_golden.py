"""not gpu: labelled triplet batches against the reference's own results (tests/golden/labelled_batches.npz, written by
tests/make_golden_labelled.py from datasets/ACDC/data_with_labels.py, datasets/shared_transforms.py and prepare_batch_pairs of the
reference; tests/golden/inplane_labels.npz, written by tests/make_golden_inplane_labels.py from its apply_2d_zoom_3d / _4d(order=0)).

- A numpy restatement of the pipeline, kept in this file (``restate_batch``): gather the six channels, pad, centre crop, random crop, the
  sigmoid on the image channels only (float64 on float32 data, as the reference evaluates it), rot90, the 6-channel layout of
  prepare_batch_pairs.  From the recorded draws it reproduces every fixture batch: labels exactly, images within 2e-6 (the bound
  tests/test_gpu_augment.py holds the existing augmenter to).  It shares no code with the package.
- ``LabelledTripletAugmenter.draw_sample`` / ``draw_transform`` reproduce every recorded slice id and every number the transforms drew, with one
  shared RandomState and with two.  The descriptors they give, run through a numpy statement of the kernel's contract
  (``gather_by_descriptor``: include/aesr_hip_labelprep.h), reproduce the batches too -- the test transform's two branches included.
- The ``order=0`` tables of ``datasets.common.zoom_tables``, applied in numpy, equal inplane_labels.npz exactly.
- Every argument refusal of the two entry points returns its code before anything touches the device: callable without a GPU.
- Every host refusal of the loader and the augmenter; the command line."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = {"aesr_labelled_triplet_assemble", "aesr_labelled_triplet_assemble_raw"}
TOL = 2e-6          # tests/test_gpu_augment.py: fp32 expf against the reference's float64 curve
_FX = {}


def fixture():
    if not _FX:
        _FX.update(np.load(os.path.join(HERE, "golden", "labelled_batches.npz")))
    return _FX, [str(t) for t in _FX["legs"]]


def leg_volumes(fx, leg):
    vols, labs = [], []
    while "%s/vol%d" % (leg, len(vols)) in fx:
        labs.append(fx["%s/lab%d" % (leg, len(vols))])
        vols.append((fx["%s/vol%d" % (leg, len(vols))] / 1024.0).astype(np.float32))
    return vols, labs


def leg_settings(fx, leg):
    """(width, aug_patch_size, slice_selection, test transform, its padding branch)"""
    return (int(fx[leg + "/width"]), int(fx[leg + "/aug_patch_size"]), str(fx[leg + "/slice_selection"]), bool(fx[leg + "/test"]),
            bool(fx[leg + "/pad_branch"]))


def make_augmenter(fx, leg, arrangement, device):
    """The augmenter that mirrors the reference's dataset + transforms of a leg.  The padding branch of the test transform belongs to
    width > 128 in the training script; the fixture's slices are small, so that leg names its canvas (``size=``) instead."""
    from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter
    width, aug, sel, _, _ = leg_settings(fx, leg)
    one, d_seed, t_seed = (int(s) for s in fx["seeds"])
    vols, labs = leg_volumes(fx, leg)
    if arrangement == "one":
        rs = np.random.RandomState(one)
        return LabelledTripletAugmenter(vols, labs, width, aug, slice_selection=sel, rs=rs, device=device)
    return LabelledTripletAugmenter(vols, labs, width, aug, slice_selection=sel, rs=np.random.RandomState(d_seed),
                                    rs_transform=np.random.RandomState(t_seed), device=device)


def draw_leg(fx, leg, arrangement, aug):
    """The samples of a leg drawn the way the reference's loop draws them -> (samples, is_inbetween, transforms, canvas of a raw leg)"""
    key = "%s/%s" % (leg, arrangement)
    _, _, _, test, pad_branch = leg_settings(fx, leg)
    size = aug.width if pad_branch else None
    samples, inb, transforms = [], [], []
    for vid, sid in zip(fx[key + "/vol"], fx[key + "/slice_id"]):
        s, i, t = aug.draw_sample(int(vid), int(sid), raw=test)
        samples.append(s)
        inb.append(i)
        transforms.append(aug.test_transform(int(vid), size) if test else t)
    return samples, inb, transforms, size


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _pad_to(x, patch):
    """AdjustToPatchSize((patch, patch)) on [C, H, W]: zeros, the odd one on the far side"""
    _, h, w = x.shape
    dh, dw = max(0, patch - h), max(0, patch - w)
    return np.pad(x, ((0, 0), (dh // 2, dh - dh // 2), (dw // 2, dw - dw // 2)), "constant")


def _centre_crop(x, size):
    _, h, w = x.shape
    half = int(size / 2)
    assert h // 2 - half >= 0 and w // 2 - half >= 0
    return x[:, h // 2 - half:h // 2 + half, w // 2 - half:w // 2 + half]


def restate_batch(fx, leg, arrangement):
    """(image [2B, 2, W, W], slice_between [B, 2, W, W]) float32 from the volumes and the RECORDED draws of a leg."""
    key = "%s/%s" % (leg, arrangement)
    width, aug, _, test, pad_branch = leg_settings(fx, leg)
    vols, labs = leg_volumes(fx, leg)
    rows = []
    for n in range(len(fx[key + "/vol"])):
        v, l = vols[int(fx[key + "/vol"][n])], labs[int(fx[key + "/vol"][n])]
        zs = [int(fx["%s/%s" % (key, name)][n]) for name in ("id_from", "id_to", "id_between")]
        x = np.stack([a[z] for z in zs for a in (v, l)]).astype(np.float32)          # image, labels, image, labels, image, labels
        if test:
            x = _centre_crop(_pad_to(x, width), width) if pad_branch else _centre_crop(x, aug)
        else:
            x = _centre_crop(_pad_to(x, aug), aug)
            top, left = int(fx[key + "/top"][n]), int(fx[key + "/left"][n])
            if top >= 0:
                x = x[:, top:top + width, left:left + width]
            assert x.shape == (6, width, width)
            gain, cutoff = float(fx[key + "/gain"][n]), float(fx[key + "/cutoff"][n])
            x = x.copy()
            x[0::2] = (1.0 / (1.0 + np.exp(gain * (cutoff - x[0::2].astype(np.float64))))).astype(np.float32)
            x = np.rot90(x, int(fx[key + "/k"][n]), (1, 2))
        rows.append(x)
    rows = np.stack(rows)
    return np.concatenate([rows[:, 0:2], rows[:, 2:4]]), rows[:, 4:6]


def gather_by_descriptor(vols, labs, samples, transforms, W, raw):
    """include/aesr_hip_labelprep.h in numpy: out[i][j] = src[oy + u][ox + v], (u, v) = rot90^-k (i, j), 0 outside; the curve in float64."""
    ii, jj = np.mgrid[0:W, 0:W]
    out = np.zeros((len(samples), 3, 2, W, W), np.float32)
    for b, ((vid, zf, zt, zb), (oy, ox, gain, cutoff, k)) in enumerate(zip(samples, transforms)):
        u, v = [(ii, jj), (jj, W - 1 - ii), (W - 1 - ii, W - 1 - jj), (W - 1 - jj, ii)][k]
        y, x = oy + u, ox + v
        _, H, Wv = vols[vid].shape
        inside = (y >= 0) & (y < H) & (x >= 0) & (x < Wv)
        yc, xc = np.clip(y, 0, H - 1), np.clip(x, 0, Wv - 1)
        for s, z in enumerate((zf, zt, zb)):
            img = np.where(inside, vols[vid][z][yc, xc], np.float32(0))
            out[b, s, 0] = img if raw else (1.0 / (1.0 + np.exp(gain * (cutoff - img.astype(np.float64))))).astype(np.float32)
            out[b, s, 1] = np.where(inside, labs[vid][z][yc, xc], 0).astype(np.float32)
    return np.concatenate([out[:, 0], out[:, 1]]), out[:, 2]


def assert_batch(got_image, got_between, fx, key, exact_images):
    for name, got in (("image", got_image), ("slice_between", got_between)):
        want = fx["%s/%s" % (key, name)]
        assert got.shape == want.shape and got.dtype == np.float32, (key, name, got.shape, want.shape)
        assert np.array_equal(got[:, 1], want[:, 1]), "%s %s: %d label(s) differ" % (key, name, int((got[:, 1] != want[:, 1]).sum()))
        err = float(np.abs(got[:, 0].astype(np.float64) - want[:, 0]).max())
        assert (np.array_equal(got[:, 0], want[:, 0]) if exact_images else err <= TOL), (key, name, err)


LEG_IDS = ["a_crop", "b_nocrop", "c_mix", "d_adj", "e_test128", "e_testpad"]


def test_fixture_is_what_the_issue_asked_for():
    fx, legs = fixture()
    assert legs == LEG_IDS
    assert os.path.getsize(os.path.join(HERE, "golden", "labelled_batches.npz")) < 1 << 20
    shapes = {leg: [v.shape for v in leg_volumes(fx, leg)[0]] for leg in legs}
    assert shapes["a_crop"] == [(7, 20, 18)] * 2 + [(6, 13, 24)] * 2 and shapes["b_nocrop"] == [(5, 11, 9)] * 4
    assert leg_settings(fx, "a_crop")[:2] == (8, 12) and leg_settings(fx, "b_nocrop")[:2] == (16, 16)
    for leg in legs:
        vols, labs = leg_volumes(fx, leg)
        for v, l in zip(vols, labs):
            assert l.dtype == np.uint8 and l.shape == v.shape and set(np.unique(l)) == {0, 1, 2, 3} and 0 <= v.min() and v.max() <= 1
        test = leg_settings(fx, leg)[3]
        for arrangement in ("one", "two"):
            key = "%s/%s" % (leg, arrangement)
            B = len(fx[key + "/vol"])
            assert B >= 12 and fx[key + "/image"].shape[:2] == (2 * B, 2) and fx[key + "/slice_between"].shape[:2] == (B, 2)
            assert test or set(fx[key + "/k"]) == {0, 1, 2, 3}
            assert ((fx[key + "/top"] >= 0).all() and (fx[key + "/left"] >= 0).all()) if leg in ("a_crop", "c_mix", "d_adj") else (fx[key + "/top"] == -1).all()
            assert fx[key + "/batch_is_inbetween"].shape == (2 * B, 1) and fx[key + "/batch_loss_mask"].shape == (2 * B, 1)
    for arrangement in ("one", "two"):
        assert set(fx["c_mix/%s/step" % arrangement]) == {1, 2} and set(fx["c_mix/%s/is_inbetween" % arrangement]) == {0, 1}
        assert set(fx["d_adj/%s/step" % arrangement]) == {1} and set(fx["d_adj/%s/is_inbetween" % arrangement]) == {0}
        assert set(fx["a_crop/%s/step" % arrangement]) == {2} and set(fx["a_crop/%s/is_inbetween" % arrangement]) == {1}


@pytest.mark.parametrize("arrangement", ["one", "two"])
@pytest.mark.parametrize("leg", LEG_IDS)
def test_restatement_reproduces_the_reference(leg, arrangement):
    fx, _ = fixture()
    image, between = restate_batch(fx, leg, arrangement)
    assert_batch(image, between, fx, "%s/%s" % (leg, arrangement), exact_images=leg_settings(fx, leg)[3])


@pytest.mark.parametrize("arrangement", ["one", "two"])
@pytest.mark.parametrize("leg", LEG_IDS)
def test_draws_and_descriptors_reproduce_the_reference(leg, arrangement):
    fx, _ = fixture()
    key = "%s/%s" % (leg, arrangement)
    width, _, _, test, _ = leg_settings(fx, leg)
    aug = make_augmenter(fx, leg, arrangement, "cpu")
    assert (aug.rs_transform is aug.rs) == (arrangement == "one")
    samples, inb, transforms, size = draw_leg(fx, leg, arrangement, aug)
    for n, ((vid, zf, zt, zb), i, (oy, ox, gain, cutoff, k)) in enumerate(zip(samples, inb, transforms)):
        assert (zf, zt, zb, i) == tuple(int(fx["%s/%s" % (key, name)][n]) for name in ("id_from", "id_to", "id_between", "is_inbetween"))
        assert abs(zf - zt) == int(fx[key + "/step"][n])
        assert (k, gain, cutoff) == (int(fx[key + "/k"][n]), float(fx[key + "/gain"][n]), float(fx[key + "/cutoff"][n])), (key, n)
        if not test:
            goy, gox, _, _ = aug._geometry(*aug.shapes[vid][1:])
            top, left = max(0, int(fx[key + "/top"][n])), max(0, int(fx[key + "/left"][n]))
            assert (oy, ox) == (goy + top, gox + left), (key, n)
    vols, labs = leg_volumes(fx, leg)
    W = aug.test_size(size) if test else width
    image, between = gather_by_descriptor(vols, labs, samples, transforms, W, raw=test)
    assert_batch(image, between, fx, key, exact_images=test)
    assert np.array_equal(np.array(inb * 2, np.float32).reshape(-1, 1), fx[key + "/batch_is_inbetween"])
    assert (fx[key + "/batch_loss_mask"] == 1).all()


def test_test_transform_branches_by_width():
    """width <= 128: a centre crop of aug_patch_size; above: zero padding to width and a centre crop of width (train_cardiac_aesr.py:99-104)."""
    from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter
    v, l = np.zeros((4, 200, 190), np.float32), np.zeros((4, 200, 190), np.uint8)
    small = LabelledTripletAugmenter([v], [l], 128, 180, device="cpu")
    assert small.test_size() == 180 and small.test_transform(0) == (100 - 90, 95 - 90, 0.0, 0.0, 0)
    large = LabelledTripletAugmenter([v], [l], 224, 256, device="cpu")
    assert large.test_size() == 224 and large.test_transform(0) == (-12, -17, 0.0, 0.0, 0)          # 200 -> 224: 12 rows of padding; 190: 17
    odd = LabelledTripletAugmenter([v], [l], 64, 181, device="cpu")
    assert odd.test_size() == 180          # CenterCrop keeps 2 * int(181 / 2)


# ---- order=0 in-plane resampling ---------------------------------------------------------------------------------------------------
def test_order0_tables_equal_the_reference_exactly():
    from superresolution_aniso_mri_amd.datasets import common as dc
    fx = np.load(os.path.join(HERE, "golden", "inplane_labels.npz"))
    tags = [str(t) for t in fx["tags"]]
    assert {"d_quirk", "d_quirk224", "t_ties", "g_4d"} <= set(tags) and fx["g_4d/in"].ndim == 4
    dead = ties = 0
    for tag in tags:
        a, want = fx[tag + "/in"], fx[tag + "/out"]
        assert a.min() >= 1 and a.max() == 4
        zoom = dc.zoom_factors(fx[tag + "/spacing"], fx[tag + "/new_spacing"])
        H, W = a.shape[-2:]
        Ho, Wo = dc.out_size(H, zoom[0]), dc.out_size(W, zoom[1])
        (iy, ty), (ix, tx) = dc.zoom_tables(H, Ho, order=0), dc.zoom_tables(W, Wo, order=0)
        assert not ty.any() and not tx.any() and iy.max() <= H - 1 and ix.max() <= W - 1
        got = a[..., np.maximum(iy, 0), :][..., :, np.maximum(ix, 0)].astype(np.int64)
        got[..., iy < 0, :] = 0
        got[..., :, ix < 0] = 0
        assert got.shape == want.shape and np.array_equal(got, want), (tag, int((got != want).sum()))
        dead += int((iy < 0).any()) + int((ix < 0).any())
        for n, n_out in ((H, Ho), (W, Wo)):
            c = np.arange(n_out, dtype=np.float64) * (np.float64(n - 1) / np.float64(max(1, n_out - 1)))
            ties += int((c - np.floor(c) == 0.5).any())
        # the linear tables are what they were: the new argument's default changes nothing
        assert all(np.array_equal(p, q) for p, q in zip(dc.zoom_tables(H, Ho), dc.zoom_tables(H, Ho, False, 1)))
    assert dead >= 4 and ties >= 2
    # clamp_edges: a dead line reads the edge instead
    iy, _ = dc.zoom_tables(229, 224, clamp_edges=True, order=0)
    assert iy[-1] == 228 and dc.zoom_tables(229, 224, order=0)[0][-1] == -1
    with pytest.raises(NotImplementedError, match="order"):
        dc.apply_2d_zoom_3d(np.zeros((1, 4, 4), np.float32), (1.0, 1.0), (1.4, 1.4), order=3)
    with pytest.raises(NotImplementedError, match="order"):
        dc.apply_2d_zoom_4d(np.zeros((1, 1, 4, 4), np.float32), (1.0, 1.0), (1.4, 1.4), order=2)


# ---- the entry points ------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    fake = ctypes.c_void_p(4096)

    def descs(n=2, **over):
        d = (_hip.TripletDesc * max(1, n))()
        for i in range(max(1, n)):
            d[i] = _hip.TripletDesc(0, 5, 6, 0, 1, 2, 0, 0, i % 4, 3.0, 0.5)
        for k, v in over.items():
            setattr(d[max(1, n) - 1], k, v)
        return d

    names = ["images", "labels", "desc", "B", "W", "image", "between", "stream"]
    ok = [fake, fake, descs(), 2, 8, fake, fake, None]
    bad = [(n, None) for n in ("images", "labels", "desc", "image", "between")]
    bad += [("B", 0), ("B", -1), ("B", 65), ("W", 0), ("W", -8), ("W", 32768), ("W", 46341)]
    bad += [("desc", descs(k=4)), ("desc", descs(k=-1)), ("desc", descs(H=0)), ("desc", descs(W=-3)), ("desc", descs(vol_off=-1)),
            ("desc", descs(z_from=-1)), ("desc", descs(z_to=-2)), ("desc", descs(z_between=-1)), ("desc", descs(H=32768, W=32768))]
    for fname in sorted(NAMES):
        call = getattr(_hip.lib, fname)
        for name, value in bad:
            args = list(ok)
            args[names.index(name)] = value
            rc = call(*args)
            assert rc == 1 and (fname + ":") in _hip.last_error(), (fname, name, value, rc, _hip.last_error())


# ---- host refusals -----------------------------------------------------------------------------------------------------------------
def _pair_dirs(tmp_path, images, labels):
    d, l = tmp_path / "vols", tmp_path / "labels"
    d.mkdir(parents=True)
    l.mkdir(parents=True)
    for name, a in images.items():
        np.save(str(d / name), a)
    for name, a in labels.items():
        np.save(str(l / name), a)
    return str(d), str(l)


def test_loader_pairs_by_name_and_refuses(tmp_path):
    from superresolution_aniso_mri_amd.data_device import load_labelled_volume_dir
    rs = np.random.RandomState(3)
    img, lab = rs.rand(5, 6, 7).astype(np.float32), rs.randint(0, 4, (5, 6, 7))
    img4, lab4 = 300 * rs.rand(2, 4, 6, 7).astype(np.float32), rs.randint(0, 256, (2, 4, 6, 7)).astype(np.float64)
    d, l = _pair_dirs(tmp_path / "ok", {"b.npy": img, "a4d.npy": img4}, {"b.npy": lab, "a4d.npy": lab4})
    (tmp_path / "ok" / "vols" / "notes.txt").write_text("not a volume")
    vols, labs = load_labelled_volume_dir(d, l)
    assert [v.shape for v in vols] == [(4, 6, 7), (4, 6, 7), (5, 6, 7)] and all(x.dtype == np.uint8 for x in labs)          # sorted by name, a frame each
    assert np.array_equal(vols[2], img) and np.array_equal(labs[2], lab) and np.array_equal(labs[1], lab4[1])
    assert all(0 <= v.min() and v.max() <= 1 for v in vols) and vols[0].max() == 1          # rescaled as load_volume_dir does
    cases = {"shape": ({"v.npy": img}, {"v.npy": lab[:4]}, ValueError, "shape"),
             "fraction": ({"v.npy": img}, {"v.npy": lab + 0.5}, ValueError, "integral"),
             "above": ({"v.npy": img}, {"v.npy": lab + 253}, ValueError, "255"),
             "below": ({"v.npy": img}, {"v.npy": lab - 1}, ValueError, "255"),
             "nolabel": ({"v.npy": img, "w.npy": img}, {"v.npy": lab}, FileNotFoundError, r"w\.npy"),
             "noimage": ({"v.npy": img}, {"v.npy": lab, "x.npy": lab}, FileNotFoundError, r"x\.npy")}
    for tag, (images, labels, exc, match) in cases.items():
        d, l = _pair_dirs(tmp_path / tag, images, labels)
        with pytest.raises(exc, match=match) as e:
            load_labelled_volume_dir(d, l)
        assert "labels" in str(e.value) or "vols" in str(e.value), "the message names the file: %s" % e.value
    d, l = _pair_dirs(tmp_path / "empty", {}, {})
    with pytest.raises(FileNotFoundError):
        load_labelled_volume_dir(d, l)
    d, l = _pair_dirs(tmp_path / "npy_spacing", {"v.npy": img}, {"v.npy": lab})
    with pytest.raises(ValueError, match="spacing"):          # a .npy file carries no spacing to resample from
        load_labelled_volume_dir(d, l, resample=True)


def test_augmenter_refuses_on_the_host():
    from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter as A
    v = lambda z, h=6, w=6: np.zeros((z, h, w), np.float32)          # noqa: E731
    l = lambda z, h=6, w=6: np.zeros((z, h, w), np.uint8)          # noqa: E731
    with pytest.raises(ValueError, match="slice_selection"):
        A([v(5)], [l(5)], 4, 4, slice_selection="random", device="cpu")
    for sel, z, ok in (("adjacent_plus", 3, False), ("adjacent_plus", 4, True), ("mix", 3, False), ("mix", 4, True), ("adjacent", 1, False),
                       ("adjacent", 2, True)):
        if ok:
            a = A([v(z)], [l(z)], 4, 4, slice_selection=sel, rs=np.random.RandomState(1), device="cpu")
            for sid in range(z):          # the neighbour rule stays inside the volume from 2 * step slices on
                for _ in range(4):
                    (_, zf, zt, zb), _, _ = a.draw_sample(0, sid)
                    assert 0 <= zf < z and 0 <= zt < z and 0 <= zb < z
        else:
            with pytest.raises(ValueError, match="at least %d" % (2 if sel == "adjacent" else 4)):
                A([v(5), v(z)], [l(5), l(z)], 4, 4, slice_selection=sel, device="cpu")
    with pytest.raises(ValueError, match="label map"):
        A([v(5)], [l(5, 6, 5)], 4, 4, device="cpu")
    with pytest.raises(ValueError, match="label maps"):
        A([v(5), v(5)], [l(5)], 4, 4, device="cpu")
    with pytest.raises(ValueError, match="integral"):
        A([v(5)], [l(5) + 0.25], 4, 4, device="cpu")
    with pytest.raises(ValueError, match="255"):
        A([v(5)], [l(5).astype(np.int64) + 256], 4, 4, device="cpu")
    a = A([v(5), v(6)], [l(5), l(6)], 4, 4, device="cpu")
    for bad in ((0, 5, 0, 1), (0, 0, -1, 1), (1, 0, 2, 6), (0, 0, 2, 5)):
        with pytest.raises(ValueError, match="slice index outside"):
            a.assemble([(1, 0, 2, 1), bad], transforms=[(0, 0, 3.0, 0.5, 0)] * 2)
    with pytest.raises(ValueError, match="slice index outside"):
        a.draw_sample(0, 5)
    with pytest.raises(ValueError, match="raw"):
        a.assemble([(1, 0, 2, 1)], size=8)


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_labels_dir_on_the_command_line(tmp_path):
    from superresolution_aniso_mri_amd import train_aesr
    from superresolution_aniso_mri_amd.kwatsch.arguments import parse_args
    _, d = parse_args(["--dataset=ACDCLBL", "--downsample_steps=2", "--volumes_dir=/v", "--labels_dir=/l"])
    assert d["labels_dir"] == "/l" and d["volumes_dir"] == "/v" and d["aug_patch_size"] == 180
    assert parse_args(["--downsample_steps=2"])[1]["labels_dir"] is None
    common = ["--dataset=ACDCLBL", "--model=ae", "--downsample_steps=2", "--exper_id=m", "--output_dir=" + str(tmp_path / "out")]
    with pytest.raises(NotImplementedError, match="label-aware") as e:
        train_aesr.main(common + ["--volumes_dir=" + str(tmp_path)])
    assert "--labels_dir" in str(e.value)
    with pytest.raises(NotImplementedError, match="val_volumes_dir"):
        train_aesr.main(common + ["--volumes_dir=" + str(tmp_path), "--labels_dir=" + str(tmp_path), "--val_volumes_dir=" + str(tmp_path)])
    with pytest.raises(ValueError, match="labels_dir"):
        train_aesr.main(["--dataset=ACDC", "--downsample_steps=2", "--volumes_dir=" + str(tmp_path), "--labels_dir=" + str(tmp_path),
                         "--exper_id=m", "--output_dir=" + str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()          # every refusal comes before anything is written
