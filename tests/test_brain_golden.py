"""not gpu: the brain data path against the reference's own results (tests/golden/brain_data.npz, written by tests/make_golden_brain.py
from datasets/common_brains.py, OASIS/dataset.py, dHCP/dataset.py and shared_transforms.py of the reference).

- A numpy restatement of the thick-slice blur, kept in this file (``restate_blur``): scipy's weights, the ``reflect`` boundary, the sum in
  double in scipy's order (centre, then the pairs from the outermost inwards), one rounding -- equals every fixture case BITWISE, for
  ``z_step = 1`` and for ``[::k]``.  It shares no code with the package; the kernel is held to it and to the fixture on the GPU.
- ``BrainSampler`` reproduces every slice id and coefficient the reference's datasets drew, ``BrainTripletAugmenter.draw_transform`` every
  number its transforms drew (two RandomStates, two seeds); ``adjacent`` raises the documented ``ValueError``.
- Every refusal of ``aesr_thick_slices`` returns its code before anything touches the device: callable without a GPU.
- ``get_file_suffix_blurred`` and ``determine_interpol_coefficients`` against recorded values."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = (2, 3, 5, 6)            # z_step values every case is run with: 39, 36, 40, 2, 1, 0, 8 = Z - 1 of the cases; 5 and 6 exceed Z = 3, 2, 1
# (set, leg) -> the augmenter that mirrors the reference's dataset + transform of that leg: dataset, width, aug_patch_size, downsample_steps
LEGS = {("oasis", "crop"): ("OASIS", 200, 220, 3), ("oasis", "nocrop"): ("OASIS", 220, 220, 3), ("oasis", "test"): ("OASIS", 220, 220, 3),
        ("dhcp", "crop"): ("dHCP", 24, 256, 5), ("dhcp", "nocrop"): ("dHCP", 28, None, 5), ("dhcp", "test"): ("dHCP", 28, None, 5)}
_FX = {}


def fixture():
    if not _FX:
        _FX.update(np.load(os.path.join(HERE, "golden", "brain_data.npz")))
    return _FX, [str(t) for t in _FX["thick/tags"]]


def case_input(fx, tag):
    x = fx["thick/%s/in" % tag]
    return x if x.dtype == np.float32 else (x / 1024.0).astype(np.float32)


def leg_volumes(fx, name, leg):
    key, out = "%s/%s" % (name, leg), []
    while "%s/vol%d" % (key, len(out)) in fx:
        out.append((fx["%s/vol%d" % (key, len(out))] / 1024.0).astype(np.float32))
    return out


def make_augmenter(fx, name, leg, device):
    from superresolution_aniso_mri_amd.data_device import BrainTripletAugmenter
    dataset, width, aug, steps = LEGS[(name, leg)]
    d_seed, t_seed = (int(s) for s in fx["seeds"])
    return BrainTripletAugmenter(leg_volumes(fx, name, leg), width, aug, dataset=dataset, slice_selection="adjacent_plus", downsample_steps=steps,
                                 rs=np.random.RandomState(d_seed), rs_transform=np.random.RandomState(t_seed), device=device)


def draw_leg(fx, name, leg, aug):
    """The 12 samples of a leg drawn the way the reference's loop draws them: per sample the dataset's numbers, then the transform's."""
    key = "%s/%s" % (name, leg)
    trips, alphas, transforms = [], [], []
    for vid, sid in zip(fx[key + "/vol"], fx[key + "/slice_id"]):
        zf, zt, zb, af, at = aug.sampler.draw(int(sid), aug.shapes[int(vid)][0])
        trips.append((int(vid), zf, zt, zb))
        alphas.append((af, at))
        transforms.append(aug.test_transform(int(vid)) if leg == "test" else aug.draw_transform(int(vid)))
    return trips, alphas, transforms


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def restate_blur(x, thickness, k=1):
    """float32 [Z, H, W] -> float32 [ceil(Z / k), H, W] = gaussian_filter1d(x, thickness / 2.355, axis=0)[::k]"""
    sigma = float(thickness) / 2.355
    r = int(4.0 * sigma + 0.5)
    t = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * t ** 2)
    w = w / w.sum()
    Z = x.shape[0]
    xd = x.astype(np.float64)
    centres = np.arange(0, Z, k)

    def take(off):
        i = (centres + off) % (2 * Z)
        return xd[np.where(i < Z, i, 2 * Z - 1 - i)]          # d c b a | a b c d, as often as needed

    acc = take(0) * w[r]
    for l in range(r, 0, -1):          # noqa: E741
        acc = acc + (take(-l) + take(l)) * w[r - l]
    return acc.astype(np.float32)


def test_fixture_is_what_the_issue_asked_for():
    fx, tags = fixture()
    assert tags == ["oasis3", "oasis6", "dhcp5", "odd", "short", "two", "one", "const"]
    shapes = {"oasis3": (40, 16, 12), "oasis6": (40, 16, 12), "dhcp5": (37, 8, 10), "odd": (41, 7, 5), "short": (3, 4, 4), "two": (2, 5, 3),
              "one": (1, 4, 8), "const": (9, 4, 4)}
    for tag in tags:
        assert fx["thick/%s/in" % tag].shape == fx["thick/%s/out" % tag].shape == shapes[tag] and fx["thick/%s/out" % tag].dtype == np.float32
    radius = lambda tag: int(4.0 * float(fx["thick/%s/thickness" % tag]) / 2.355 + 0.5)      # noqa: E731
    assert [radius(t) for t in ("oasis3", "oasis6", "dhcp5", "odd")] == [5, 10, 4, 7] and radius("short") > 3
    assert (fx["thick/const/in"] == np.float32(0.7)).all()
    assert os.path.getsize(os.path.join(HERE, "golden", "brain_data.npz")) < 1 << 20
    for (name, leg), (_, width, _, _) in LEGS.items():
        key = "%s/%s" % (name, leg)
        assert fx[key + "/image"].shape == (24, 1, width, width) and fx[key + "/slice_between"].shape == (12, 1, width, width)
        assert fx[key + "/alpha_from"].shape == (12, 1) and fx[key + "/alpha_from"].dtype == np.float32
    assert len({v.shape[1:] for v in leg_volumes(fx, "oasis", "crop")}) == 2 and len({v.shape[1:] for v in leg_volumes(fx, "dhcp", "crop")}) == 2
    assert {round(float(a), 3) for a in fx["dhcp/crop/alpha_from"].ravel()} <= {0.2, 0.4, 0.6, 0.8} and len(set(fx["dhcp/crop/alpha_from"].ravel())) > 2
    assert (fx["oasis/crop/alpha_from"] == 0.5).all()               # OASIS regularises on neighbours 2 apart: one slice in between


def test_restatement_equals_the_reference_bitwise():
    fx, tags = fixture()
    for tag in tags:
        x, want, th = case_input(fx, tag), fx["thick/%s/out" % tag], float(fx["thick/%s/thickness" % tag])
        got = restate_blur(x, th)
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), (tag, np.abs(got - want).max())
        for k in STEPS + (int(fx["thick/%s/steps" % tag]),):
            sub = restate_blur(x, th, k)
            assert sub.shape[0] == -(-x.shape[0] // k) and np.array_equal(sub.view(np.int32), want[::k].view(np.int32)), (tag, k)
    assert np.abs(fx["thick/const/out"] - np.float32(0.7)).max() <= np.spacing(np.float32(0.7))


def test_restatement_weights_are_the_packages():
    from superresolution_aniso_mri_amd.datasets import common_brains as cb
    from superresolution_aniso_mri_amd.datasets.common import gaussian_weights
    for th in (1.5, 2.5, 3, 4, 5, 6, 9.7):
        w, r = gaussian_weights(th / cb.FWHM)
        assert r == int(4.0 * th / 2.355 + 0.5) <= cb.MAX_RADIUS and np.array_equal(w, w[::-1]) and abs(w.sum() - 1) <= 1e-12
    assert gaussian_weights(9.8 / cb.FWHM)[1] == 17


@pytest.mark.parametrize("name,leg", sorted(LEGS))
def test_sampler_and_transform_draws_equal_the_references(name, leg):
    fx, _ = fixture()
    key = "%s/%s" % (name, leg)
    aug = make_augmenter(fx, name, leg, "cpu")                 # host only: nothing is launched
    trips, alphas, transforms = draw_leg(fx, name, leg, aug)
    assert [t[1] for t in trips] == fx[key + "/slice_idx_from"].tolist() and [t[2] for t in trips] == fx[key + "/slice_idx_to"].tolist()
    assert [t[3] for t in trips] == fx[key + "/inbetween_slice_id"].tolist()
    a = np.array(alphas, np.float32)
    assert a.dtype == np.float32 and np.array_equal(a[:, 0], fx[key + "/alpha_from"][:, 0]) and np.array_equal(a[:, 1], fx[key + "/alpha_to"][:, 0])
    width = LEGS[(name, leg)][1]
    for i, (oy, ox, gain, cutoff, k) in enumerate(transforms):
        vid = int(fx[key + "/vol"][i])
        pt, pl, _, _ = aug._padded(vid, aug.aug if aug.crops else width)
        top, left = int(fx[key + "/top"][i]), int(fx[key + "/left"][i])
        assert (top >= 0) == (leg == "crop")
        assert (oy, ox) == (max(top, 0) - pt, max(left, 0) - pl), (key, i)
        assert k == int(fx[key + "/k"][i]) and gain == float(fx[key + "/gain"][i]) and cutoff == float(fx[key + "/cutoff"][i]), (key, i)
    # both streams are where the reference left them: the next numbers agree with fresh states advanced by the reference's calls only
    assert aug.rs is aug.sampler.rs and aug.rs is not aug.rs_transform


def test_adjacent_and_mix_raise_where_the_reference_does():
    from superresolution_aniso_mri_amd.data_device import BrainSampler
    with pytest.raises(ValueError, match="no slice between"):
        BrainSampler("OASIS", "adjacent", 3, np.random.RandomState(0)).draw(4, 20)
    with pytest.raises(ValueError, match="no slice between"):
        BrainSampler("dHCP", "adjacent", 5, np.random.RandomState(0)).draw(0, 20)
    mix = BrainSampler("dHCP", "mix", 5, np.random.RandomState(0))
    seen = set()
    for _ in range(40):
        try:
            f, t, b, af, at = mix.draw(10, 30)
            assert abs(f - t) == 5 and min(f, t) < b < max(f, t) and abs(float(af) + float(at) - 1) < 1e-6
            seen.add("drawn")
        except ValueError as e:
            assert "step 1" in str(e)
            seen.add("raised")
    assert seen == {"drawn", "raised"}
    with pytest.raises(ValueError, match="slice_selection"):
        BrainSampler("OASIS", "random")
    with pytest.raises(ValueError, match="no neighbour"):
        BrainSampler("dHCP", "adjacent_plus", 5).draw(1, 4)
    assert BrainSampler("OASIS", "adjacent_plus", 6).slice_step() == 2 and BrainSampler("ADNI", "adjacent_plus", 6).slice_step() == 6


def test_augmenter_refuses_what_the_transforms_cannot_do():
    from superresolution_aniso_mri_amd.data_device import BrainTripletAugmenter
    big, small, flat = np.zeros((4, 40, 40), np.float32), np.zeros((4, 20, 20), np.float32), np.zeros((4, 20, 32), np.float32)
    with pytest.raises(ValueError, match="no crop"):             # larger than the patch, no crop branch: there is no centre crop
        BrainTripletAugmenter([big], 32, None, dataset="OASIS", device="cpu").draw_transform(0)
    with pytest.raises(ValueError, match="no crop"):             # dHCP slices are never padded
        BrainTripletAugmenter([small], 32, None, dataset="dHCP", device="cpu").draw_transform(0)
    with pytest.raises(ValueError, match="cannot be cropped"):
        BrainTripletAugmenter([small], 32, 256, dataset="dHCP", device="cpu").draw_transform(0)
    with pytest.raises(ValueError, match="does not crop"):
        BrainTripletAugmenter([big], 32, 220, dataset="OASIS", device="cpu").test_transform(0)
    ok = BrainTripletAugmenter([small, flat], 32, None, dataset="OASIS", device="cpu")
    assert ok.draw_transform(0)[:2] == (-6, -6) and ok.draw_transform(1)[:2] == (-6, 0) and ok.test_transform(1)[:2] == (-6, 0)
    with pytest.raises(ValueError, match="at least 10"):
        BrainTripletAugmenter([np.zeros((9, 32, 32), np.float32)], 32, None, dataset="dHCP", downsample_steps=5, device="cpu")
    assert BrainTripletAugmenter([big, flat], 32, 220, dataset="OASIS", device="cpu").eval_size(8) == 40
    assert BrainTripletAugmenter([small, flat], 30, None, dataset="dHCP", device="cpu").eval_size(8) == 32


# ---- the third header --------------------------------------------------------------------------------------------------------------
def test_out_slices_is_ceil():
    from superresolution_aniso_mri_amd import _hip
    f = _hip.lib.aesr_thick_slices_out_slices
    for Z in (1, 2, 3, 37, 40, 41, 176, 2 ** 31 - 1):
        for k in (1, 2, 3, 5, 6, 41, 2 ** 31 - 1):
            assert f(Z, k) == -(-Z // k) == len(range(0, Z, k)), (Z, k)
    assert f(0, 1) == 0 and f(-3, 2) == 0 and f(5, 0) == 0 and f(5, -1) == 0
    sb = _hip.lib.aesr_thick_slices_store_bytes
    P = ctypes.c_void_p
    assert sb(12, P(4096), P(8192)) == 16 and sb(10, P(4096), P(8192)) == 4 and sb(12, P(4100), P(8192)) == 4 and sb(12, P(4096), P(8200)) == 4
    assert sb(0, P(4096), P(8192)) == 4


def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    from superresolution_aniso_mri_amd.datasets.common import gaussian_weights
    call = _hip.lib.aesr_thick_slices
    D = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_hip.DP)       # noqa: E731
    fake = ctypes.c_void_p(4096)
    w, r = gaussian_weights(3 / 2.355)
    names = ["inp", "out", "Z", "H", "W", "z_step", "weights", "radius", "stream"]
    ok = [fake, fake, 40, 16, 12, 3, D(w), r, None]

    def rc(**over):
        args = list(ok)
        for k, v in over.items():
            args[names.index(k)] = v
        return call(*args)

    assert rc(inp=None) == 1 and "in is a null" in _hip.last_error()
    assert rc(out=None) == 1 and "out is a null" in _hip.last_error()
    assert rc(weights=None) == 1 and "weights_host" in _hip.last_error()
    for dim in ("Z", "H", "W"):
        assert rc(**{dim: 0}) == 1 and "Z, H, W" in _hip.last_error() and rc(**{dim: -4}) == 1
    assert rc(z_step=0) == 1 and "z_step" in _hip.last_error() and rc(z_step=-2) == 1
    assert rc(Z=2048, H=1024, W=1024) == 1 and "2^31" in _hip.last_error()
    assert rc(Z=2047, H=1024, W=1024, radius=-1) == 1 and "radius" in _hip.last_error()       # just below 2^31: the next check speaks
    w17, r17 = gaussian_weights(9.8 / 2.355)
    assert r17 == 17 and rc(weights=D(w17), radius=r17) == 3 and "radius" in _hip.last_error() and "16" in _hip.last_error()
    bad = w.copy()
    bad[0] = np.nextafter(bad[0], 1.0)
    assert rc(weights=D(bad)) == 1 and "symmetric" in _hip.last_error()
    bad = w * (1 + 4e-12)
    assert rc(weights=D(bad)) == 1 and "sums to" in _hip.last_error()
    assert rc(weights=D(w[1:-1]), radius=r - 1) == 1 and "sums to" in _hip.last_error()     # a truncated kernel is symmetric, not normalised
    # the raw assembly: the checks of aesr_triplet_assemble
    desc = (_hip.TripletDesc * 1)(_hip.TripletDesc(0, 8, 8, 0, 1, 2, 0, 0, 0, 0.0, 0.0))
    raw = _hip.lib.aesr_triplet_assemble_raw
    assert raw(None, desc, 1, 8, fake, fake, None) == 1 and "aesr_triplet_assemble_raw" in _hip.last_error()
    assert raw(fake, desc, 0, 8, fake, fake, None) == 1 and raw(fake, desc, 65, 8, fake, fake, None) == 1 and "B=65" in _hip.last_error()
    assert raw(fake, desc, 1, 0, fake, fake, None) == 1
    desc[0].k = 4
    assert raw(fake, desc, 1, 8, fake, fake, None) == 1 and "descriptor 0" in _hip.last_error()


def test_python_interface_and_helpers():
    import torch
    from datasets.common_brains import determine_interpol_coefficients, get_file_suffix_blurred, process_img, simulate_thick_slices
    from superresolution_aniso_mri_amd.datasets import common_brains as cb
    assert simulate_thick_slices is cb.simulate_thick_slices and process_img is cb.process_img          # the root shim
    fx, _ = fixture()
    for arg, want in zip(fx["suffix/args"], fx["suffix/out"]):
        name, suffix, k = str(arg).split("|")
        assert get_file_suffix_blurred(name, suffix, int(k)) == str(want)
    with pytest.raises(NotImplementedError):
        get_file_suffix_blurred("ACDC", ".nii.gz", 3)
    for args, want in zip(fx["coef/args"], fx["coef/out"]):
        assert tuple(determine_interpol_coefficients(*(int(a) for a in args))) == tuple(want)
    assert cb.default_slice_thickness("OASIS", 3) == 3 and cb.default_slice_thickness("dHCP", 5) == 2.5
    with pytest.raises(ValueError, match="3-D"):
        simulate_thick_slices(np.zeros((4, 4), np.float32), 3)
    with pytest.raises(RuntimeError, match="GPU"):
        simulate_thick_slices(torch.zeros(3, 4, 4), 3)                     # a CPU tensor: no fallback
    # process_img is the reference's composition, host arithmetic: [::k] then the (0, 100) window
    x = fx["thick/oasis3/out"]
    got = process_img(x, None, True, 3, True)
    assert np.array_equal(got, fx["thick/oasis3/proc"])
    assert np.array_equal(process_img(x, lambda s: {"image": s["image"][:, ::2]}, False, 3, False), x[:, ::2])


def test_cli_flags():
    from superresolution_aniso_mri_amd.kwatsch.arguments import parse_args
    base = ["--model=ae", "--downsample_steps=5"]
    assert parse_args(base + ["--dataset=dHCP"])[1]["thick_slices"] == 2.5
    assert parse_args(base + ["--dataset=OASIS"])[1]["thick_slices"] == 5.0
    assert parse_args(base + ["--dataset=ACDC"])[1]["thick_slices"] is None
    assert parse_args(base + ["--dataset=OASIS", "--thick_slices=4"])[1]["thick_slices"] == 4.0
    a = parse_args(base + ["--dataset=OASIS", "--no_thick_slices"])[1]
    assert a["thick_slices"] is None and a["no_thick_slices"]
    with pytest.raises(ValueError, match="exclude"):
        parse_args(base + ["--dataset=OASIS", "--no_thick_slices", "--thick_slices=3"])
