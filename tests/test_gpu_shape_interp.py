"""GPU: csrc/shape_interp.hip (signed distance maps of every class and slice; blend and arg-max) and the layers above it against the numpy
restatement of tests/test_shape_interp_golden.py and the scipy fixture of tests/make_golden_shape_interp.py.

Bounds.  The device's signed maps are BIT-EQUAL to the restatement's: both take the minimum of the same fp64 expression,
(dy sy) (dy sy) + (dx sx) (dx sx), not contracted, and one correctly rounded sqrt (the surface-distance lists of test_gpu_seg_metrics are
the precedent); they are within 1e-12 * BIG of scipy's.  The device's labels are EQUAL to what the restated blend and arg-max rule gives on
the device's own maps, and equal to the fixture's wherever the fixture's margin exceeds 1e-9 * BIG, which may leave out 0.1 % of a case at
most (both stated in test_shape_interp_golden).  Measured on an MI355X: 0 map values differ in bits and 0 labels differ from the rule, in
every case (each test prints its counts; profiles/shape_interp.txt).  Then: alpha 0 / 1 reproduce input slices, the 4-D call equals its frames, the 32-bit
store path equals the byte path, num_interpolations equals its grid, gap tables out of range are clamped, guard bands with NaN / finite /
byte poisons and shifted pointers, every refusal, the evaluation protocol beside the nearest-slice baseline, and both tools."""
import ctypes

import numpy as np
import pytest
import torch

import memguard as mg
import test_shape_interp_golden as tm

pytestmark = pytest.mark.gpu
CASES = tm.CASES
# GUARDED_ENTRIES and EXEMPT partition ``_hip.SIGNATURES_SHAPE`` (tests/test_abi.py checks that without a GPU)
GUARDED_ENTRIES = {
    "aesr_shape_signed_distances": "test_guard_bands_poisons_and_shifted_pointers",
    "aesr_shape_interpolate": "test_guard_bands_poisons_and_shifted_pointers",
}
EXEMPT = {"aesr_shape_workspace_bytes": "a size query on the host: it is given no buffer"}
_DEVICE = {}


def si():
    from superresolution_aniso_mri_amd.evaluate import shape_interp
    return shape_interp


def zgrid(c):
    """the fixture's grid as a ZGrid"""
    from superresolution_aniso_mri_amd.evaluate.z_grid import ZGrid
    gap, alpha = c["gap"].astype(np.int64), c["alpha"].astype(np.float64)
    return ZGrid(c["labels"].shape[1], 1.0, 1.0, gap + alpha, gap, alpha)


def device(name):
    """(maps fp64 [N, C, Z, H, W], labels uint8 [N, J, H, W]) of the device for a case as numpy, through the public functions; made once"""
    if name not in _DEVICE:
        c = tm.case(name)
        lab = torch.from_numpy(c["labels"]).cuda()
        maps, classes = si().signed_distance_maps(lab, c["spacing"], c["classes"])
        out = si().shape_interpolate(lab, grid=zgrid(c), spacing_yx=c["spacing"], classes=c["classes"])
        assert classes == c["classes"] and maps.is_cuda and out.is_cuda and maps.dtype == torch.float64 and out.dtype == torch.uint8
        _DEVICE[name] = (maps.cpu().numpy(), out.cpu().numpy())
    return _DEVICE[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_signed_maps_are_the_restatements_bit_for_bit_and_scipys_within_the_bound(name):
    c = tm.case(name)
    want, _ = tm.restated(name)
    got, _ = device(name)
    worst = float(np.abs(got - c["sdm"]).max())
    print("%s: %d of %d map values differ in bits from the restatement; worst |device - scipy| %.3g, bound %.3g"
          % (name, int((got.view(np.int64) != want.view(np.int64)).sum()), got.size, worst, tm.MAP_BOUND * c["big"]))
    assert same_bits(got, want)
    assert worst <= tm.MAP_BOUND * c["big"]


@pytest.mark.parametrize("name", CASES)
def test_labels_are_the_rule_on_the_devices_maps_and_the_fixtures_under_the_margin_rule(name):
    c = tm.case(name)
    maps, got = device(name)
    want, _ = tm.blend_np(maps, c["gap"], c["alpha"], c["classes"])
    print("%s: %d of %d labels differ from the rule on the device's maps; %d left out by the margin rule"
          % (name, int((got != want).sum()), got.size, int(tm.left_out(c).sum())))
    assert got.shape == want.shape and np.array_equal(got, want)
    tm.assert_labels_match_fixture(got, c, name)
    g, g1 = tm.clamp_gap(c["gap"], c["labels"].shape[1])
    originals = 0
    for j, a in enumerate(c["alpha"]):
        if a == 0.0 or a == 1.0:
            originals += 1
            assert np.array_equal(got[:, j], c["labels"][:, g[j] if a == 0.0 else g1[j]]), (name, j)
    assert originals >= 1


def test_input_slices_come_back_at_alpha_zero_and_one_whatever_the_gap():
    c = tm.case("oneslice")          # a class in one slice only, a class that fills a slice: +-BIG on both sides of the blend
    Z = c["labels"].shape[1]
    lab = torch.from_numpy(c["labels"]).cuda()
    sdm = si()._sdm(lab, c["classes"], c["spacing"])
    gap = torch.tensor([0, 0, 1, 1], dtype=torch.int32, device="cuda")
    alpha = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=torch.float64, device="cuda")
    out = si()._blend(sdm, gap, alpha, c["classes"]).cpu().numpy()
    assert Z == 3 and np.array_equal(out[0], c["labels"][0][[0, 1, 1, 2]])


def test_the_4d_call_equals_its_frames_and_numpy_goes_through_the_device():
    c = tm.case("frames")
    _, whole = device("frames")
    grid = zgrid(c)
    for n in range(c["labels"].shape[0]):
        one = si().shape_interpolate(torch.from_numpy(c["labels"][n]).cuda(), grid=grid, spacing_yx=c["spacing"], classes=c["classes"])
        assert one.dim() == 3 and np.array_equal(one.cpu().numpy(), whole[n]), n
    # chunks of one frame, and host data in -> host data out
    split = si().shape_interpolate(c["labels"], grid=grid, spacing_yx=c["spacing"], classes=c["classes"], max_workspace_bytes=1)
    assert isinstance(split, np.ndarray) and split.dtype == np.uint8 and np.array_equal(split, whole)
    maps, classes = si().signed_distance_maps(c["labels"][0].astype(np.float32), c["spacing"], c["classes"])
    assert isinstance(maps, np.ndarray) and classes == c["classes"] and same_bits(maps, device("frames")[0][0])


@pytest.mark.parametrize("name", ["w64", "z7", "frames"])
def test_the_word_store_path_equals_the_byte_path(name):
    c = tm.case(name)
    N, Z, H, W = c["labels"].shape
    _, want = device(name)
    sdm = si()._sdm(torch.from_numpy(c["labels"]).cuda(), c["classes"], c["spacing"])
    gap, alpha = si().grid_tables(zgrid(c), "cuda")
    J = int(gap.numel())
    assert (H * W) % 4 == 0
    for shift in (0, 1, 2, 3):
        backing = torch.full((N * J * H * W + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        off = (-backing.data_ptr()) % 4 + shift
        out = backing[off:off + N * J * H * W].view(N, J, H, W)
        assert si().store_path(out, H * W) == ("word4" if shift == 0 else "byte1")
        si()._blend(sdm, gap, alpha, c["classes"], out)
        assert np.array_equal(out.cpu().numpy(), want), shift
        rest = torch.cat([backing[:off], backing[off + N * J * H * W:]])
        assert bool((rest == 0xEE).all()), shift
    odd = tm.case("w63")["labels"]
    assert (odd.shape[2] * odd.shape[3]) % 4 and si().store_path(torch.empty(4, dtype=torch.uint8, device="cuda"), odd.shape[2] * odd.shape[3]) == "byte1"


def test_num_interpolations_is_its_grid():
    from superresolution_aniso_mri_amd.evaluate.z_grid import target_grid
    c = tm.case("z7")
    lab = torch.from_numpy(c["labels"][0]).cuda()
    for n in (1, 6):
        a = si().shape_interpolate(lab, num_interpolations=n, classes=c["classes"])
        b = si().shape_interpolate(lab, grid=target_grid(7, 1.0, 1.0 / (n + 1)), classes=c["classes"])
        assert tuple(a.shape) == (6 * (n + 1) + 1, 12, 20) and torch.equal(a, b), n
        assert torch.equal(a[::n + 1], lab)
    assert np.array_equal(si().shape_interpolate(lab, num_interpolations=6, classes=c["classes"]).cpu().numpy(), device("z7")[1][0])
    same = si().shape_interpolate(lab, num_interpolations=0)
    assert torch.equal(same, lab)


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------
SDM_ARGS = ("labels", "sdm", "workspace", "workspace_bytes", "N", "Z", "H", "W", "classes_host", "C", "sy", "sx")
BLEND_ARGS = ("sdm", "gap", "alpha", "out", "N", "C", "Z", "H", "W", "J", "classes_host")
BYTE_POISON = {mg.POISON_NAN: 0x7E, mg.POISON_FINITE: 0x5A}
SLACK = 0xA5


class ByteBuffer:
    """n bytes starting ``shift`` (0..3) bytes behind a 16-byte boundary, inside a guarded allocation of n + 3 bytes whose slack holds SLACK"""

    def __init__(self, n, shift, name, data=None, fill=None):
        self.g = mg.guarded(n + 3, torch.uint8, torch.device("cuda"), SLACK, 0, name)
        self.n, self.shift = n, shift
        self.view = self.g.view[shift:shift + n]
        assert self.view.data_ptr() % 16 == shift
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).cuda())
        else:
            self.view.fill_(BYTE_POISON[fill])

    def assert_intact(self):
        mg.assert_guards_intact([self.g])
        slack = torch.cat([self.g.view[:self.shift], self.g.view[self.shift + self.n:]])
        assert bool((slack == SLACK).all()), "%s: a byte next to the buffer was written" % self.g.name


def _lib():
    from superresolution_aniso_mri_amd import _hip
    return _hip, _hip.lib


def call_sdm(a):
    _hip, lib = _lib()
    return lib.aesr_shape_signed_distances(*[a[k] for k in SDM_ARGS], _hip.stream())


def call_blend(a):
    _hip, lib = _lib()
    return lib.aesr_shape_interpolate(*[a[k] for k in BLEND_ARGS], _hip.stream())


def at(view, offset=0):
    return ctypes.c_void_p(view.data_ptr() + offset)


def guarded_call(name, fill, byte_shift, sdm_shift, gap_host=None, refuse=False):
    """Both entry points with every buffer at exactly its contractual size between guard bands: labels and out ``byte_shift`` bytes off a
    16-byte boundary, sdm ``sdm_shift`` elements.  Returns (maps, labels) as numpy; with ``refuse`` every refusal is tried instead and
    nothing may have been written."""
    _hip, lib = _lib()
    c = tm.case(name)
    N, Z, H, W = c["labels"].shape
    C, dev = len(c["classes"]), torch.device("cuda")
    gap_host = c["gap"] if gap_host is None else gap_host
    J = len(gap_host)
    lab = ByteBuffer(N * Z * H * W, byte_shift, "labels", data=c["labels"])
    out = ByteBuffer(N * J * H * W, byte_shift, "out", fill=fill)
    nbytes = lib.aesr_shape_workspace_bytes(N, Z, H, W, C)
    assert nbytes == (N * C * 2 * Z * H * W * 4 + 15) // 16 * 16
    sdm = mg.guarded(N * C * Z * H * W, torch.float64, dev, fill, sdm_shift, "sdm")
    ws = mg.guarded(nbytes, torch.uint8, dev, fill, 0, "workspace")
    gap = mg.guarded(J, torch.int32, dev, torch.from_numpy(np.asarray(gap_host, dtype=np.int32)), sdm_shift, "gap")
    alpha = mg.guarded(J, torch.float64, dev, torch.from_numpy(np.asarray(c["alpha"], dtype=np.float64)), sdm_shift, "alpha")
    assert sdm.view.data_ptr() % 16 == 8 * sdm_shift and ws.view.data_ptr() % 16 == 0 and alpha.view.data_ptr() % 8 == 0
    everything = [sdm, ws, gap, alpha]
    saved = [mg.bits(lab.view), mg.bits(gap.view), mg.bits(alpha.view)]
    cls = _hip.int_array(c["classes"])
    a1 = dict(labels=at(lab.view), sdm=at(sdm.view), workspace=at(ws.view), workspace_bytes=nbytes, N=N, Z=Z, H=H, W=W, classes_host=cls, C=C,
              sy=c["spacing"][0], sx=c["spacing"][1])
    a2 = dict(sdm=at(sdm.view), gap=at(gap.view), alpha=at(alpha.view), out=at(out.view), N=N, C=C, Z=Z, H=H, W=W, J=J, classes_host=cls)

    def untouched():
        torch.cuda.synchronize()
        assert mg.poison_left(sdm.view, fill).numel() == sdm.view.numel() and mg.poison_left(ws.view, fill).numel() == ws.view.numel()
        assert int((out.view == BYTE_POISON[fill]).sum()) == out.n
        mg.assert_guards_intact(everything)
        lab.assert_intact()
        out.assert_intact()

    if refuse:
        ARG, UNSUPPORTED = 1, 3
        desc = _hip.int_array([c["classes"][-1]] + c["classes"][:-1]) if C > 1 else _hip.int_array([256])
        twice = _hip.int_array([c["classes"][0]] * C) if C > 1 else _hip.int_array([-1])
        shared = [(dict(classes_host=None), ARG, "classes_host"), (dict(N=0), ARG, "N"), (dict(Z=0), ARG, "Z"), (dict(H=-1), ARG, "H"),
                  (dict(W=0), ARG, "W"), (dict(C=0), ARG, "C"), (dict(C=9), ARG, "C"), (dict(classes_host=desc), ARG, "classes_host"),
                  (dict(classes_host=twice), ARG, "classes_host"), (dict(classes_host=_hip.int_array([300] * C)), ARG, "classes_host"),
                  (dict(N=1 << 16, Z=1 << 15), ARG, "2^31"), (dict(sdm=None), ARG, "sdm"), (dict(sdm=at(sdm.view, 4)), ARG, "sdm")]
        first = shared + [
            (dict(labels=None), ARG, "labels"), (dict(workspace=None), ARG, "workspace"), (dict(workspace=at(ws.view, 8)), ARG, "workspace"),
            (dict(sy=0.0), ARG, "sy"), (dict(sy=float("inf")), ARG, "sy"), (dict(sx=-1.0), ARG, "sx"), (dict(sx=float("nan")), ARG, "sx"),
            (dict(workspace_bytes=nbytes - 1), ARG, "workspace_bytes"), (dict(workspace_bytes=0), ARG, "workspace_bytes"),
            (dict(W=4097, H=1, Z=1, N=1, C=1, classes_host=_hip.int_array([0])), UNSUPPORTED, "W"),
            (dict(workspace=at(sdm.view, 16 - 8 * sdm_shift)), UNSUPPORTED, "overlaps"), (dict(sdm=at(lab.view, (-lab.view.data_ptr()) % 8)), UNSUPPORTED, "overlaps")]
        second = shared + [
            (dict(gap=None), ARG, "gap"), (dict(alpha=None), ARG, "alpha"), (dict(out=None), ARG, "out"), (dict(alpha=at(alpha.view, 4)), ARG, "alpha"),
            (dict(gap=at(gap.view, 2)), ARG, "gap"), (dict(J=0), ARG, "J"), (dict(J=1 << 30, N=2), ARG, "2^31"),
            (dict(out=at(sdm.view, 3)), UNSUPPORTED, "out"), (dict(out=at(alpha.view)), UNSUPPORTED, "out")]
        for call, base, table, fn in ((call_sdm, a1, first, "aesr_shape_signed_distances"), (call_blend, a2, second, "aesr_shape_interpolate")):
            for over, code, word in table:
                a = dict(base)
                a.update(over)
                rc = call(a)
                assert rc == code, (fn, sorted(over), rc, _hip.last_error())
                assert fn in _hip.last_error() and word in _hip.last_error(), (fn, sorted(over), _hip.last_error())
        untouched()
        for g, s in zip((lab, gap, alpha), saved):
            mg.assert_unchanged(g.view, s, g.g.name if isinstance(g, ByteBuffer) else g.name)
        return None

    _hip.check(call_sdm(a1), "aesr_shape_signed_distances")
    torch.cuda.synchronize()
    mg.assert_guards_intact(everything)
    lab.assert_intact()
    assert mg.poison_left(sdm.view, fill).numel() == 0 and int((out.view == BYTE_POISON[fill]).sum()) == out.n
    saved_sdm = mg.bits(sdm.view)
    _hip.check(call_blend(a2), "aesr_shape_interpolate")
    torch.cuda.synchronize()
    mg.assert_guards_intact(everything)
    lab.assert_intact()
    out.assert_intact()
    assert int((out.view == BYTE_POISON[fill]).sum()) == 0          # class values are small: a poison byte left is an element never written
    mg.assert_unchanged(lab.view, saved[0], "labels")
    mg.assert_unchanged(gap.view, saved[1], "gap")
    mg.assert_unchanged(alpha.view, saved[2], "alpha")
    mg.assert_unchanged(sdm.view, saved_sdm, "sdm")
    return sdm.view.cpu().numpy().reshape(N, C, Z, H, W), out.view.cpu().numpy().reshape(N, J, H, W)


LEGS = ((0, 0), (1, 1), (2, 0), (3, 1))          # labels and out by 0..3 bytes; sdm, alpha (and gap, by 4) by 8 bytes


@pytest.mark.parametrize("name", ["w64", "w63", "ychunk", "eight", "frames"])
def test_guard_bands_poisons_and_shifted_pointers(name):
    maps, labels = device(name)
    assert max(tm.case(name)["classes"]) < min(BYTE_POISON.values())
    for fill in (mg.POISON_NAN, mg.POISON_FINITE):
        for byte_shift, sdm_shift in LEGS:
            got = guarded_call(name, fill, byte_shift, sdm_shift)
            assert same_bits(got[0], maps) and same_bits(got[1], labels), (fill, byte_shift, sdm_shift)


@pytest.mark.parametrize("name,byte_shift,sdm_shift", [("w64", 0, 0), ("frames", 3, 1), ("bgonly", 1, 0)])
def test_refusals_write_nothing_and_name_the_argument(name, byte_shift, sdm_shift):
    for fill in (mg.POISON_NAN, mg.POISON_FINITE):
        assert guarded_call(name, fill, byte_shift, sdm_shift, refuse=True) is None


@pytest.mark.parametrize("name", ["z7", "z1", "w64"])
def test_gap_tables_out_of_range_are_clamped(name):
    c = tm.case(name)
    Z, J = c["labels"].shape[1], len(c["gap"])
    wild = np.array(c["gap"], dtype=np.int64)
    wild[0::3], wild[1::3] = -5, Z + 5
    clamped = np.clip(wild, 0, max(Z - 2, 0))
    assert J == 1 or ((wild < 0).any() and (wild > Z - 1).any())
    maps, _ = device(name)
    want, _ = tm.blend_np(maps, clamped, c["alpha"], c["classes"])
    for byte_shift, sdm_shift in ((0, 0), (1, 1)):
        got = guarded_call(name, mg.POISON_NAN, byte_shift, sdm_shift, gap_host=wild)          # guards are checked inside
        assert same_bits(got[0], maps) and np.array_equal(got[1], want)
    extreme = np.where(np.arange(J) % 2 == 0, -2 ** 31, 2 ** 31 - 1)
    got = guarded_call(name, mg.POISON_FINITE, 0, 0, gap_host=extreme)
    assert np.array_equal(got[1], tm.blend_np(maps, np.clip(extreme, 0, max(Z - 2, 0)), c["alpha"], c["classes"])[0])


# ---- the evaluation protocol ----------------------------------------------------------------------------------------------------------
def sphere_labels(Z=8, S=28):
    """two nested balls whose radius shrinks along z: what a slice in the middle of a gap holds lies between its neighbours"""
    zz, yy, xx = np.meshgrid(np.arange(float(Z)), np.arange(float(S)), np.arange(float(S)), indexing="ij")
    r = np.sqrt((yy - 13.3) ** 2 + (xx - 13.6) ** 2)
    outer = 11.5 - 1.3 * zz
    return ((r <= outer).astype(np.uint8) + (r <= 0.5 * outer).astype(np.uint8)).astype(np.uint8)


def dice_np(pred, ref, classes):
    return np.array([[2.0 * ((pred == c) & (ref == c)).sum() / ((pred == c).sum() + (ref == c).sum()) for c in classes]])


def test_shape_baseline_and_score_label_supervolume_beside_nearest():
    import test_gpu_multichannel as tgm
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    from superresolution_aniso_mri_amd.evaluate.common import create_simple_interpolation
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    full = sphere_labels()
    Z, f, spacing, classes = full.shape[0], 2, (10.0, 1.25, 1.5), [1, 2]
    # in numpy first: the protocol on the restatement, and the nearest slice (x = o / f rounds half up: the later slice)
    kept, last, remain = si().baseline_plan(Z, f)
    assert (kept, last, remain) == ([0, 2, 4, 6], 6, 1)
    grid = si().resolve_grid(len(kept), num_interpolations=f - 1)
    maps = tm.signed_maps_np(full[None, ::f], [0, 1, 2], spacing[1], spacing[2])
    shape_np = np.concatenate([tm.blend_np(maps, grid.gap, grid.alpha, [0, 1, 2])[0][0][:last + 1], full[-remain:]])
    near_np = np.concatenate([full[::f][np.floor(np.arange(last + 1) / float(f) + 0.5).astype(int)], full[-remain:]])
    assert shape_np.shape == near_np.shape == full.shape
    d_shape, d_near = dice_np(shape_np, full, classes), dice_np(near_np, full, classes)
    print("numpy dice per class: shape %s, nearest %s" % (d_shape, d_near))
    assert (d_shape > d_near).all() and (d_near < 1.0).all()
    # the device: shape_baseline is the restated protocol, for host and device data
    got = si().shape_baseline(full, f, spacing)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, shape_np)
    got_dev = si().shape_baseline(torch.from_numpy(full.astype(np.float32)).cuda(), f, spacing)
    assert got_dev.is_cuda and got_dev.dtype == torch.uint8 and np.array_equal(got_dev.cpu().numpy(), shape_np)
    three = si().shape_baseline(full[:7], 3, spacing)
    assert three.shape == (7, 28, 28) and np.array_equal(three[::3], full[:7:3])
    # the scorer: the default is what it was, "shape" is one more table
    torch.manual_seed(11)
    tr = get_trainer_dynamic(tgm.trainer_args("ae", "mse", width=28, latent_width=7))
    tr.model.eval()
    labels = torch.from_numpy(full.astype(np.float32))
    images = torch.from_numpy((full / 2.0).astype(np.float32))
    default = seg_metrics.score_label_supervolume(tr, images, labels, f, spacing, classes=classes)
    assert sorted(default) == ["model", "nearest"]
    near = create_simple_interpolation(labels.cuda(), spacing, expand_factor=f, interpol_filter="nearest", generate_inbetween_slices=True, align="grid")
    today = seg_metrics.segmentation_scores(near.array, labels, spacing, classes=classes)
    assert np.array_equal(near.array.cpu().numpy(), near_np.astype(np.float32))
    both = seg_metrics.score_label_supervolume(tr, images, labels, f, spacing, classes=classes, baselines=("nearest", "shape"))
    assert sorted(both) == ["model", "nearest", "shape"]
    for k in today:
        assert np.array_equal(default["nearest"][k], today[k], equal_nan=True), k
        assert np.array_equal(both["nearest"][k], today[k], equal_nan=True) and np.array_equal(both["model"][k], default["model"][k], equal_nan=True), k
    want = seg_metrics.segmentation_scores(shape_np.astype(np.float32), labels, spacing, classes=classes)
    for k in seg_metrics.SCORE_KEYS:
        assert both["shape"][k].shape == (1, 2) and np.isfinite(both["shape"][k]).all(), k
        assert np.array_equal(both["shape"][k], want[k]), k
    assert np.array_equal(both["shape"]["dice"], d_shape) and np.array_equal(both["nearest"]["dice"], d_near)
    assert (both["shape"]["dice"] >= both["nearest"]["dice"]).all()
    only = seg_metrics.score_label_supervolume(tr, images, labels, f, spacing, classes=classes, baselines=("shape",))
    assert sorted(only) == ["model", "shape"]


# ---- the tools ------------------------------------------------------------------------------------------------------------------------
def test_both_tools_end_to_end(tmp_path, capsys):
    from superresolution_aniso_mri_amd import volume_io
    from superresolution_aniso_mri_amd.evaluate import compare_label_methods as clm
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    from superresolution_aniso_mri_amd.evaluate.common import create_simple_interpolation
    from superresolution_aniso_mri_amd.evaluate.z_grid import target_grid
    src, dst = tmp_path / "labels", tmp_path / "out"
    src.mkdir()
    one, frames = tm.case("z7")["labels"][0], tm.case("frames")["labels"]          # [7, 12, 20] and [2, 5, 10, 12]
    sp = (10.0, 1.25, 1.5)
    arr = one.astype(np.int16)
    volume_io.write_volume(str(src / "p01.nii.gz"), volume_io.Volume(arr, (sp[2], sp[1], sp[0]), "array", {}), arr)
    np.save(str(src / "p02.npy"), frames)
    written = si().main(["--labels_dir", str(src), "--output_dir", str(dst), "--num_interpolations", "2", "--spacing", "1.25", "1.5"])
    text = capsys.readouterr().out
    assert "p01.nii.gz: shape, 7 -> 19 slices" in text and "p02.npy: shape, 5 -> 13 slices" in text
    assert [w[0] for w in written] == [str(dst / "p01_ni02.nii.gz"), str(dst / "p02_ni02.npy")]
    back = volume_io.read_volume(str(dst / "p01_ni02.nii.gz"))
    assert back.array.shape == (19, 12, 20) and back.array.dtype == np.int16
    assert abs(back.spacing[2] - 10.0 / 3) < 1e-6 and back.spacing[:2] == (1.5, 1.25)
    want = si().shape_interpolate(one, num_interpolations=2, spacing_yx=sp[1:])
    assert np.array_equal(back.array, want) and np.array_equal(back.array[::3], one)
    back2 = np.load(str(dst / "p02_ni02.npy"))
    assert back2.shape == (2, 13, 10, 12) and back2.dtype == np.uint8
    assert np.array_equal(back2, si().shape_interpolate(frames, num_interpolations=2, spacing_yx=sp[1:]))
    # the nearest slice instead
    near = si().main(["--labels_dir", str(src / "p01.nii.gz"), "--output_dir", str(tmp_path / "near"), "--num_interpolations", "2", "--method", "nearest"])
    ref = create_simple_interpolation(one.astype(np.float32), sp, expand_factor=3, interpol_filter="nearest", align="grid").array
    assert near[0][1].shape == (19, 12, 20) and np.array_equal(near[0][1], ref.astype(np.int16))
    assert np.array_equal(volume_io.read_volume(str(tmp_path / "near" / "p01_ni02.nii.gz")).array, ref.astype(np.int16))
    # a target slice spacing: the .npy file needs --spacing_z
    with pytest.raises(SystemExit):
        si().main(["--labels_dir", str(src), "--output_dir", str(tmp_path / "sz"), "--target_spacing_z", "1.4"])
    capsys.readouterr()
    grid = si().main(["--labels_dir", str(src), "--output_dir", str(tmp_path / "sz"), "--target_spacing_z", "1.4", "--spacing_z", "10", "--spacing", "1.25", "1.5"])
    assert [w[1].shape for w in grid] == [(43, 12, 20), (2, 29, 10, 12)] and [w[2] for w in grid] == [1.4, 1.4]
    assert np.array_equal(grid[1][1], device("frames")[1]) and (tmp_path / "sz" / "p02_sz1.4.npy").exists()
    sz = volume_io.read_volume(str(tmp_path / "sz" / "p01_sz1.4.nii.gz"))
    assert abs(sz.spacing[2] - 1.4) < 1e-6 and np.array_equal(sz.array, si().shape_interpolate(one, grid=target_grid(7, 10.0, 1.4), spacing_yx=sp[1:]))
    capsys.readouterr()
    # the comparison: held-out slices of the sphere, nearest beside shape
    cmp_dir = tmp_path / "cmp"
    cmp_dir.mkdir()
    full = sphere_labels()
    np.save(str(cmp_dir / "ball.npy"), full)
    out = tmp_path / "scores.npz"
    res = clm.main(["--labels_dir", str(cmp_dir), "--downsample_steps", "2", "--spacing", "10", "1.25", "1.5", "--out", str(out)])
    text = capsys.readouterr().out
    assert "held-out label slices at 2x, 1 volume(s)" in text and "nearest" in text and "shape" in text and "assd" in text
    assert list(res["classes"]) == [1, 2] and list(res["names"]) == ["ball"]
    ref_t = torch.from_numpy(full.astype(np.float32)).cuda()
    want = seg_metrics.segmentation_scores(si().shape_baseline(full, 2, sp).astype(np.float32), ref_t, sp, classes=[1, 2])
    saved = np.load(str(out))
    for k in seg_metrics.SCORE_KEYS:
        assert np.array_equal(res["shape"][k], want[k], equal_nan=True) and np.array_equal(saved["shape/" + k], want[k], equal_nan=True), k
        assert saved["nearest/" + k].shape == (1, 2)
    assert (res["shape"]["dice"] > res["nearest"]["dice"]).all()
