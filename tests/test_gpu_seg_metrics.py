"""GPU: csrc/seg_metrics.hip (overlap counts, borders, exact surface distances, compaction) and the layers above it against the numpy
restatement of tests/test_seg_metrics_golden.py and the fixture of the reference's kwatsch/medpy_metrics.py
(tests/make_golden_seg_metrics.py).

Bounds: counts are integers and exactly equal.  A distance is sqrt of a minimum of sums of squared fp64 products, made in the stated
association on both sides, so device and restatement are expected to agree bit for bit; they are held to 1e-12 relative (the bound the
restatement itself is held to against scipy), and so are hd / hd95 / asd / assd, whose sums run in another order than numpy's pairwise one
(a few hundred to a few thousand terms: relative error of some 1e-16 each).  Order and length of every list are exact.  Measured on an MI355X: 0
for every distance of every case (profiles/seg_metrics.txt).  Then two runs bit
for bit, frames against the batch, chunked batches, both label load paths, foreign labels, guard bands with NaN / 3e38 poisons and
shifted pointers, the mirror module, the model scorer and the command line."""

import numpy as np
import pytest
import torch

import memguard as mg
import test_seg_metrics_golden as tm

pytestmark = pytest.mark.gpu
REL = tm.REL
CASES = ["aniso", "ties", "multiwg", "img2d", "z1", "frames", "eight", "extreme", "faces", "oneside"]

GUARDED_ENTRIES = {
    "aesr_surface_borders": "test_guard_bands_poisons_and_shifted_pointers",
    "aesr_surface_distances": "test_guard_bands_poisons_and_shifted_pointers",
}
EXEMPT = {"aesr_surface_workspace_bytes": "a size query on the host: it is given no buffer"}


def modes(rank):
    return [(2, 1), (2, 2)] if rank == 2 else [(3, 1), (3, 2), (3, 3), (2, 1), (2, 2)]


def device_lists(name, nd, k):
    """surface_distance_lists of a whole case (all frames and classes in one call) -> (dict, list(n, c, d) accessor)"""
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    r, g, sp, classes, _, _ = tm.case_frames(name)
    out = seg_metrics.surface_distance_lists(r, g, sp, classes=classes, ndim=nd, connectivity=k)

    def lst(n, ci, d):
        o, ln = int(out["offsets"][n, ci, d]), int(out["lengths"][n, ci, d])
        return out["distances"][o:o + ln]
    return out, lst


@pytest.mark.parametrize("name", CASES)
def test_counts_equal_numpy(name):
    from superresolution_aniso_mri_amd import ops
    r, g, sp, classes, _, rank = tm.case_frames(name)
    for nd, k in modes(rank):
        counts, _ = ops.surface_borders(torch.from_numpy(r).cuda(), torch.from_numpy(g).cuda(), classes, ndim=nd, connectivity=k)
        counts = counts.cpu().numpy()
        assert counts.shape == (r.shape[0], len(classes), 7) and counts.dtype == np.int64
        for n in range(r.shape[0]):
            for ci, c in enumerate(classes):
                A, B = r[n] == c, g[n] == c
                want = tm.counts_np(A, B) + [int(tm.border_np(A, nd, k).sum()), int(tm.border_np(B, nd, k).sum())]
                assert list(counts[n, ci]) == want, (name, nd, k, n, c)


@pytest.mark.parametrize("name", CASES)
def test_lists_and_scores_against_restatement_and_fixture(name):
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    rec = tm.fixture()
    r, g, sp, classes, empty, rank = tm.case_frames(name)
    restated = tm.restated_lists(name)
    worst, seen = 0.0, 0
    for nd, k in modes(rank):
        out, lst = device_lists(name, nd, k)
        scores = seg_metrics.segmentation_scores(r, g, sp, classes=classes, ndim=nd, connectivity=k)
        assert sorted(scores) == sorted(seg_metrics.SCORE_KEYS + ("counts", "volume_ml_result", "volume_ml_reference", "classes"))
        assert np.array_equal(scores["counts"], out["counts"]) and scores["dice"].shape == (r.shape[0], len(classes))
        for n in range(r.shape[0]):
            for ci, c in enumerate(classes):
                key = "%s/n%d/c%d/d%d/k%d" % (name, n, c, nd, k)
                A, B = r[n] == c, g[n] == c
                over = [scores[q][n, ci] for q in ("dice", "jc", "precision", "recall", "specificity", "ravd")]
                assert tm.close(over, rec["%s/n%d/c%d/overlap" % (name, n, c)]), key
                vox_ml = sp[0] * sp[1] * sp[2] / 1000.0
                assert scores["volume_ml_result"][n, ci] == A.sum() * vox_ml and scores["volume_ml_reference"][n, ci] == B.sum() * vox_ml
                dist = [scores[q][n, ci] for q in ("hd", "hd95", "asd_result_to_reference", "asd_reference_to_result", "assd")]
                if c in empty:
                    # the empty-mask rule: no lists, NaN distance scores, dice 0.0 as the reference's ZeroDivisionError branch gives
                    assert len(lst(n, ci, 0)) == 0 and len(lst(n, ci, 1)) == 0 and all(np.isnan(v) for v in dist), key
                    assert scores["dice"][n, ci] == 0.0
                    continue
                if key not in restated:          # slice-wise mode with a one-sided slice: the reference raises there; see the test below
                    continue
                seen += 1
                for d, tag in ((0, "sds_rg"), (1, "sds_gr")):
                    got, want, fix = lst(n, ci, d), restated[key][d], rec["%s/%s" % (key, tag)]
                    assert got.shape == want.shape == fix.shape, (key, tag)          # element by element below: raster order
                    assert tm.close(got, want) and tm.close(got, fix), (key, tag)
                    worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
                assert tm.close(dist, rec[key + "/scores"]), (key, dist, rec[key + "/scores"])
    assert seen
    print("%s: %d records, worst relative difference device - restatement %.3g" % (name, seen, worst))


def test_slice_wise_mode_gives_infinity_where_a_slice_has_no_partner():
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    r = np.zeros((3, 6, 7), dtype=np.float32)
    g = np.zeros((3, 6, 7), dtype=np.float32)
    r[:, 1:4, 1:5] = 1
    g[0, 2:5, 2:6] = g[2, 0:3, 0:3] = 1          # slice 1 of the reference holds nothing
    out = seg_metrics.surface_distance_lists(r, g, (5.0, 1.0, 2.0), classes=[1], ndim=2, connectivity=1)
    got = out["distances"][:int(out["lengths"][0, 0, 0])]
    want = tm.surface_distances_np(r == 1, g == 1, (5.0, 1.0, 2.0), 2, 1)
    assert np.array_equal(got, want) and np.isinf(got).sum() == tm.border_np(r[1:2] == 1, 2, 1).sum() and not np.isnan(got).any()
    s = seg_metrics.segmentation_scores(r, g, (5.0, 1.0, 2.0), classes=[1], ndim=2)
    assert np.isinf(s["hd"][0, 0]) and np.isinf(s["hd95"][0, 0]) and s["dice"][0, 0] > 0


def _raw(name, nd=3, k=1, max_ws=1 << 30):
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    r, g, sp, classes, _, _ = tm.case_frames(name)
    rr, gg = torch.from_numpy(r).cuda(), torch.from_numpy(g).cuda()
    counts, stats, lengths, dist = seg_metrics._run(rr, gg, sp, classes, nd, k, max_ws)
    return counts, stats, lengths, dist.cpu().numpy()


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) and x.shape == y.shape for x, y in zip(a, b))


def test_two_runs_frames_and_chunks_agree_bit_for_bit():
    from superresolution_aniso_mri_amd import ops
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    first = _raw("frames")
    assert _same(first, _raw("frames")) and _same(_raw("multiwg", 3, 3), _raw("multiwg", 3, 3))
    # the batch equals its frames
    r, g, sp, classes, _, _ = tm.case_frames("frames")
    parts = [seg_metrics._run(torch.from_numpy(r[n:n + 1]).cuda(), torch.from_numpy(g[n:n + 1]).cuda(), sp, classes, 3, 1, 1 << 30)
             for n in range(r.shape[0])]
    glued = [np.concatenate([p[i] for p in parts]) for i in range(3)] + [torch.cat([p[3] for p in parts]).cpu().numpy()]
    assert _same(first, glued)
    # a workspace limit that holds two frames, then one, then less than one: N is split, nothing changes
    one = ops.surface_workspace_bytes(1, 6, 20, 18, 3)
    assert seg_metrics._frames_per_call(3, 6, 20, 18, 3, 1 << 30) == 3 and seg_metrics._frames_per_call(3, 6, 20, 18, 3, 2 * one + 64) == 2
    assert seg_metrics._frames_per_call(3, 6, 20, 18, 3, one) == 1 and seg_metrics._frames_per_call(3, 6, 20, 18, 3, 10) == 1
    for limit in (2 * one + 64, one, 10):
        assert _same(first, _raw("frames", max_ws=limit)), limit
    a = seg_metrics.segmentation_scores(r, g, sp, classes=classes)
    b = seg_metrics.segmentation_scores(r, g, sp, classes=classes, max_workspace_bytes=one)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    # a device tensor in, the same tables out; classes=None is 1 ... the largest reference label
    c = seg_metrics.segmentation_scores(torch.from_numpy(r).cuda(), torch.from_numpy(g).cuda(), sp)
    assert list(c["classes"]) == [1, 2, 3] and all(np.array_equal(a[k], c[k], equal_nan=True) for k in a)
    lists = seg_metrics.surface_distance_lists(torch.from_numpy(r).cuda(), torch.from_numpy(g).cuda(), sp, classes=classes)
    assert torch.is_tensor(lists["distances"]) and lists["distances"].is_cuda and np.array_equal(lists["distances"].cpu().numpy(), first[3])


def _phases(rt, gt, classes, sp, nd=3, k=1):
    from superresolution_aniso_mri_amd import ops
    counts, ws = ops.surface_borders(rt, gt, classes, ndim=nd, connectivity=k)
    dist, stats, lengths = ops.surface_distances(ws, counts, rt.shape, sp, ndim=nd)
    return counts.cpu().numpy(), stats.cpu().numpy(), lengths, dist.cpu().numpy()


def test_both_label_load_paths_agree_and_are_taken():
    from superresolution_aniso_mri_amd import ops
    r, g, sp, classes, _, _ = tm.case_frames("frames")
    dev = torch.device("cuda")
    n = r.size
    aligned = [mg.guarded(n, torch.float32, dev, torch.from_numpy(x), 0, nm).view.view(r.shape) for x, nm in ((r, "result"), (g, "reference"))]
    assert ops.surface_label_path(*aligned) == "vec16" and aligned[0].data_ptr() % 16 == 0 and r[0].size % 4 == 0
    base = _phases(aligned[0], aligned[1], classes, sp)
    for shift in (1, 2, 3):
        moved = [mg.guarded(n, torch.float32, dev, torch.from_numpy(x), shift, nm).view.view(r.shape) for x, nm in ((r, "result"), (g, "reference"))]
        assert ops.surface_label_path(*moved) == "scalar4" and moved[0].data_ptr() % 16 == 4 * shift
        assert _same(base, _phases(moved[0], moved[1], classes, sp)), shift
        assert ops.surface_label_path(aligned[0], moved[1]) == "scalar4" and _same(base, _phases(aligned[0], moved[1], classes, sp))
    # a volume whose voxel count is no multiple of 4 takes the 4-byte path whatever the alignment; it is checked against numpy above
    r2, g2, _, _, _, _ = tm.case_frames("ties")
    assert r2[0].size % 4 == 1 and ops.surface_label_path(torch.from_numpy(r2).cuda(), torch.from_numpy(g2).cuda()) == "scalar4"


def test_foreign_labels_belong_to_no_class():
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    r, g, sp, classes, _, _ = tm.case_frames("aniso")
    r, g = r.copy(), g.copy()
    rng = np.random.default_rng(5)
    for vol in (r, g):
        idx = rng.choice(vol.size, 60, replace=False)
        vol.reshape(-1)[idx] = np.resize(np.array([np.nan, 2.5, -1.0, 7.0, np.inf, 1.0000001], dtype=np.float32), 60)
    out = seg_metrics.surface_distance_lists(r, g, sp, classes=classes, connectivity=2)
    for ci, c in enumerate(classes):
        A, B = r[0] == c, g[0] == c
        assert list(out["counts"][0, ci, :5]) == tm.counts_np(A, B)
        for d, (X, Y) in enumerate(((A, B), (B, A))):
            o, ln = int(out["offsets"][0, ci, d]), int(out["lengths"][0, ci, d])
            assert tm.close(out["distances"][o:o + ln], tm.surface_distances_np(X, Y, sp, 3, 2)), (c, d)
    # a class list in another order, and with an id that occurs nowhere
    s = seg_metrics.segmentation_scores(r, g, sp, classes=[3, 9, 1])
    t = seg_metrics.segmentation_scores(r, g, sp, classes=[1, 2, 3])
    assert np.array_equal(s["hd95"][:, [2, 0]], t["hd95"][:, [0, 2]]) and np.isnan(s["hd"][0, 1]) and s["dice"][0, 1] == 0.0


# ---- guard bands -------------------------------------------------------------------------------------------------------------------
def _guarded_call(name, nd, k, fill, label_shift, out_shift, refuse=None):
    """Both entry points with every buffer at exactly its contractual size between guard bands.  Returns (counts, stats, distances)."""
    from superresolution_aniso_mri_amd import _hip
    lib = _hip.lib
    r, g, sp, classes, _, _ = tm.case_frames(name)
    N, Z, H, W = r.shape
    C = len(classes)
    dev = torch.device("cuda")
    G = lambda n, dt, f, s, nm: mg.guarded(n, dt, dev, f, s, nm)          # noqa: E731
    res, ref = G(r.size, torch.float32, torch.from_numpy(r), label_shift, "result"), G(g.size, torch.float32, torch.from_numpy(g), label_shift, "reference")
    ws = G(lib.aesr_surface_workspace_bytes(N, Z, H, W, C), torch.uint8, fill, 0, "workspace")
    cnt = G(N * C * 7, torch.int64, fill, out_shift, "counts")
    assert ws.view.data_ptr() % 16 == 0 and cnt.view.data_ptr() % 8 == 0
    saved = [mg.bits(res.view), mg.bits(ref.view)]
    cls = _hip.int_array(classes)
    if refuse == "borders":
        for bad in (dict(connectivity=0), dict(ndim=4), dict(classes=_hip.int_array([classes[0]] * C))):
            a = dict(ndim=nd, connectivity=k, classes=cls)
            a.update(bad)
            assert lib.aesr_surface_borders(_hip.ptr(res.view), _hip.ptr(ref.view), _hip.ptr(ws.view), _hip.ptr(cnt.view), N, Z, H, W,
                                            a["classes"], C, a["ndim"], a["connectivity"], _hip.stream()) == 1
        torch.cuda.synchronize()
        assert mg.poison_left(cnt.view, fill).numel() == cnt.view.numel() and mg.poison_left(ws.view, fill).numel() == ws.view.numel()
        mg.assert_guards_intact([res, ref, ws, cnt])
        return None
    _hip.check(lib.aesr_surface_borders(_hip.ptr(res.view), _hip.ptr(ref.view), _hip.ptr(ws.view), _hip.ptr(cnt.view), N, Z, H, W, cls, C, nd, k,
                                        _hip.stream()), "aesr_surface_borders")
    torch.cuda.synchronize()
    mg.assert_guards_intact([res, ref, ws, cnt])
    assert mg.poison_left(cnt.view, fill).numel() == 0
    host = cnt.view.cpu().numpy().reshape(N, C, 7).copy()
    total = int(np.where(((host[..., 0] > 0) & (host[..., 1] > 0))[..., None], host[..., 5:], 0).sum())
    dist = G(total, torch.float64, fill, out_shift, "distances")
    stats = G(N * C * 4, torch.float64, fill, out_shift, "stats")
    saved_cnt, spacing = mg.bits(cnt.view), _hip.double_array(sp)
    args = lambda cap, s: (_hip.ptr(ws.view), _hip.ptr(cnt.view), host.ctypes.data_as(_hip.LLP), _hip.ptr(dist.view), cap,          # noqa: E731
                           _hip.ptr(stats.view), N, Z, H, W, C, nd, s, _hip.stream())
    if refuse == "distances":
        ws_before = mg.bits(ws.view)
        assert lib.aesr_surface_distances(*args(total - 1, spacing)) == 1 and "distances" in _hip.last_error()
        assert lib.aesr_surface_distances(*args(total, _hip.double_array([1.0, 0.0, 1.0]))) == 1
        torch.cuda.synchronize()
        assert mg.poison_left(dist.view, fill).numel() == total and mg.poison_left(stats.view, fill).numel() == N * C * 4
        mg.assert_unchanged(ws.view, ws_before, "workspace")
        mg.assert_guards_intact([ws, cnt, dist, stats])
        return None
    _hip.check(lib.aesr_surface_distances(*args(total, spacing)), "aesr_surface_distances")
    torch.cuda.synchronize()
    mg.assert_guards_intact([res, ref, ws, cnt, dist, stats])
    mg.assert_unchanged(res.view, saved[0], "result")
    mg.assert_unchanged(ref.view, saved[1], "reference")
    mg.assert_unchanged(cnt.view, saved_cnt, "counts")
    assert mg.poison_left(dist.view, fill).numel() == 0 and mg.poison_left(stats.view, fill).numel() == 0
    return host, stats.view.cpu().numpy().reshape(N, C, 2, 2), dist.view.cpu().numpy()


@pytest.mark.parametrize("name,nd,k", [("frames", 3, 1), ("ties", 3, 3), ("multiwg", 3, 2), ("z1", 2, 2), ("oneside", 2, 1)])
def test_guard_bands_poisons_and_shifted_pointers(name, nd, k):
    counts, stats, lengths, dist = _raw(name, nd, k)
    for fill in (mg.POISON_NAN, mg.POISON_FINITE):
        for label_shift, out_shift in ((0, 0), (1, 1), (2, 0), (3, 1)):          # labels by 4 / 8 / 12 bytes; 8-byte outputs by 8 bytes
            got = _guarded_call(name, nd, k, fill, label_shift, out_shift)
            assert _same((counts, stats, dist), got), (fill, label_shift, out_shift)
        assert _guarded_call(name, nd, k, fill, 1, 1, refuse="borders") is None
        assert _guarded_call(name, nd, k, fill, 0, 1, refuse="distances") is None


# ---- the mirror module -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aniso", "img2d", "z1", "extreme", "faces"])
def test_mirror_functions_equal_the_fixture(name):
    import kwatsch.medpy_metrics as m
    rec = tm.fixture()
    res, ref, sp = rec[name + "/result"], rec[name + "/reference"], tuple(float(s) for s in rec[name + "/spacing"])
    rank = len(sp)
    for c in (int(v) for v in rec[name + "/classes"]):
        a, b = (res == c).astype(np.uint8), (ref == c).astype(np.int32) * 5          # any type; binarised by != 0
        over = [m.dc(a, b), m.jc(a, b), m.precision(a, b), m.recall(a, b), m.specificity(a, b), m.ravd(a, b)]
        assert tm.close(over, rec["%s/n0/c%d/overlap" % (name, c)]), (name, c)
        assert m.sensitivity(a, b) == m.recall(a, b) == m.true_positive_rate(a, b) == m.true_negative_rate(a, b)
        assert m.positive_predictive_value(a, b) == m.precision(a, b)
        for k in range(1, rank + 1):
            want = rec["%s/n0/c%d/d%d/k%d/scores" % (name, c, rank, k)]
            got = [m.hd(a, b, sp, k), m.hd95(a, b, sp, k), m.asd(a, b, sp, k), m.asd(b, a, sp, k), m.assd(a, b, sp, k)]
            assert tm.close(got, want), (name, c, k, got, want)
    a = torch.from_numpy((res == 1).astype(np.float32))
    on_device = m.hd(a.cuda(), torch.from_numpy((ref == 1).astype(np.float32)).cuda(), voxelspacing=sp)
    assert tm.close([on_device], rec["%s/n0/c1/d%d/k1/scores" % (name, rank)][:1])


def test_mirror_spacing_and_errors():
    import kwatsch.medpy_metrics as m
    a = np.zeros((4, 5, 6))
    a[1:3, 1:4, 2:5] = 1
    b = np.roll(a, 1, axis=2)
    assert m.hd(a, b) == m.hd(a, b, 1.0) == m.hd(a, b, (1, 1, 1)) == 1.0 and m.hd(a, b, 2.5) == 2.5 and m.hd(a, b, (7, 7, 0.5)) == 0.5
    zero = np.zeros_like(a)
    with pytest.raises(RuntimeError, match="^The first supplied array does not contain any binary object.$"):
        m.hd(zero, a)
    with pytest.raises(RuntimeError, match="^The second supplied array does not contain any binary object.$"):
        m.assd(a, zero)
    with pytest.raises(RuntimeError, match="^The second supplied array does not contain any binary object.$"):
        m.ravd(a, zero)
    with pytest.raises(ZeroDivisionError):
        m.jc(zero, zero)
    assert m.dc(zero, zero) == 0.0 and m.precision(zero, a) == 0.0 and m.recall(a, zero) == 0.0
    with pytest.raises(ValueError, match="rank"):
        m.dc(np.ones(5), np.ones(5))


# ---- a model's label output --------------------------------------------------------------------------------------------------------
def test_score_label_supervolume_on_the_small_multichannel_model():
    import test_gpu_multichannel as tgm
    from superresolution_aniso_mri_amd.evaluate import common as ec
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    from superresolution_aniso_mri_amd.kwatsch.get_trainer import get_trainer_dynamic
    torch.manual_seed(11)
    tr = get_trainer_dynamic(tgm.trainer_args("ae", "mse", width=28, latent_width=7))
    tr.model.eval()
    zz, yy, xx = np.meshgrid(np.arange(7.0), np.arange(28.0), np.arange(28.0), indexing="ij")
    field = np.exp(-((yy - 13 - 0.5 * zz) ** 2 + (xx - 14 + 0.4 * zz) ** 2) / (2 * 7.0 ** 2))
    labels = torch.from_numpy(np.floor(4 * 0.999 * field).astype(np.float32))
    images = torch.from_numpy(field.astype(np.float32))
    spacing = (10.0, 1.4, 1.4)
    got = seg_metrics.score_label_supervolume(tr, images, labels, 2, spacing, classes=[1, 2, 3])
    assert sorted(got) == ["model", "nearest"]
    out = ec.create_super_volume(tr, images, alpha_range=[0.5], downsample_steps=2, generate_inbetween_slices=True, labels=labels)
    assert tuple(out["upsampled_labels"].shape) == (7, 28, 28)
    want = seg_metrics.segmentation_scores(out["upsampled_labels"].float(), labels, spacing, classes=[1, 2, 3])
    for k in want:
        assert np.array_equal(got["model"][k], want[k], equal_nan=True), k
    near = got["nearest"]
    for k in seg_metrics.SCORE_KEYS:
        assert near[k].shape == (1, 3) and np.isfinite(near[k]).all(), k
    assert (near["dice"] > 0.5).all() and (near["dice"] < 1.0).any()          # kept slices are exact, the ones in between are not
    with pytest.raises(ValueError, match="do not match"):
        seg_metrics.score_label_supervolume(tr, images, labels[:6], 2, spacing, classes=[1, 2, 3])


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_score_labels_end_to_end(tmp_path, capsys):
    from superresolution_aniso_mri_amd import volume_io
    from superresolution_aniso_mri_amd.evaluate import score_labels, seg_metrics
    rec = tm.fixture()
    (tmp_path / "pred").mkdir()
    (tmp_path / "ref").mkdir()
    sp = (10.0, 1.4, 1.4)
    vols = {"p01": (rec["aniso/result"], rec["aniso/reference"]), "p02": (rec["frames/result"][:2], rec["frames/reference"][:2])}
    for stem, (r, g) in vols.items():
        for d, arr in (("pred", r), ("ref", g)):
            arr = arr.astype(np.int16)
            like = volume_io.Volume(arr, (sp[2], sp[1], sp[0]) + ((1.0,) if arr.ndim == 4 else ()), "array", {})
            volume_io.write_volume(str(tmp_path / d / (stem + ".nii.gz")), like, arr)
    out = tmp_path / "scores.npz"
    scores = score_labels.main(["--pred", str(tmp_path / "pred"), "--ref", str(tmp_path / "ref"), "--classes", "1", "2", "3", "--out", str(out)])
    text = capsys.readouterr().out
    assert "2 file(s), 3 frame(s)" in text and "hd95" in text and text.count("\n") >= 6
    saved = np.load(str(out))
    assert list(saved["names"]) == ["p01", "p02", "p02"]
    sp32 = tuple(float(np.float32(s)) for s in sp)          # the header stores the spacing as fp32
    want = [seg_metrics.segmentation_scores(r.astype(np.float32), g.astype(np.float32), sp32, classes=[1, 2, 3]) for r, g in vols.values()]
    for k in seg_metrics.SCORE_KEYS + ("counts",):
        assert np.array_equal(scores[k], np.concatenate([w[k] for w in want]), equal_nan=True), k
        assert np.array_equal(saved[k], scores[k], equal_nan=True), k
    # one file against one file, classes from the reference
    one = score_labels.main(["--pred", str(tmp_path / "pred" / "p01.nii.gz"), "--ref", str(tmp_path / "ref" / "p01.nii.gz"), "--ndim", "2",
                             "--connectivity", "2"])
    assert list(one["classes"]) == [1, 2, 3] and one["dice"].shape == (1, 3)
