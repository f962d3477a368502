"""GPU: csrc/components.hip and what stands on it against the fixture of scipy.ndimage and the reference's kwatsch/medpy_metrics.py
(tests/golden/components.npz) and the numpy restatement of tests/test_components_golden.py.

Labels, counts and tables equal the fixture exactly for every case, ndim and connectivity; overlap runs equal the restated rule and their
pair sets a brute force; the clean-up equals its restatement; the object-wise scores equal the reference's (counts, tpr, fpr exactly, the
distances to 1e-12 relative: only the order of the mean's sum differs); two runs give the same bits; guard bands, poisoned workspace and
outputs and shifted pointers for every guarded entry point; the command lines end to end.

GUARDED_ENTRIES and EXEMPT partition ``_hip.SIGNATURES_COMPONENTS`` (tests/test_abi.py checks that without a GPU)."""
import os

import numpy as np
import pytest
import torch

import memguard as mg
import test_components_golden as tm

pytestmark = pytest.mark.gpu

REL = 1e-12
GUARDED_ENTRIES = {
    "aesr_components_label": "_guarded_sequence: vol, labels, n_components, workspace",
    "aesr_components_tables": "_guarded_sequence: table",
    "aesr_components_overlap_count": "_guarded_sequence: count",
    "aesr_components_overlap_runs": "_guarded_sequence: runs",
    "aesr_components_apply_table": "_guarded_sequence: the fp32 table, out",
}
EXEMPT = {"aesr_components_workspace_bytes": "a size query on the host: it is given no buffer"}
_CACHE = {}


def case(name):
    rec = tm.fixture()
    return tm.frames4(rec[name + "/vol"]), [int(c) for c in rec[name + "/classes"]]


def device_labelling(name, nd, k):
    """(labels, n, table) of the device as numpy, computed once per (case, mode)"""
    from superresolution_aniso_mri_amd import ops
    key = (name, nd, k)
    if key not in _CACHE:
        vol, classes = case(name)
        v = torch.from_numpy(vol).cuda()
        lab, n, ws = ops.components_label(v, classes, ndim=nd, connectivity=k)
        table, host = ops.components_tables(v, lab, n, classes, ndim=nd, workspace=ws)
        assert np.array_equal(host, n.cpu().numpy())
        _CACHE[key] = (lab.cpu().numpy(), host, table.cpu().numpy())
    return _CACHE[key]


# ---- labelling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tm.LABEL_CASES)
def test_labels_counts_and_tables_equal_the_fixture(name):
    rec = tm.fixture()
    for nd, k in tm.case_modes(name):
        labels, n, table = device_labelling(name, nd, k)
        key = "%s/d%d/k%d" % (name, nd, k)
        want = tm.frames4(rec[key + "/labels"])
        bad = np.argwhere(labels != want)
        assert not len(bad), "%s: %d voxels differ, first at %s: %d, scipy %d" % (key, len(bad), bad[0], labels[tuple(bad[0])], want[tuple(bad[0])])
        assert labels.dtype == np.int32 and n.dtype == np.int32 and table.dtype == np.int64
        assert np.array_equal(n, rec[key + "/n"]), key
        assert np.array_equal(table, rec[key + "/table"]), key


def test_label_components_keeps_shape_and_container():
    from superresolution_aniso_mri_amd.evaluate.components import label_components
    rec = tm.fixture()
    out = label_components(rec["img2d/vol"][None], classes=[1, 2, 3], ndim=2, connectivity=2)          # [Z = 1, H, W] numpy in
    assert isinstance(out["labels"], np.ndarray) and np.array_equal(out["labels"][0], rec["img2d/d2/k2/labels"])
    table = rec["img2d/d2/k2/table"]
    assert np.array_equal(out["n_components"], rec["img2d/d2/k2/n"]) and np.array_equal(out["sizes"], table[:, 0])
    assert np.array_equal(out["boxes"], table[:, 1:7]) and np.array_equal(out["first_voxels"], table[:, 7])
    assert out["offsets"].tolist() == [(np.cumsum(rec["img2d/d2/k2/n"].reshape(-1)) - rec["img2d/d2/k2/n"].reshape(-1)).tolist()]
    dev = label_components(torch.from_numpy(rec["eight/vol"]).cuda(), classes=list(range(8)))          # [N, Z, H, W] CUDA tensor in
    assert dev["labels"].is_cuda and dev["sizes"].is_cuda and tuple(dev["labels"].shape) == rec["eight/vol"].shape
    assert np.array_equal(dev["labels"].cpu().numpy(), rec["eight/d3/k1/labels"]) and list(dev["classes"]) == list(range(8))
    top = label_components(rec["full/vol"])          # classes = None: 1 ... the largest label
    assert list(top["classes"]) == [1] and top["n_components"].tolist() == [[1]] and top["sizes"].tolist() == [120]


def test_foreign_values_belong_to_no_class():
    from superresolution_aniso_mri_amd import ops
    vol = np.zeros((1, 2, 3, 8), dtype=np.float32)
    vol[0, 0, 0] = [1, 1.5, 1, np.nan, 1, np.inf, -1, 1]
    vol[0, 1, 0, :2] = [7, 1]
    lab, n, _ = ops.components_label(torch.from_numpy(vol).cuda(), [1, -1], ndim=3, connectivity=1)
    assert lab.cpu().numpy()[0, 0, 0].tolist() == [1, 0, 2, 0, 3, 0, 1, 4] and n.cpu().numpy().tolist() == [[5, 1]]
    assert lab.cpu().numpy()[0, 1, 0].tolist() == [0, 5, 0, 0, 0, 0, 0, 0]


# ---- overlap runs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "slices6", "eight", "diagonal", "multiwg"])
def test_overlap_runs_and_pair_sets(name):
    from superresolution_aniso_mri_amd import ops
    vol, classes = case(name)
    other = np.roll(vol, (1, 2), axis=(2, 3))
    va, vb = torch.from_numpy(vol).cuda(), torch.from_numpy(other).cuda()
    for nd, k in tm.case_modes(name):
        la, _, ws = ops.components_label(va, classes, ndim=nd, connectivity=k)
        lb, _, _ = ops.components_label(vb, classes, ndim=nd, connectivity=k)
        runs = ops.components_overlaps(va, la, vb, lb, classes, ndim=nd, workspace=ws).cpu().numpy()
        want_b, _, _ = tm.label_np(other, classes, nd, k)
        assert np.array_equal(lb.cpu().numpy(), want_b)
        la_np = la.cpu().numpy()
        assert np.array_equal(runs, tm.overlap_runs_np(vol, la_np, other, want_b, classes, nd)), (name, nd, k)
        ka, kb = tm.class_index_np(vol, classes), tm.class_index_np(other, classes)
        both = (ka >= 0) & (ka == kb)
        Vu = vol[0, 0].size if nd == 2 else vol[0].size
        unit = (np.arange(vol.size) // Vu).reshape(vol.shape)
        brute = np.unique(np.stack([unit[both], ka[both], la_np[both], want_b[both]], axis=1), axis=0)
        assert np.array_equal(np.unique(runs, axis=0), brute), (name, nd, k)


# ---- clean-up ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nd,k", [("tie", 3, 1), ("tie", 2, 1), ("ties", 3, 2), ("eight", 3, 1), ("slices6", 2, 2), ("img2d", 2, 1)])
def test_clean_up_equals_the_restatement(name, nd, k):
    from superresolution_aniso_mri_amd.evaluate.components import keep_largest_component, remove_small_components
    rec = tm.fixture()
    vol, classes = case(name)
    given = rec[name + "/vol"] if rec[name + "/vol"].ndim >= 3 else rec[name + "/vol"][None]          # [Z, H, W] or [N, Z, H, W]
    for largest, min_size in ((True, 0), (False, 4), (False, 1)):
        want = tm.keep_np(vol, classes, nd, k, largest, min_size).reshape(given.shape)
        fn = (lambda v: keep_largest_component(v, classes, nd, k)) if largest else (lambda v: remove_small_components(v, min_size, classes, nd, k))
        got = fn(given)
        assert isinstance(got, np.ndarray) and got.dtype == given.dtype and np.array_equal(got, want, equal_nan=True), (name, largest, min_size)
        dev = fn(torch.from_numpy(given).cuda())
        assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(dev.cpu().numpy(), want, equal_nan=True)
    if name == "tie":          # the first of two equal components survives; values outside `classes` pass through, 2.5 and 7 included
        kept = keep_largest_component(given, classes, nd, k)
        if nd == 3:
            assert (kept[0:2, 0:2, 0:2] == 1).all() and not (kept[2:4, 3:5, 5:7] != 0).any() and (kept == 2).sum() == 5 and (kept[2, 0, 0:5] == 2).all()
        assert kept[1, 3, 3] == 7 and kept[1, 3, 4] == 2.5
        only1 = keep_largest_component(given, [1], nd, k)
        assert np.array_equal(only1[given == 2], given[given == 2])
    if name == "eight":          # integer containers keep their dtype
        for dt in (np.uint8, np.int16, np.int64):
            got = keep_largest_component(given.astype(dt), classes, nd, k)
            assert got.dtype == dt and np.array_equal(got, tm.keep_np(vol, classes, nd, k, True).reshape(given.shape).astype(dt))
        t = keep_largest_component(torch.from_numpy(given.astype(np.int16)).cuda(), classes, nd, k)
        assert t.is_cuda and t.dtype == torch.int16


# ---- object-wise scores --------------------------------------------------------------------------------------------------------------
def close(got, want, rel=REL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same_nan = np.isnan(got) == np.isnan(want)
    fin = ~np.isnan(want)
    return bool(got.shape == want.shape and same_nan.all() and (np.abs(got[fin] - want[fin]) <= rel * np.abs(want[fin])).all())


@pytest.mark.parametrize("name", tm.SCORE_CASES)
def test_object_scores_equal_the_reference(name):
    from superresolution_aniso_mri_amd.evaluate import object_metrics as om
    rec = tm.fixture()
    frames, sp, classes, conn, rank = tm.score_frames(name)
    nd = 3 if rank == 3 else 2
    r = np.stack([tm.frames4(f[1])[0] for f in frames])
    g = np.stack([tm.frames4(f[2])[0] for f in frames])
    s = om.object_scores(r, g, [1.0] * (3 - rank) + sp, classes=classes, ndim=nd, connectivity=conn)
    for n, _, _ in frames:
        for ci, c in enumerate(classes):
            key = "%s/n%d/c%d" % (name, n, c)
            want = rec[key + "/scores"]
            print(key, [s[k][n, ci] for k in om.OBJECT_KEYS], want)
            assert [int(s["n_objects_result"][n, ci]), int(s["n_objects_reference"][n, ci])] == rec[key + "/counts"].tolist(), key
            assert int(s["n_matched"][n, ci]) == len(rec[key + "/map_ref"]), key
            assert np.array_equal([s["obj_tpr"][n, ci], s["obj_fpr"][n, ci]], want[:2], equal_nan=True), key
            assert close([s["obj_asd_result_to_reference"][n, ci], s["obj_asd_reference_to_result"][n, ci], s["obj_assd"][n, ci]], want[4:]), key
    assert s["obj_tpr"].dtype == np.float64 and s["n_matched"].dtype == np.int64 and s["obj_tpr"].shape == (len(frames), len(classes))
    # the other call direction: tpr / fpr of (reference, result)
    t = om.object_scores(g, r, [1.0] * (3 - rank) + sp, classes=classes, ndim=nd, connectivity=conn)
    for n, _, _ in frames:
        for ci, c in enumerate(classes):
            want = rec["%s/n%d/c%d/scores" % (name, n, c)]
            assert np.array_equal([t["obj_tpr"][n, ci], t["obj_fpr"][n, ci]], want[2:4], equal_nan=True)
            assert close([t["obj_asd_result_to_reference"][n, ci], t["obj_asd_reference_to_result"][n, ci]], want[[5, 4]])
    if len(frames) == 1 and len(classes) == 1:          # the functions with the reference's names: one binary pair of the frame's own rank
        a, b = frames[0][1] == classes[0], frames[0][2] == classes[0]
        want = rec["%s/n0/c%d/scores" % (name, classes[0])]
        if name == "empty":
            with pytest.raises(ZeroDivisionError):
                om.obj_tpr(a, b, conn)
            with pytest.raises(ZeroDivisionError):
                om.obj_fpr(b, a, conn)
            assert om.obj_fpr(a, b, conn) == want[1] == 1.0 and np.isnan(om.obj_asd(a, b, sp, conn)) and np.isnan(om.obj_assd(a, b, sp, conn))
        else:
            assert [om.obj_tpr(a, b, conn), om.obj_fpr(a, b, conn), om.obj_tpr(b, a, conn), om.obj_fpr(b, a, conn)] == want[:4].tolist()
            assert close([om.obj_asd(a, b, sp, conn), om.obj_asd(b, a, sp, conn), om.obj_assd(a, b, sp, conn)], want[4:])
            assert close(om.obj_asd(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda() * 3, sp, conn), want[4])          # any non-zero is object


def test_mirror_functions_on_lines_and_defaults():
    from superresolution_aniso_mri_amd.evaluate import object_metrics as om
    a, b = np.array([1, 0, 1, 0, 0]), np.array([1, 0, 1, 0, 1])
    assert om.obj_tpr(a, b) == 1.0 and om.obj_tpr(b, a) == 2 / 3.0 and om.obj_fpr(a, b) == 1 / 3.0 and om.obj_fpr(b, a) == 0.0
    assert om.obj_asd(a, b) == 0.0 and om.obj_asd(a, b, voxelspacing=2.5) == 0.0
    with pytest.raises(ValueError):
        om.obj_asd(np.ones((3, 3)), np.ones((3, 3)), voxelspacing=(1, 2, 3))
    with pytest.raises(ValueError, match="Z == 1"):
        om.object_scores(np.ones((2, 3, 4), dtype=np.float32), np.ones((2, 3, 4), dtype=np.float32), (1, 1, 1), classes=[1], ndim=2)


def test_volume_correlations_equal_the_reference():
    from superresolution_aniso_mri_amd.evaluate import object_metrics as om
    rec = tm.fixture()
    for name in [str(s) for s in rec["sequences"]]:
        res, ref = rec[name + "/results"], rec[name + "/references"]
        assert np.array_equal(np.asarray(om.volume_correlation(res, ref)), rec[name + "/vc"]), name
        assert np.array_equal(np.asarray(om.volume_change_correlation(list(res), list(ref))), rec[name + "/vcc"]), name


# ---- reproducibility -----------------------------------------------------------------------------------------------------------------
def _everything(name, nd, k):
    from superresolution_aniso_mri_amd import ops
    vol, classes = case(name)
    va, vb = torch.from_numpy(vol).cuda(), torch.from_numpy(np.roll(vol, (1, 2), axis=(2, 3))).cuda()
    la, na, ws = ops.components_label(va, classes, ndim=nd, connectivity=k)
    lb, nb, _ = ops.components_label(vb, classes, ndim=nd, connectivity=k)
    table, host = ops.components_tables(va, la, na, classes, ndim=nd, workspace=ws)
    runs = ops.components_overlaps(va, la, vb, lb, classes, ndim=nd, workspace=ws)
    out = ops.components_apply_table(va, la, na, torch.arange(1, int(host.sum()) + 1, device="cuda", dtype=torch.float32), classes, ndim=nd,
                                     workspace=ws, n_components_host=host)
    return [mg.bits(t) for t in (la, na, lb, nb, table, runs, out)]


@pytest.mark.parametrize("name,nd,k", [("multiwg", 3, 1), ("multiwg", 2, 2), ("checker", 3, 3), ("serpentine", 2, 1)])
def test_two_runs_give_the_same_bits(name, nd, k):
    first, second = _everything(name, nd, k), _everything(name, nd, k)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
def _guarded_sequence(name, nd, k, fill, vol_shift, out_shift):
    """All five guarded entry points with every buffer at exactly its contractual size between guard bands, the workspace and every output
    poisoned.  Returns (labels, n, table, runs, out) as numpy."""
    from superresolution_aniso_mri_amd import _hip
    lib, ptr = _hip.lib, _hip.ptr
    vol, classes = case(name)
    other = np.roll(vol, (1, 2), axis=(2, 3))
    N, Z, H, W = vol.shape
    C, T = len(classes), vol.size
    U = N * Z if nd == 2 else N
    dev = torch.device("cuda")
    G = lambda n, dt, f, s, nm: mg.guarded(n, dt, dev, f, s, nm)          # noqa: E731
    va, vb = G(T, torch.float32, torch.from_numpy(vol), vol_shift, "vol_a"), G(T, torch.float32, torch.from_numpy(other), vol_shift, "vol_b")
    la, lb = G(T, torch.int32, fill, out_shift, "labels_a"), G(T, torch.int32, fill, out_shift, "labels_b")
    na, nb = G(U * C, torch.int32, fill, out_shift, "n_a"), G(U * C, torch.int32, fill, out_shift, "n_b")
    ws = G(lib.aesr_components_workspace_bytes(N, Z, H, W, C), torch.uint8, fill, 0, "workspace")
    saved = [mg.bits(va.view), mg.bits(vb.view)]
    cls, st, dims = _hip.int_array(classes), _hip.stream(), (N, Z, H, W)
    # refusals write nothing
    assert lib.aesr_components_label(ptr(va.view), ptr(la.view), ptr(na.view), ptr(ws.view), *dims, cls, C, nd, 0, st) == 1
    assert C > 1 and lib.aesr_components_label(ptr(va.view), ptr(la.view), ptr(na.view), ptr(ws.view), *dims, _hip.int_array([classes[0]] * C), C,
                                               nd, k, st) == 1
    torch.cuda.synchronize()
    assert mg.poison_left(la.view, fill).numel() == T and mg.poison_left(ws.view, fill).numel() == ws.view.numel()
    assert mg.poison_left(na.view, fill).numel() == U * C
    for v, l, n in ((va, la, na), (vb, lb, nb)):
        _hip.check(lib.aesr_components_label(ptr(v.view), ptr(l.view), ptr(n.view), ptr(ws.view), *dims, cls, C, nd, k, st), "aesr_components_label")
    torch.cuda.synchronize()
    mg.assert_guards_intact([va, vb, la, lb, na, nb, ws])
    host = na.view.cpu().numpy().copy()
    rows = int(host.sum())
    assert rows > 0
    hp = host.ctypes.data_as(_hip.IP)
    table = G(rows * 8, torch.int64, fill, out_shift, "table")
    saved_l = [mg.bits(la.view), mg.bits(na.view)]
    assert lib.aesr_components_tables(ptr(va.view), ptr(la.view), ptr(na.view), hp, ptr(ws.view), ptr(table.view), rows - 1, *dims, cls, C, nd, st) == 1
    torch.cuda.synchronize()
    assert mg.poison_left(table.view, fill).numel() == rows * 8
    _hip.check(lib.aesr_components_tables(ptr(va.view), ptr(la.view), ptr(na.view), hp, ptr(ws.view), ptr(table.view), rows, *dims, cls, C, nd, st),
               "aesr_components_tables")
    count = G(1, torch.int64, fill, out_shift, "count")
    _hip.check(lib.aesr_components_overlap_count(ptr(va.view), ptr(la.view), ptr(vb.view), ptr(lb.view), ptr(ws.view), ptr(count.view), *dims, cls, C,
                                                 nd, st), "aesr_components_overlap_count")
    K = int(count.view.item())
    assert 0 < K <= T
    runs = G(K * 4, torch.int32, fill, out_shift, "runs")
    assert lib.aesr_components_overlap_runs(ptr(va.view), ptr(la.view), ptr(vb.view), ptr(lb.view), ptr(ws.view), K, ptr(runs.view), K - 1, *dims, cls,
                                            C, nd, st) == 1
    torch.cuda.synchronize()
    assert mg.poison_left(runs.view, fill).numel() == K * 4
    _hip.check(lib.aesr_components_overlap_runs(ptr(va.view), ptr(la.view), ptr(vb.view), ptr(lb.view), ptr(ws.view), K, ptr(runs.view), K, *dims, cls,
                                                C, nd, st), "aesr_components_overlap_runs")
    ftab = G(rows, torch.float32, torch.arange(1, rows + 1, dtype=torch.float32), out_shift, "fp32 table")
    out = G(T, torch.float32, fill, out_shift, "out")
    _hip.check(lib.aesr_components_apply_table(ptr(va.view), ptr(la.view), ptr(na.view), hp, ptr(ws.view), ptr(ftab.view), rows, ptr(out.view), *dims,
                                               cls, C, nd, st), "aesr_components_apply_table")
    torch.cuda.synchronize()
    mg.assert_guards_intact([va, vb, la, lb, na, nb, ws, table, count, runs, ftab, out])
    mg.assert_unchanged(va.view, saved[0], "vol_a")
    mg.assert_unchanged(vb.view, saved[1], "vol_b")
    mg.assert_unchanged(la.view, saved_l[0], "labels_a")
    mg.assert_unchanged(na.view, saved_l[1], "n_a")
    for g in (la, lb, na, nb, table, count, runs, out):          # every output is written in full, and no poison came through the workspace
        assert mg.poison_left(g.view, fill).numel() == 0, g.name
    return (la.view.cpu().numpy().reshape(vol.shape), host.reshape(U, C), table.view.cpu().numpy().reshape(rows, 8),
            runs.view.cpu().numpy().reshape(K, 4), out.view.cpu().numpy().reshape(vol.shape))


@pytest.mark.parametrize("name,nd,k", [("ties", 3, 3), ("ties", 2, 2), ("multiwg", 3, 1), ("multiwg", 2, 1)])
def test_guard_bands_poisons_and_shifted_pointers(name, nd, k):
    vol, classes = case(name)
    labels, n, table = device_labelling(name, nd, k)
    other = np.roll(vol, (1, 2), axis=(2, 3))
    want_b, _, _ = tm.label_np(other, classes, nd, k)
    want_runs = tm.overlap_runs_np(vol, labels, other, want_b, classes, nd)
    offs = (np.cumsum(n.reshape(-1)) - n.reshape(-1)).astype(np.int64)
    Vu = vol[0, 0].size if nd == 2 else vol[0].size
    unit = (np.arange(vol.size) // Vu).reshape(vol.shape)
    kidx = tm.class_index_np(vol, classes)
    want_out = np.where(labels > 0, offs[(unit * len(classes) + np.maximum(kidx, 0)).reshape(-1)].reshape(vol.shape) + labels, 0).astype(np.float32)
    for fill in (mg.POISON_NAN, mg.POISON_FINITE):
        for vol_shift, out_shift in ((0, 0), (1, 1), (2, 0), (3, 1)):          # volumes by 4 / 8 / 12 bytes: both load paths of the tile kernel
            got = _guarded_sequence(name, nd, k, fill, vol_shift, out_shift)
            for g, w, what in zip(got, (labels, n, table, want_runs, want_out), ("labels", "n_components", "table", "runs", "out")):
                assert np.array_equal(g, w), (what, fill, vol_shift, out_shift)


# ---- the command lines ---------------------------------------------------------------------------------------------------------------
def test_score_labels_objects_and_largest_component_end_to_end(tmp_path, capsys):
    from superresolution_aniso_mri_amd.evaluate import components, object_metrics, score_labels, seg_metrics
    rec = tm.fixture()
    (tmp_path / "pred").mkdir()
    (tmp_path / "ref").mkdir()
    pred, ref = rec["classes3/result"], rec["classes3/reference"]
    np.save(str(tmp_path / "pred" / "a.npy"), pred)
    np.save(str(tmp_path / "ref" / "a.npy"), ref)
    base = ["--pred", str(tmp_path / "pred"), "--ref", str(tmp_path / "ref"), "--spacing", "2.5", "1.25", "1.25", "--classes", "1", "2", "3"]
    plain = score_labels.main(base + ["--out", str(tmp_path / "plain.npz")])
    text = capsys.readouterr().out
    assert "obj_tpr" not in text and not any(k.startswith(("obj_", "n_objects", "n_matched")) for k in plain)
    assert sorted(np.load(str(tmp_path / "plain.npz")).files) == sorted(seg_metrics.SCORE_KEYS + ("counts", "volume_ml_result",
                                                                                                  "volume_ml_reference", "classes", "names"))
    full = score_labels.main(base + ["--objects", "--largest_component", "--out", str(tmp_path / "full.npz")])
    text = capsys.readouterr().out
    assert "obj_tpr" in text and "obj_assd" in text
    cleaned = components.keep_largest_component(pred[None], classes=[1, 2, 3])
    assert np.array_equal(cleaned, tm.keep_np(pred[None], [1, 2, 3], 3, 1, True))
    want = seg_metrics.segmentation_scores(cleaned, ref[None], (2.5, 1.25, 1.25), classes=[1, 2, 3])
    obj = object_metrics.object_scores(cleaned, ref[None], (2.5, 1.25, 1.25), classes=[1, 2, 3])
    saved = np.load(str(tmp_path / "full.npz"))
    for k in seg_metrics.SCORE_KEYS:
        assert np.array_equal(full[k], want[k], equal_nan=True) and np.array_equal(saved[k], want[k], equal_nan=True), k
    for k in object_metrics.OBJECT_KEYS:
        assert np.array_equal(full[k], obj[k], equal_nan=True) and np.array_equal(saved[k], obj[k], equal_nan=True), k
    assert (full["n_objects_result"] <= 1).all() and (plain["counts"][..., 0] >= full["counts"][..., 0]).all()


def test_generate_hr_volumes_cleans_the_label_volume(tmp_path):
    from superresolution_aniso_mri_amd import generate_hr_volumes, train_aesr
    from superresolution_aniso_mri_amd.data_synth import synthetic_labelled_batch
    out = str(tmp_path / "expers")
    train_aesr.main(["--dataset=ACDCLBL", "--model=ae_combined", "--batch_size=4", "--test_batch_size=4", "--latent=16", "--latent_width=8",
                     "--width=32", "--depth=8", "--downsample_steps=2", "--epochs=2", "--lr=0.001", "--ex_loss_weight1=0.05", "--exper_id=m1",
                     "--output_dir=" + out, "--synthetic", "--iters_per_epoch=3", "--image_mix_loss_func=mse", "--epoch_threshold=0"])
    src = os.path.join(out, "m1")
    b = synthetic_labelled_batch(5, 32, 32, seed=3)["slice_between"]
    data, labs = tmp_path / "vols", tmp_path / "labels"
    data.mkdir()
    labs.mkdir()
    np.save(str(data / "vol0.npy"), b[:, 0].numpy())
    np.save(str(labs / "vol0.npy"), b[:, 1].numpy().astype(np.uint8))
    base = ["--exper_dir=" + src, "--model_nbr=2", "--num_interpolations=3", "--data_input_dir=" + str(data), "--labels_input_dir=" + str(labs), "--save"]
    read = lambda d, f: open(str(tmp_path / d / f), "rb").read()          # noqa: E731
    generate_hr_volumes.main(base + ["--output_dir=" + str(tmp_path / "hr")])
    generate_hr_volumes.main(base + ["--output_dir=" + str(tmp_path / "hr0"), "--min_component_size=0"])
    for f in ("vol0.npy", "vol0_labels.npy"):          # the defaults leave every output byte for byte
        assert read("hr", f) == read("hr0", f)
    generate_hr_volumes.main(base + ["--output_dir=" + str(tmp_path / "hr1"), "--largest_component"])
    generate_hr_volumes.main(base + ["--output_dir=" + str(tmp_path / "hr2"), "--min_component_size=6"])
    raw = np.load(str(tmp_path / "hr" / "vol0_labels.npy"))
    classes = list(range(1, int(raw.max()) + 1))
    assert read("hr", "vol0.npy") == read("hr1", "vol0.npy") == read("hr2", "vol0.npy") and classes
    for d, largest, size in (("hr1", True, 0), ("hr2", False, 6)):
        got = np.load(str(tmp_path / d / "vol0_labels.npy"))
        assert got.dtype == np.uint8 and np.array_equal(got, tm.keep_np(raw[None].astype(np.float32), classes, 3, 1, largest, size)[0].astype(np.uint8)), d
    with pytest.raises(SystemExit):
        generate_hr_volumes.main(["--exper_dir=" + src, "--data_input_dir=" + str(data), "--largest_component", "--output_dir=" + str(tmp_path / "x")])
