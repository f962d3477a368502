"""No GPU: the segmentation scores (Dice and its relatives, HD, HD95, ASD / ASSD) against fixtures of the reference's own
kwatsch/medpy_metrics.py (tests/make_golden_seg_metrics.py -> tests/golden/seg_metrics.npz).

- ``surface_distances_np`` below -- borders by the neighbourhood rule, then brute force over all pairs of border voxels in float64 with the
  association sqrt(min (dz sz)^2 + ((dy sy)^2 + (dx sx)^2)), the reference every device test of csrc/seg_metrics.hip compares against --
  reproduces the fixture's ``__surface_distances`` lists (same length, same order) and scores within 1e-12 relative;
- every refusal of the two launch entry points comes back on the host; the workspace query's values;
- the mirror module's import paths, what it does not provide, the no-CPU-fallback error, the command line's refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "seg_metrics.npz")
REL = 1e-12
_CACHE = {}


def fixture():
    if "rec" not in _CACHE:
        _CACHE["rec"] = dict(np.load(GOLDEN))
    return _CACHE["rec"]


def case_names():
    return [str(c) for c in fixture()["cases"]]


def case_frames(name):
    """(result [N, Z, H, W], reference [N, Z, H, W], spacing (sz, sy, sx), classes, empty classes, rank of a frame in the fixture)"""
    rec = fixture()
    r, g, sp = rec[name + "/result"], rec[name + "/reference"], [float(s) for s in rec[name + "/spacing"]]
    rank = len(sp)
    if r.ndim == rank:
        r, g = r[None], g[None]
    if rank == 2:
        r, g, sp = r[:, None], g[:, None], [1.0] + sp
    return r, g, sp, [int(c) for c in rec[name + "/classes"]], [int(c) for c in rec[name + "/empty"]], rank


def recorded(name, n, c):
    """[(ndim, connectivity, key prefix)] of the list records the fixture holds for frame n, class c of a case"""
    rec, out = fixture(), []
    for nd in (2, 3):
        for k in (1, 2, 3):
            key = "%s/n%d/c%d/d%d/k%d" % (name, n, c, nd, k)
            if key + "/scores" in rec:
                out.append((nd, k, key))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def border_np(M, ndim, connectivity):
    """M bool [Z, H, W] -> its border voxels: in M with a neighbour (offsets o != 0 in {-1, 0, 1}^ndim, |o|_1 <= connectivity) not in M;
    outside the array is not in M.  ndim = 2 has no z neighbours."""
    Z, H, W = M.shape
    P = np.zeros((Z + 2, H + 2, W + 2), dtype=bool)
    P[1:-1, 1:-1, 1:-1] = M
    inside = np.ones_like(M)
    for dz in ((-1, 0, 1) if ndim == 3 else (0,)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                l1 = abs(dz) + abs(dy) + abs(dx)
                if l1 == 0 or l1 > connectivity:
                    continue
                inside &= P[1 + dz:1 + dz + Z, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return M & ~inside


def surface_distances_np(A, B, spacing, ndim=3, connectivity=1):
    """For every border voxel of A in raster order the distance to the nearest border voxel of B; with ndim = 2 only within the slice
    (+inf where the slice has none).  Brute force over the pairs of border voxels, one pair of slices at a time, nearest slices first:
    a slice is left out only when its (dz sz)^2 alone exceeds every minimum found so far, which changes no bit because rounding and +
    are monotone (dz^2 + v >= dz^2); for the same reason min_q (dz^2 + v_q) is taken as dz^2 + min_q v_q."""
    sz, sy, sx = (np.float64(s) for s in spacing)
    p = np.argwhere(border_np(A, ndim, connectivity))
    q = np.argwhere(border_np(B, ndim, connectivity))
    out = np.full(len(p), np.inf)
    by_slice = {int(z): q[q[:, 0] == z].astype(np.float64) for z in np.unique(q[:, 0])}
    for z in np.unique(p[:, 0]):
        sel = np.nonzero(p[:, 0] == z)[0]
        py, px = p[sel, 1].astype(np.float64)[:, None], p[sel, 2].astype(np.float64)[:, None]
        m = np.full(len(sel), np.inf)
        for zz in ([int(z)] if ndim == 2 else sorted(by_slice, key=lambda t: abs(t - int(z)))):
            if zz not in by_slice:
                continue
            dz = np.float64(int(z) - zz) * sz
            if dz * dz > m.max():
                break
            qs = by_slice[zz]
            dy, dx = (py - qs[None, :, 1]) * sy, (px - qs[None, :, 2]) * sx
            inplane = (dy * dy + dx * dx).min(axis=1)
            m = np.minimum(m, dz * dz + inplane if ndim == 3 else inplane)
        out[sel] = np.sqrt(m)
    return out


def counts_np(A, B):
    """the seven counts of include/aesr_hip_surface.h without the two border counts: |A|, |B|, |A n B|, |A u B|, voxels"""
    return [int(A.sum()), int(B.sum()), int((A & B).sum()), int((A | B).sum()), int(A.size)]


def scores_np(rg, gr):
    """(hd, hd95, asd_rg, asd_gr, assd) from the two lists"""
    return np.array([max(rg.max(), gr.max()), np.percentile(np.hstack((rg, gr)), 95), rg.mean(), gr.mean(), (rg.mean() + gr.mean()) / 2])


def overlap_np(A, B):
    """(dc, jc, precision, recall, specificity, ravd) with the reference's rules; NaN where the reference raises"""
    a, b, i, u, t = counts_np(A, B)
    nan = float("nan")
    return np.array([2.0 * i / (a + b) if a + b else 0.0, i / u if u else nan, i / a if a else 0.0, i / b if b else 0.0,
                     (t - u) / (t - b) if t - b else 0.0, (a - b) / b if b else nan])


def close(got, want, rel=REL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    same_nan = np.isnan(got) == np.isnan(want)
    fin = ~np.isnan(want)
    return bool(same_nan.all() and (np.abs(got[fin] - want[fin]) <= rel * np.abs(want[fin])).all())


def restated_lists(name):
    """{key prefix: (rg, gr)} of the restatement for every record of a case, computed once"""
    if ("lists", name) not in _CACHE:
        r, g, sp, classes, empty, _ = case_frames(name)
        out = {}
        for n in range(r.shape[0]):
            for c in classes:
                for nd, k, key in recorded(name, n, c):
                    A, B = r[n] == c, g[n] == c
                    out[key] = (surface_distances_np(A, B, sp, nd, k), surface_distances_np(B, A, sp, nd, k))
        _CACHE[("lists", name)] = out
    return _CACHE[("lists", name)]


@pytest.mark.parametrize("name", ["aniso", "ties", "multiwg", "img2d", "z1", "frames", "eight", "extreme", "faces", "oneside"])
def test_restatement_reproduces_the_reference_lists_and_scores(name):
    rec = fixture()
    assert name in case_names()
    lists = restated_lists(name)
    assert lists, name
    worst = 0.0
    for key, (rg, gr) in lists.items():
        for got, want in ((rg, rec[key + "/sds_rg"]), (gr, rec[key + "/sds_gr"])):
            assert got.shape == want.shape, key          # same length; the comparison below is element by element: same order
            assert close(got, want), key
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
        assert close(scores_np(rg, gr), rec[key + "/scores"]), key
    print("%s: %d records, worst relative difference of a distance %.3g" % (name, len(lists), worst))
    r, g, _, classes, empty, _ = case_frames(name)
    for n in range(r.shape[0]):
        for c in classes:
            assert close(overlap_np(r[n] == c, g[n] == c), rec["%s/n%d/c%d/overlap" % (name, n, c)]), (name, n, c)
            if c in empty:
                assert not recorded(name, n, c) and (r[n] == c).any() != (g[n] == c).any()
            else:
                assert (r[n] == c).any() and (g[n] == c).any()


def test_fixture_covers_the_cases_the_kernels_need():
    rec = fixture()
    assert set(case_names()) == {"aniso", "ties", "multiwg", "img2d", "z1", "frames", "eight", "extreme", "faces", "oneside"}
    assert rec["aniso/result"].shape == (6, 20, 18) and list(rec["aniso/spacing"]) == [10.0, 1.4, 1.4]
    assert rec["ties/result"].shape == (5, 7, 67) and rec["multiwg/result"].shape == (12, 64, 80)
    assert rec["img2d/result"].shape == (9, 13) and rec["z1/result"].shape == (1, 9, 13) and rec["frames/result"].shape == (3, 6, 20, 18)
    assert np.array_equal(rec["img2d/result"], rec["z1/result"][0]) and len(rec["eight/classes"]) == 8
    assert rec["extreme/result"].all() and rec["extreme/reference"].sum() == 1 and list(rec["oneside/empty"]) == [2]
    f = rec["faces/result"] == 1
    assert f[0].any() and f[-1].any() and f[:, 0].any() and f[:, -1].any() and f[:, :, 0].any() and f[:, :, -1].any()
    # 3-D mode of a Z = 1 volume: every object voxel is border; slice-wise records of real volumes exist
    assert len(rec["z1/n0/c1/d3/k1/sds_rg"]) == int((rec["z1/result"] == 1).sum())
    assert sum(1 for k in rec if "/d2/" in k and k.endswith("/scores") and not k.startswith(("img2d", "z1"))) >= 4
    assert os.path.getsize(GOLDEN) < 512 * 1024


# ---- the eighth header -------------------------------------------------------------------------------------------------------------
def workspace_bytes_restated(N, Z, H, W, C):
    up = lambda v: (v + 15) // 16 * 16          # noqa: E731
    V = Z * H * W
    Vp, nb, lists = (V + 3) // 4 * 4, (V + 1023) // 1024, N * C * 2
    return up(lists * V * 8) + up(lists * 16) + up(lists * V * 4) + up(N * nb * C * 5 * 4) + up(lists * nb * 4) + up(N * 2 * Vp)


def test_workspace_query():
    from superresolution_aniso_mri_amd import _hip
    ws = _hip.lib.aesr_surface_workspace_bytes
    for shape in ((1, 6, 20, 18, 3), (3, 5, 7, 67, 8), (2, 12, 64, 80, 1)):
        assert ws(*shape) == workspace_bytes_restated(*shape) and ws(*shape) % 16 == 0, shape
    assert ws(1, 6, 20, 18, 3) == 160208
    for bad in ((0, 4, 4, 4, 1), (1, 0, 4, 4, 1), (1, 4, -1, 4, 1), (1, 4, 4, 0, 1), (1, 4, 4, 4, 0), (1, 4, 4, 4, 9),
                (2, 1024, 1024, 1024, 1), (1, 2, 2, 4097, 1), (1 << 28, 1, 1, 1, 4)):
        assert ws(*bad) == 0, bad


def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the device pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    P = ctypes.c_void_p
    lib, err = _hip.lib, _hip.last_error
    res, ref, ws, cnt, dist, stats = (P((i + 1) << 28) for i in range(6))
    N, Z, H, W, C = 2, 3, 4, 5, 2
    classes = _hip.int_array([1, 2])
    bnames = ["result", "reference", "workspace", "counts", "N", "Z", "H", "W", "classes", "C", "ndim", "connectivity", "stream"]
    bok = [res, ref, ws, cnt, N, Z, H, W, classes, C, 3, 1, None]
    host = np.zeros((N, C, 7), dtype=np.int64)
    host[..., :4] = [[10, 12, 5, 17]]
    host[..., 4] = Z * H * W
    host[..., 5:] = [[8, 9]]
    need = int(host[..., 5:].sum())
    dnames = ["workspace", "counts", "counts_host", "distances", "capacity", "stats", "N", "Z", "H", "W", "C", "ndim", "spacing", "stream"]
    dok = [ws, cnt, host.ctypes.data_as(_hip.LLP), dist, need, stats, N, Z, H, W, C, 3, _hip.double_array([10.0, 1.4, 1.4]), None]

    def call(fn, names, ok, **over):
        args = list(ok)
        for k, v in over.items():
            args[names.index(k)] = v
        return fn(*args)

    B, D = lib.aesr_surface_borders, lib.aesr_surface_distances
    for fn, names, ok, tag in ((B, bnames, bok, "aesr_surface_borders"), (D, dnames, dok, "aesr_surface_distances")):
        for bad in (dict(N=0), dict(Z=-1), dict(H=0), dict(W=0), dict(C=0), dict(C=9), dict(ndim=1), dict(ndim=4),
                    dict(N=1 << 11, Z=1 << 10, H=1 << 10), dict(workspace=None), dict(counts=None), dict(workspace=P((1 << 20) + 8)),
                    dict(counts=P((1 << 21) + 4))):
            assert call(fn, names, ok, **bad) == 1, (tag, bad)
            assert tag in err()
        assert call(fn, names, ok, W=4097) == 3 and "4096" in err()
    for bad in (dict(result=None), dict(reference=None), dict(classes=None), dict(result=P((1 << 20) + 2)), dict(reference=P((1 << 20) + 1)),
                dict(connectivity=0), dict(connectivity=4), dict(ndim=2, connectivity=3), dict(classes=_hip.int_array([2, 2])),
                dict(classes=_hip.int_array([1, 1 << 25]))):
        assert call(B, bnames, bok, **bad) == 1, bad
    assert call(B, bnames, bok, classes=_hip.int_array([2, 2])) == 1 and "twice" in err()
    assert call(B, bnames, bok, connectivity=3, ndim=2) == 1 and "connectivity=3" in err()
    for sp in ([0.0, 1, 1], [1, -1.0, 1], [1, 1, float("inf")], [float("nan"), 1, 1]):
        assert call(D, dnames, dok, spacing=_hip.double_array(sp)) == 1 and "spacing" in err(), sp
    for bad in (dict(counts_host=None), dict(stats=None), dict(spacing=None), dict(distances=None), dict(distances=P((1 << 22) + 4)),
                dict(stats=P((1 << 22) + 4)), dict(capacity=need - 1), dict(capacity=0)):
        assert call(D, dnames, dok, **bad) == 1, bad
    assert call(D, dnames, dok, capacity=need - 1) == 1 and "distances" in err()
    # host counts that the borders call cannot have written
    for idx, val in (((0, 0, 4), 7), ((1, 1, 5), 11), ((0, 1, 0), -1)):
        broken = host.copy()
        broken[idx] = val
        assert call(D, dnames, dok, counts_host=broken.ctypes.data_as(_hip.LLP)) == 1 and "counts_host" in err()
    # a class that is empty on one side has no lists: fewer distances are needed
    onesided = host.copy()
    onesided[0, 0, 0] = onesided[0, 0, 5] = 0
    assert call(D, dnames, dok, counts_host=onesided.ctypes.data_as(_hip.LLP), capacity=need - 17 - 1) == 1
    # outputs that overlap inputs or each other are refused as unsupported
    assert call(B, bnames, bok, counts=res) == 3 and "overlaps" in err()
    assert call(B, bnames, bok, workspace=ref) == 3 and "overlaps" in err()
    assert call(B, bnames, bok, counts=ws) == 3
    assert call(D, dnames, dok, distances=ws) == 3 and "overlaps" in err()
    assert call(D, dnames, dok, stats=cnt) == 3 and call(D, dnames, dok, stats=dist) == 3 and call(D, dnames, dok, distances=cnt) == 3


# ---- host layer --------------------------------------------------------------------------------------------------------------------
def test_mirror_module_imports_through_both_paths():
    import kwatsch.medpy_metrics as shim
    import superresolution_aniso_mri_amd.kwatsch.medpy_metrics as impl
    for name in ("dc", "jc", "precision", "recall", "sensitivity", "specificity", "true_positive_rate", "true_negative_rate",
                 "positive_predictive_value", "hd", "hd95", "asd", "assd", "ravd"):
        assert getattr(shim, name) is getattr(impl, name), name
    import inspect
    for name in ("hd", "hd95", "asd", "assd"):
        assert str(inspect.signature(getattr(impl, name))) == "(result, reference, voxelspacing=None, connectivity=1)"
    assert impl.EMPTY_FIRST.startswith("The first supplied array") and impl.EMPTY_SECOND.startswith("The second supplied array")


def test_object_scores_are_not_provided():
    import kwatsch.medpy_metrics as m
    a = np.ones((3, 3))
    for name in ("obj_assd", "obj_asd", "obj_fpr", "obj_tpr"):
        with pytest.raises(NotImplementedError, match="connected components"):
            getattr(m, name)(a, a)
    for name in ("volume_correlation", "volume_change_correlation"):
        with pytest.raises(NotImplementedError):
            getattr(m, name)([a], [a])


def test_host_input_without_a_gpu_raises(monkeypatch):
    import kwatsch.medpy_metrics as m
    from superresolution_aniso_mri_amd import ops
    from superresolution_aniso_mri_amd.evaluate import seg_metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = np.ones((2, 3, 4), dtype=np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_metrics.segmentation_scores(a, a, (1, 1, 1), classes=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_metrics.surface_distance_lists(torch.from_numpy(a), torch.from_numpy(a), (1, 1, 1), classes=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.dc(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.hd(a[0], a[0], voxelspacing=2.0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.surface_borders(torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3, 4), [1])


def test_overlap_scores_follow_the_reference_rules():
    from superresolution_aniso_mri_amd.evaluate.seg_metrics import overlap_scores
    rec = fixture()
    for name in ("aniso", "oneside", "extreme"):
        r, g, _, classes, _, _ = case_frames(name)
        for c in classes:
            A, B = r[0] == c, g[0] == c
            s = overlap_scores(np.array(counts_np(A, B) + [0, 0]))
            got = [float(s[k]) for k in ("dice", "jc", "precision", "recall", "specificity", "ravd")]
            assert close(got, rec["%s/n0/c%d/overlap" % (name, c)]), (name, c)
    s = overlap_scores(np.array([0, 0, 0, 0, 24, 0, 0]))
    assert float(s["dice"]) == 0.0 and np.isnan(float(s["jc"])) and np.isnan(float(s["ravd"])) and float(s["specificity"]) == 1.0


def test_command_line_refusals(tmp_path, capsys):
    from superresolution_aniso_mri_amd.evaluate import score_labels
    (tmp_path / "pred").mkdir()
    (tmp_path / "ref").mkdir()
    vol = np.zeros((2, 3, 4), dtype=np.float32)
    vol[1, 1, 1] = 1
    for d, names in (("pred", ("a", "b")), ("ref", ("a", "c"))):
        for n in names:
            np.save(str(tmp_path / d / (n + ".npy")), vol)
    with pytest.raises(SystemExit) as e:
        score_labels.main(["--pred", str(tmp_path / "pred"), "--ref", str(tmp_path / "ref"), "--spacing", "1", "1", "1"])
    assert e.value.code == 2 and "no partner for: b, c" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        score_labels.main(["--pred", str(tmp_path / "pred" / "a.npy"), "--ref", str(tmp_path / "ref" / "a.npy")])
    assert e.value.code == 2 and "--spacing" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        score_labels.main(["--pred", str(tmp_path / "nothing"), "--ref", str(tmp_path / "ref")])
    assert score_labels.match_files(str(tmp_path / "pred" / "b.npy"), str(tmp_path / "ref" / "c.npy"))[0][0] == "c"
