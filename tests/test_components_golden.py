"""No GPU: connected components and the object-wise scores against fixtures of scipy.ndimage and the reference's own
kwatsch/medpy_metrics.py (tests/make_golden_components.py -> tests/golden/components.npz).

- ``label_np`` below -- a plain union-find over the x-runs of equal class, the definition of include/aesr_hip_components.h restated, the
  reference every device test of csrc/components.hip compares against -- reproduces the fixture's labels, counts, boxes and sizes exactly;
- the restated overlap-run rule yields exactly the pair set of a brute-force np.unique over voxel pairs;
- ``evaluate.object_metrics.correspondences`` reproduces every stored mapping and every stored obj_tpr / obj_fpr;
- every refusal of the entry points comes back on the host; the workspace query's values;
- the no-CPU-fallback error; ``kwatsch.medpy_metrics.obj_tpr`` still raises."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "components.npz")
LABEL_CASES = ["ties", "multiwg", "serpentine", "helix", "comb_last", "comb_first", "checker", "diagonal", "eight", "slices6", "img2d", "z1",
               "full", "faces", "tie"]
SCORE_CASES = ["aniso_a", "aniso_b", "aniso_k2", "aniso_k3", "iso", "flat_a", "flat_k2", "classes3", "frames", "apart", "empty"]
_CACHE = {}


def fixture():
    if "rec" not in _CACHE:
        _CACHE["rec"] = dict(np.load(GOLDEN))
    return _CACHE["rec"]


def frames4(vol):
    """[H, W], [Z, H, W] or [N, Z, H, W] -> [N, Z, H, W]"""
    vol = np.asarray(vol)
    return vol.reshape((1,) * (4 - vol.ndim) + vol.shape)


def case_modes(name):
    return [(int(nd), int(k)) for nd, k in fixture()[name + "/modes"]]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def class_index_np(vol, classes):
    """int [..]: the index in ``classes`` of every voxel, -1 where it has no class (NaN, not integral, not listed)"""
    k = np.full(vol.shape, -1, dtype=np.int64)
    for i, c in enumerate(classes):
        k[vol == np.float32(c)] = i
    return k


def label_np(vol, classes, ndim, connectivity):
    """vol [N, Z, H, W] -> (labels int32 [N, Z, H, W], n int32 [U, C], table int64 [R, 8]) by the definition: adjacency = offsets o != 0 in
    {-1, 0, 1}^ndim with |o|_1 <= connectivity; components of equal class within a unit; numbered per (unit, class) in raster order of
    their first voxel.  A union-find over the x-runs of equal class."""
    N, Z, H, W = vol.shape
    C = len(classes)
    k = class_index_np(vol, classes)
    flat = k.reshape(-1)
    x = np.tile(np.arange(W), N * Z * H)
    start = (flat >= 0) & ((x == 0) | (flat != np.roll(flat, 1)))
    run_of = np.cumsum(start) - 1                      # the run of every voxel that has a class
    run_first = np.flatnonzero(start)                  # linear index of every run's first voxel: ascending
    parent = np.arange(len(run_first))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    idx = np.arange(flat.size).reshape(N, Z, H, W)
    for dz in ((-1, 0) if ndim == 3 else (0,)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                l1 = abs(dz) + abs(dy) + abs(dx)
                if l1 == 0 or l1 > connectivity or (dz, dy, dx) > (0, 0, 0) or (dz == 0 and dy == 0):
                    continue                           # backward offsets only; (0, 0, -1) is what the runs already are
                dst = (slice(None), slice(max(-dz, 0), Z - max(dz, 0)), slice(max(-dy, 0), H - max(dy, 0)), slice(max(-dx, 0), W - max(dx, 0)))
                src = (slice(None), slice(max(dz, 0), Z - max(-dz, 0)), slice(max(dy, 0), H - max(-dy, 0)), slice(max(dx, 0), W - max(-dx, 0)))
                same = (k[dst] >= 0) & (k[dst] == k[src])
                pairs = np.unique(np.stack([run_of[idx[dst][same]], run_of[idx[src][same]]], axis=1), axis=0)
                for a, b in pairs:
                    ra, rb = find(a), find(b)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)          # runs are numbered in raster order: the root is the first run
    roots = np.array([find(a) for a in range(len(parent))], dtype=np.int64)
    Vu = H * W if ndim == 2 else Z * H * W
    U = N * Z if ndim == 2 else N
    n = np.zeros((U, C), dtype=np.int32)
    number = np.zeros(len(parent), dtype=np.int64)
    is_root = np.flatnonzero(roots == np.arange(len(parent)))
    for r in is_root:                                  # ascending first voxel: raster order within every (unit, class)
        u, c = run_first[r] // Vu, flat[run_first[r]]
        n[u, c] += 1
        number[r] = n[u, c]
    labels = np.zeros(flat.size, dtype=np.int32)
    has = flat >= 0
    labels[has] = number[roots[run_of[has]]]
    labels = labels.reshape(N, Z, H, W)
    rows = {}
    for r in is_root:
        u, c = run_first[r] // Vu, flat[run_first[r]]
        rows[(u, c, number[r])] = r
    comp_of = roots[run_of[has]]
    where = np.flatnonzero(has)
    table = []
    for key in sorted(rows):
        p = where[comp_of == rows[key]]
        z, y, xx = (p // (H * W)) % Z, (p // W) % H, p % W
        table.append([len(p), z.min(), z.max() + 1, y.min(), y.max() + 1, xx.min(), xx.max() + 1, p.min() % (Z * H * W)])
    return labels, n, np.asarray(table, dtype=np.int64).reshape(-1, 8)


def restated(name, ndim, connectivity):
    key = ("label", name, ndim, connectivity)
    if key not in _CACHE:
        rec = fixture()
        _CACHE[key] = label_np(frames4(rec[name + "/vol"]), [int(c) for c in rec[name + "/classes"]], ndim, connectivity)
    return _CACHE[key]


def overlap_runs_np(vol_a, lab_a, vol_b, lab_b, classes, ndim):
    """The rule of include/aesr_hip_components.h: (unit, class index, label A, label B) at every voxel with the same class in A and B whose
    x-predecessor in the row does not carry the same tuple, in raster order.  int32 [K, 4]."""
    N, Z, H, W = vol_a.shape
    ka, kb = class_index_np(vol_a, classes), class_index_np(vol_b, classes)
    Vu = H * W if ndim == 2 else Z * H * W
    unit = (np.arange(vol_a.size) // Vu).reshape(vol_a.shape)
    valid = (ka >= 0) & (ka == kb) & (lab_a > 0) & (lab_b > 0)
    tup = np.stack([unit, ka, lab_a, lab_b], axis=-1)
    same_as_left = np.zeros(vol_a.shape, dtype=bool)
    same_as_left[..., 1:] = valid[..., 1:] & valid[..., :-1] & (tup[..., 1:, :] == tup[..., :-1, :]).all(axis=-1)
    emit = valid & ~same_as_left
    return tup[emit].astype(np.int32).reshape(-1, 4)


def keep_np(vol, classes, ndim, connectivity, largest, min_size=0):
    """The clean-up of evaluate/components.py restated on label_np: [N, Z, H, W] float in, the same out."""
    labels, n, table = label_np(vol, classes, ndim, connectivity)
    N, Z, H, W = vol.shape
    Vu = H * W if ndim == 2 else Z * H * W
    out = vol.copy().reshape(-1)
    k = class_index_np(vol, classes).reshape(-1)
    unit = np.arange(vol.size) // Vu
    lab = labels.reshape(-1)
    row = 0
    for u in range(n.shape[0]):
        for c in range(n.shape[1]):
            sizes = table[row:row + n[u, c], 0]
            row += n[u, c]
            if not len(sizes):
                continue
            keep = np.zeros(len(sizes) + 1, dtype=bool)
            if largest:
                keep[1 + int(np.argmax(sizes))] = True
            else:
                keep[1:] = sizes >= min_size
            sel = (unit == u) & (k == c)
            out[sel & ~keep[np.where(sel, lab, 0)]] = 0
    return out.reshape(vol.shape)


# ---- labelling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LABEL_CASES)
def test_restatement_reproduces_scipy_labels_counts_and_tables(name):
    rec = fixture()
    assert name in [str(c) for c in rec["label_cases"]]
    for nd, k in case_modes(name):
        labels, n, table = restated(name, nd, k)
        key = "%s/d%d/k%d" % (name, nd, k)
        assert np.array_equal(labels.reshape(rec[key + "/labels"].shape), rec[key + "/labels"]), key
        assert np.array_equal(n, rec[key + "/n"]), key
        assert np.array_equal(table, rec[key + "/table"]), key


def test_fixture_covers_the_cases_the_kernels_need():
    rec = fixture()
    assert [str(c) for c in rec["label_cases"]] == LABEL_CASES and [str(c) for c in rec["score_cases"]] == SCORE_CASES
    assert rec["ties/vol"].shape == (5, 7, 67) and case_modes("ties") == [(3, 1), (3, 2), (3, 3), (2, 1), (2, 2)]
    assert rec["multiwg/vol"].shape == (12, 64, 80) and rec["serpentine/vol"].shape == (33, 33) and rec["helix/vol"].shape[0] == 9
    # the serpentine and the helix are one component each; the combs join only in their last / first row
    assert rec["serpentine/d2/k1/n"].tolist() == [[1]] and rec["helix/d3/k1/n"].tolist() == [[1]]
    assert rec["comb_last/d2/k1/n"].tolist() == [[1]] and rec["comb_first/d2/k1/n"].tolist() == [[1]]
    assert not rec["comb_last/vol"][:-1, 1::2].any() and not rec["comb_first/vol"][1:, 1::2].any()
    # the checkerboard: every voxel its own component at connectivity 1, collapsing at 2 (2-D: per slice) and at 2 / 3 in 3-D
    ones = int((rec["checker/vol"] == 1).sum())
    assert rec["checker/vol"].shape == (9, 17, 70) and int(rec["checker/d3/k1/n"].sum()) == ones == int(rec["checker/d2/k1/n"].sum())
    assert rec["checker/d3/k2/n"].tolist() == [[1]] and rec["checker/d3/k3/n"].tolist() == [[1]] and (rec["checker/d2/k2/n"] == 1).all()
    assert int(rec["diagonal/d2/k1/n"].sum()) == rec["diagonal/vol"].size and (rec["diagonal/d2/k2/n"] == 1).all()
    assert len(rec["eight/classes"]) == 8 and rec["eight/vol"].shape[0] == 3
    # ndim = 2 on a volume: the numbering restarts in every slice
    assert rec["slices6/d2/k1/n"].shape == (6, 3) and (rec["slices6/d2/k1/n"][:, 0] >= 1).all()
    assert all(rec["slices6/d2/k1/labels"][z][rec["slices6/vol"][z] == 1].min() == 1 for z in range(6))
    assert int(rec["slices6/d2/k1/n"].sum()) > int(rec["slices6/d3/k1/n"].sum())
    assert np.array_equal(rec["img2d/vol"], rec["z1/vol"][0]) and np.array_equal(rec["img2d/d2/k1/labels"], rec["z1/d2/k1/labels"][0])
    assert rec["full/d3/k1/n"].tolist() == [[1, 0]] and rec["full/d3/k1/table"][0].tolist() == [120, 0, 4, 0, 5, 0, 6, 0]
    assert rec["faces/d3/k1/table"][0, 1:7].tolist() == [0, 5, 0, 8, 0, 9]
    assert rec["tie/d3/k1/table"][:, 0].tolist() == [8, 8, 3, 5, 5]
    deferred = [n for n in SCORE_CASES if max(int(rec[k]) for k in rec if k.startswith(n + "/") and k.endswith("/deferred")) >= 2]
    assert len(deferred) >= 4
    assert np.isnan(rec["apart/n0/c1/scores"][4:]).all() and rec["apart/n0/c1/scores"][0] == 0.0 and len(rec["apart/n0/c1/map_ref"]) == 0
    assert np.isnan(rec["empty/n0/c1/scores"][0]) and list(rec["aniso_a/spacing"]) == [10.0, 1.4, 1.4]
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("name", ["ties", "slices6", "eight", "diagonal"])
def test_overlap_runs_give_the_pair_set_of_all_voxel_pairs(name):
    rec = fixture()
    vol = frames4(rec[name + "/vol"])
    classes = [int(c) for c in rec[name + "/classes"]]
    other = np.roll(vol, (1, 2), axis=(2, 3))          # the same objects, shifted: partial overlaps
    for nd, k in case_modes(name):
        la, _, _ = restated(name, nd, k)
        lb, _, _ = label_np(other, classes, nd, k)
        runs = overlap_runs_np(vol, la, other, lb, classes, nd)
        ka, kb = class_index_np(vol, classes), class_index_np(other, classes)
        both = (ka >= 0) & (ka == kb)
        Vu = vol[0, 0].size if nd == 2 else vol[0].size
        unit = (np.arange(vol.size) // Vu).reshape(vol.shape)
        brute = np.unique(np.stack([unit[both], ka[both], la[both], lb[both]], axis=1), axis=0)
        assert len(runs) and np.array_equal(np.unique(runs, axis=0), brute), (name, nd, k)
        assert len(runs) <= int(both.sum())


def test_restated_clean_up_on_the_tie_case():
    """keep_np is what the device's clean-up is compared against: the first of two equal components survives, foreign values pass."""
    vol = frames4(fixture()["tie/vol"])
    kept = keep_np(vol, [1, 2], 3, 1, True)[0]
    assert (kept[0:2, 0:2, 0:2] == 1).all() and (kept == 1).sum() == 8 and (kept == 2).sum() == 5 and (kept[2, 0, 0:5] == 2).all()
    assert kept[1, 3, 3] == 7 and kept[1, 3, 4] == 2.5
    small = keep_np(vol, [1, 2], 3, 1, False, 4)[0]
    assert (small == 1).sum() == 16 and (small == 2).sum() == 10 and not small[0, 5, 0:3].any()
    flat = keep_np(vol, [1, 2], 2, 1, True)[0]          # per slice: every slice keeps its own largest component of a class
    assert (flat == 1).sum() == 16 and (flat == 2).sum() == 13


# ---- correspondences -----------------------------------------------------------------------------------------------------------------
def score_frames(name):
    """[(n, result [Z, H, W] or [H, W], reference)], spacing, classes, connectivity, rank of a frame"""
    rec = fixture()
    r, g, sp = rec[name + "/result"], rec[name + "/reference"], [float(s) for s in rec[name + "/spacing"]]
    frames = [(0, r, g)] if r.ndim == len(sp) else [(n, r[n], g[n]) for n in range(r.shape[0])]
    return frames, sp, [int(c) for c in rec[name + "/classes"]], int(rec[name + "/connectivity"]), len(sp)


@pytest.mark.parametrize("name", SCORE_CASES)
def test_correspondences_reproduce_the_reference_mappings(name):
    from superresolution_aniso_mri_amd.evaluate.object_metrics import correspondences
    rec = fixture()
    frames, _, classes, conn, rank = score_frames(name)
    nd = 3 if rank == 3 else 2
    for n, r, g in frames:
        la, na, _ = label_np(frames4(r), classes, nd, conn)
        lb, nb, _ = label_np(frames4(g), classes, nd, conn)
        for ci, c in enumerate(classes):
            key = "%s/n%d/c%d" % (name, n, c)
            both = (frames4(r) == c) & (frames4(g) == c)
            pairs = np.unique(np.stack([la[both], lb[both]], axis=1), axis=0).reshape(-1, 2)
            n_res, n_ref = int(na[0, ci]), int(nb[0, ci])
            assert [n_res, n_ref] == rec[key + "/counts"].tolist(), key
            from_ref = correspondences([(b, a) for a, b in pairs], n_ref)
            from_res = correspondences(pairs, n_res)
            assert sorted(from_ref.items()) == [tuple(p) for p in rec[key + "/map_ref"].tolist()], key
            assert sorted(from_res.items()) == [tuple(p) for p in rec[key + "/map_res"].tolist()], key
            want = rec[key + "/scores"]
            m, nan = len(from_ref), float("nan")
            got = [m / n_res if n_res else nan, (n_ref - m) / n_ref if n_ref else nan]
            m2 = len(from_res)
            got += [m2 / n_ref if n_ref else nan, (n_res - m2) / n_res if n_res else nan]
            assert np.array_equal(np.asarray(got), want[:4], equal_nan=True), (key, got, want[:4])


# ---- the eleventh header ----------------------------------------------------------------------------------------------------------------
def workspace_bytes_restated(N, Z, H, W, C):
    up = lambda v: (v + 15) // 16 * 16          # noqa: E731
    T = N * Z * H * W
    nb2, nbT = (H * W + 255) // 256, (T + 255) // 256
    return up(T * 4) + 2 * up(N * Z * nb2 * C * 4) + up((N * Z * C + 1) * 4) + 2 * up(nbT * 4)


def test_workspace_query():
    from superresolution_aniso_mri_amd import _hip
    ws = _hip.lib.aesr_components_workspace_bytes
    for shape in ((1, 6, 20, 18, 3), (3, 5, 7, 67, 8), (2, 12, 64, 80, 1), (1, 1, 1, 1, 1)):
        assert ws(*shape) == workspace_bytes_restated(*shape) and ws(*shape) % 16 == 0, shape
    for bad in ((0, 4, 4, 4, 1), (1, 0, 4, 4, 1), (1, 4, -1, 4, 1), (1, 4, 4, 0, 1), (1, 4, 4, 4, 0), (1, 4, 4, 4, 9),
                (2, 1024, 1024, 1024, 1), (1 << 15, 1 << 14, 1, 1, 4)):
        assert ws(*bad) == 0, bad
    assert ws(1, 2, 2, 5000, 1) > 0          # no limit on the length of a line


def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the device pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    P = ctypes.c_void_p
    lib, err = _hip.lib, _hip.last_error
    vol, lab, ncd, ws, tab, out, vol2, lab2, cnt, runs, ftab = (P((i + 1) << 28) for i in range(11))
    N, Z, H, W, C = 2, 3, 4, 5, 2
    classes = _hip.int_array([1, 2])
    host = np.array([[3, 0], [2, 4]], dtype=np.int32)          # ndim = 3: U = N
    hp = host.ctypes.data_as(_hip.IP)
    rows = int(host.sum())
    tail = [N, Z, H, W, classes, C, 3]
    tnames = ["N", "Z", "H", "W", "classes", "C", "ndim"]
    table = {
        "aesr_components_label": (["vol", "labels", "n_components", "workspace"] + tnames + ["connectivity", "stream"],
                                  [vol, lab, ncd, ws] + tail + [1, None]),
        "aesr_components_tables": (["vol", "labels", "n_components", "n_components_host", "workspace", "table", "capacity"] + tnames + ["stream"],
                                   [vol, lab, ncd, hp, ws, tab, rows] + tail + [None]),
        "aesr_components_overlap_count": (["vol_a", "labels_a", "vol_b", "labels_b", "workspace", "count"] + tnames + ["stream"],
                                          [vol, lab, vol2, lab2, ws, cnt] + tail + [None]),
        "aesr_components_overlap_runs": (["vol_a", "labels_a", "vol_b", "labels_b", "workspace", "count_host", "runs", "capacity"] + tnames
                                         + ["stream"], [vol, lab, vol2, lab2, ws, 7, runs, 7] + tail + [None]),
        "aesr_components_apply_table": (["vol", "labels", "n_components", "n_components_host", "workspace", "table", "table_len", "out"] + tnames
                                        + ["stream"], [vol, lab, ncd, hp, ws, ftab, rows, out] + tail + [None]),
    }

    def call(tag, **over):
        names, ok = table[tag]
        args = list(ok)
        for k, v in over.items():
            args[names.index(k)] = v
        return getattr(lib, tag)(*args)

    for tag, (names, ok) in table.items():
        for bad in (dict(N=0), dict(Z=-1), dict(H=0), dict(W=0), dict(C=0), dict(C=9), dict(ndim=1), dict(ndim=4),
                    dict(N=1 << 11, Z=1 << 10, H=1 << 10), dict(workspace=None), dict(workspace=P((1 << 20) + 8)), dict(classes=None),
                    dict(classes=_hip.int_array([2, 2])), dict(classes=_hip.int_array([1, 1 << 25]))):
            assert call(tag, **bad) == 1, (tag, bad)
            assert tag in err(), (tag, bad, err())
        for name in names:          # every device pointer: null and misaligned
            if name in ("vol", "labels", "n_components", "vol_a", "labels_a", "vol_b", "labels_b", "out", "count", "n_components_host"):
                assert call(tag, **{name: None}) == 1, (tag, name)
                if name != "n_components_host":
                    assert call(tag, **{name: P((1 << 20) + 2)}) == 1, (tag, name)
        assert call(tag, classes=_hip.int_array([2, 2])) == 1 and "twice" in err()
    L = "aesr_components_label"
    for bad in (dict(connectivity=0), dict(connectivity=4), dict(ndim=2, connectivity=3)):
        assert call(L, **bad) == 1, bad
    assert call(L, ndim=2, connectivity=3) == 1 and "connectivity=3" in err()
    assert call(L, labels=vol) == 3 and "overlaps" in err()
    assert call(L, workspace=vol) == 3 and call(L, n_components=lab) == 3 and call(L, n_components=ws) == 3
    T, A = "aesr_components_tables", "aesr_components_apply_table"
    assert call(T, table=None) == 1 and call(T, table=P((1 << 22) + 4)) == 1 and call(T, capacity=rows - 1) == 1 and "rows" in err()
    assert call(A, table=None) == 1 and call(A, table=P((1 << 22) + 2)) == 1 and call(A, table_len=rows - 1) == 1 and "table" in err()
    for tag in (T, A):
        for idx, val in (((0, 0), -1), ((1, 1), Z * H * W + 1)):          # host counts that the labelling cannot have written
            broken = host.copy()
            broken[idx] = val
            assert call(tag, n_components_host=broken.ctypes.data_as(_hip.IP)) == 1 and "n_components_host" in err(), (tag, idx)
        # more than 2^24 components in one (unit, class): unsupported (needs a unit that large to be consistent at all)
        big = np.array([[(1 << 24) + 1, 0]], dtype=np.int32)
        over = dict(N=1, Z=1 << 6, H=1 << 10, W=1 << 9, n_components_host=big.ctypes.data_as(_hip.IP))
        over.update(dict(capacity=1 << 25) if tag == T else dict(table_len=1 << 25))
        assert call(tag, **over) == 3 and "2^24" in err(), tag
    empty = np.zeros((2, 2), dtype=np.int32)
    assert call(T, table=ws) == 3 and "overlaps" in err() and call(T, workspace=lab) == 3
    assert call(A, out=vol) == 3 and "overlaps" in err() and call(A, out=ftab) == 3 and call(A, out=ws) == 3
    del empty
    OC, OR = "aesr_components_overlap_count", "aesr_components_overlap_runs"
    assert call(OC, count=P((1 << 22) + 4)) == 1 and call(OC, count=ws) == 3 and call(OC, workspace=lab2) == 3 and "overlaps" in err()
    for bad in (dict(count_host=-1), dict(count_host=N * Z * H * W + 1, capacity=1 << 20), dict(capacity=6), dict(runs=None),
                dict(runs=P((1 << 22) + 2))):
        assert call(OR, **bad) == 1, bad
    assert call(OR, capacity=6) == 1 and "runs" in err()
    assert call(OR, runs=vol2) == 3 and "overlaps" in err() and call(OR, runs=ws) == 3


# ---- host layer ----------------------------------------------------------------------------------------------------------------------
def test_host_input_without_a_gpu_raises(monkeypatch):
    from superresolution_aniso_mri_amd import ops
    from superresolution_aniso_mri_amd.evaluate import components, object_metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = np.ones((2, 3, 4), dtype=np.float32)
    for fn in (components.label_components, components.keep_largest_component, lambda v: components.remove_small_components(v, 2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.from_numpy(a))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        object_metrics.object_scores(a, a, (1, 1, 1), classes=[1])
    for fn in (object_metrics.obj_tpr, object_metrics.obj_fpr, object_metrics.obj_asd, object_metrics.obj_assd):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, a)
    for fn in (object_metrics.volume_correlation, object_metrics.volume_change_correlation):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn([a, a, a], [a, a, a])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.components_label(torch.zeros(1, 2, 3, 4), [1])


def test_object_scores_refuse_slice_wise_volumes_and_the_mirror_stub_still_raises(monkeypatch):
    import kwatsch.medpy_metrics as m
    from superresolution_aniso_mri_amd.evaluate import object_metrics
    with pytest.raises(NotImplementedError, match="connected components"):          # the working one is evaluate.object_metrics.obj_tpr
        m.obj_tpr(np.ones((3, 3)), np.ones((3, 3)))
    assert "kwatsch.medpy_metrics" in object_metrics.__doc__ and "smallest id" in object_metrics.__doc__
    monkeypatch.setattr(object_metrics.sm, "_as_batch", lambda r, g: (torch.as_tensor(r), torch.as_tensor(g), True))
    with pytest.raises(ValueError, match="Z == 1"):
        object_metrics.object_scores(np.ones((1, 2, 3, 4), dtype=np.float32), np.ones((1, 2, 3, 4), dtype=np.float32), (1, 1, 1), classes=[1],
                                     ndim=2)
