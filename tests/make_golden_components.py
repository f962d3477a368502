#!/usr/bin/env python
"""Generate tests/golden/components.npz from scipy.ndimage (label, find_objects) and the REFERENCE's own kwatsch/medpy_metrics.py
(imported from the reference checkout as tests/make_golden_seg_metrics.py does; nothing of it is copied).  A script, not a test; the GPU
box does not have the reference.  Only data is written.

Keys.  ``label_cases`` names the labelling cases; per case ``<case>/vol`` (fp32 class ids, [H, W], [Z, H, W] or [N, Z, H, W]),
``<case>/classes``, ``<case>/modes`` ([M, 2]: ndim, connectivity) and per mode ``<case>/d<ndim>/k<connectivity>/labels`` (int32, the
shape of vol: 0 or scipy's label of the voxel within its (unit, class)), ``.../n`` (int32 [U, C]) and ``.../table`` (int64 [R, 8], one
row per component in the order (unit, class, number): voxel count, find_objects' z0, z1, y0, y1, x0, x1 within the frame, linear index
of the first voxel within the frame).  A unit is a frame with ndim = 3 and a slice with ndim = 2.

``score_cases`` names the score cases; per case ``<case>/result``, ``<case>/reference`` ([H, W], [Z, H, W] or [N, Z, H, W]),
``<case>/spacing`` (one entry per axis of a frame), ``<case>/classes``, ``<case>/connectivity`` and per frame n and class c
``<case>/n<n>/c<c>/map_ref`` ([M, 2]: the mapping of __distinct_binary_object_correspondences(reference, result) as sorted (reference id,
result id) rows), ``.../map_res`` (the other call direction: (result id, reference id)), ``.../counts`` (objects of result, of
reference), ``.../deferred`` (the largest set of a deferred component in either direction, 0: none) and ``.../scores`` = obj_tpr(r, g),
obj_fpr(r, g), obj_tpr(g, r), obj_fpr(g, r), obj_asd(r, g), obj_asd(g, r), obj_assd(r, g); NaN where the reference divides by zero or
has nothing to average.  ``sequences``: per name ``<name>/results``, ``<name>/references`` ([F, ...]), ``<name>/vc`` and ``<name>/vcc``
(r, p of volume_correlation and volume_change_correlation).

The reference serves a deferred component with set.pop(), an arbitrary element; evaluate/object_metrics.py takes the smallest id.  Every
stored score case is one where the two rules give the same mapping in both directions: a candidate that does not is replaced by the
next seed."""
import os
import sys
import warnings

import numpy as np
from scipy.ndimage import find_objects, generate_binary_structure, label

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden_seg_metrics as mgs  # noqa: E402

OUT = os.path.join(HERE, "golden", "components.npz")


# ---- labelling cases -----------------------------------------------------------------------------------------------------------------
def noisy_labels(shape, K, rng, p):
    field, _ = mgs.blob(shape, rng)
    vol = np.floor(K * 0.999 * field)
    salt = rng.random(shape) < p
    vol[salt] = rng.integers(0, K, size=int(salt.sum()))
    return vol.astype(np.float32)


def serpentine(n):
    v = np.zeros((n, n), dtype=np.float32)
    v[0::2] = 1
    for i, y in enumerate(range(1, n, 2)):
        v[y, -1 if i % 2 == 0 else 0] = 1
    return v


def helix(slices):
    ring = [(1, x) for x in range(1, 9)] + [(y, 8) for y in range(2, 9)] + [(8, x) for x in range(7, 0, -1)] + [(y, 1) for y in range(7, 1, -1)]
    v = np.zeros((slices, 10, 10), dtype=np.float32)
    for z in range(slices):
        for y, x in ring[3 * z:3 * z + 4]:
            v[z, y, x] = 1
    return v


def comb(H, W):
    v = np.zeros((H, W), dtype=np.float32)
    v[:, 0::2] = 1
    v[-1] = 1
    return v


def label_cases():
    rng = np.random.default_rng(20240917)
    both = [(3, 1), (3, 2), (3, 3), (2, 1), (2, 2)]
    flat = [(2, 1), (2, 2)]
    out = []

    def add(name, vol, classes, modes):
        out.append(dict(name=name, vol=np.asarray(vol, dtype=np.float32), classes=np.asarray(classes, dtype=np.int64), modes=modes))

    add("ties", noisy_labels((5, 7, 67), 4, rng, 0.10), (1, 2, 3), both)
    add("multiwg", noisy_labels((12, 64, 80), 4, rng, 0.02), (1, 2, 3), both)
    add("serpentine", serpentine(33), (1,), flat)
    add("helix", helix(9), (1,), [(3, 1), (3, 2), (2, 1)])
    add("comb_last", comb(20, 67), (1,), flat)
    add("comb_first", comb(20, 67)[::-1].copy(), (1,), flat)
    z, y, x = np.meshgrid(np.arange(9), np.arange(17), np.arange(70), indexing="ij")
    add("checker", (z + y + x) % 2, (1,), both)
    z, y, x = np.meshgrid(np.arange(4), np.arange(9), np.arange(13), indexing="ij")
    add("diagonal", 1 + (y + x) % 2, (1, 2), both)
    add("eight", np.stack([noisy_labels((4, 10, 12), 8, rng, 0.05) for _ in range(3)]), tuple(range(8)), both)
    add("slices6", noisy_labels((6, 20, 18), 4, rng, 0.05), (1, 2, 3), [(2, 1), (2, 2), (3, 1)])
    img = noisy_labels((9, 13), 4, rng, 0.08)
    add("img2d", img, (1, 2, 3), flat)
    add("z1", img[None], (1, 2, 3), both)
    add("full", np.ones((4, 5, 6)), (1, 2), both)
    cross = np.zeros((5, 8, 9))
    cross[:, 4, 4] = cross[2, :, 4] = cross[2, 4, :] = 1
    add("faces", cross, (1,), both)
    tie = np.zeros((4, 6, 8))
    tie[0:2, 0:2, 0:2] = 1
    tie[2:4, 3:5, 5:7] = 1          # two components of 8 voxels: the first survives
    tie[0, 5, 0:3] = 2
    tie[2, 0, 0:5] = 2
    tie[3, 5, 0:5] = 2              # 3, 5 and 5 voxels
    tie[1, 3, 3] = 7                # a class that is not asked for
    tie[1, 3, 4] = 2.5              # not integral: no class
    add("tie", tie, (1, 2), [(3, 1), (2, 1)])
    return out


def frames_of(vol):
    """vol -> [N, Z, H, W]"""
    if vol.ndim == 2:
        return vol[None, None]
    if vol.ndim == 3:
        return vol[None]
    return vol


def scipy_labelling(vol, classes, ndim, conn):
    v = frames_of(vol)
    N, Z, H, W = v.shape
    labels = np.zeros(v.shape, dtype=np.int32)
    counts, rows = [], []
    units = [(n, None) for n in range(N)] if ndim == 3 else [(n, z) for n in range(N) for z in range(Z)]
    for n, z in units:
        per = []
        for c in classes:
            mask = v[n] == c if z is None else v[n, z] == c
            lab, k = label(mask, generate_binary_structure(mask.ndim, conn))
            if z is None:
                labels[n][mask] = lab[mask]
            else:
                labels[n, z][mask] = lab[mask]
            per.append(k)
            sizes = np.bincount(lab.reshape(-1), minlength=k + 1)
            for i, sl in enumerate(find_objects(lab)):
                first = int(np.flatnonzero(lab.reshape(-1) == i + 1)[0])
                if z is None:
                    box = [sl[0].start, sl[0].stop, sl[1].start, sl[1].stop, sl[2].start, sl[2].stop]
                else:
                    box = [z, z + 1, sl[0].start, sl[0].stop, sl[1].start, sl[1].stop]
                    first += z * H * W
                rows.append([int(sizes[i + 1])] + box + [first])
        counts.append(per)
    return labels.reshape(vol.shape), np.asarray(counts, dtype=np.int32), np.asarray(rows, dtype=np.int64).reshape(-1, 8)


# ---- score cases ---------------------------------------------------------------------------------------------------------------------
def boxes_pair(shape, rng, n_obj, classes=(1,)):
    """two label maps of small cuboids: the reference's are the result's shifted, some bridged to a neighbour, some split, some extra"""
    res, ref = np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)
    rank = len(shape)
    for _ in range(n_obj):
        c = float(rng.choice(classes))
        lo = [int(rng.integers(0, s - 3)) for s in shape]
        ext = [int(rng.integers(2, max(3, s // 4))) for s in shape]
        sl = tuple(slice(a, min(a + e, s)) for a, e, s in zip(lo, ext, shape))
        kind = rng.integers(0, 5)
        if kind != 0:
            res[sl] = c
        if kind != 1:
            sh = [int(rng.integers(-2, 3)) for _ in range(rank)]
            sl2 = tuple(slice(max(a.start + d, 0), max(min(a.stop + d, s), 0)) for a, d, s in zip(sl, sh, shape))
            ref[sl2] = c
            if kind == 2:          # a bar along the last axis: bridges to whatever lies there
                bar = list(sl2)
                bar[-1] = slice(0, shape[-1])
                bar[-2] = slice(sl2[-2].start, sl2[-2].start + 1)
                ref[tuple(bar)] = c
            if kind == 3:          # a cut through the middle: one object of the result meets two of the reference
                cut = list(sl2)
                mid = (sl2[-1].start + sl2[-1].stop) // 2
                cut[-1] = slice(mid, mid + 1)
                ref[tuple(cut)] = 0
    return res, ref


def smallest_id_mapping(first, other, conn):
    """the rule of evaluate/object_metrics.py on scipy's label maps: ({first id: other id}, largest deferred set)"""
    from superresolution_aniso_mri_amd.evaluate.object_metrics import correspondences
    st = generate_binary_structure(first.ndim, conn)
    la, na = label(first, st)
    lb, _ = label(other, st)
    both = (la > 0) & (lb > 0)
    pairs = np.unique(np.stack([la[both], lb[both]], axis=1), axis=0) if both.any() else np.zeros((0, 2), dtype=np.int64)
    fan = np.bincount(pairs[:, 0], minlength=na + 1).max() if len(pairs) else 0
    return correspondences(pairs, na), int(fan) if fan >= 2 else 0


def score_record(ref, r, g, spacing, conn):
    """None when the smallest-id rule and the reference disagree on a mapping"""
    corr = getattr(ref, "__distinct_binary_object_correspondences")
    rec = {}
    _, _, n_res, n_ref, m_ref = corr(g, r, conn)          # visits the reference's components
    _, _, _, _, m_res = corr(r, g, conn)                   # visits the result's
    mine_ref, fan_ref = smallest_id_mapping(g, r, conn)
    mine_res, fan_res = smallest_id_mapping(r, g, conn)
    if {int(k): int(v) for k, v in m_ref.items()} != mine_ref or {int(k): int(v) for k, v in m_res.items()} != mine_res:
        return None
    rec["map_ref"] = np.asarray(sorted((int(k), int(v)) for k, v in m_ref.items()), dtype=np.int64).reshape(-1, 2)
    rec["map_res"] = np.asarray(sorted((int(k), int(v)) for k, v in m_res.items()), dtype=np.int64).reshape(-1, 2)
    rec["counts"] = np.asarray([n_res, n_ref], dtype=np.int64)
    rec["deferred"] = np.asarray(max(fan_ref, fan_res), dtype=np.int64)

    def safe(fn, *a):
        try:
            return float(fn(*a))
        except ZeroDivisionError:
            return float("nan")
    sp = tuple(spacing)
    rec["scores"] = np.asarray([safe(ref.obj_tpr, r, g, conn), safe(ref.obj_fpr, r, g, conn), safe(ref.obj_tpr, g, r, conn),
                                safe(ref.obj_fpr, g, r, conn), safe(ref.obj_asd, r, g, sp, conn), safe(ref.obj_asd, g, r, sp, conn),
                                safe(ref.obj_assd, r, g, sp, conn)], dtype=np.float64)
    return rec


def score_cases(ref):
    """[(name, result, reference, spacing, classes, connectivity, {key: array})]"""
    plans = [("aniso_a", (8, 24, 28), (10.0, 1.4, 1.4), (1,), 1, 9), ("aniso_b", (8, 24, 28), (10.0, 1.4, 1.4), (1,), 1, 12),
             ("aniso_k2", (8, 24, 28), (10.0, 1.4, 1.4), (1,), 2, 10), ("aniso_k3", (6, 20, 24), (10.0, 1.4, 1.4), (1,), 3, 9),
             ("iso", (7, 22, 26), (1.0, 1.0, 1.0), (1,), 1, 10), ("flat_a", (30, 40), (1.5, 0.75), (1,), 1, 12),
             ("flat_k2", (30, 40), (1.5, 0.75), (1,), 2, 12), ("classes3", (8, 24, 28), (2.5, 1.25, 1.25), (1, 2, 3), 1, 14),
             ("frames", (3, 6, 20, 18), (10.0, 1.4, 1.4), (1, 2), 1, 8)]
    out, seed = [], 1000
    for name, shape, spacing, classes, conn, n_obj in plans:
        while True:
            seed += 1
            rng = np.random.default_rng(seed)
            if len(shape) == len(spacing):
                r, g = boxes_pair(shape, rng, n_obj, classes)
            else:
                pairs = [boxes_pair(shape[1:], rng, n_obj, classes) for _ in range(shape[0])]
                r, g = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
            frames = [(r, g)] if len(shape) == len(spacing) else list(zip(r, g))
            recs, ok = {}, True
            for n, (fr, fg) in enumerate(frames):
                for c in classes:
                    rec = score_record(ref, fr == c, fg == c, spacing, conn)
                    if rec is None:
                        ok = False
                        break
                    for k, v in rec.items():
                        recs["n%d/c%d/%s" % (n, c, k)] = v
                if not ok:
                    break
            deferred = max([int(v) for k, v in recs.items() if k.endswith("/deferred")] or [0])
            if ok and deferred >= 2:          # every planned case goes through the deferred branch with a set of two or more
                break
        out.append((name, r, g, spacing, classes, conn, recs))
    # no overlap at all: nothing is mapped, obj_asd has nothing to average
    r, g = np.zeros((5, 12, 14), dtype=np.float32), np.zeros((5, 12, 14), dtype=np.float32)
    r[1:3, 2:5, 2:5] = 1
    r[3:5, 8:11, 9:12] = 1
    g[0:2, 7:10, 2:5] = 1
    rec = score_record(ref, r == 1, g == 1, (10.0, 1.4, 1.4), 1)
    out.append(("apart", r, g, (10.0, 1.4, 1.4), (1,), 1, {"n0/c1/" + k: v for k, v in rec.items()}))
    # an empty result: the reference divides by zero
    rec = score_record(ref, np.zeros_like(g) == 1, g == 1, (10.0, 1.4, 1.4), 1)
    out.append(("empty", np.zeros_like(g), g, (10.0, 1.4, 1.4), (1,), 1, {"n0/c1/" + k: v for k, v in rec.items()}))
    return out


def sequences(ref):
    rng = np.random.default_rng(77)
    out = {}
    for name, frames, shape in (("cycle", 8, (4, 12, 14)), ("flat", 5, (16, 18))):
        res, refs = [], []
        for f in range(frames):
            field, centres = mgs.blob(shape, rng)
            level = 0.35 + 0.25 * np.sin(2 * np.pi * f / frames)
            refs.append((field > level).astype(np.float32) * 2)          # any non-zero value is object
            res.append((mgs.blob(shape, rng, centres, jitter=1.0)[0] > level + 0.05 * rng.standard_normal()).astype(np.float32))
        res, refs = np.stack(res), np.stack(refs)
        out[name + "/results"], out[name + "/references"] = res, refs
        out[name + "/vc"] = np.asarray(ref.volume_correlation(res, refs), dtype=np.float64)
        out[name + "/vcc"] = np.asarray(ref.volume_change_correlation(res, refs), dtype=np.float64)
    return out


def main():
    ref = mgs.reference_module()
    rec = {}
    lc = label_cases()
    rec["label_cases"] = np.asarray([c["name"] for c in lc])
    for case in lc:
        name = case["name"]
        rec[name + "/vol"], rec[name + "/classes"] = case["vol"], case["classes"]
        rec[name + "/modes"] = np.asarray(case["modes"], dtype=np.int64)
        for nd, k in case["modes"]:
            labels, n, table = scipy_labelling(case["vol"], case["classes"], nd, k)
            key = "%s/d%d/k%d" % (name, nd, k)
            rec[key + "/labels"], rec[key + "/n"], rec[key + "/table"] = labels, n, table
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sc = score_cases(ref)
        seq = sequences(ref)
    rec["score_cases"] = np.asarray([c[0] for c in sc])
    deferred = 0
    for name, r, g, spacing, classes, conn, recs in sc:
        rec[name + "/result"], rec[name + "/reference"] = r.astype(np.float32), g.astype(np.float32)
        rec[name + "/spacing"], rec[name + "/classes"] = np.asarray(spacing, dtype=np.float64), np.asarray(classes, dtype=np.int64)
        rec[name + "/connectivity"] = np.asarray(conn, dtype=np.int64)
        for k, v in recs.items():
            rec[name + "/" + k] = v
        deferred += max(int(v) for k, v in recs.items() if k.endswith("/deferred")) >= 2
    assert deferred >= 4, "too few cases go through the deferred, one-to-many branch: %d" % deferred
    rec["sequences"] = np.asarray(sorted({k.split("/")[0] for k in seq}))
    rec.update(seq)
    np.savez_compressed(OUT, **rec)
    print("%s: %d arrays, %d score cases with a deferred set of two or more, %.1f KB" % (OUT, len(rec), deferred, os.path.getsize(OUT) / 1024.0))


if __name__ == "__main__":
    main()
