"""Object-wise scores of label volumes on the device: how many connected components of a segmentation have a partner in the reference
(obj_tpr, obj_fpr) and how far apart the partners' surfaces are (obj_asd, obj_assd), plus the two volume correlations -- what the
reference's kwatsch/medpy_metrics.py (medpy) computes with scipy on the host.

Why they live here and not in ``kwatsch.medpy_metrics``: that mirror module's ``obj_*`` and ``volume_*correlation`` are pinned by the
suite to raise NotImplementedError (they were recorded as not built when the surface scores were), so the working functions are in this
module, under the reference's names, argument order and defaults.

What is computed is what the reference's CODE computes (its docstrings disagree with it in places):
- components are labelled by csrc/components.hip (include/aesr_hip_components.h: scipy.ndimage.label's numbering); the pairs of components
  that share a voxel come from its overlap runs;
- correspondences (``correspondences`` below, pure host code over the pair list): the components of the FIRST side are visited in number
  order; one that overlaps exactly one component of the other side takes it if that one is unused; one that overlaps several is deferred;
  the deferred ones are served in rounds: drop used ids, drop empty sets, stable-sort by set size, serve the first, drop it, repeat;
- with M mapped pairs, obj_tpr(result, reference) = M / n_objects(result) and obj_fpr(result, reference) = (n_objects(reference) - M) /
  n_objects(reference), the visited side being ``reference``;
- obj_asd(a, b) visits the components of ``a`` and is the mean over the surface distances of all mapped pairs, taken from the partner
  in ``b`` to the component of ``a``; NaN when nothing is mapped; obj_assd is the mean of the two call directions.  The reference crops
  every pair to the union of the two bounding boxes, which changes nothing (outside it neither object has a voxel), so the pairs are
  scored on the full array: ``aesr_components_apply_table`` writes two volumes in which pair k's components carry the value k, and the
  surface-distance kernels of evaluate/seg_metrics.py score them as classes 1 ... K, eight at a time; sums and lengths are pooled.

One deviation: where the reference serves a deferred component it takes ``set.pop()``, an arbitrary element; here the smallest id is
taken.  The number of matches, and with it obj_tpr / obj_fpr, was the same on every random mask tried; the mapping itself can differ.

There is no CPU fallback."""
import numpy as np
import torch

from .. import ops
from . import components as cc
from . import seg_metrics as sm

OBJECT_KEYS = ("n_objects_result", "n_objects_reference", "n_matched", "obj_tpr", "obj_fpr", "obj_asd_result_to_reference",
               "obj_asd_reference_to_result", "obj_assd")


def correspondences(pairs, n_first):
    """pairs: the (id on the first side, id on the other side) of every two components that share a voxel; n_first: the number of
    components of the first side.  Returns {first id: other id}, one-to-one, by the reference's rules with the smallest id served where
    it pops an arbitrary one."""
    by = {}
    for a, b in pairs:
        by.setdefault(int(a), set()).add(int(b))
    mapping, used, one_to_many = {}, set(), []
    for i in range(1, int(n_first) + 1):
        ids = by.get(i, ())
        if len(ids) == 1:
            j = next(iter(ids))
            if j not in used:
                mapping[i] = j
                used.add(j)
        elif len(ids) > 1:
            one_to_many.append((i, set(ids)))
    while True:
        one_to_many = [(i, ids - used) for i, ids in one_to_many]
        one_to_many = [x for x in one_to_many if x[1]]
        one_to_many = sorted(one_to_many, key=lambda x: len(x[1]))
        if not one_to_many:
            break
        j = min(one_to_many[0][1])
        mapping[one_to_many[0][0]] = j
        used.add(j)
        one_to_many = one_to_many[1:]
    return mapping


def _pair_distances(first, lab_first, n_first, off_first, second, lab_second, n_second, off_second, mappings, classes, spacing, ndim,
                    connectivity, max_workspace_bytes):
    """mappings[n][c]: {id in first: id in second}.  Returns (sum [N, C], length [N, C]) of the surface distances of all mapped pairs,
    from the component of ``second`` to its partner in ``first`` (the direction of the reference's obj_asd(first, second))."""
    N, C = len(mappings), len(classes)
    tab_first = np.zeros(int(n_first.sum()), dtype=np.float32)
    tab_second = np.zeros(int(n_second.sum()), dtype=np.float32)
    owner = []          # per frame: the class index of pair 1, 2, ...
    for n in range(N):
        own = []
        for c in range(C):
            for a, b in sorted(mappings[n][c].items()):
                own.append(c)
                tab_first[off_first[n, c] + a - 1] = len(own)
                tab_second[off_second[n, c] + b - 1] = len(own)
        owner.append(own)
    sums, lens = np.zeros((N, C)), np.zeros((N, C), dtype=np.int64)
    K = max(len(o) for o in owner)
    if K == 0:
        return sums, lens
    dev = first.device
    vol_first = ops.components_apply_table(first, lab_first[0], lab_first[1], torch.from_numpy(tab_first).to(dev), classes, ndim=ndim,
                                           n_components_host=n_first)
    vol_second = ops.components_apply_table(second, lab_second[0], lab_second[1], torch.from_numpy(tab_second).to(dev), classes, ndim=ndim,
                                            n_components_host=n_second)
    for k0 in range(0, K, 8):
        ks = list(range(k0 + 1, min(k0 + 8, K) + 1))
        _, stats, lengths, _ = sm._run(vol_second, vol_first, spacing, ks, ndim, connectivity, max_workspace_bytes)
        for n in range(N):
            for i, k in enumerate(ks):
                if k <= len(owner[n]):
                    sums[n, owner[n][k - 1]] += stats[n, i, 0, 0]
                    lens[n, owner[n][k - 1]] += lengths[n, i, 0]
    return sums, lens


def object_scores(result, reference, spacing, classes=None, ndim=3, connectivity=1, max_workspace_bytes=1 << 30):
    """result, reference: label volumes [Z, H, W] or [N, Z, H, W] (class ids; numpy, CPU or CUDA tensors), spacing (z, y, x) in mm.
    Returns a dict of numpy arrays [N, C]: n_objects_result, n_objects_reference, n_matched (int64); obj_tpr, obj_fpr,
    obj_asd_result_to_reference (= the reference's obj_asd(result, reference)), obj_asd_reference_to_result, obj_assd (float64); plus
    classes.  A zero denominator, and an obj_asd with nothing mapped, is NaN.  ``classes=None``: 1 ... the largest label of the
    reference.  ``ndim=2`` labels and scores images: it requires Z == 1 and raises ValueError otherwise (the objects of a volume's
    slices would have to be matched slice by slice, which the reference does not define)."""
    r, g, _ = sm._as_batch(result, reference)
    spacing = sm._spacing3(spacing)
    classes = sm._classes(classes, g)
    ndim, connectivity = int(ndim), int(connectivity)
    N, Z = int(r.shape[0]), int(r.shape[1])
    if ndim == 2 and Z != 1:
        raise ValueError("ndim=2 scores images: it needs Z == 1, got Z = %d" % Z)
    C = len(classes)
    lab_r, n_r, ws = ops.components_label(r, classes, ndim=ndim, connectivity=connectivity)
    lab_g, n_g, _ = ops.components_label(g, classes, ndim=ndim, connectivity=connectivity)
    runs = ops.components_overlaps(r, lab_r, g, lab_g, classes, ndim=ndim, workspace=ws)
    hr, hg = n_r.cpu().numpy().astype(np.int64), n_g.cpu().numpy().astype(np.int64)          # [N, C]: a unit is a frame here
    pairs = np.unique(runs.cpu().numpy(), axis=0) if runs.shape[0] else np.zeros((0, 4), dtype=np.int32)
    by = {}
    for u, c, a, b in pairs:
        by.setdefault((int(u), int(c)), []).append((int(a), int(b)))
    # visiting the reference's components (obj_tpr, obj_fpr, obj_asd(reference, result)) and the result's (obj_asd(result, reference))
    from_ref = [[correspondences([(b, a) for a, b in by.get((n, c), ())], hg[n, c]) for c in range(C)] for n in range(N)]
    from_res = [[correspondences(by.get((n, c), ()), hr[n, c]) for c in range(C)] for n in range(N)]
    matched = np.array([[len(from_ref[n][c]) for c in range(C)] for n in range(N)], dtype=np.int64).reshape(N, C)
    off = lambda h: (np.cumsum(h.reshape(-1)) - h.reshape(-1)).reshape(h.shape)          # noqa: E731
    args = (classes, spacing, ndim, connectivity, max_workspace_bytes)
    s_rg, l_rg = _pair_distances(r, (lab_r, n_r), hr, off(hr), g, (lab_g, n_g), hg, off(hg), from_res, *args)
    s_gr, l_gr = _pair_distances(g, (lab_g, n_g), hg, off(hg), r, (lab_r, n_r), hr, off(hr), from_ref, *args)
    nan = np.full((N, C), np.nan)
    asd_rg = np.where(l_rg > 0, s_rg / np.where(l_rg > 0, l_rg, 1), nan)
    asd_gr = np.where(l_gr > 0, s_gr / np.where(l_gr > 0, l_gr, 1), nan)
    return {"n_objects_result": hr, "n_objects_reference": hg, "n_matched": matched,
            "obj_tpr": sm._ratio(matched, hr, np.nan), "obj_fpr": sm._ratio(hg - matched, hg, np.nan),
            "obj_asd_result_to_reference": asd_rg, "obj_asd_reference_to_result": asd_gr, "obj_assd": (asd_rg + asd_gr) / 2.0,
            "classes": np.asarray(classes, dtype=np.int64)}


# ---- the reference's names, argument order and defaults ------------------------------------------------------------------------------
def _binary(x, name):
    """array_like of rank 1 ... 3 -> (fp32 0 / 1 array [1, Z, H, W], rank); a CUDA tensor stays on the device"""
    if torch.is_tensor(x) and x.is_cuda:
        b = (x != 0).to(torch.float32)
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("%s: %s" % (name, cc.NO_FALLBACK))
        b = (np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x) != 0).astype(np.float32)
    rank = b.ndim
    if not 1 <= rank <= 3:
        raise ValueError("%s must have 1 to 3 dimensions, got %d" % (name, rank))
    return b.reshape((1,) * (4 - rank) + tuple(b.shape)), rank


def _mirror(result, reference, voxelspacing, connectivity):
    r, rank = _binary(result, "result")
    g, rank_g = _binary(reference, "reference")
    if rank != rank_g:
        raise ValueError("result and reference differ in rank")
    if voxelspacing is None:
        sp = [1.0] * rank
    else:
        sp = [float(v) for v in np.asarray(voxelspacing, dtype=np.float64).reshape(-1)]
        sp = sp * rank if len(sp) == 1 else sp
        if len(sp) != rank:
            raise ValueError("voxelspacing must have one entry per axis")
    ndim = 3 if rank == 3 else 2
    return object_scores(r, g, [1.0] * (3 - rank) + sp, classes=[1], ndim=ndim, connectivity=min(int(connectivity), ndim))


def obj_tpr(result, reference, connectivity=1):
    """The reference's obj_tpr: mapped pairs / distinct objects of ``result`` (ZeroDivisionError when it has none)."""
    s = _mirror(result, reference, None, connectivity)
    return int(s["n_matched"][0, 0]) / float(int(s["n_objects_result"][0, 0]))


def obj_fpr(result, reference, connectivity=1):
    """The reference's obj_fpr: (objects of ``reference`` - mapped pairs) / objects of ``reference`` (ZeroDivisionError when it has none)."""
    s = _mirror(result, reference, None, connectivity)
    n = int(s["n_objects_reference"][0, 0])
    return (n - int(s["n_matched"][0, 0])) / float(n)


def obj_asd(result, reference, voxelspacing=None, connectivity=1):
    """The reference's obj_asd (NaN when no pair of objects overlaps)."""
    return float(_mirror(result, reference, voxelspacing, connectivity)["obj_asd_result_to_reference"][0, 0])


def obj_assd(result, reference, voxelspacing=None, connectivity=1):
    """The reference's obj_assd: the mean of obj_asd in both call directions."""
    return float(_mirror(result, reference, voxelspacing, connectivity)["obj_assd"][0, 0])


def _volumes(frames, name):
    """sequence of array_like -> voxel counts of (frame != 0), counted on the device"""
    if not torch.cuda.is_available():
        raise RuntimeError("%s: %s" % (name, cc.NO_FALLBACK))
    arr = np.atleast_2d(np.asarray([np.asarray(f.detach().cpu().numpy() if torch.is_tensor(f) else f) for f in frames]) != 0)
    n = arr.shape[0]
    flat = arr.reshape(n, -1).astype(np.float32)
    flat = np.pad(flat, ((0, 0), (0, -flat.shape[1] % 1024)))          # rows of 1024 voxels; the zeros added count for nothing
    v = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda").reshape(n, 1, -1, 1024)
    counts, _, _, _ = sm._run(v, v, [1.0, 1.0, 1.0], [1], 3, 1, 1 << 30, want_distances=False)
    return counts[:, 0, 0].astype(np.int64)


def volume_correlation(results, references):
    """The reference's volume_correlation: scipy.stats.pearsonr of the object volumes (voxel counts, from the device) of successive
    binary images.  Returns (r, p)."""
    from scipy.stats import pearsonr
    return pearsonr(_volumes(results, "results"), _volumes(references, "references"))


def volume_change_correlation(results, references):
    """The reference's volume_change_correlation: pearsonr of the frame-to-frame changes of the object volumes.  Returns (r, p)."""
    from scipy.stats import pearsonr
    a, b = _volumes(results, "results"), _volumes(references, "references")
    return pearsonr(a[1:] - a[:-1], b[1:] - b[:-1])
