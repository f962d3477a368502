"""The binary segmentation scores under the names and argument order of the reference's kwatsch/medpy_metrics.py (medpy's metrics), computed
on the device by ``evaluate.seg_metrics`` (csrc/seg_metrics.hip; definitions in include/aesr_hip_surface.h).

Inputs of rank 2 or 3 (numpy arrays, CPU or CUDA tensors) are binarised by ``!= 0``; the rank sets the neighbourhood's dimension;
``voxelspacing`` is one number for all axes, one per axis, or None for 1; ``connectivity`` 1 ... rank picks the border neighbourhood.
A host array goes through the GPU: without one these functions raise, there is no CPU fallback.

Kept as the reference has them: ``true_negative_rate`` returns the SENSITIVITY (the reference's function calls ``sensitivity``, not
``specificity``); ``jc`` of two empty inputs divides by zero; the distance functions raise RuntimeError when an input holds no object.
Not provided: ``obj_*``, ``volume_correlation`` and ``volume_change_correlation`` need connected components / a list protocol that the
device path does not have -- they raise NotImplementedError."""
import numpy as np
import torch

from ..evaluate import seg_metrics as _sm

EMPTY_FIRST = "The first supplied array does not contain any binary object."
EMPTY_SECOND = "The second supplied array does not contain any binary object."


def _binary(x):
    if torch.is_tensor(x):
        b = (x != 0).to(torch.float32)
    else:
        b = (np.asarray(x) != 0).astype(np.float32)
    if b.ndim == 2:
        return b[None, None], 2
    if b.ndim == 3:
        return b[None], 3
    raise ValueError("the device scores take arrays of rank 2 or 3, got rank %d" % b.ndim)


def _pair(result, reference):
    r, nd = _binary(result)
    g, nd_g = _binary(reference)
    if nd != nd_g or tuple(r.shape) != tuple(g.shape):
        raise ValueError("result %s and reference %s differ in shape" % (tuple(r.shape), tuple(g.shape)))
    return r, g, nd


def _spacing(voxelspacing, nd):
    if voxelspacing is None:
        return [1.0, 1.0, 1.0]
    s = np.asarray(voxelspacing, dtype=np.float64).reshape(-1)
    if s.size == 1:
        s = np.repeat(s, nd)
    if s.size != nd:
        raise RuntimeError("sequence argument must have length equal to input rank")
    return [1.0] * (3 - nd) + [float(v) for v in s]


def _counts(result, reference):
    r, g, nd = _pair(result, reference)
    rr, gg, _ = _sm._as_batch(r, g)
    counts, _, _, _ = _sm._run(rr, gg, [1.0, 1.0, 1.0], [1], nd, 1, 1 << 30, want_distances=False)
    return [int(v) for v in counts[0, 0]]


def _distances(result, reference, voxelspacing, connectivity):
    """(scores of the single class, list result -> reference, list reference -> result)"""
    r, g, nd = _pair(result, reference)
    rr, gg, _ = _sm._as_batch(r, g)
    spacing = _spacing(voxelspacing, nd)
    counts, stats, lengths, dist = _sm._run(rr, gg, spacing, [1], nd, int(connectivity), 1 << 30)
    if counts[0, 0, 0] == 0:
        raise RuntimeError(EMPTY_FIRST)
    if counts[0, 0, 1] == 0:
        raise RuntimeError(EMPTY_SECOND)
    d = dist.cpu().numpy()
    n0 = int(lengths[0, 0, 0])
    return stats[0, 0], d[:n0], d[n0:]


def dc(result, reference):
    A, B, I = _counts(result, reference)[:3]
    return 2.0 * I / float(A + B) if A + B else 0.0


def jc(result, reference):
    c = _counts(result, reference)
    return float(c[2]) / float(c[3])


def precision(result, reference):
    A, _, I = _counts(result, reference)[:3]
    return I / float(A) if A else 0.0


def recall(result, reference):
    _, B, I = _counts(result, reference)[:3]
    return I / float(B) if B else 0.0


def sensitivity(result, reference):
    return recall(result, reference)


def specificity(result, reference):
    _, B, _, U, T = _counts(result, reference)[:5]
    return (T - U) / float(T - B) if T - B else 0.0


def true_negative_rate(result, reference):
    return sensitivity(result, reference)          # as in the reference: NOT the specificity


def true_positive_rate(result, reference):
    return recall(result, reference)


def positive_predictive_value(result, reference):
    return precision(result, reference)


def hd(result, reference, voxelspacing=None, connectivity=1):
    stats, _, _ = _distances(result, reference, voxelspacing, connectivity)
    return float(max(stats[0, 1], stats[1, 1]))


def hd95(result, reference, voxelspacing=None, connectivity=1):
    _, d0, d1 = _distances(result, reference, voxelspacing, connectivity)
    return float(np.percentile(np.hstack((d0, d1)), 95))


def asd(result, reference, voxelspacing=None, connectivity=1):
    stats, d0, _ = _distances(result, reference, voxelspacing, connectivity)
    return float(stats[0, 0] / d0.size)


def assd(result, reference, voxelspacing=None, connectivity=1):
    stats, d0, d1 = _distances(result, reference, voxelspacing, connectivity)
    return float((stats[0, 0] / d0.size + stats[1, 0] / d1.size) / 2.0)


def ravd(result, reference):
    A, B = _counts(result, reference)[:2]
    if B == 0:
        raise RuntimeError(EMPTY_SECOND)
    return (A - B) / float(B)


def _not_provided(name):
    def fn(*args, **kwargs):
        raise NotImplementedError("%s needs connected components, which the device scores do not have" % name)
    fn.__name__ = name
    return fn


obj_assd, obj_asd, obj_fpr, obj_tpr = (_not_provided(n) for n in ("obj_assd", "obj_asd", "obj_fpr", "obj_tpr"))
volume_correlation, volume_change_correlation = (_not_provided(n) for n in ("volume_correlation", "volume_change_correlation"))
