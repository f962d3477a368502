"""Scores of a label volume against its reference on the device: Dice, Jaccard, precision, recall, specificity, relative volume difference,
Hausdorff distance, its 95th percentile, average (symmetric) surface distance -- the definitions of the reference's
kwatsch/medpy_metrics.py (medpy), stated in include/aesr_hip_surface.h and computed by csrc/seg_metrics.hip for every frame and class in
one launch sequence.  The reference does this with scipy on the host, one class and one direction at a time.

There is no CPU fallback: numpy arrays and CPU tensors are uploaded once, scored on the GPU, and the small tables come back."""
import numpy as np
import torch

from .. import ops

SCORE_KEYS = ("dice", "jc", "precision", "recall", "specificity", "ravd", "hd", "hd95", "assd", "asd_result_to_reference",
              "asd_reference_to_result")
NO_FALLBACK = "the segmentation scores are HIP kernels: they need the GPU, there is no CPU fallback"


def _to_device(x, name):
    """numpy / CPU tensor / CUDA tensor -> (contiguous fp32 CUDA tensor, True when the caller gave host data)."""
    host = not (torch.is_tensor(x) and x.is_cuda)
    if host:
        if not torch.cuda.is_available():
            raise RuntimeError("%s: %s" % (name, NO_FALLBACK))
        x = torch.as_tensor(np.ascontiguousarray(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float32))).to("cuda")
    return x.detach().to(torch.float32).contiguous(), host


def _as_batch(result, reference):
    r, host_r = _to_device(result, "result")
    g, host_g = _to_device(reference, "reference")
    if g.device != r.device:
        g = g.to(r.device)
    if tuple(r.shape) != tuple(g.shape):
        raise ValueError("result %s and reference %s differ in shape" % (tuple(r.shape), tuple(g.shape)))
    if r.dim() == 3:
        r, g = r[None], g[None]
    if r.dim() != 4:
        raise ValueError("label volumes must be [Z, H, W] or [N, Z, H, W], got %s" % (tuple(result.shape),))
    return r, g, host_r and host_g


def _spacing3(spacing):
    s = [float(v) for v in np.asarray(spacing, dtype=np.float64).reshape(-1)]
    if len(s) == 1:
        s = s * 3
    if len(s) != 3:
        raise ValueError("spacing must be (z, y, x) or one number, got %r" % (spacing,))
    return s


def _classes(classes, reference):
    if classes is None:
        top = float(reference.max()) if reference.numel() else 0.0          # one host read
        if not np.isfinite(top) or top < 1:
            raise ValueError("classes=None needs a reference with a largest label >= 1 (got %r)" % top)
        classes = range(1, int(top) + 1)
    classes = [int(c) for c in classes]
    if not 1 <= len(classes) <= 8:
        raise ValueError("1 to 8 classes per call are supported, got %d" % len(classes))
    return classes


def _frames_per_call(N, Z, H, W, C, max_workspace_bytes):
    one = ops.surface_workspace_bytes(1, Z, H, W, C)
    if one == 0:
        raise ValueError("the library refuses volumes of %d x %d x %d with %d classes" % (Z, H, W, C))
    k = max(1, min(N, int(max_workspace_bytes) // one))
    while k > 1 and not 0 < ops.surface_workspace_bytes(k, Z, H, W, C) <= max_workspace_bytes:
        k -= 1
    return k          # one volume is never split: a single frame larger than the limit still runs


def _run(r, g, spacing, classes, ndim, connectivity, max_workspace_bytes, want_distances=True):
    """The two phases over chunks of frames.  Returns (counts [N, C, 7] numpy, stats [N, C, 2, 2] numpy or None, lengths [N, C, 2] numpy,
    distances: the packed lists of all frames as one CUDA fp64 tensor, or None)."""
    N, Z, H, W = (int(s) for s in r.shape)
    C = len(classes)
    step = _frames_per_call(N, Z, H, W, C, max_workspace_bytes)
    counts, stats, lengths, dists = [], [], [], []
    for n0 in range(0, N, step):
        rr, gg = r[n0:n0 + step], g[n0:n0 + step]
        cnt, ws = ops.surface_borders(rr, gg, classes, ndim=ndim, connectivity=connectivity)
        host = cnt.cpu().numpy()
        counts.append(host)
        if want_distances:
            d, st, ln = ops.surface_distances(ws, cnt, rr.shape, spacing, ndim=ndim, counts_host=host)
            dists.append(d)
            stats.append(st.cpu().numpy())
            lengths.append(ln)
        else:
            lengths.append(ops.surface_list_lengths(host))
        del ws
    counts, lengths = np.concatenate(counts), np.concatenate(lengths)
    if not want_distances:
        return counts, None, lengths, None
    return counts, np.concatenate(stats), lengths, torch.cat(dists)


def _ratio(num, den, empty):
    """num / den elementwise in float64, ``empty`` where den == 0 (the reference's ZeroDivisionError branches)."""
    num, den = num.astype(np.float64), den.astype(np.float64)
    return np.where(den != 0, num / np.where(den != 0, den, 1.0), empty)


def overlap_scores(counts):
    """The count-based scores of [.., 7] counts (|A|, |B|, |A n B|, |A u B|, voxels, ...) as the reference defines them: dice and
    precision / recall / specificity are 0.0 where their denominator is 0; jc and ravd, which the reference lets fail there, are NaN."""
    c = np.asarray(counts, dtype=np.int64)
    A, B, I, U, T = (c[..., i] for i in range(5))
    return {"dice": _ratio(2 * I, A + B, 0.0), "jc": _ratio(I, U, np.nan), "precision": _ratio(I, A, 0.0), "recall": _ratio(I, B, 0.0),
            "specificity": _ratio(T - U, T - B, 0.0), "ravd": _ratio(A - B, B, np.nan)}


def segmentation_scores(result, reference, spacing, classes=None, ndim=3, connectivity=1, max_workspace_bytes=1 << 30):
    """result, reference: label volumes [Z, H, W] or [N, Z, H, W] (class ids; numpy, CPU or CUDA tensors), spacing (z, y, x) in mm.
    Returns a dict of float64 numpy arrays [N, C]: dice, jc, precision, recall, specificity, ravd, hd, hd95, assd,
    asd_result_to_reference, asd_reference_to_result; plus counts int64 [N, C, 7], volume_ml_result / volume_ml_reference (voxel count x
    voxel volume / 1000) and classes.  ``classes=None``: 1 ... the largest label of the reference.  ``ndim=2`` scores every slice as an
    image of its own.  Where either mask of a (frame, class) is empty the four distance scores are NaN.  Frames are processed in chunks
    whose workspace stays under ``max_workspace_bytes``."""
    r, g, _ = _as_batch(result, reference)
    spacing = _spacing3(spacing)
    classes = _classes(classes, g)
    counts, stats, lengths, dist = _run(r, g, spacing, classes, int(ndim), int(connectivity), max_workspace_bytes)
    out = overlap_scores(counts)
    both = (counts[..., 0] > 0) & (counts[..., 1] > 0)
    ln = lengths.astype(np.float64)
    nan = np.full(both.shape, np.nan)
    asd = [np.where(both, stats[..., d, 0] / np.where(ln[..., d] > 0, ln[..., d], 1.0), nan) for d in (0, 1)]
    out["asd_result_to_reference"], out["asd_reference_to_result"] = asd
    out["assd"] = (asd[0] + asd[1]) / 2.0
    out["hd"] = np.where(both, np.maximum(stats[..., 0, 1], stats[..., 1, 1]), nan)
    # hd95: numpy's percentile (linear interpolation) of both directions' lists, which lie side by side in the packed buffer
    packed = dist.cpu().numpy()
    hd95 = nan.copy()
    ends = np.cumsum(lengths.reshape(-1, 2).sum(axis=1))
    for i, (e, on) in enumerate(zip(ends, both.reshape(-1))):
        n_i = int(lengths.reshape(-1, 2)[i].sum())
        if on and n_i:
            with np.errstate(invalid="ignore"):          # slice-wise lists may hold +inf: interpolating between two of them is inf, not NaN
                v = np.percentile(packed[e - n_i:e], 95)
            hd95.reshape(-1)[i] = np.inf if np.isnan(v) else v
    out["hd95"] = hd95
    voxel_ml = spacing[0] * spacing[1] * spacing[2] / 1000.0
    out["counts"] = counts
    out["volume_ml_result"], out["volume_ml_reference"] = counts[..., 0] * voxel_ml, counts[..., 1] * voxel_ml
    out["classes"] = np.asarray(classes, dtype=np.int64)
    return out


def surface_distance_lists(result, reference, spacing, classes=None, ndim=3, connectivity=1, max_workspace_bytes=1 << 30):
    """The packed surface-distance lists themselves: dict(distances fp64 1-D -- numpy when both inputs were host data, else a CUDA
    tensor --, lengths int64 [N, C, 2], offsets int64 [N, C, 2], counts, classes).  List (n, c, 0) runs from the border voxels of
    ``result == c`` (raster order) to the border of ``reference == c``, list (n, c, 1) the other way; ``distances[o:o + l]`` is one list."""
    r, g, host = _as_batch(result, reference)
    spacing = _spacing3(spacing)
    classes = _classes(classes, g)
    counts, _, lengths, dist = _run(r, g, spacing, classes, int(ndim), int(connectivity), max_workspace_bytes)
    flat = lengths.reshape(-1)
    offsets = (np.cumsum(flat) - flat).reshape(lengths.shape)
    return {"distances": dist.cpu().numpy() if host else dist, "lengths": lengths, "offsets": offsets, "counts": counts,
            "classes": np.asarray(classes, dtype=np.int64)}


LABEL_BASELINES = ("nearest", "shape")


def score_label_supervolume(trainer, images, labels, downsample_steps, spacing, classes=None, baselines=("nearest",)):
    """Score what a multi-channel model makes of every ``downsample_steps``-th slice: ``create_super_volume(labels=)`` keeps those slices,
    synthesises the ones in between and returns a label volume as deep as ``labels``, which is scored against the full-resolution
    ``labels`` -- beside the nearest-slice baseline (``create_simple_interpolation(..., "nearest", align="grid")``, cut and extended the
    same way), the comparison the multi-channel model exists for.  Returns {"model": scores, "nearest": scores}.  ``baselines`` names the
    conventional methods scored beside the model on the same reference: "nearest" and / or "shape" (shape-based interpolation,
    ``evaluate.shape_interp.shape_baseline``); one table each under its name."""
    from .common import create_simple_interpolation, create_super_volume
    f = int(downsample_steps)
    if f < 2:
        raise ValueError("downsample_steps must be at least 2, got %r" % (downsample_steps,))
    baselines = tuple(baselines)
    if any(b not in LABEL_BASELINES for b in baselines) or len(set(baselines)) != len(baselines):
        raise ValueError("baselines=%r: each of %s at most once" % (baselines, ", ".join(LABEL_BASELINES)))
    if tuple(labels.shape) != tuple(images.shape):
        raise ValueError("the labels %s do not match the images %s" % (tuple(labels.shape), tuple(images.shape)))
    alphas = [k / float(f) for k in range(1, f)]
    out = create_super_volume(trainer, images, alpha_range=alphas, downsample_steps=f, generate_inbetween_slices=True, labels=labels)
    pred = out["upsampled_labels"]
    if pred is None:
        raise ValueError("the trainer's model returns no label volume: score_label_supervolume needs a multi-channel model")
    if tuple(pred.shape) != tuple(labels.shape):
        raise ValueError("the synthesised label volume %s does not match the labels %s" % (tuple(pred.shape), tuple(labels.shape)))
    if not torch.cuda.is_available():
        raise RuntimeError(NO_FALLBACK)
    ref = torch.as_tensor(labels).to("cuda", torch.float32)
    if classes is None:
        classes = _classes(None, ref)
    scores = {"model": segmentation_scores(pred.to("cuda", torch.float32), ref, spacing, classes=classes)}
    for name in baselines:
        if name == "nearest":
            vol = create_simple_interpolation(ref, spacing, expand_factor=f, interpol_filter="nearest", generate_inbetween_slices=True,
                                              align="grid").array
        else:
            from .shape_interp import shape_baseline
            vol = shape_baseline(ref, f, spacing).to(torch.float32)
        if tuple(vol.shape) != tuple(labels.shape):
            raise ValueError("the %s volume %s does not match the labels %s" % (name, tuple(vol.shape), tuple(labels.shape)))
        scores[name] = segmentation_scores(vol, ref, spacing, classes=classes)
    return scores
