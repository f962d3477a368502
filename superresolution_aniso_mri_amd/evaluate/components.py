"""Connected components of label volumes on the device: labelling, the per-component table, largest-component and minimum-size clean-up.
The definitions (adjacency, units, numbering = scipy.ndimage.label's) are stated in include/aesr_hip_components.h and computed by
csrc/components.hip for every frame and class in one launch sequence; the reference labels on the host with scipy, one mask at a time
(kwatsch/medpy_metrics.py, datasets/brainMASI/common.py).

There is no CPU fallback: numpy arrays and CPU tensors are uploaded once, labelled on the GPU, and the results come back as numpy; a CUDA
tensor in gives CUDA tensors out."""
import numpy as np
import torch

from .. import ops

NO_FALLBACK = "connected components are HIP kernels: they need the GPU, there is no CPU fallback"


def _to_device(x, name):
    """numpy / CPU tensor / CUDA tensor -> (contiguous fp32 CUDA tensor [N, Z, H, W], host input?, the input had no frame axis?)"""
    host = not (torch.is_tensor(x) and x.is_cuda)
    if host:
        if not torch.cuda.is_available():
            raise RuntimeError("%s: %s" % (name, NO_FALLBACK))
        x = torch.as_tensor(np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x))).to("cuda")
    v = x.detach().to(torch.float32).contiguous()
    single = v.dim() == 3
    if single:
        v = v[None]
    if v.dim() != 4:
        raise ValueError("%s must be [Z, H, W] or [N, Z, H, W], got %s" % (name, tuple(x.shape)))
    return v, host, single


def _classes(classes, vol):
    if classes is None:
        top = float(vol.max()) if vol.numel() else 0.0          # one host read
        if not np.isfinite(top) or top < 1:
            raise ValueError("classes=None needs a volume with a largest label >= 1 (got %r)" % top)
        classes = range(1, int(top) + 1)
    classes = [int(c) for c in classes]
    if not 1 <= len(classes) <= 8:
        raise ValueError("1 to 8 classes per call are supported, got %d" % len(classes))
    return classes


def _label(v, classes, ndim, connectivity):
    """labels, n_components (device), table (device), n_components_host"""
    lab, ncomp, ws = ops.components_label(v, classes, ndim=ndim, connectivity=connectivity)
    table, host = ops.components_tables(v, lab, ncomp, classes, ndim=ndim, workspace=ws)
    return lab, ncomp, table, host, ws


def label_components(labels, classes=None, ndim=3, connectivity=1):
    """labels: a label volume [Z, H, W] or [N, Z, H, W] (class ids; numpy, CPU or CUDA tensor).  Returns a dict:
    labels int32 (the input's shape: 0 or the voxel's component number within its (unit, class), scipy.ndimage.label's numbering),
    n_components int32 [U, C] (a unit is a frame with ndim = 3, a slice with ndim = 2), and per component in the order (unit, class,
    number): sizes int64 [R], boxes int64 [R, 6] (half-open z0, z1, y0, y1, x0, x1: scipy's find_objects), first_voxels int64 [R] (linear
    index within the frame); offsets int64 [U, C] (row of component 1 of a (unit, class)), classes.  ``classes=None``: 1 ... the
    largest label.  numpy in gives numpy out, a CUDA tensor in gives CUDA tensors out."""
    v, host, single = _to_device(labels, "labels")
    classes = _classes(classes, v)
    lab, ncomp, table, nhost, _ = _label(v, classes, int(ndim), int(connectivity))
    if single:
        lab = lab[0]
    offsets = (np.cumsum(nhost.reshape(-1).astype(np.int64)) - nhost.reshape(-1)).reshape(nhost.shape)
    out = {"labels": lab, "n_components": ncomp, "sizes": table[:, 0], "boxes": table[:, 1:7], "first_voxels": table[:, 7]}
    if host:
        out = {k: t.cpu().numpy() for k, t in out.items()}
    out["offsets"] = offsets
    out["classes"] = np.asarray(classes, dtype=np.int64)
    return out


def _keep_table(sizes, nhost, classes, largest, min_size):
    """fp32 per component: its class id where it survives, else 0 (host arithmetic over the small table)."""
    keep = np.zeros(len(sizes), dtype=np.float32)
    row = 0
    for uc, n in enumerate(nhost.reshape(-1)):
        n = int(n)
        if n:
            s = sizes[row:row + n]
            cid = float(classes[uc % len(classes)])
            if largest:
                keep[row + int(np.argmax(s))] = cid          # argmax: the first maximum, so a tie goes to the lowest number
            else:
                keep[row:row + n] = np.where(s >= min_size, cid, 0.0)
        row += n
    return keep


def _clean(labels, classes, ndim, connectivity, largest, min_size):
    v, host, single = _to_device(labels, "labels")
    classes = _classes(classes, v)
    lab, ncomp, table, nhost, ws = _label(v, classes, int(ndim), int(connectivity))
    keep = _keep_table(table[:, 0].cpu().numpy(), nhost, classes, largest, min_size)
    kept = ops.components_apply_table(v, lab, ncomp, torch.from_numpy(keep).to(v.device), classes, ndim=int(ndim), workspace=ws,
                                      n_components_host=nhost)
    out = torch.where(lab > 0, kept, v)          # voxels with no class in `classes` pass through unchanged
    if single:
        out = out[0]
    if host:
        return out.cpu().numpy().astype(labels.dtype if isinstance(labels, np.ndarray) else np.asarray(labels).dtype)
    return out.to(labels.dtype)


def keep_largest_component(labels, classes=None, ndim=3, connectivity=1):
    """Per (unit, class) the component with the most voxels survives (a tie goes to the lowest number); every other voxel of that class
    becomes 0; voxels with no class in ``classes`` pass through unchanged.  Shape, container and dtype of the input are kept."""
    return _clean(labels, classes, ndim, connectivity, True, 0)


def remove_small_components(labels, min_size, classes=None, ndim=3, connectivity=1):
    """Components with fewer than ``min_size`` voxels become 0; everything else as ``keep_largest_component``."""
    return _clean(labels, classes, ndim, connectivity, False, int(min_size))
