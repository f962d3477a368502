#!/usr/bin/env python
"""Times connected-component labelling (aesr_components_label / aesr_components_tables, csrc/components.hip) on the reference volume of the
70 x 224 x 224 three-class pair scripts/seg_metrics_bench.py uses, 3-D, connectivity 1.  Needs the GPU; prints a table (kept in
profiles/components.txt).

- label / label + tables: HIP events around the C entry points into preallocated buffers (the tables from a host copy of the counts made
  beforehand), after ``--warmup`` calls; median / min / max of ``--reps`` calls.
- call: host clock around ``evaluate.components.label_components`` on a device tensor, device synchronised: both entry points, the
  allocations and the copy of the counts in between.
- parity and cpu: if scipy is importable, ``scipy.ndimage.label`` per class on this machine's host, once, and whether the device's label
  map equals it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from seg_metrics_bench import CLASSES, SHAPE, event_times, label_pair, row  # noqa: E402
from superresolution_aniso_mri_amd import _hip, ops  # noqa: E402
from superresolution_aniso_mri_amd.evaluate import components  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "components_bench.py measures on the GPU; there is no CPU fallback"
    Z, H, W = SHAPE
    C = len(CLASSES)
    _, ref = label_pair(SHAPE, np.random.default_rng(7))
    v = torch.from_numpy(ref).cuda()[None]
    print("device: %s; %d warm-up calls, %d samples; %d x %d x %d, classes %s, ndim 3, connectivity 1" % (
        torch.cuda.get_device_name(0), args.warmup, args.reps, Z, H, W, list(CLASSES)))
    nbytes = ops.components_workspace_bytes(1, Z, H, W, C)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    labels = torch.empty((1, Z, H, W), device="cuda", dtype=torch.int32)
    ncomp = torch.empty((1, C), device="cuda", dtype=torch.int32)
    cls = _hip.int_array(CLASSES)

    def label():
        _hip.check(_hip.lib.aesr_components_label(_hip.ptr(v), _hip.ptr(labels), _hip.ptr(ncomp), _hip.ptr(ws), 1, Z, H, W, cls, C, 3, 1,
                                                  _hip.stream()), "aesr_components_label")
    label()
    host = np.ascontiguousarray(ncomp.cpu().numpy(), dtype=np.int32)
    rows = int(host.sum())
    table = torch.empty((max(rows, 1), _hip.COMPONENTS_COLUMNS), device="cuda", dtype=torch.int64)

    def label_and_tables():
        label()
        _hip.check(_hip.lib.aesr_components_tables(_hip.ptr(v), _hip.ptr(labels), _hip.ptr(ncomp), host.ctypes.data_as(_hip.IP), _hip.ptr(ws),
                                                   _hip.ptr(table), max(rows, 1), 1, Z, H, W, cls, C, 3, _hip.stream()), "aesr_components_tables")
    label_and_tables()
    print("workspace %.1f MB; components per class %s; largest component per class %s voxels" % (
        nbytes / 1e6, host[0].tolist(), [int(t[:, 0].max()) if len(t) else 0 for t in torch.split(table[:rows].cpu(), host[0].tolist())]))
    print("%-44s | %9s %9s %9s" % ("", "med [ms]", "min [ms]", "max [ms]"))
    row("label: aesr_components_label (6 launches)", event_times(label, args.warmup, args.reps))
    row("label + tables (6 + 3 launches)", event_times(label_and_tables, args.warmup, args.reps))

    def whole():
        t0 = time.perf_counter()
        whole.out = components.label_components(v, classes=CLASSES)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for _ in range(args.warmup):
        whole()
    row("call: label_components, device tensor in", [whole() for _ in range(args.reps)], note="(host clock)")
    if args.no_cpu:
        return
    try:
        import scipy
        from scipy import ndimage as ndi
    except ImportError:
        print("cpu: NOT MEASURED (scipy is not importable here)")
        return
    got = whole.out["labels"].cpu().numpy()[0]
    per_class, same = [], True
    for c in CLASSES:
        t0 = time.perf_counter()
        lab, _ = ndi.label(ref == c, ndi.generate_binary_structure(3, 1))
        per_class.append(time.perf_counter() - t0)
        same = same and np.array_equal(lab[ref == c], got[ref == c])
    print("cpu: scipy %s ndimage.label on this host, once per class: %s s (classes %s), %.3f s for all three; the device's label map %s" % (
        scipy.__version__, " ".join("%.3f" % t for t in per_class), list(CLASSES), sum(per_class), "equals scipy's" if same else "DIFFERS"))


if __name__ == "__main__":
    main()
