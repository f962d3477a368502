#!/usr/bin/env python
"""Times the labelled batch assembly (aesr_labelled_triplet_assemble, csrc/augment_labelled.hip) at the training recipe's batch: 12 samples
of 160 x 160 cropped from a 180 x 180 canvas over 216 x 256 slices, beside the existing one-channel aesr_triplet_assemble at the same B, W,
descriptors and image cache in the same run -- the thing to read it against.  Needs the GPU; prints a table (kept in
profiles/labelled_batches.txt).

- kernel: HIP events around ``--batch`` back-to-back calls of the C entry point into one preallocated output, divided by ``--batch`` (the
          launch latency of a single call is hidden behind the previous kernel); median / min / max of ``--reps`` such batches.  The two
          kernels alternate batch by batch, so that a drift of the machine meets both.
          ``rocprofv3 --kernel-trace --stats -- python scripts/labelled_batch_bench.py --reps 20`` gives the same figure from the profiler
          (labelled_triplet_assemble_kernel<false> / triplet_assemble_kernel<false>).
- call:   HIP events around ``LabelledTripletAugmenter.assemble`` / ``TripletAugmenter.assemble`` with the transforms given (descriptor table
          on the host, the outputs' allocation, one launch), and around ``next_batch`` (the host's random draws too); after ``--warmup``
          calls, median / min / max of ``--reps`` calls.
- bytes:  algorithmic: 3 B W^2 gathered samples of 4 + 1 bytes and 3 B W^2 x 2 floats written for the labelled kernel, 3 B W^2 x (4 + 4) for
          the one-channel kernel; the share of the 8 TB/s HBM peak is those bytes over the kernel time.  A batch of 12 MB is
          over in microseconds, so the launch is latency-bound: the share says how far, not how well the kernel streams."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import _hip  # noqa: E402
from superresolution_aniso_mri_amd.data_device import LabelledTripletAugmenter, TripletAugmenter  # noqa: E402

HBM_PEAK = 8.0e12


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def row(name, ts, nbytes=None):
    med = statistics.median(ts)
    tail = "" if nbytes is None else " | %8.1f %7.2f%% | %.2f" % (nbytes / med / 1e9, 100 * nbytes / med / HBM_PEAK, nbytes / 1e6)
    print("%-58s | %8.2f %8.2f %8.2f%s" % (name, med * 1e6, min(ts) * 1e6, max(ts) * 1e6, tail))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("-B", type=int, default=12)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--aug_patch_size", type=int, default=180)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "labelled_batch_bench.py measures on the GPU; there is no CPU fallback"
    B, W = args.B, args.width
    rs = np.random.RandomState(1)
    shapes = [(10, 216, 256), (9, 256, 216), (12, 224, 224), (8, 154, 184)] * 5          # 20 volumes, one of them smaller than the canvas
    vols = [rs.rand(*s).astype(np.float32) for s in shapes]
    labs = [rs.randint(0, 4, s).astype(np.uint8) for s in shapes]
    lab_aug = LabelledTripletAugmenter(vols, labs, W, args.aug_patch_size, rs=np.random.RandomState(2))
    img_aug = TripletAugmenter(vols, W, args.aug_patch_size, rs=np.random.RandomState(2))
    samples, transforms = [], []
    for _ in range(B):
        vid = int(rs.randint(0, len(shapes)))
        s, _, t = lab_aug.draw_sample(vid, int(rs.randint(0, shapes[vid][0])))
        samples.append(s)
        transforms.append(t)
    descs = (_hip.TripletDesc * B)()
    for i, ((vid, zf, zt, zb), (oy, ox, gain, cutoff, k)) in enumerate(zip(samples, transforms)):
        descs[i] = _hip.TripletDesc(lab_aug.offsets[vid], shapes[vid][1], shapes[vid][2], zf, zt, zb, oy, ox, k, gain, cutoff)
    lab_out = torch.empty((3 * B, 2, W, W), device="cuda")
    img_out = torch.empty((3 * B, 1, W, W), device="cuda")
    L, p = _hip.lib, _hip.ptr

    def labelled():
        for _ in range(args.batch):
            L.aesr_labelled_triplet_assemble(p(lab_aug.cache), p(lab_aug.label_cache), descs, B, W, p(lab_out[:2 * B]), p(lab_out[2 * B:]), _hip.stream())

    def plain():
        for _ in range(args.batch):
            L.aesr_triplet_assemble(p(img_aug.cache), descs, B, W, p(img_out[:2 * B]), p(img_out[2 * B:]), _hip.stream())

    for _ in range(3):
        labelled()
        plain()
    torch.cuda.synchronize()
    assert torch.equal(lab_out[:, 0], img_out[:, 0]), "channel 0 of the labelled batch is not the one-channel kernel's"
    t_lab, t_img = [], []
    for _ in range(args.reps):
        t_lab.append(event_time(labelled) / args.batch)
        t_img.append(event_time(plain) / args.batch)
    n = 3 * B * W * W
    print("device: %s; B = %d samples of %d x %d from a %d x %d canvas (%d slices per batch); %d warm-up calls, %d samples; kernel = %d back-to-back "
          "launches / %d, the two kernels alternating" % (torch.cuda.get_device_name(0), B, W, W, args.aug_patch_size, args.aug_patch_size, 3 * B,
                                                          args.warmup, args.reps, args.batch, args.batch))
    print("%-58s | %-26s | %8s %8s | %s" % ("", "med / min / max [us]", "GB/s", "of 8TB/s", "MB moved"))
    row("kernel aesr_labelled_triplet_assemble", t_lab, n * (4 + 1) + n * 8)
    row("kernel aesr_triplet_assemble (one channel)", t_img, n * (4 + 4))
    for name, aug in (("LabelledTripletAugmenter", lab_aug), ("TripletAugmenter", img_aug)):
        trips = samples
        for _ in range(args.warmup):
            aug.assemble(trips, transforms)
            aug.next_batch(B)
        torch.cuda.synchronize()
        row("call   %s.assemble" % name, [event_time(lambda: aug.assemble(trips, transforms)) for _ in range(args.reps)])
        row("call   %s.next_batch" % name, [event_time(lambda: aug.next_batch(B)) for _ in range(args.reps)])
        row("call   %s.next_batch(reuse_output)" % name, [event_time(lambda: aug.next_batch(B, reuse_output=True)) for _ in range(args.reps)])


if __name__ == "__main__":
    main()
