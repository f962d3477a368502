#!/usr/bin/env python
"""What a launch of conv_wgrad_wino_f32 spends outside its tile loop: for three weight-gradient layers of the c2 step (12 triplets), the time
of back-to-back launches (HIP events) and ONE stamped launch (AESR_WGRAD_WINO_DBG=1: wall-clock stamps of every wave's life,
csrc/conv_wgrad_wino.hip).  The prologue / epilogue form is the process's: run once as it is and once with AESR_WGRAD_WINO_LEAN=0.
   wgrad_stamps.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superresolution_aniso_mri_amd import _hip as hip  # noqa: E402
from scripts.bench_conv import timeit  # noqa: E402

L = hip.lib
LAYERS = [("dec.12 32->32 @160 (up2)", 36, 160, 32, 32, 1), ("enc.9 64->64 @81", 24, 81, 64, 64, 0), ("enc.15 128->128 @40", 24, 40, 128, 128, 0)]
print("# AESR_WGRAD_WINO_LEAN=%s" % os.environ.get("AESR_WGRAD_WINO_LEAN", "(default)"), file=sys.stderr, flush=True)
for name, n, h, cin, cout, up2 in LAYERS:
    g = torch.Generator(device="cuda").manual_seed(h + cin)
    x = torch.randn((n, h // 2, h // 2, cin) if up2 else (n, h, h, cin), device="cuda", generator=g)
    dy = torch.randn(n, h, h, cout, device="cuda", generator=g)
    dw, db = torch.empty(cout, cin, 3, 3, device="cuda"), torch.empty(cout, device="cuda")
    ws = torch.empty(L.aesr_conv2d_wgrad_workspace_floats(n, h, h, cin, cout, 3, 1), device="cuda")
    if up2:
        fn = lambda: hip.check(L.aesr_conv2d_wgrad_up2(hip.ptr(x), hip.ptr(dy), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), n, h, h, cin, cout, hip.stream()), "w")
    else:
        fn = lambda: hip.check(L.aesr_conv2d_wgrad(hip.ptr(x), hip.ptr(dy), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), n, h, h, cin, cout, 3, 1, hip.stream()), "w")
    t = timeit(fn, iters=50) * 1e6
    print("%-26s N=%-2d  %6.1f us per call (kernel + slab reduction; events around back-to-back calls)" % (name, n, t), file=sys.stderr, flush=True)
    os.environ["AESR_WGRAD_WINO_DBG"] = "1"
    for _ in range(3):              # three stamped launches: the phases of a launch vary with what the memory system does
        fn()
        torch.cuda.synchronize()
    del os.environ["AESR_WGRAD_WINO_DBG"]
