#!/usr/bin/env python
"""Every library call the engine makes, as text: for refactors of superresolution_aniso_mri_amd/engine.py, which must not move a call, an
argument or a tensor.

    python scripts/launch_dump.py [-o dump.txt]          # the launch dump: needs no device
    python scripts/launch_dump.py --run [--root DIR]     # the same cases for real on cuda:0: one sha256 per case

The dump runs small stacks (encoder and decoder blocks, eval passes, stacks without BatchNorm, stride-2, small-Cin, 8 / 16 channels,
AESR_WINO=0, the data-parallel routes, a deferred-reduction block) forward and backward on CPU tensors with these substitutions:
``engine.lib`` records every launching entry point and returns 0 (the host-only queries *_supported / *_floats / *_words / *_kernel go to the
real library); ``engine.stream`` gives None; ``engine.ptr`` keeps every tensor it is given alive, so no address is used twice;
``_hip.require_gpu_tensor`` accepts CPU tensors; no stream is "capturing"; ``engine.PROFILER`` records (kind, flops, bytes) and the nesting.
aesr_bn_fused1_supported is the one query whose answer the device decides (csrc/bn_fused.hip: bf_device_ok): every case FORCES it, through
the recorder, so that the dump is the same on every machine and both answers are dumped; a case may force aesr_bn_fused_supported too.

A recorded call prints its name, every scalar, and every pointer as a symbol: the tensors a case made by name (input, gout, parameters and
buffers by state_dict key, grad:<key>), any other tensor as t<k>[elements] in the order of first appearance in the dump, a pointer into a
tensor as name+bytes, NULL, and UNKNOWN (an error) for an address no known tensor holds; host arrays (nstart, counts, PrepJob / WgradReduceJob tables) by
content.  The tool fails unless its cases reach every launching entry point engine.py names.

Two engines make the same calls when their dumps are equal byte for byte.  tests/golden/engine_launches.txt is the dump of the engine BEFORE
its routes moved into one function per step kind; to reproduce it check out that commit (the parent of the one that added this file), copy
this file into scripts/ and run it.  tests/test_engine_launches.py compares a fresh dump with the stored one.

--run launches the same cases on the GPU (no recorder, no forced answers, fixed seeds; the cases marked dump-only are left out) and prints one
sha256 per case over the output, the input gradient, every parameter gradient and the BatchNorm buffers.  --root DIR imports the package
from DIR instead of this checkout (another version of the Python layer over the same library, with AESR_LIB naming the library)."""
import argparse
import ctypes
import hashlib
import os
import re
import sys
from ctypes import c_void_p

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY = ("_supported", "_floats", "_words", "_kernel")
SWITCHES = ("FUSE_STEM", "FUSE_COUT1_BWD", "BN_POOL_ONCE", "USE_WINO", "FOLD_UPSAMPLE", "FUSE_EVAL_BN")          # of engine.py: all on by default


class Recorder:
    """stands in for engine.lib, engine.ptr and engine.PROFILER of one case"""

    def __init__(self, engine, real, out):
        self.engine, self.real, self.out = engine, real, out
        self.forced = {}
        self.storages = {}       # storage address -> (tensor kept alive, bytes, elements)
        self.names = {}          # storage address -> symbol
        self.nanon = 0
        self.lines = []
        self.depth = 0
        self.open = []
        self.called = set()

    # ---- engine.ptr ----
    def keep(self, t, name=None):
        st = t.untyped_storage()
        base = st.data_ptr()
        if base and base not in self.storages:
            self.storages[base] = (t, st.nbytes(), st.nbytes() // t.element_size())
        if name is not None and base:
            self.names[base] = name
        return t

    def ptr(self, t):
        if t is None:
            return None
        self.keep(t)
        return c_void_p(t.data_ptr())

    # ---- symbols ----
    def _find(self, addr):
        for base, (_, nbytes, _) in self.storages.items():
            if base <= addr < base + nbytes:
                return base
        return None

    def sym(self, addr):
        if isinstance(addr, c_void_p):
            addr = addr.value
        if not addr:
            return "NULL"
        base = self._find(addr)
        if base is None:
            return "UNKNOWN"
        if base not in self.names:
            self.names[base] = "t%d[%d]" % (self.nanon, self.storages[base][2])
            self.nanon += 1
        return self.names[base] + ("+%d" % (addr - base) if addr != base else "")

    def fmt(self, a):
        if a is None or isinstance(a, c_void_p):
            return self.sym(a)
        if isinstance(a, ctypes.Array):
            if issubclass(a._type_, ctypes.Structure):
                return "[" + ", ".join("{" + " ".join("%s=%s" % (f, self.sym(getattr(j, f)) if t is c_void_p else getattr(j, f))
                                                      for f, t in j._fields_) + "}" for j in a) + "]"
            if a._type_ is c_void_p:
                return "[" + ", ".join(self.sym(v) for v in a) + "]"
            return "[" + ", ".join(repr(v) for v in a) + "]"
        if isinstance(a, (bool, int, float)):
            return repr(a)
        raise TypeError("argument of type %s in a library call" % type(a))

    def line(self, text, args=None):
        self.lines.append((self.depth, text, args))

    def flush(self):
        """Symbols are given when the case is over: a job table carries addresses (data_ptr()) of tensors that no ptr() has seen yet -- the
        operands of the steps, the gradients a pass returns -- which the harness has handed to ``keep`` by then."""
        for depth, text, args in self.lines:
            self.out.append("  " * depth + (text if args is None else "%s(%s)" % (text, ", ".join(self.fmt(a) for a in args))))
        self.lines = []

    # ---- engine.lib ----
    def __getattr__(self, name):
        if name.endswith(QUERY):
            if name in self.forced:
                return lambda *a: self.forced[name]
            return getattr(self.real, name)
        getattr(self.real, name)          # a name the library does not have is an error here too

        def call(*args):
            self.called.add(name)
            self.line(name, args)
            return 0
        return call

    # ---- engine.PROFILER ----
    def begin(self, kind, flops, nbytes=0.0):
        self.line("[ %s flops=%r bytes=%r" % (kind, float(flops), float(nbytes)))
        self.depth += 1
        self.open.append(kind)
        return len(self.open) - 1

    def end(self, record=None):
        kind = self.open.pop()
        if record is not None and record != len(self.open):
            raise RuntimeError("profiler record %r closed while %d are open" % (record, len(self.open) + 1))
        self.depth -= 1
        self.line("] %s" % kind)


class FakePeers:
    """what the engine reads of parallel.PeerExchange"""

    def __init__(self, T):
        self.peers, self.world, self.rank, self.nscale = (c_void_p * 2)(), 2, 0, 1.0
        self.gen = T.named("p2p.gen", torch.zeros(1, dtype=torch.int32))
        self.slot = 0

    def next_slot(self):
        self.slot += 1
        return self.slot - 1


# ---- the stacks -----------------------------------------------------------------------------------------------------
def encoder():
    return nn.Sequential(nn.Conv2d(1, 32, 1, padding=1), nn.Conv2d(32, 32, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(32, 32, 3, padding=1),
                         nn.LeakyReLU(0.01), nn.BatchNorm2d(32), nn.AvgPool2d(2))


def decoder():
    return nn.Sequential(nn.Conv2d(32, 32, 3, padding=1), nn.LeakyReLU(0.01), nn.BatchNorm2d(32), nn.Upsample(scale_factor=2, mode="nearest"),
                         nn.Conv2d(32, 32, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(32, 1, 3, padding=1), nn.Sigmoid())


def wide():          # 64 channels, BatchNorm without resampling behind it
    return nn.Sequential(nn.Conv2d(32, 64, 3, padding=1), nn.LeakyReLU(0.01), nn.BatchNorm2d(64), nn.Conv2d(64, 32, 3, padding=1), nn.ReLU())


def plain():         # no BatchNorm: stand-alone pooling and bilinear upsampling, 8 and 16 channels
    return nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.LeakyReLU(0.01), nn.AvgPool2d(2), nn.Conv2d(16, 16, 3, padding=1), nn.LeakyReLU(0.01),
                         nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False), nn.Conv2d(16, 8, 3, padding=1), nn.ReLU())


def strided():
    return nn.Sequential(nn.Conv2d(4, 8, 2, stride=2), nn.BatchNorm2d(8), nn.Conv2d(8, 16, 2, stride=2), nn.Conv2d(16, 8, 1), nn.ReLU())


def smallcin():      # a 2-channel 1x1 stem behind two 2 -> 2 layers
    return nn.Sequential(nn.Conv2d(2, 2, 1), nn.LeakyReLU(0.01), nn.Conv2d(2, 2, 1), nn.Conv2d(2, 32, 1, padding=1),
                         nn.Conv2d(32, 32, 3, padding=1), nn.LeakyReLU(0.01))


def odd_thin():      # a single-output 3x3 convolution whose input channels are no 4 * 2^k: where the thin-convolution predicates differ
    return nn.Sequential(nn.Conv2d(32, 12, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(12, 1, 3, padding=1), nn.Sigmoid())


class Harness:
    """one case: its tensors, its switches, what it keeps for the hashes"""

    def __init__(self, engine, run, rec, seed):
        self.engine, self.run, self.rec = engine, run, rec
        self.gen = torch.Generator().manual_seed(seed)
        self.kept = []
        self.runners = []
        self.saved_attrs = []
        self.saved_env = {}
        torch.manual_seed(seed)
        self.switch(**{k: True for k in SWITCHES})          # whatever AESR_* the process was started with

    def named(self, name, t):
        if self.run:
            t = t.cuda()
        else:
            self.rec.keep(t, name)
        return t

    def randn(self, name, *shape):
        return self.named(name, torch.randn(*shape, generator=self.gen))

    def switch(self, **kw):
        for k, v in kw.items():
            self.saved_attrs.append((k, getattr(self.engine, k)))
            setattr(self.engine, k, v)

    def force(self, one_launch, allreduce_fused=None):
        """the answers of the device-decided query (and of aesr_bn_fused_supported); for real, only AESR_BN_FUSED=0 can say no"""
        if self.run:
            self.saved_env.setdefault("AESR_BN_FUSED", os.environ.get("AESR_BN_FUSED"))
            os.environ["AESR_BN_FUSED"] = "1" if one_launch else "0"
            return
        self.rec.forced["aesr_bn_fused1_supported"] = int(one_launch)
        if allreduce_fused is not None:
            self.rec.forced["aesr_bn_fused_supported"] = int(allreduce_fused)

    def restore(self):
        for k, v in reversed(self.saved_attrs):
            setattr(self.engine, k, v)
        for k, v in self.saved_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def runner(self, build, prefix="", fresh_grads=False):
        seq = build()
        with torch.no_grad():
            for m in seq:
                if isinstance(m, nn.BatchNorm2d):      # away from gamma = 1, beta = 0, mean = 0, var = 1
                    m.weight.copy_(torch.rand(m.weight.shape, generator=self.gen) + 0.5)
                    m.bias.copy_(torch.randn(m.bias.shape, generator=self.gen) * 0.2)
                    m.running_mean.copy_(torch.randn(m.bias.shape, generator=self.gen) * 0.1)
                    m.running_var.copy_(torch.rand(m.bias.shape, generator=self.gen) + 0.5)
        if self.run:
            seq = seq.cuda()
        for k, t in seq.state_dict(keep_vars=True).items():
            if not self.run:
                self.rec.keep(t, prefix + k)
            if fresh_grads and isinstance(t, nn.Parameter):          # as after HipAdam.zero_grad: gradients go straight into p.grad
                t.grad = torch.zeros_like(t)
                t._aesr_grad_fresh = True
                if not self.run:
                    self.rec.keep(t.grad, "grad:" + prefix + k)
        r = self.engine.SequentialRunner(seq)
        self.runners.append(r)
        return r

    def note(self, text):
        if not self.run:
            self.rec.line("-- " + text)

    def forward(self, r, x, nstart, train, save, **kw):
        self.note("forward train=%d save=%d %s" % (train, save, " ".join("%s=%r" % kv for kv in sorted(kw.items()))))
        out, saved, steps = r.forward(x, nstart, train, save, **kw)
        self.note("-> %s, steps %s" % (tuple(out.shape), " ".join(s.kind for s in steps)))
        self.kept.append(out)
        return out, saved, steps

    def backward(self, r, out, saved, nstart, ngrad, need_input_grad, steps, name="gout"):
        gout = self.randn(name, *out.shape)
        self.note("backward ngrad=%d need_input_grad=%d" % (ngrad, need_input_grad))
        dx, grads = r.backward(gout, saved, nstart, ngrad, need_input_grad, steps=steps)
        if not self.run:
            for t in grads.values():
                if t is not None:
                    self.rec.keep(t)
        self.note("-> dx %s" % (None if dx is None else tuple(dx.shape),))
        self.kept.append(dx)
        for p in r.params:
            self.kept.append(grads.get(p) if grads.get(p) is not None else p.grad)
        self.kept += [b for b in r.seq.buffers()]
        return dx

    def train_pass(self, build, shape, nstart, fused=True, need_input_grad=False, ngrad=None, dirty=False, sync=None, fresh_grads=False, prefix=""):
        r = self.runner(build, prefix, fresh_grads)
        if sync in ("allreduce", "p2p"):
            r.sync_bn = lambda sums: self.note("sync_bn(%s)" % (tuple(sums.shape),))
        if sync == "p2p":
            r.sync_p2p = FakePeers(self)
        x = self.randn(prefix + "input", *shape)
        out, saved, steps = self.forward(r, x, nstart, True, True, fused=fused)
        if dirty:
            self.note("mark_weights_dirty")
            r.mark_weights_dirty()
        self.backward(r, out, saved, nstart, shape[0] if ngrad is None else ngrad, need_input_grad, steps, prefix + "gout")
        return r

    def eval_pass(self, build, shape, nstart, **kw):
        r = self.runner(build)
        x = self.randn("input", *shape)
        self.forward(r, x, nstart, True, False)                     # running statistics exist
        self.forward(r, x, nstart, False, False, **kw)
        self.forward(r, x, nstart, False, False, **kw)              # the eval-mode scale / shift cache answers
        return r


ENC10, ENC4 = ((10, 21, 19, 1), (0, 7, 10)), ((4, 20, 18, 1), (0, 2, 4))
DEC10, DEC4 = ((10, 10, 9, 32), (0, 7, 10)), ((4, 11, 9, 32), (0, 2, 4))


def cases():
    """(name, function of the harness, also for real?)"""
    C = []

    def add(name, fn, real=True):
        C.append((name, fn, real))

    for tag, (shape, ns) in (("10", ENC10), ("4", ENC4)):
        for pool_once in (1, 0):
            for one in (0, 1):
                def f(T, shape=shape, ns=ns, pool_once=pool_once, one=one):
                    T.switch(BN_POOL_ONCE=bool(pool_once))
                    T.force(one)
                    T.train_pass(encoder, shape, ns)
                add("encoder n%s fused-stem pool_once=%d one_launch=%d" % (tag, pool_once, one), f)

                def f(T, shape=shape, ns=ns, pool_once=pool_once, one=one):
                    T.switch(BN_POOL_ONCE=bool(pool_once))
                    T.force(one)
                    T.train_pass(encoder, shape, ns, fused=False, need_input_grad=True)
                add("encoder n%s unfused input-grad pool_once=%d one_launch=%d" % (tag, pool_once, one), f)

    def f(T):
        T.force(0)
        T.train_pass(encoder, ENC10[0], ENC10[1], ngrad=7)
    add("encoder n10 gradients for the first group only", f)

    for tag, (shape, ns) in (("10", DEC10), ("4", DEC4)):
        for cout1 in (1, 0):
            for fold in (1, 0):
                def f(T, shape=shape, ns=ns, cout1=cout1, fold=fold, one=int(tag == "4")):
                    T.switch(FUSE_COUT1_BWD=bool(cout1), FOLD_UPSAMPLE=bool(fold))
                    T.force(one)
                    T.train_pass(decoder, shape, ns, need_input_grad=True)
                add("decoder n%s fuse_cout1_bwd=%d fold_upsample=%d" % (tag, cout1, fold), f)
    for cout1 in (1, 0):
        def f(T, cout1=cout1):
            T.switch(FUSE_COUT1_BWD=bool(cout1))
            T.force(0)
            T.train_pass(decoder, DEC4[0], DEC4[1], need_input_grad=True, dirty=True)
        add("decoder n4 weights marked dirty between forward and backward fuse_cout1_bwd=%d" % cout1, f)

    def f(T):
        T.force(0)
        T.train_pass(decoder, DEC4[0], DEC4[1], need_input_grad=False, fresh_grads=True)
    add("decoder n4 gradients straight into p.grad, no input gradient", f)

    for one in (0, 1):
        def f(T, one=one):
            T.force(one)
            T.train_pass(wide, (3, 9, 7, 32), (0, 3), need_input_grad=True)
        add("wide n3 one_launch=%d" % one, f)

    # eval passes
    for fuse in (1, 0):
        def f(T, fuse=fuse):
            T.switch(FUSE_EVAL_BN=bool(fuse))
            T.force(0)
            T.eval_pass(encoder, (3, 21, 19, 1), (0, 3))
        add("eval encoder fuse_eval_bn=%d" % fuse, f)

        def f(T, fuse=fuse):
            T.switch(FUSE_EVAL_BN=bool(fuse))
            T.force(0)
            T.eval_pass(decoder, (3, 10, 9, 32), (0, 3))
        add("eval decoder fuse_eval_bn=%d" % fuse, f)

        def f(T, fuse=fuse):
            T.switch(FUSE_EVAL_BN=bool(fuse))
            T.force(0)
            T.eval_pass(wide, (3, 9, 7, 32), (0, 3))
        add("eval wide fuse_eval_bn=%d" % fuse, f)

    def f(T):
        T.force(0)
        T.eval_pass(encoder, ENC4[0], ENC4[1])
    add("eval encoder two groups", f)

    def f(T):
        T.force(0)
        r = T.runner(decoder)
        x = T.randn("input", 3, 10, 9, 32)
        T.forward(r, x, (0, 3), True, False)
        z, _, _ = T.forward(r, x, (0, 3), False, False, first=0, last=1, raw_last=True)
        T.forward(r, z, (0, 3), False, False, first=1)
        T.forward(r, x, (0, 3), False, False, raw_last=True, first=0, last=4)
    add("eval decoder partial passes, raw_last", f)

    # other stacks
    def f(T):
        T.train_pass(plain, (3, 20, 18, 8), (0, 3), need_input_grad=True)
    add("plain: stand-alone AvgPool and bilinear Upsample, 8 / 16 channels", f)

    def f(T):
        T.force(0)
        T.train_pass(strided, (3, 24, 20, 4), (0, 2, 3), need_input_grad=True)
    add("strided: 2x2 stride-2 convolutions", f)

    def f(T):
        T.train_pass(smallcin, (3, 9, 7, 2), (0, 3), need_input_grad=True)
    add("smallcin: 2-channel layers with an input gradient", f, real=False)          # the library takes no 2-channel weight gradient

    def f(T):
        T.train_pass(smallcin, (3, 9, 7, 2), (0, 3), need_input_grad=False)
    add("smallcin: no input gradient", f, real=False)

    def f(T):
        T.train_pass(odd_thin, (2, 9, 7, 32), (0, 2), need_input_grad=True)
    add("odd_thin: 12 -> 1 channels", f, real=False)

    for build, (shape, ns), tag in ((encoder, ENC4, "encoder"), (decoder, DEC4, "decoder")):
        def f(T, build=build, shape=shape, ns=ns):
            T.switch(USE_WINO=False)
            T.force(0)
            T.train_pass(build, shape, ns, need_input_grad=build is decoder)
        add("AESR_WINO=0 %s" % tag, f)

    def f(T):
        T.switch(FUSE_STEM=False)
        T.force(0)
        T.train_pass(encoder, ENC4[0], ENC4[1])
    add("AESR_FUSE_STEM=0 encoder", f)

    # data-parallel routes in one process
    for build, (shape, ns), tag in ((encoder, ENC4, "encoder"), (decoder, DEC4, "decoder")):
        for fused in (1, 0):
            def f(T, build=build, shape=shape, ns=ns, fused=fused):
                T.force(0, allreduce_fused=fused)
                T.train_pass(build, shape, ns, need_input_grad=build is decoder, sync="allreduce")
            add("sync_bn %s finalize_apply=%d" % (tag, fused), f, real=bool(fused))

        def f(T, build=build, shape=shape, ns=ns):
            T.force(1)
            T.train_pass(build, shape, ns, need_input_grad=build is decoder, sync="p2p")
        add("sync_p2p %s" % tag, f, real=False)

    def f(T):
        T.force(0, allreduce_fused=1)
        r = T.runner(encoder)
        r.sync_bn = lambda sums: None
        T.forward(r, T.randn("input", 3, 21, 19, 1), (0, 3), False, False)
    add("sync_bn eval encoder", f)

    # a deferred-reduction block around two passes
    for fresh in (1, 0):
        def f(T, fresh=fresh):
            T.force(0)
            enc, dec = T.runner(encoder, "enc.", bool(fresh)), T.runner(decoder, "dec.", bool(fresh))
            xe, xd = T.randn("enc.input", *ENC4[0]), T.randn("dec.input", *DEC4[0])
            oe, se, ste = T.forward(enc, xe, ENC4[1], True, True)
            od, sd, std = T.forward(dec, xd, DEC4[1], True, True)
            T.note("deferred_wgrad_reductions: open")
            with T.engine.deferred_wgrad_reductions():
                T.backward(dec, od, sd, DEC4[1], 4, True, std, "dec.gout")
                T.backward(enc, oe, se, ENC4[1], 4, False, ste, "enc.gout")
                T.note("deferred_wgrad_reductions: close")
        add("deferred reductions fresh_grads=%d" % fresh, f)
    return C


def named_entry_points(engine):
    """the launching entry points engine.py names: as lib.NAME(...) or as launch("NAME", ...)"""
    src = open(engine.__file__.replace(".pyc", ".py")).read()
    return sorted(n for n in set(re.findall(r"(?:\blib\.|\blaunch\(\s*\")(aesr_[a-z0-9_]+)", src)) if not n.endswith(QUERY))


def load(root):
    sys.path.insert(0, os.path.abspath(root))
    try:
        from superresolution_aniso_mri_amd import _hip, engine
    finally:
        sys.path.pop(0)          # the importing process (a test run) keeps its own path
    if os.path.dirname(os.path.dirname(os.path.abspath(engine.__file__))) != os.path.abspath(root):
        raise RuntimeError("the package came from %s, not from %s" % (engine.__file__, root))
    return _hip, engine


def dump(root=ROOT):
    """the launch dump as text; raises when a launching entry point of engine.py is not reached"""
    _hip, engine = load(root)
    saved = (engine.lib, engine.ptr, engine.stream, engine.PROFILER, _hip.require_gpu_tensor, torch.cuda.is_current_stream_capturing,
             os.environ.pop("AESR_BN_FUSED", None))
    out, called = [], set()
    try:
        _hip.require_gpu_tensor = lambda t, name, dtype=torch.float32: t
        torch.cuda.is_current_stream_capturing = lambda: False
        engine.stream = lambda: None
        for k, (name, fn, real) in enumerate(cases()):
            rec = Recorder(engine, saved[0], out)
            engine.lib, engine.ptr, engine.PROFILER = rec, rec.ptr, rec
            T = Harness(engine, False, rec, 100 + k)
            out.append("==== %s%s" % (name, "" if real else " (dump only)"))
            try:
                fn(T)
            finally:
                T.restore()
            for r in T.runners:          # the operands the steps hold
                for s in r.steps + (r.steps_fused or []):
                    for t in vars(s).values():
                        if isinstance(t, torch.Tensor):
                            rec.keep(t)
            rec.flush()
            if rec.open:
                raise RuntimeError("%s: profiler records left open: %s" % (name, rec.open))
            called |= rec.called
    finally:
        engine.lib, engine.ptr, engine.stream, engine.PROFILER, _hip.require_gpu_tensor, torch.cuda.is_current_stream_capturing = saved[:6]
        if saved[6] is not None:
            os.environ["AESR_BN_FUSED"] = saved[6]
    if any("UNKNOWN" in l for l in out):
        raise RuntimeError("addresses no known tensor holds: %s" % [l for l in out if "UNKNOWN" in l][:3])
    named = named_entry_points(engine)
    missed = [n for n in named if n not in called]
    if missed or not named:
        raise RuntimeError("the cases do not reach %s" % (missed or "anything: no entry point found in engine.py"))
    out.append("==== %d cases reach the %d launching entry points engine.py names: %s" % (len(cases()), len(named), " ".join(named)))
    return "\n".join(out) + "\n"


def run(root):
    _hip, engine = load(root)
    torch.cuda.set_device(0)
    every = hashlib.sha256()
    for k, (name, fn, real) in enumerate(cases()):
        if not real:
            continue
        T = Harness(engine, True, None, 100 + k)
        try:
            fn(T)
        except RuntimeError as e:
            # a call the library's host code refuses before it launches (AESR_ERR_ARG 1, AESR_ERR_UNSUPPORTED 3) is a result like any other; a HIP
            # error (code 2) or anything else ends the run: nothing more is started on a device that may have faulted
            if re.search(r"failed \(code (1|3)\)", str(e)) is None:
                raise
            print("%-64s  %s" % ("refused: " + str(e)[:54], name), flush=True)
            continue
        finally:
            T.restore()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in T.kept:
            h.update(b"none" if t is None else t.detach().cpu().contiguous().numpy().tobytes())
        every.update(h.digest())
        print("%s  %s" % (h.hexdigest(), name), flush=True)
    _hip.check_device_watchdogs("launch_dump --run")
    print("%s  all cases" % every.hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.run:
        run(args.root)
        return 0
    text = dump(args.root)
    if args.out:
        open(args.out, "w").write(text)
    print("%d cases, %d lines, sha256 %s" % (len(cases()), text.count("\n"), hashlib.sha256(text.encode()).hexdigest()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
