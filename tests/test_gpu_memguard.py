"""-m gpu: does a kernel touch only the memory it was given, and depend only on the memory it was told to read?

Every launch entry point of include/aesr_hip.h is called through the C ABI on buffers placed between guard bands (tests/memguard.py), each
buffer at EXACTLY its contractual size (output shape, the matching *_workspace_* query, or the documented constant).  Per case, four legs,
each on a fresh set of buffers:

  1. outputs and scratch poisoned with a NaN pattern, all pointers 16-byte aligned: rc == 0, every guard intact, every `const` input bit
     for bit unchanged, every output element written, outputs against an fp64 CPU reference at the tolerance of the op's existing test
     (cited at the case), caller-zeroed state back at its documented value;
  2. the same with a large FINITE poison (a NaN read from scratch can be masked away by a max / select; 3e38 cannot): outputs bit-identical
     to leg 1;
  3. cases with caller-zeroed state (aesr_mse3_fwd workspace, Adam state, one-launch BatchNorm barrier words): a second call on the same,
     not re-zeroed state gives bit-identical outputs (Adam: the correct second step);
  4. offset pointers: (p) every parameter-class buffer (weights, biases, gamma / beta, running statistics, weight gradients, Adam buffers)
     starts 4 bytes after a 16-byte boundary, as ops.HipAdam's flat buffers place them -- must work, bit-identical to leg 1; (t) every
     tensor-class buffer (activations, images, workspaces) does -- either bit-identical to leg 1, or refused with a message that names the
     alignment and nothing written.  Never a third outcome.

What a green run does NOT say: out-of-range READS are invisible to guard bands (a guard is not changed by a read), and so is a store
that lands 4 096 elements or more away from its buffer.

The case table and EXEMPT partition _hip.SIGNATURES (tests/test_abi.py checks that without a GPU).
"""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memguard as mg
from superresolution_aniso_mri_amd import _hip as hip

pytestmark = pytest.mark.gpu
L_ = hip.lib
f32, f64 = torch.float32, torch.float64

# name -> reason.  Only pure host queries (no device pointer) and the entry points that need a peer or a communicator may stand here.
EXEMPT = {
    "aesr_version": "host query", "aesr_last_error_string": "host query",
    "aesr_conv2d_packed_floats": "host query", "aesr_conv2d_workspace_floats": "host query", "aesr_conv2d_dgrad_workspace_floats": "host query",
    "aesr_conv2d_wgrad_workspace_floats": "host query", "aesr_small_wgrad_workspace_floats": "host query",
    "aesr_conv2d_cout1_workspace_floats": "host query", "aesr_stemconv_folded_floats": "host query", "aesr_stemconv_workspace_floats": "host query",
    "aesr_bn_fused_supported": "host query", "aesr_bn_fused1_supported": "host query", "aesr_bn_fused1_workspace_floats": "host query",
    "aesr_bn_fused1_barrier_words": "host query", "aesr_bn_fused1_timeouts": "host query (reads a device symbol of the library itself)",
    "aesr_ssim_workspace_doubles": "host query", "aesr_vif_workspace_bytes": "host query", "aesr_adam_state_init": "fills a HOST array, no launch",
    "aesr_conv2d_wino_supported": "host query", "aesr_conv2d_wino_kernel": "host query",
    "aesr_conv2d_wino_ring_timeouts": "host query (reads a device symbol of the library itself)", "aesr_conv2d_wino_packed_floats": "host query",
    "aesr_conv2d_wino_workspace_floats": "host query", "aesr_conv2d_wino_fwd_bn_supported": "host query", "aesr_conv2d_wgrad_up2_supported": "host query",
    "aesr_p2p_alloc": "needs a peer", "aesr_p2p_free": "needs a peer", "aesr_p2p_get_handle": "needs a peer", "aesr_p2p_open": "needs a peer",
    "aesr_p2p_close": "needs a peer", "aesr_p2p_region_bytes": "host query", "aesr_p2p_tick": "needs a peer (the generation word of a peer exchange)",
    "aesr_bn_fused1_fwd_p2p": "needs a peer", "aesr_bn_fused1_bwd_p2p": "needs a peer",
    "aesr_comm_rccl_version": "needs a communicator", "aesr_comm_unique_id": "needs a communicator", "aesr_comm_init": "needs a communicator",
    "aesr_comm_destroy": "needs a communicator", "aesr_comm_abort": "needs a communicator", "aesr_comm_allreduce": "needs a communicator",
    "aesr_comm_allreduce_many": "needs a communicator", "aesr_comm_broadcast": "needs a communicator",
}


# ---- the leg: a set of guarded buffers --------------------------------------------------------------------------------------------------
class Leg:
    def __init__(self, poison, shift_param=0, shift_tensor=0):
        self.poison, self.sp, self.st = poison, shift_param, shift_tensor
        self.bufs = {}
        self.keep = []

    def _add(self, name, role, cls, n, dtype, fill, untouched=None):
        assert name not in self.bufs and cls in ("param", "tensor")
        g = mg.guarded(n, dtype, "cuda", fill, self.sp if cls == "param" else self.st, name)
        self.bufs[name] = types.SimpleNamespace(g=g, role=role, cls=cls, saved=None, untouched=untouched, dtype=dtype)
        return ctypes.c_void_p(g.view.data_ptr())

    def inp(self, name, t, cls="tensor"):
        t = t.detach().contiguous()
        return self._add(name, "in", cls, t.numel(), t.dtype, t)

    def out(self, name, n, cls="tensor", dtype=f32, untouched=None):
        return self._add(name, "out", cls, n, dtype, self.poison, untouched)

    def scratch(self, name, n, cls="tensor", dtype=f32):
        return self._add(name, "scratch", cls, n, dtype, self.poison)

    def state(self, name, t, cls="tensor"):
        t = t.detach().contiguous()
        return self._add(name, "state", cls, t.numel(), t.dtype, t)

    def inout(self, name, t, cls="param"):
        t = t.detach().contiguous()
        return self._add(name, "inout", cls, t.numel(), t.dtype, t)

    def v(self, name):
        return self.bufs[name].g.view

    def at(self, name, elem):
        """Pointer to element `elem` of a buffer (two arguments that are parts of one tensor, as ops.py passes flat[n1:])."""
        v = self.v(name)
        return ctypes.c_void_p(v.data_ptr() + elem * v.element_size())

    def freeze(self):
        for b in self.bufs.values():
            if b.role in ("in", "inout", "state"):
                b.saved = mg.bits(b.g.view)

    def repoison(self):
        for b in self.bufs.values():
            if b.role in ("out", "scratch"):
                fresh = mg.guarded(b.g.view.numel(), b.dtype, "cuda", self.poison)
                b.g.view.copy_(fresh.view)
            elif b.role == "inout":
                kind = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[b.g.view.element_size()]
                b.g.view.view(kind).copy_(b.saved.cuda())

    def result_bits(self):
        return {k: mg.bits(b.g.view) for k, b in self.bufs.items() if b.role in ("out", "inout")}


class SubLeg:
    """A case's buffers under a name prefix inside another leg (composite cases); the names in `shared` are one buffer for all members."""

    def __init__(self, leg, prefix, shared=()):
        self.leg, self.prefix, self.shared = leg, prefix, shared

    def _name(self, name):
        return name if name in self.shared else self.prefix + name

    def inp(self, name, *a, **k):
        return self.leg.inp(self._name(name), *a, **k)

    def out(self, name, *a, **k):
        return self.leg.out(self._name(name), *a, **k)

    def scratch(self, name, *a, **k):
        return self.leg.scratch(self._name(name), *a, **k)

    def inout(self, name, *a, **k):
        return self.leg.inout(self._name(name), *a, **k)

    def state(self, name, *a, **k):
        if name in self.shared and name in self.leg.bufs:
            return ctypes.c_void_p(self.leg.v(name).data_ptr())
        return self.leg.state(self._name(name), *a, **k)

    def v(self, name):
        return self.leg.v(self._name(name))

    def at(self, name, elem):
        return self.leg.at(self._name(name), elem)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def close(leg, name, ref, tol, what="rel"):
    got = leg.v(name).cpu()
    ref = torch.as_tensor(ref).reshape(-1)
    assert got.numel() == ref.numel(), (name, got.numel(), ref.numel())
    if what == "rel":
        e = rel_l2(got, ref)
        assert e < tol, "%s: rel-L2 %.3g (bound %.3g)" % (name, e, tol)
    elif what == "eq":
        assert torch.equal(got, ref.to(got.dtype)), "%s: not bit-equal to the reference expression" % name
    elif what == "abs":
        e = float((got.double() - ref.double()).abs().max())
        assert e < tol, "%s: max abs error %.3g (bound %.3g)" % (name, e, tol)
    else:
        raise AssertionError(what)


def gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def st():
    return hip.stream()


def pack_igemm(w, transpose):
    cout, cin, ks, _ = w.shape
    p = torch.empty(L_.aesr_conv2d_packed_floats(cout, cin, ks, transpose), device="cuda")
    hip.check(L_.aesr_conv2d_pack(hip.ptr(w), hip.ptr(p), cout, cin, ks, transpose, st()), "pack")
    torch.cuda.synchronize()
    return p


def pack_wino(w, transpose):
    cout, cin = w.shape[:2]
    buf = torch.empty(L_.aesr_conv2d_wino_packed_floats(cout, cin, transpose), device="cuda")
    job = (hip.PackJob * 1)(hip.PackJob(w.data_ptr(), buf.data_ptr(), cout, cin, 3, transpose))
    hip.check(L_.aesr_conv2d_wino_pack_many(job, 1, st()), "wino_pack")
    torch.cuda.synchronize()
    return buf


def act_ref(t, act, slope=0.01):
    return {0: t, 1: F.leaky_relu(t, slope), 2: F.relu(t), 3: torch.sigmoid(t)}[act]


def mask_ref(xs, mask_act, slope=0.01):
    if mask_act == 1:
        return torch.where(xs > 0, 1.0, slope).double()
    if mask_act == 2:
        return (xs > 0).double()
    return torch.ones_like(xs).double()


CASES = []
SEEN = {"wino_fwd": set(), "wino_dgrad": set(), "igemm_ksplit": 0, "ring_ksplit": 0, "bn_fused1": 0, "poisons": set(), "ran": set(),
        "legs": 0, "refused": []}


def case(cid, entries, env=None):
    """Decorator: the function builds the buffers of one leg and returns dict(call=..., verify=..., [state_ok=..., reuse=...])."""
    def deco(build):
        CASES.append(types.SimpleNamespace(id=cid, entries=(entries,) if isinstance(entries, str) else tuple(entries), env=env or {}, build=build))
        return build
    return deco


# ---- implicit-GEMM convolutions (tolerances: tests/test_gpu_kernels.py test_conv_fwd / test_conv_dgrad 1e-5, test_conv_wgrad 2e-5) --------
IGEMM_SHAPES = [(1, 1, 1, 16, 32, 3, 1), (3, 7, 9, 16, 32, 3, 1), (2, 33, 35, 8, 16, 3, 1), (1, 20, 20, 16, 1, 3, 1), (2, 17, 19, 16, 32, 1, 0),
                (1, 7, 7, 4, 8, 3, 1), (7, 10, 10, 128, 96, 3, 1), (1, 33, 130, 32, 32, 3, 1), (2, 162, 162, 32, 32, 3, 1), (3, 81, 81, 32, 64, 3, 1),
                (2, 40, 40, 64, 128, 3, 1), (5, 10, 10, 64, 64, 3, 1), (2, 33, 47, 80, 160, 3, 1)]


def _random_shapes(seed, n, cins, couts, ks_choices=((3, 1),), hw=(1, 21), nmax=5):
    """Seeded small layers: odd sizes, partial tiles, channel counts around the kernels' block sizes."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        ks, pad = ks_choices[int(rng.randint(len(ks_choices)))]
        sh = (int(rng.randint(1, nmax + 1)), int(rng.randint(hw[0], hw[1])), int(rng.randint(hw[0], hw[1])), int(rng.choice(cins)), int(rng.choice(couts)), ks, pad)
        if sh not in out:
            out.append(sh)
    return out


IGEMM_SHAPES += [sh for sh in _random_shapes(101, 24, [4, 8, 12, 16, 20, 32, 48], [1, 2, 3, 4, 8, 12, 16, 24, 32, 40, 64, 72], ((3, 1), (1, 0), (3, 0), (3, 2)))
                 if sh[1] + 2 * sh[6] >= sh[5] and sh[2] + 2 * sh[6] >= sh[5] and sh not in IGEMM_SHAPES]
# forced input-channel split: image counts no other test uses (the library caches one tile plan per shape, test_conv_ksplit_workspace_paths)
IGEMM_KSPLIT = [(13, 10, 10, 256, 128, 4), (6, 9, 11, 128, 64, 2)]


def _conv_io(shape, seed):
    N, H, W, Cin, Cout, KS, pad = shape
    g = gen(seed, *shape)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KS, KS, generator=g) / np.sqrt(Cin * KS * KS)
    b = torch.randn(Cout, generator=g)
    return x, w, b, H + 2 * pad - KS + 1, W + 2 * pad - KS + 1


def _igemm_fwd(shape, entry, ws, act=1, bias=True):
    def build(leg):
        N, H, W, Cin, Cout, KS, pad = shape
        x, w, b, Ho, Wo = _conv_io(shape, 1)
        px, pp, pb = leg.inp("in", nhwc(x)), leg.inp("packed", pack_igemm(w.cuda(), 0)), (leg.inp("bias", b, "param") if bias else None)
        po = leg.out("out", N * Ho * Wo * Cout)
        if entry == "aesr_conv2d_fwd":
            call = lambda: L_.aesr_conv2d_fwd(px, pp, pb, po, N, H, W, Cin, Cout, KS, pad, act, 0.01, st())
        else:
            nws = L_.aesr_conv2d_workspace_floats(N, H, W, Cin, Cout, KS, pad)
            if ws == "forced":
                assert nws == int(leg_env["AESR_IGEMM_KSPLIT"]) * N * Ho * Wo * Cout > 0, nws
                SEEN["igemm_ksplit"] += 1
            pw = leg.scratch("workspace", nws) if (nws and ws != "null") else None
            call = lambda: L_.aesr_conv2d_fwd_ws(px, pp, pb, po, pw, N, H, W, Cin, Cout, KS, pad, act, 0.01, st())
        ref = lambda: nhwc(act_ref(F.conv2d(x.double(), w.double(), b.double() if bias else None, padding=pad), act))
        return dict(call=call, verify=lambda: close(leg, "out", ref(), 1e-5))
    return build


def _igemm_dgrad(shape, entry, ws, mask_act=1):
    def build(leg):
        N, H, W, Cin, Cout, KS, pad = shape
        g = gen(2, *shape)
        w = torch.randn(Cout, Cin, KS, KS, generator=g) / np.sqrt(Cout * KS * KS)
        Ho, Wo = H + 2 * pad - KS + 1, W + 2 * pad - KS + 1
        dy = torch.randn(N, Cout, Ho, Wo, generator=g)
        xs = torch.randn(N, Cin, H, W, generator=g)
        pdy, pp, pxs = leg.inp("dy", nhwc(dy)), leg.inp("packed_t", pack_igemm(w.cuda(), 1)), (leg.inp("x_saved", nhwc(xs)) if mask_act else None)
        pdx = leg.out("dx", N * H * W * Cin)
        if entry == "aesr_conv2d_dgrad":
            call = lambda: L_.aesr_conv2d_dgrad(pdy, pp, pxs, pdx, N, H, W, Cin, Cout, KS, pad, mask_act, 0.01, st())
        else:
            nws = L_.aesr_conv2d_dgrad_workspace_floats(N, H, W, Cin, Cout, KS, pad)
            if ws == "forced":
                assert nws == int(leg_env["AESR_IGEMM_KSPLIT"]) * N * H * W * Cin > 0, nws
                SEEN["igemm_ksplit"] += 1
            pw = leg.scratch("workspace", nws) if (nws and ws != "null") else None
            call = lambda: L_.aesr_conv2d_dgrad_ws(pdy, pp, pxs, pdx, pw, N, H, W, Cin, Cout, KS, pad, mask_act, 0.01, st())
        ref = lambda: nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), padding=pad) * mask_ref(xs, mask_act))
        return dict(call=call, verify=lambda: close(leg, "dx", ref(), 1e-5))
    return build


leg_env = {}           # the environment of the case that is running (set by the test, read by the builders' assertions)

for s in IGEMM_SHAPES:
    tag = "x".join(map(str, s))
    case("conv_fwd-" + tag, "aesr_conv2d_fwd")(_igemm_fwd(s, "aesr_conv2d_fwd", None, act=3 if s[4] == 1 else 1))
    if s[4] % 4 == 0:
        case("conv_dgrad-" + tag, "aesr_conv2d_dgrad")(_igemm_dgrad(s, "aesr_conv2d_dgrad", None))
for s in [(3, 7, 9, 16, 32, 3, 1), (2, 33, 35, 8, 16, 3, 1), (2, 17, 19, 16, 32, 1, 0), (7, 10, 10, 128, 96, 3, 1)]:           # bias / x_saved may be NULL
    tag = "x".join(map(str, s))
    case("conv_fwd-nobias-" + tag, "aesr_conv2d_fwd")(_igemm_fwd(s, "aesr_conv2d_fwd", None, act=0, bias=False))
    case("conv_dgrad-nomask-" + tag, "aesr_conv2d_dgrad")(_igemm_dgrad(s, "aesr_conv2d_dgrad", None, 0))
for s in [(3, 7, 9, 16, 32, 3, 1), (3, 10, 10, 512, 512, 3, 1)]:
    tag = "x".join(map(str, s))
    case("conv_fwd_ws-query-" + tag, "aesr_conv2d_fwd_ws")(_igemm_fwd(s, "aesr_conv2d_fwd_ws", "query", act=2))
    case("conv_fwd_ws-null-" + tag, "aesr_conv2d_fwd_ws")(_igemm_fwd(s, "aesr_conv2d_fwd_ws", "null", act=2))
    case("conv_dgrad_ws-query-" + tag, "aesr_conv2d_dgrad_ws")(_igemm_dgrad(s, "aesr_conv2d_dgrad_ws", "query", 2))
    case("conv_dgrad_ws-null-" + tag, "aesr_conv2d_dgrad_ws")(_igemm_dgrad(s, "aesr_conv2d_dgrad_ws", "null", 2))
for N, H, W, cin, cout, ks in IGEMM_KSPLIT:
    s = (N, H, W, cin, cout, 3, 1)
    tag = "x".join(map(str, s)) + "-k%d" % ks
    case("conv_fwd_ws-forced-" + tag, "aesr_conv2d_fwd_ws", {"AESR_IGEMM_KSPLIT": ks})(_igemm_fwd(s, "aesr_conv2d_fwd_ws", "forced", act=2))
    sd = (N, H, W, cout, cin, 3, 1)            # the data gradient's K side is Cout: the same channel counts, roles swapped
    case("conv_dgrad_ws-forced-" + tag, "aesr_conv2d_dgrad_ws", {"AESR_IGEMM_KSPLIT": ks})(_igemm_dgrad(sd, "aesr_conv2d_dgrad_ws", "forced", 2))


# ---- weight packing / preparation: verified by USING the packed operand (test_conv_fwd 1e-5) and bitwise against the single-filter entry ----
def _pack_cases():
    def functional_igemm(packed, w, transpose):
        cout, cin, ks, _ = w.shape
        g = gen(3, cout, cin, ks)
        if not transpose:
            x = torch.randn(2, cin, 5, 6, generator=g)
            out = torch.empty(2, 5 + 2 * (ks // 2) - ks + 1, 6 + 2 * (ks // 2) - ks + 1, cout, device="cuda")
            hip.check(L_.aesr_conv2d_fwd(hip.ptr(nhwc(x).cuda()), hip.ptr(packed), None, hip.ptr(out), 2, 5, 6, cin, cout, ks, ks // 2, 0, 0.0, st()), "fwd")
            torch.cuda.synchronize()
            assert rel_l2(out, nhwc(F.conv2d(x.double(), w.double().cpu(), None, padding=ks // 2))) < 1e-5
        else:
            dy = torch.randn(2, cout, 5, 6, generator=g)
            dx = torch.empty(2, 5, 6, cin, device="cuda")
            hip.check(L_.aesr_conv2d_dgrad(hip.ptr(nhwc(dy).cuda()), hip.ptr(packed), None, hip.ptr(dx), 2, 5, 6, cin, cout, ks, ks // 2, 0, 0.0, st()), "dgrad")
            torch.cuda.synchronize()
            assert rel_l2(dx, nhwc(torch.nn.grad.conv2d_input((2, cin, 5, 6), w.double().cpu(), dy.double(), padding=ks // 2))) < 1e-5

    def functional_wino(packed, w, transpose):
        cout, cin = w.shape[:2]
        g = gen(4, cout, cin)
        if not transpose:
            x = torch.randn(2, cin, 5, 6, generator=g)
            out = torch.empty(2, 5, 6, cout, device="cuda")
            hip.check(L_.aesr_conv2d_wino_fwd(hip.ptr(nhwc(x).cuda()), hip.ptr(packed), None, hip.ptr(out), 2, 5, 6, cin, cout, 0, 0.0, st()), "wino")
            torch.cuda.synchronize()
            assert rel_l2(out, nhwc(F.conv2d(x.double(), w.double().cpu(), None, padding=1))) < 1e-5
        else:
            dy = torch.randn(2, cout, 5, 6, generator=g)
            dx = torch.empty(2, 5, 6, cin, device="cuda")
            hip.check(L_.aesr_conv2d_wino_dgrad(hip.ptr(nhwc(dy).cuda()), hip.ptr(packed), None, hip.ptr(dx), 2, 5, 6, cin, cout, 0, 0.0, st()), "wino")
            torch.cuda.synchronize()
            assert rel_l2(dx, nhwc(torch.nn.grad.conv2d_input((2, cin, 5, 6), w.double().cpu(), dy.double(), padding=1))) < 1e-5

    for cout, cin, ks, tr in [(32, 16, 3, 0), (32, 16, 3, 1), (1, 16, 3, 0), (8, 4, 3, 1), (32, 12, 1, 0), (96, 128, 3, 0)]:
        @case("pack-%dx%dx%d-t%d" % (cout, cin, ks, tr), "aesr_conv2d_pack")
        def build(leg, cout=cout, cin=cin, ks=ks, tr=tr):
            w = torch.randn(cout, cin, ks, ks, generator=gen(5, cout, cin, ks))
            pw = leg.inp("w", w, "param")
            pp = leg.out("packed", L_.aesr_conv2d_packed_floats(cout, cin, ks, tr))
            return dict(call=lambda: L_.aesr_conv2d_pack(pw, pp, cout, cin, ks, tr, st()), verify=lambda: functional_igemm(leg.v("packed"), w, tr))

    @case("pack_many", "aesr_conv2d_pack_many")
    def build(leg):
        specs = [(32, 16, 3, 0), (16, 8, 3, 1), (1, 16, 3, 0), (32, 12, 1, 0)] * 9          # 36 jobs: two launches of <= 32
        ws, jobs = [], []
        for k, (cout, cin, ks, tr) in enumerate(specs):
            w = torch.randn(cout, cin, ks, ks, generator=gen(6, k))
            ws.append(w)
            jobs.append(hip.PackJob(leg.inp("w%d" % k, w, "param").value, leg.out("packed%d" % k, L_.aesr_conv2d_packed_floats(cout, cin, ks, tr)).value,
                                    cout, cin, ks, tr))
        arr = (hip.PackJob * len(jobs))(*jobs)

        def verify():
            for k, (cout, cin, ks, tr) in enumerate(specs):
                assert torch.equal(leg.v("packed%d" % k), pack_igemm(ws[k].cuda(), tr)), k
            functional_igemm(leg.v("packed0"), ws[0], 0)
        return dict(call=lambda: L_.aesr_conv2d_pack_many(arr, len(jobs), st()), verify=verify)

    @case("wino_pack_many", "aesr_conv2d_wino_pack_many")
    def build(leg):
        specs = [(32, 16, 0), (16, 32, 1), (96, 48, 0), (64, 64, 1), (160, 80, 0)]
        ws, jobs = [], []
        for k, (cout, cin, tr) in enumerate(specs):
            w = torch.randn(cout, cin, 3, 3, generator=gen(7, k)) / np.sqrt(9 * cin)
            ws.append(w)
            jobs.append(hip.PackJob(leg.inp("w%d" % k, w, "param").value,
                                    leg.out("upacked%d" % k, L_.aesr_conv2d_wino_packed_floats(cout, cin, tr)).value, cout, cin, 3, tr))
        arr = (hip.PackJob * len(jobs))(*jobs)

        def verify():
            for k, (cout, cin, tr) in enumerate(specs):
                functional_wino(leg.v("upacked%d" % k), ws[k], tr)
        return dict(call=lambda: L_.aesr_conv2d_wino_pack_many(arr, len(jobs), st()), verify=verify)

    @case("weight_prep_many", "aesr_weight_prep_many")
    def build(leg):
        """All four kinds, 38 jobs (two launches); test_weight_prep_many_equals_the_separate_launches: bitwise the separate launches."""
        jobs, checks = [], []
        k = 0
        for rep in range(9):
            for cout, cin, ks in [(32, 32, 3), (16, 8, 3), (32, 12, 1)]:
                w = torch.randn(cout, cin, ks, ks, generator=gen(8, k))
                pw = leg.inp("filter%d" % k, w, "param").value
                tr = rep % 2
                if (cout if tr else cin) % 4 == 0:
                    po = leg.out("pack%d" % k, L_.aesr_conv2d_packed_floats(cout, cin, ks, tr)).value
                    jobs.append(hip.PrepJob(pw, None, None, po, hip.PREP_PACK, cout, cin, ks, tr))
                    checks.append(("pack%d" % k, lambda w=w, tr=tr: pack_igemm(w.cuda(), tr)))
                if ks == 3 and L_.aesr_conv2d_wino_supported(cin, cout, 3, 1, tr):
                    po = leg.out("wino%d" % k, L_.aesr_conv2d_wino_packed_floats(cout, cin, tr)).value
                    jobs.append(hip.PrepJob(pw, None, None, po, hip.PREP_WINO_PACK, cout, cin, 3, tr))
                    checks.append(("wino%d" % k, lambda w=w, tr=tr: pack_wino(w.cuda(), tr)))
                k += 1
        g = gen(9)
        wst, bst, w1 = torch.randn(32, generator=g), torch.randn(32, generator=g), torch.randn(32, 32, 3, 3, generator=g)
        po = leg.out("folded", L_.aesr_stemconv_folded_floats(32)).value
        jobs.append(hip.PrepJob(leg.inp("w1", w1, "param").value, leg.inp("w_stem", wst, "param").value, leg.inp("b_stem", bst, "param").value, po,
                                hip.PREP_STEM_FOLD, 32, 32, 3, 0))

        def fold_ref():
            want = torch.empty(L_.aesr_stemconv_folded_floats(32), device="cuda")
            a, b, c = wst.cuda(), bst.cuda(), w1.cuda()
            hip.check(L_.aesr_stemconv_fold(hip.ptr(a), hip.ptr(b), hip.ptr(c), hip.ptr(want), 32, 32, st()), "fold")
            torch.cuda.synchronize()
            return want
        checks.append(("folded", fold_ref))
        wc = torch.randn(1, 32, 3, 3, generator=g)
        jobs.append(hip.PrepJob(leg.inp("wc", wc, "param").value, None, None, leg.out("flipped", 9 * 32).value, hip.PREP_COUT1_FLIP, 1, 32, 3, 0))
        checks.append(("flipped", lambda: wc.reshape(32, 9).flip(1).t().contiguous().cuda()))
        assert len(jobs) > 32
        arr = (hip.PrepJob * len(jobs))(*jobs)

        def verify():
            for name, want in checks:
                assert torch.equal(leg.v(name), want().reshape(-1)), name
        return dict(call=lambda: L_.aesr_weight_prep_many(arr, len(jobs), st()), verify=verify)


_pack_cases()


# ---- Winograd convolutions (test_conv_wino_fwd / _dgrad 1e-5; test_conv_wino_channel_split 1e-5; test_conv_wino_folded_upsample 1e-5 / 2e-5;
#      test_conv_wino_eval_bn_epilogue 2e-6) -----------------------------------------------------------------------------------------
WINO_SHAPES = [(1, 1, 1, 16, 32), (3, 7, 9, 16, 32), (2, 33, 47, 80, 160), (1, 33, 130, 32, 32), (7, 10, 10, 128, 96), (2, 162, 162, 32, 32),
               (2, 81, 81, 64, 64), (3, 81, 81, 32, 64), (2, 40, 40, 128, 64), (5, 10, 10, 64, 64), (2, 2, 3, 48, 96), (3, 40, 40, 64, 128),
               (2, 16, 24, 48, 96), (4, 20, 20, 128, 64), (1, 40, 40, 256, 32), (3, 10, 10, 512, 512)]
WINO_SHAPES += [sh[:5] for sh in _random_shapes(102, 20, [16, 32, 48, 64, 80, 128, 160], [32, 64, 96], hw=(1, 30), nmax=7) if sh[:5] not in WINO_SHAPES]
RING_KSPLIT = [(2, 10, 10, 512, 64, 8), (3, 20, 12, 256, 96, 4), (1, 7, 9, 96, 32, 4), (4, 40, 40, 128, 64, 2), (1, 5, 3, 64, 32, 2)]


def _wino_fwd(shape, entry="aesr_conv2d_wino_fwd", ws=None, act=1, bias=True):
    def build(leg):
        N, H, W, Cin, Cout = shape
        x, w, b, _, _ = _conv_io(shape + (3, 1), 11)
        if entry == "aesr_conv2d_wino_fwd":
            SEEN["wino_fwd"].add(L_.aesr_conv2d_wino_kernel(N, H, W, Cin, Cout, 3, 1, 0))
        px, pu, pb = leg.inp("in", nhwc(x)), leg.inp("upacked", pack_wino(w.cuda(), 0)), (leg.inp("bias", b, "param") if bias else None)
        po = leg.out("out", N * H * W * Cout)
        if entry == "aesr_conv2d_wino_fwd":
            call = lambda: L_.aesr_conv2d_wino_fwd(px, pu, pb, po, N, H, W, Cin, Cout, act, 0.01, st())
        else:
            nws = L_.aesr_conv2d_wino_workspace_floats(N, H, W, Cin, Cout, 0)
            if ws == "forced":
                assert nws >= 2 * N * H * W * Cout, nws
                SEEN["ring_ksplit"] += 1
            if ws == "small":           # "a NULL or smaller workspace is legal: the layer then runs unsplit" -- one slab is too small for any split
                nws = N * H * W * Cout
            pw = leg.scratch("workspace", nws) if (nws and ws != "null") else None
            nws = nws if pw else 0
            call = lambda: L_.aesr_conv2d_wino_fwd_ws(px, pu, pb, po, pw, nws, N, H, W, Cin, Cout, act, 0.01, st())
        ref = lambda: nhwc(act_ref(F.conv2d(x.double(), w.double(), b.double() if bias else None, padding=1), act))
        return dict(call=call, verify=lambda: close(leg, "out", ref(), 1e-5))
    return build


def _wino_dgrad(shape, entry="aesr_conv2d_wino_dgrad", ws=None, mask_act=1):
    def build(leg):
        N, H, W, Cout, Cin = shape            # roles swapped so that the data-gradient constraints (Cout % 16, Cin % 32) hold
        g = gen(12, *shape)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cout * 9)
        dy = torch.randn(N, Cout, H, W, generator=g)
        xs = torch.randn(N, Cin, H, W, generator=g)
        if entry == "aesr_conv2d_wino_dgrad":
            SEEN["wino_dgrad"].add(L_.aesr_conv2d_wino_kernel(N, H, W, Cin, Cout, 3, 1, 1))
        pdy, pu, pxs = leg.inp("dy", nhwc(dy)), leg.inp("upacked_t", pack_wino(w.cuda(), 1)), (leg.inp("x_saved", nhwc(xs)) if mask_act else None)
        pdx = leg.out("dx", N * H * W * Cin)
        if entry == "aesr_conv2d_wino_dgrad":
            call = lambda: L_.aesr_conv2d_wino_dgrad(pdy, pu, pxs, pdx, N, H, W, Cin, Cout, mask_act, 0.01, st())
        else:
            nws = L_.aesr_conv2d_wino_workspace_floats(N, H, W, Cin, Cout, 1)
            if ws == "forced":
                assert nws >= 2 * N * H * W * Cin, nws
                SEEN["ring_ksplit"] += 1
            if ws == "small":
                nws = N * H * W * Cin
            pw = leg.scratch("workspace", nws) if (nws and ws != "null") else None
            nws = nws if pw else 0
            call = lambda: L_.aesr_conv2d_wino_dgrad_ws(pdy, pu, pxs, pdx, pw, nws, N, H, W, Cin, Cout, mask_act, 0.01, st())
        ref = lambda: nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), padding=1) * mask_ref(xs, mask_act))
        return dict(call=call, verify=lambda: close(leg, "dx", ref(), 1e-5))
    return build


for ring in (1, 2):
    for s in [(3, 7, 9, 16, 32), (7, 10, 10, 128, 96), (2, 33, 47, 80, 160)]:           # bias / x_saved may be NULL
        tag = "x".join(map(str, s)) + "-ring%d" % ring
        case("wino_fwd-nobias-" + tag, "aesr_conv2d_wino_fwd", {"AESR_WINO_RING": ring})(_wino_fwd(s, act=0, bias=False))
        case("wino_dgrad-nomask-" + tag, "aesr_conv2d_wino_dgrad", {"AESR_WINO_RING": ring})(_wino_dgrad(s, mask_act=0))
for ring in (1, 2):           # as the streamed_kernel fixture of tests/test_gpu_kernels.py: 1 = the planner's choice, 2 = every streamed layer on the ring kernel
    for s in WINO_SHAPES:
        tag = "x".join(map(str, s)) + "-ring%d" % ring
        case("wino_fwd-" + tag, "aesr_conv2d_wino_fwd", {"AESR_WINO_RING": ring})(_wino_fwd(s))
        case("wino_dgrad-" + tag, "aesr_conv2d_wino_dgrad", {"AESR_WINO_RING": ring})(_wino_dgrad(s))
for N, H, W, cin, cout, S in RING_KSPLIT:
    env = {"AESR_WINO_RING": 2, "AESR_RING_KSPLIT": S}
    tag = "x".join(map(str, (N, H, W, cin, cout))) + "-s%d" % S
    case("wino_fwd_ws-forced-" + tag, "aesr_conv2d_wino_fwd_ws", env)(_wino_fwd((N, H, W, cin, cout), "aesr_conv2d_wino_fwd_ws", "forced"))
    case("wino_fwd_ws-small-" + tag, "aesr_conv2d_wino_fwd_ws", env)(_wino_fwd((N, H, W, cin, cout), "aesr_conv2d_wino_fwd_ws", "small"))
    case("wino_dgrad_ws-small-" + tag, "aesr_conv2d_wino_dgrad_ws", env)(_wino_dgrad((N, H, W, cin, cout), "aesr_conv2d_wino_dgrad_ws", "small", 2))
    case("wino_fwd_ws-null-" + tag, "aesr_conv2d_wino_fwd_ws", env)(_wino_fwd((N, H, W, cin, cout), "aesr_conv2d_wino_fwd_ws", "null"))
    case("wino_dgrad_ws-forced-" + tag, "aesr_conv2d_wino_dgrad_ws", env)(_wino_dgrad((N, H, W, cin, cout), "aesr_conv2d_wino_dgrad_ws", "forced", 2))
    case("wino_dgrad_ws-null-" + tag, "aesr_conv2d_wino_dgrad_ws", env)(_wino_dgrad((N, H, W, cin, cout), "aesr_conv2d_wino_dgrad_ws", "null", 2))
case("wino_fwd_ws-query-3x10x10x512x512", "aesr_conv2d_wino_fwd_ws")(_wino_fwd((3, 10, 10, 512, 512), "aesr_conv2d_wino_fwd_ws", "query", 2))
case("wino_dgrad_ws-query-3x10x10x512x512", "aesr_conv2d_wino_dgrad_ws")(_wino_dgrad((3, 10, 10, 512, 512), "aesr_conv2d_wino_dgrad_ws", "query", 2))


def _wino_fwd_bn(shape, pool, act):
    def build(leg):
        N, H, W, Cin, Cout = shape
        assert L_.aesr_conv2d_wino_fwd_bn_supported(N, H, W, Cin, Cout)
        x, w, b, _, _ = _conv_io(shape + (3, 1), 13)
        g = gen(14, *shape)
        sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
        px, pu, pb = leg.inp("in", nhwc(x)), leg.inp("upacked", pack_wino(w.cuda(), 0)), leg.inp("bias", b, "param")
        psc, psh = leg.inp("bn_scale", sc), leg.inp("bn_shift", sh)
        Ho, Wo = (H // 2, W // 2) if pool else (H, W)
        po = leg.out("out", N * Ho * Wo * Cout)

        def ref():
            r = act_ref(F.conv2d(x.double(), w.double(), b.double(), padding=1), act)
            r = F.avg_pool2d(r, 2) if pool else r
            return nhwc(r * sc.double()[None, :, None, None] + sh.double()[None, :, None, None])
        return dict(call=lambda: L_.aesr_conv2d_wino_fwd_bn(px, pu, pb, psc, psh, po, N, H, W, Cin, Cout, act, 0.01, pool, st()),
                    verify=lambda: close(leg, "out", ref(), 2e-6))
    return build


for s, pool, act in [((2, 37, 41, 32, 32), 1, 1), ((2, 37, 41, 32, 32), 0, 2), ((1, 6, 6, 32, 64), 1, 0), ((3, 81, 81, 32, 64), 1, 1),
                     ((2, 16, 24, 48, 96), 1, 1), ((4, 20, 20, 128, 64), 1, 1), ((2, 57, 55, 64, 128), 1, 1), ((2, 57, 55, 64, 128), 0, 0),
                     ((2, 28, 28, 128, 256), 1, 2), ((1, 81, 81, 64, 64), 1, 1)]:
    case("wino_fwd_bn-%s-p%d-a%d" % ("x".join(map(str, s)), pool, act), "aesr_conv2d_wino_fwd_bn")(_wino_fwd_bn(s, pool, act))


def _up2_io(shape):
    N, H, W, Cin, Cout = shape
    g = gen(15, *shape)
    xh = torch.randn(N, Cin, H // 2, W // 2, generator=g, dtype=f64).requires_grad_(True)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g, dtype=f64) / np.sqrt(Cin * 9)).requires_grad_(True)
    b = torch.randn(Cout, generator=g, dtype=f64).requires_grad_(True)
    dy = torch.randn(N, Cout, H, W, generator=g, dtype=f64)
    pre = F.conv2d(F.interpolate(xh, scale_factor=2, mode="nearest"), w, b, padding=1)
    pre.backward(dy)
    return xh, w, b, dy, pre.detach()


for s in [(2, 6, 10, 32, 64), (1, 2, 2, 32, 32), (3, 24, 40, 64, 128)]:
    tag = "x".join(map(str, s))
    for ring in (1, 2):
        @case("wino_fwd_up2-%s-ring%d" % (tag, ring), "aesr_conv2d_wino_fwd_up2", {"AESR_WINO_RING": ring})
        def build(leg, s=s):
            N, H, W, Cin, Cout = s
            xh, w, b, dy, pre = _up2_io(s)
            px, pu, pb = leg.inp("in_half", nhwc(xh.float())), leg.inp("upacked", pack_wino(w.detach().float().cuda(), 0)), leg.inp("bias", b.float(), "param")
            po = leg.out("out", N * H * W * Cout)
            return dict(call=lambda: L_.aesr_conv2d_wino_fwd_up2(px, pu, pb, po, N, H, W, Cin, Cout, 1, 0.01, st()),
                        verify=lambda: close(leg, "out", nhwc(F.leaky_relu(pre, 0.01)), 1e-5))

        @case("wino_dgrad_sum2-%s-ring%d" % (tag, ring), "aesr_conv2d_wino_dgrad_sum2", {"AESR_WINO_RING": ring})
        def build(leg, s=s):
            N, H, W, Cin, Cout = s
            xh, w, b, dy, pre = _up2_io(s)
            pdy, pu = leg.inp("dy", nhwc(dy.float())), leg.inp("upacked_t", pack_wino(w.detach().float().cuda(), 1))
            po = leg.out("dx_half", N * (H // 2) * (W // 2) * Cin)
            return dict(call=lambda: L_.aesr_conv2d_wino_dgrad_sum2(pdy, pu, po, N, H, W, Cin, Cout, st()),
                        verify=lambda: close(leg, "dx_half", nhwc(xh.grad), 1e-5))

    @case("wgrad_up2-" + tag, "aesr_conv2d_wgrad_up2")
    def build(leg, s=s):
        N, H, W, Cin, Cout = s
        assert L_.aesr_conv2d_wgrad_up2_supported(Cin, Cout) == 1
        xh, w, b, dy, pre = _up2_io(s)
        px, pdy = leg.inp("x_half", nhwc(xh.detach().float())), leg.inp("dy", nhwc(dy.float()))
        pdw, pdb = leg.out("dw", Cout * Cin * 9, "param"), leg.out("db", Cout, "param")
        pws = leg.scratch("workspace", L_.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, 3, 1))

        def verify():
            close(leg, "dw", w.grad, 2e-5)
            close(leg, "db", b.grad, 2e-5)
        return dict(call=lambda: L_.aesr_conv2d_wgrad_up2(px, pdy, pdw, pdb, pws, N, H, W, Cin, Cout, st()), verify=verify)


# ---- weight gradients (test_conv_wgrad / test_conv_wgrad_wino 2e-5) -------------------------------------------------------------------
WGRAD_SHAPES = [(2, 33, 35, 8, 16, 3, 1), (1, 7, 7, 4, 8, 3, 1), (2, 17, 19, 16, 32, 1, 0), (7, 10, 10, 128, 96, 3, 1), (3, 7, 9, 32, 32, 3, 1),
                (1, 1, 1, 32, 32, 3, 1), (2, 2, 3, 64, 96, 3, 1), (1, 33, 130, 32, 32, 3, 1), (2, 162, 162, 32, 32, 3, 1), (3, 81, 81, 32, 64, 3, 1),
                (2, 40, 40, 128, 64, 3, 1), (5, 10, 10, 64, 64, 3, 1)]
WGRAD_SHAPES += [sh for sh in _random_shapes(103, 20, [4, 8, 12, 16, 32, 64, 96], [4, 8, 16, 24, 32, 64, 96], ((3, 1), (1, 0), (3, 0)))
                 if sh[1] + 2 * sh[6] >= sh[5] and sh[2] + 2 * sh[6] >= sh[5] and sh not in WGRAD_SHAPES]


def _wgrad_io(shape, seed):
    N, H, W, Cin, Cout, KS, pad = shape
    g = gen(seed, *shape)
    x = torch.randn(N, Cin, H, W, generator=g)
    dy = torch.randn(N, Cout, H + 2 * pad - KS + 1, W + 2 * pad - KS + 1, generator=g)
    ref_w = lambda: torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, KS, KS), dy.double(), padding=pad)
    return x, dy, ref_w, lambda: dy.double().sum((0, 2, 3))


for s in WGRAD_SHAPES:
    @case("wgrad-" + "x".join(map(str, s)), "aesr_conv2d_wgrad")
    def build(leg, s=s):
        N, H, W, Cin, Cout, KS, pad = s
        x, dy, ref_w, ref_b = _wgrad_io(s, 16)
        px, pdy = leg.inp("x", nhwc(x)), leg.inp("dy", nhwc(dy))
        pdw, pdb = leg.out("dw", Cout * Cin * KS * KS, "param"), leg.out("db", Cout, "param")
        pws = leg.scratch("workspace", L_.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, KS, pad))

        def verify():
            close(leg, "dw", ref_w(), 2e-5)
            close(leg, "db", ref_b(), 2e-5)
        return dict(call=lambda: L_.aesr_conv2d_wgrad(px, pdy, pdw, pdb, pws, N, H, W, Cin, Cout, KS, pad, st()), verify=verify)


for s in [(2, 33, 35, 8, 16, 3, 1), (3, 7, 9, 32, 32, 3, 1), (2, 17, 19, 16, 32, 1, 0)]:
    @case("wgrad-nodb-" + "x".join(map(str, s)), "aesr_conv2d_wgrad")
    def build(leg, s=s):
        N, H, W, Cin, Cout, KS, pad = s
        x, dy, ref_w, ref_b = _wgrad_io(s, 16)
        px, pdy = leg.inp("x", nhwc(x)), leg.inp("dy", nhwc(dy))
        pdw = leg.out("dw", Cout * Cin * KS * KS, "param")
        pws = leg.scratch("workspace", L_.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, KS, pad))
        return dict(call=lambda: L_.aesr_conv2d_wgrad(px, pdy, pdw, None, pws, N, H, W, Cin, Cout, KS, pad, st()), verify=lambda: close(leg, "dw", ref_w(), 2e-5))


@case("wgrad_partial+reduce_many", ("aesr_conv2d_wgrad_partial", "aesr_conv2d_wgrad_reduce_many"))
def build(leg):
    """Three layers (implicit-GEMM 3x3, 1x1, Winograd with the folded upsampling) written as partial slabs, then ONE reduction launch."""
    layers = [((2, 33, 35, 8, 16, 3, 1), 0), ((2, 17, 19, 16, 32, 1, 0), 0), ((3, 7, 9, 32, 32, 3, 1), 0), ((2, 6, 10, 32, 64, 3, 1), 1)]
    calls, jobs, refs = [], [], []
    for k, (s, up2) in enumerate(layers):
        N, H, W, Cin, Cout, KS, pad = s
        if up2:
            xh, w, b, dy, _ = _up2_io(s[:5])
            x, dy, rw, rb = nhwc(xh.detach().float()), dy.float(), (lambda w=w: w.grad), (lambda b=b: b.grad)
        else:
            x, dy, rw, rb = _wgrad_io(s, 17)
            x = nhwc(x)
        px, pdy = leg.inp("x%d" % k, x), leg.inp("dy%d" % k, nhwc(dy))
        pws = leg.scratch("workspace%d" % k, L_.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, KS, pad))
        pdw = leg.out("dw%d" % k, Cout * Cin * KS * KS, "param")
        pdb = leg.out("db%d" % k, Cout, "param") if k != 1 else None          # db may be NULL
        calls.append(lambda px=px, pdy=pdy, pws=pws, s=s, up2=up2: L_.aesr_conv2d_wgrad_partial(px, pdy, pws, *s, up2, st()))
        jobs.append(hip.WgradReduceJob(pws.value, pdw.value, pdb.value if pdb else None, *s))
        refs.append((rw, rb if pdb else None))
    arr = (hip.WgradReduceJob * len(jobs))(*jobs)

    def call():
        for c in calls:
            rc = c()
            if rc:
                return rc
        return L_.aesr_conv2d_wgrad_reduce_many(arr, len(jobs), st())

    def verify():
        for k, (rw, rb) in enumerate(refs):
            close(leg, "dw%d" % k, rw(), 2e-5)
            if rb:
                close(leg, "db%d" % k, rb(), 2e-5)
    return dict(call=call, verify=verify)


# ---- bandwidth-bound special cases (test_smallcin_fwd_dgrad_wgrad: fwd 1e-6, dgrad / wgrad 1e-5; test_smallcin_bcast_matches_scaling_layer 1e-5;
#      test_cout1_conv_backward 1e-5; test_cout1_conv_forward_sigmoid 1e-6; test_stem_folded_into_first_conv 1e-5 / 2e-5) -----------------------
SMALL = [(1, 32, 1, 1), (3, 64, 3, 1), (2, 16, 3, 1), (1, 8, 1, 1)]
for cin, cout, ks, pad in SMALL:
    for N, H, W in [(2, 7, 5), (1, 1, 1)]:
        tag = "%dx%dx%d-%dto%d-k%d" % (N, H, W, cin, cout, ks)

        def _io(cin=cin, cout=cout, ks=ks, pad=pad, N=N, H=H, W=W):
            g = gen(18, cin, cout, N, H)
            x = torch.randn(N, cin, H, W, generator=g, dtype=f64).requires_grad_(True)
            w = torch.randn(cout, cin, ks, ks, generator=g, dtype=f64).requires_grad_(True)
            b = torch.randn(cout, generator=g, dtype=f64).requires_grad_(True)
            pre = F.conv2d(x, w, b, padding=pad)
            dy = torch.randn(pre.shape, generator=g, dtype=f64)
            pre.backward(dy)
            return x, w, b, pre.detach(), dy

        @case("smallcin_fwd-" + tag, "aesr_conv2d_smallcin_fwd")
        def build(leg, io=_io, cin=cin, cout=cout, ks=ks, pad=pad, N=N, H=H, W=W):
            x, w, b, pre, dy = io()
            px, pw, pb = leg.inp("in", nhwc(x.float())), leg.inp("w", w.float(), "param"), leg.inp("bias", b.float(), "param")
            po = leg.out("out", pre.numel())
            return dict(call=lambda: L_.aesr_conv2d_smallcin_fwd(px, pw, pb, None, po, N, H, W, cin, cout, ks, pad, 1, 0, 0.01, 0, 0, None, None, st()),
                        verify=lambda: close(leg, "out", nhwc(F.leaky_relu(pre, 0.01)), 1e-6))

        @case("smallcin_dgrad-" + tag, "aesr_conv2d_smallcin_dgrad")
        def build(leg, io=_io, cin=cin, cout=cout, ks=ks, pad=pad, N=N, H=H, W=W):
            x, w, b, pre, dy = io()
            pdy, pw = leg.inp("dy", nhwc(dy.float())), leg.inp("w", w.float(), "param")
            po = leg.out("dx", N * H * W * cin)
            return dict(call=lambda: L_.aesr_conv2d_smallcin_dgrad(pdy, pw, po, N, H, W, cin, cout, ks, pad, 0, None, st()),
                        verify=lambda: close(leg, "dx", nhwc(x.grad), 1e-5))

        if ks == 1:
            @case("smallcin_wgrad-" + tag, "aesr_conv2d_smallcin_wgrad")
            def build(leg, io=_io, cin=cin, cout=cout, pad=pad, N=N, H=H, W=W):
                x, w, b, pre, dy = io()
                px, pdy = leg.inp("in", nhwc(x.float())), leg.inp("dout", nhwc(dy.float()))
                pdw, pdb = leg.out("dw", cout * cin, "param"), leg.out("db", cout, "param")
                pws = leg.scratch("workspace", L_.aesr_small_wgrad_workspace_floats(cout * (cin + 1)))

                def verify():
                    close(leg, "dw", w.grad, 1e-5)
                    close(leg, "db", b.grad, 1e-5)
                return dict(call=lambda: L_.aesr_conv2d_smallcin_wgrad(px, pdy, pdw, pdb, pws, N, H, W, cin, cout, pad, st()), verify=verify)


def _bcast_io(N=2, H=9, W=7, cout=64):
    g = gen(19)
    x = torch.rand(N, 1, H, W, generator=g, dtype=f64).requires_grad_(True)
    w = torch.randn(cout, 3, 3, 3, generator=g, dtype=f64) * 0.2
    b = torch.randn(cout, generator=g, dtype=f64) * 0.1
    sc, sh = (.458, .448, .450), (-.030, -.088, -.188)
    ca, cb = [2.0 / s for s in sc], [(-1.0 - h) / s for h, s in zip(sh, sc)]
    xin = ((2 * x - 1) - torch.tensor(sh, dtype=f64)[None, :, None, None]) / torch.tensor(sc, dtype=f64)[None, :, None, None]
    pre = F.conv2d(xin, w, b, padding=1)
    dy = torch.randn(pre.shape, generator=g, dtype=f64)
    pre.backward(dy)
    return x, w, b, pre.detach(), dy, ca, cb


@case("smallcin_fwd-bcast", "aesr_conv2d_smallcin_fwd")
def build(leg):
    x, w, b, pre, dy, ca, cb = _bcast_io()
    N, _, H, W = x.shape
    px, pw, pb = leg.inp("in", x.detach().float().reshape(N, H, W, 1)), leg.inp("w", w.float(), "param"), leg.inp("bias", b.float(), "param")
    po = leg.out("out", pre.numel())
    fa, fb = hip.float_array(ca), hip.float_array(cb)
    return dict(call=lambda: L_.aesr_conv2d_smallcin_fwd(px, pw, pb, None, po, N, H, W, 3, 64, 3, 1, 2, 0, 0.0, 0, 1, fa, fb, st()),
                verify=lambda: close(leg, "out", nhwc(F.relu(pre)), 1e-5))


@case("smallcin_dgrad-bcast", "aesr_conv2d_smallcin_dgrad")
def build(leg):
    x, w, b, pre, dy, ca, cb = _bcast_io()
    N, _, H, W = x.shape
    pdy, pw = leg.inp("dy", nhwc(dy.float())), leg.inp("w", w.float(), "param")
    po = leg.out("dx", N * H * W)
    fa = hip.float_array(ca)
    return dict(call=lambda: L_.aesr_conv2d_smallcin_dgrad(pdy, pw, po, N, H, W, 3, 64, 3, 1, 1, fa, st()), verify=lambda: close(leg, "dx", x.grad, 1e-5))


def _cout1_io(shape):
    N, H, W, cin = shape
    g = gen(20, *shape)
    h = torch.randn(N, cin, H, W, generator=g, dtype=f64).requires_grad_(True)
    w = (torch.randn(1, cin, 3, 3, generator=g, dtype=f64) / np.sqrt(cin * 9)).requires_grad_(True)
    b = torch.randn(1, generator=g, dtype=f64).requires_grad_(True)
    hl = F.leaky_relu(h, 0.01)
    out = F.conv2d(hl, w, b, padding=1)
    dy = torch.randn(out.shape, generator=g, dtype=f64)
    out.backward(dy)
    return h, hl.detach(), w, b, out.detach(), dy


@case("smallcin_fwd-transpose-2x12x12x48", "aesr_conv2d_smallcin_fwd")
def build(leg):
    """The data gradient of a Cout == 1 convolution whose channel count the thin kernels do not take (test_cout1_conv_backward, 1e-5)."""
    N, H, W, cin = 2, 12, 12, 48
    h, hl, w, b, out, dy = _cout1_io((N, H, W, cin))
    pdy, pw, pys = leg.inp("in", nhwc(dy.float())), leg.inp("w", w.detach().float(), "param"), leg.inp("y_saved", nhwc(hl.float()))
    po = leg.out("out", N * H * W * cin)
    return dict(call=lambda: L_.aesr_conv2d_smallcin_fwd(pdy, pw, None, pys, po, N, H, W, 1, cin, 3, 1, 0, 1, 0.01, 1, 0, None, None, st()),
                verify=lambda: close(leg, "out", nhwc(h.grad), 1e-5))


for s in [(3, 9, 7, 8), (2, 5, 6, 12), (1, 1, 1, 32), (2, 24, 20, 32)]:
    @case("cout1_fwd-" + "x".join(map(str, s)), "aesr_conv2d_cout1_fwd")
    def build(leg, s=s):
        N, H, W, cin = s
        h, hl, w, b, out, dy = _cout1_io(s)
        px, pw, pb = leg.inp("x", nhwc(hl.float())), leg.inp("w", w.detach().float(), "param"), leg.inp("bias", b.detach().float(), "param")
        po = leg.out("out", N * H * W)
        return dict(call=lambda: L_.aesr_conv2d_cout1_fwd(px, pw, pb, po, N, H, W, cin, 3, 0.0, st()),
                    verify=lambda: close(leg, "out", nhwc(torch.sigmoid(out)), 1e-6))

for s in [(3, 7, 9, 16), (2, 12, 12, 8), (1, 1, 1, 4), (1, 9, 130, 64), (2, 5, 3, 256)]:
    tag = "x".join(map(str, s))

    @case("cout1_wgrad-" + tag, "aesr_conv2d_cout1_wgrad")
    def build(leg, s=s):
        N, H, W, cin = s
        h, hl, w, b, out, dy = _cout1_io(s)
        px, pdy = leg.inp("x", nhwc(hl.float())), leg.inp("dy", nhwc(dy.float()))
        pdw, pdb = leg.out("dw", cin * 9, "param"), leg.out("db", 1, "param")
        pws = leg.scratch("workspace", L_.aesr_conv2d_cout1_workspace_floats(cin))

        def verify():
            close(leg, "dw", w.grad, 1e-5)
            close(leg, "db", b.grad, 1e-5)
        return dict(call=lambda: L_.aesr_conv2d_cout1_wgrad(px, pdy, pdw, pdb, pws, N, H, W, cin, st()), verify=verify)

    @case("cout1_dgrad-" + tag, "aesr_conv2d_cout1_dgrad")
    def build(leg, s=s):
        N, H, W, cin = s
        h, hl, w, b, out, dy = _cout1_io(s)
        pdy, pw, pys = leg.inp("dy", nhwc(dy.float())), leg.inp("w", w.detach().float(), "param"), leg.inp("y_saved", nhwc(hl.float()))
        pdx = leg.out("dx", N * H * W * cin)
        pws = leg.scratch("workspace", 9 * cin)           # ">= 9*Cin floats (the flipped filter)"
        return dict(call=lambda: L_.aesr_conv2d_cout1_dgrad(pdy, pw, pys, pdx, pws, N, H, W, cin, 1, 0.01, st()),
                    verify=lambda: close(leg, "dx", nhwc(h.grad), 1e-5))

    @case("cout1_dgrad_pre-" + tag, "aesr_conv2d_cout1_dgrad_pre")
    def build(leg, s=s):
        N, H, W, cin = s
        h, hl, w, b, out, dy = _cout1_io(s)
        flipped = w.detach().float().reshape(cin, 9).flip(1).t().contiguous()          # wexp[t][ci] = W[0, ci, 8 - t]
        pdy, pw, pys = leg.inp("dy", nhwc(dy.float())), leg.inp("w_flipped", flipped), leg.inp("y_saved", nhwc(hl.float()))
        pdx = leg.out("dx", N * H * W * cin)
        return dict(call=lambda: L_.aesr_conv2d_cout1_dgrad_pre(pdy, pw, pys, pdx, N, H, W, cin, 1, 0.01, st()),
                    verify=lambda: close(leg, "dx", nhwc(h.grad), 1e-5))


def _stem_io(shape):
    N, H, W, Cs, C1, p = shape
    g = gen(21, *shape)
    x = torch.rand(N, 1, H, W, generator=g, dtype=f64)
    ws = torch.randn(Cs, 1, 1, 1, generator=g, dtype=f64).requires_grad_(True)
    bs = (torch.randn(Cs, generator=g, dtype=f64) * 0.3).requires_grad_(True)
    w1 = (torch.randn(C1, Cs, 3, 3, generator=g, dtype=f64) / np.sqrt(9 * Cs)).requires_grad_(True)
    b1 = (torch.randn(C1, generator=g, dtype=f64) * 0.1).requires_grad_(True)
    pre = F.conv2d(F.conv2d(x, ws, bs, padding=p), w1, b1, padding=1)
    gout = torch.randn(pre.shape, generator=g, dtype=f64)
    pre.backward(gout)
    return x, ws, bs, w1, b1, pre.detach(), gout


def _fold(ws, bs, w1, Cs, C1):
    folded = torch.empty(L_.aesr_stemconv_folded_floats(C1), device="cuda")
    a, b, c = ws.detach().float().cuda(), bs.detach().float().cuda(), w1.detach().float().cuda()
    hip.check(L_.aesr_stemconv_fold(hip.ptr(a), hip.ptr(b), hip.ptr(c), hip.ptr(folded), Cs, C1, st()), "fold")
    torch.cuda.synchronize()
    return folded


for s in [(3, 21, 37, 32, 32, 1), (2, 5, 3, 32, 128, 2), (1, 1, 1, 8, 4, 1), (1, 30, 30, 48, 16, 0), (2, 8, 70, 16, 64, 1)]:
    tag = "x".join(map(str, s))

    @case("stemconv_fold-" + tag, "aesr_stemconv_fold")
    def build(leg, s=s):
        N, H, W, Cs, C1, p = s
        x, ws, bs, w1, b1, pre, gout = _stem_io(s)
        pa, pb, pc = leg.inp("w_stem", ws.detach().float(), "param"), leg.inp("b_stem", bs.detach().float(), "param"), leg.inp("w1", w1.detach().float(), "param")
        po = leg.out("folded", L_.aesr_stemconv_folded_floats(C1))

        def verify():
            # weff[t][co] = sum_c w1[co,c,t] * w_stem[c]; beff[t][co] = sum_c w1[co,c,t] * b_stem[c] (include/aesr_hip.h); same bound as the forward (1e-5)
            w1d = w1.detach().reshape(C1, Cs, 9)
            weff = torch.einsum("oct,c->to", w1d, ws.detach().reshape(Cs))
            beff = torch.einsum("oct,c->to", w1d, bs.detach())
            close(leg, "folded", torch.cat([weff.reshape(-1), beff.reshape(-1)]), 1e-5)
        return dict(call=lambda: L_.aesr_stemconv_fold(pa, pb, pc, po, Cs, C1, st()), verify=verify)

    @case("stemconv_fwd-" + tag, "aesr_stemconv_fwd")
    def build(leg, s=s):
        N, H, W, Cs, C1, p = s
        x, ws, bs, w1, b1, pre, gout = _stem_io(s)
        px, pf, pb = leg.inp("x", x.float().reshape(N, H, W)), leg.inp("folded", _fold(ws, bs, w1, Cs, C1)), leg.inp("b1", b1.detach().float(), "param")
        po = leg.out("out", pre.numel())

        def verify():
            close(leg, "out", nhwc(F.leaky_relu(pre, 0.01)), 1e-5)
            close(leg, "out", nhwc(F.leaky_relu(pre, 0.01)), 1e-4, "abs")
        return dict(call=lambda: L_.aesr_stemconv_fwd(px, pf, pb, po, N, H, W, C1, p, 1, 0.01, st()), verify=verify)

    @case("stemconv_wgrad-" + tag, "aesr_stemconv_wgrad")
    def build(leg, s=s):
        N, H, W, Cs, C1, p = s
        x, ws, bs, w1, b1, pre, gout = _stem_io(s)
        px, pg = leg.inp("x", x.float().reshape(N, H, W)), leg.inp("g", nhwc(gout.float()))
        pa, pb, pc = leg.inp("w_stem", ws.detach().float(), "param"), leg.inp("b_stem", bs.detach().float(), "param"), leg.inp("w1", w1.detach().float(), "param")
        o1, o2, o3, o4 = leg.out("dw_stem", Cs, "param"), leg.out("db_stem", Cs, "param"), leg.out("dw1", C1 * Cs * 9, "param"), leg.out("db1", C1, "param")
        pws = leg.scratch("workspace", L_.aesr_stemconv_workspace_floats(C1))

        def verify():
            for name, ref in (("dw_stem", ws.grad), ("db_stem", bs.grad), ("dw1", w1.grad), ("db1", b1.grad)):
                close(leg, name, ref, 2e-5)
        return dict(call=lambda: L_.aesr_stemconv_wgrad(px, pg, pa, pb, pc, o1, o2, o3, o4, pws, N, H, W, Cs, C1, p, st()), verify=verify)


@case("stemconv_wgrad-nobias-2x5x3x32x128x2", "aesr_stemconv_wgrad")
def build(leg):
    """b_stem, db_stem and db1 may be NULL."""
    N, H, W, Cs, C1, p = 2, 5, 3, 32, 128, 2
    g = gen(53)
    x = torch.rand(N, 1, H, W, generator=g, dtype=f64)
    ws = torch.randn(Cs, 1, 1, 1, generator=g, dtype=f64).requires_grad_(True)
    w1 = (torch.randn(C1, Cs, 3, 3, generator=g, dtype=f64) / np.sqrt(9 * Cs)).requires_grad_(True)
    pre = F.conv2d(F.conv2d(x, ws, None, padding=p), w1, None, padding=1)
    gout = torch.randn(pre.shape, generator=g, dtype=f64)
    pre.backward(gout)
    px, pg = leg.inp("x", x.float().reshape(N, H, W)), leg.inp("g", nhwc(gout.float()))
    pa, pc = leg.inp("w_stem", ws.detach().float(), "param"), leg.inp("w1", w1.detach().float(), "param")
    o1, o3 = leg.out("dw_stem", Cs, "param"), leg.out("dw1", C1 * Cs * 9, "param")
    pws = leg.scratch("workspace", L_.aesr_stemconv_workspace_floats(C1))

    def verify():
        close(leg, "dw_stem", ws.grad, 2e-5)
        close(leg, "dw1", w1.grad, 2e-5)
    return dict(call=lambda: L_.aesr_stemconv_wgrad(px, pg, pa, None, pc, o1, None, o3, None, pws, N, H, W, Cs, C1, p, st()), verify=verify)


# ---- resampling, space-to-depth, max pooling, LPIPS pieces (test_resample2_fwd_bwd 1e-6; test_maxpool_fwd_bwd: bit-equal / 1e-6;
#      test_tap_kernels_vs_reference_head: distances rtol 1e-5, gradients 1e-4) -------------------------------------------------------------
RS_SHAPES = [(3, 7, 5, 4), (2, 1, 1, 16), (2, 2, 3, 8), (2, 12, 16, 8)]
for mode in (1, 2, 3):
    for s in RS_SHAPES:
        if mode == 1 and min(s[1:3]) < 2:
            continue
        tag = "x".join(map(str, s)) + "-m%d" % mode

        def _io(s=s, mode=mode):
            N, H, W, C = s
            g = gen(22, mode, *s)
            pre = torch.randn(N, C, H, W, generator=g, dtype=f64).requires_grad_(True)
            x = F.leaky_relu(pre, 0.01)
            ref = F.avg_pool2d(x, 2) if mode == 1 else F.interpolate(x, scale_factor=2, mode="nearest" if mode == 2 else "bilinear",
                                                                      **({} if mode == 2 else {"align_corners": False}))
            gout = torch.randn(ref.shape, generator=g, dtype=f64)
            ref.backward(gout)
            return pre, x.detach(), ref.detach(), gout

        @case("resample2_fwd-" + tag, "aesr_resample2_fwd")
        def build(leg, io=_io, s=s, mode=mode):
            pre, x, ref, gout = io()
            px, po = leg.inp("x", nhwc(x.float())), leg.out("out", ref.numel())
            return dict(call=lambda: L_.aesr_resample2_fwd(px, po, *s, mode, st()), verify=lambda: close(leg, "out", nhwc(ref), 1e-6))

        @case("resample2_bwd-" + tag, "aesr_resample2_bwd")
        def build(leg, io=_io, s=s, mode=mode):
            pre, x, ref, gout = io()
            pg, px, po = leg.inp("gout", nhwc(gout.float())), leg.inp("x_saved", nhwc(x.float())), leg.out("dx", pre.numel())
            return dict(call=lambda: L_.aesr_resample2_bwd(pg, px, po, *s, mode, 1, 0.01, st()), verify=lambda: close(leg, "dx", nhwc(pre.grad), 1e-6))

for s in [(3, 7, 5, 4), (2, 2, 3, 8), (2, 12, 16, 8), (1, 9, 9, 64)]:
    tag = "x".join(map(str, s))
    N, H, W, C = s

    def _s2d(x):            # out[n,y,x,(ky*2+kx)*C+c] = x[n,2y+ky,2x+kx,c] (include/aesr_hip.h)
        n, h, w, c = x.shape
        v = x[:, :h // 2 * 2, :w // 2 * 2].reshape(n, h // 2, 2, w // 2, 2, c)
        return v.permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4 * c)

    @case("space_to_depth2-" + tag, "aesr_space_to_depth2")
    def build(leg, s=s, f=_s2d):
        x = torch.randn(*s, generator=gen(23, *s))
        px, po = leg.inp("x", x), leg.out("out", s[0] * (s[1] // 2) * (s[2] // 2) * 4 * s[3])
        return dict(call=lambda: L_.aesr_space_to_depth2(px, po, *s, st()), verify=lambda: close(leg, "out", f(x), None, "eq"))

    @case("depth_to_space2-" + tag, "aesr_depth_to_space2")
    def build(leg, s=s, f=_s2d):
        N, H, W, C = s
        gdy = torch.randn(N, H // 2, W // 2, 4 * C, generator=gen(24, *s))
        pg, po = leg.inp("g", gdy), leg.out("dx", N * H * W * C)

        def verify():
            xx = torch.zeros(*s, dtype=f64, requires_grad=True)
            (f(xx) * gdy.double()).sum().backward()
            close(leg, "dx", xx.grad.float(), None, "eq")           # a pure scatter (zero in a dropped odd last row / column)
        return dict(call=lambda: L_.aesr_depth_to_space2(pg, po, *s, st()), verify=verify)

    def _mp(s=s):
        N, H, W, C = s
        g = gen(25, *s)
        x = F.relu(torch.randn(N, C, H, W, generator=g, dtype=f64)).requires_grad_(True)           # many exact ties at 0
        out = F.max_pool2d(x, 2)
        gout = torch.randn(out.shape, generator=g, dtype=f64)
        gadd = torch.randn(x.shape, generator=g, dtype=f64)
        out.backward(gout)
        return x, out.detach(), gout, gadd

    @case("maxpool2_fwd-" + tag, "aesr_maxpool2_fwd")
    def build(leg, s=s, io=_mp):
        x, out, gout, gadd = io()
        px, po = leg.inp("x", nhwc(x.detach().float())), leg.out("out", out.numel())
        return dict(call=lambda: L_.aesr_maxpool2_fwd(px, po, *s, st()), verify=lambda: close(leg, "out", nhwc(out.float()), None, "eq"))

    @case("maxpool2_bwd-" + tag, "aesr_maxpool2_bwd")
    def build(leg, s=s, io=_mp):
        x, out, gout, gadd = io()
        pg, px, pa = leg.inp("gout", nhwc(gout.float())), leg.inp("x", nhwc(x.detach().float())), leg.inp("gadd", nhwc(gadd.float()))
        po = leg.out("dx", x.numel())
        # the reference scatters to the first maximum of each window in fp32 data: ties are exact zeros, which the ReLU mask removes
        ref = lambda: nhwc((x.grad + gadd.float().double()) * (x.detach() > 0))
        return dict(call=lambda: L_.aesr_maxpool2_bwd(pg, px, pa, po, *s, 1, st()), verify=lambda: close(leg, "dx", ref(), 1e-6))

for s in [(3, 7, 5, 4), (2, 12, 16, 8)]:
    @case("maxpool2_bwd-plain-" + "x".join(map(str, s)), "aesr_maxpool2_bwd")
    def build(leg, s=s):
        """No gadd, no ReLU mask; continuous inputs (no ties inside a window)."""
        N, H, W, C = s
        g = gen(51, *s)
        x = torch.randn(N, C, H, W, generator=g).double().requires_grad_(True)
        out = F.max_pool2d(x, 2)
        gout = torch.randn(out.shape, generator=g).double()
        out.backward(gout)
        pg, px, po = leg.inp("gout", nhwc(gout.float())), leg.inp("x", nhwc(x.detach().float())), leg.out("dx", x.numel())
        return dict(call=lambda: L_.aesr_maxpool2_bwd(pg, px, None, po, *s, 0, st()), verify=lambda: close(leg, "dx", nhwc(x.grad), 1e-6))

    @case("resample2_bwd-nomask-" + "x".join(map(str, s)), "aesr_resample2_bwd")
    def build(leg, s=s):
        N, H, W, C = s
        g = gen(52, *s)
        x = torch.randn(N, C, H, W, generator=g).double().requires_grad_(True)
        ref = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        gout = torch.randn(ref.shape, generator=g).double()
        ref.backward(gout)
        pg, po = leg.inp("gout", nhwc(gout.float())), leg.out("dx", x.numel())
        return dict(call=lambda: L_.aesr_resample2_bwd(pg, None, po, *s, 3, 0, 0.0, st()), verify=lambda: close(leg, "dx", nhwc(x.grad), 1e-6))

CA = [2.0 / s for s in (.458, .448, .450)]
CB = [(-1.0 - h) / s for h, s in zip((-.030, -.088, -.188), (.458, .448, .450))]
for n in (1, 7, 1027, 4096):
    @case("scale_expand_fwd-%d" % n, "aesr_scale_expand_fwd")
    def build(leg, n=n):
        x = torch.rand(n, generator=gen(26, n))
        px, po = leg.inp("x", x), leg.out("out4", 4 * n)
        fa, fb = hip.float_array(CA), hip.float_array(CB)
        # out4[p][c] = ca[c]*x[p] + cb[c], channel 3 = 0 (include/aesr_hip.h); VGG conv1_1 on it is checked at 1e-5 (test_smallcin_bcast...)
        ref = lambda: torch.cat([x.double()[:, None] * torch.tensor(CA, dtype=f32).double() + torch.tensor(CB, dtype=f32).double(), torch.zeros(n, 1, dtype=f64)], 1)
        return dict(call=lambda: L_.aesr_scale_expand_fwd(px, po, n, fa, fb, st()), verify=lambda: close(leg, "out4", ref(), 1e-6))

    @case("scale_expand_bwd-%d" % n, "aesr_scale_expand_bwd")
    def build(leg, n=n):
        d4 = torch.randn(n, 4, generator=gen(27, n))
        pd, po = leg.inp("d4", d4), leg.out("dx", n)
        fa = hip.float_array(CA)
        ref = lambda: (d4.double()[:, :3] * torch.tensor(CA, dtype=f32).double()).sum(1)
        return dict(call=lambda: L_.aesr_scale_expand_bwd(pd, po, n, fa, st()), verify=lambda: close(leg, "dx", ref(), 1e-6))


def _tap_io(B, HW, C):
    g = gen(28, B, HW, C)
    f = F.relu(torch.randn(2 * B, HW, C, generator=g, dtype=f64)).requires_grad_(True)
    lw = torch.rand(C, generator=g, dtype=f64)

    def nrm(t):
        return t / (t.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    d = ((nrm(f[:B]) - nrm(f[B:])).pow(2) * lw).sum(-1)           # [B, HW]: per pixel, summed over channels
    gd = torch.randn(B, generator=g, dtype=f64)
    ((d.sum(1) / HW) * gd).sum().backward()
    return f, lw, d.detach(), gd


for B, HW, C in [(2, 35, 64), (1, 1, 128), (3, 100, 256), (2, 9, 512)]:
    tag = "%dx%dx%d" % (B, HW, C)

    @case("lpips_tap_fwd-" + tag, "aesr_lpips_tap_fwd")
    def build(leg, B=B, HW=HW, C=C):
        f, lw, d, gd = _tap_io(B, HW, C)
        pf, pw = leg.inp("f", f.detach().float()), leg.inp("lin_w", lw.float(), "param")
        po = leg.out("partial", B * hip.LPIPS_NCH)

        def verify():
            got = leg.v("partial").cpu().double().reshape(B, hip.LPIPS_NCH).sum(1)
            np.testing.assert_allclose(got.numpy(), d.sum(1).numpy(), rtol=1e-5)
        return dict(call=lambda: L_.aesr_lpips_tap_fwd(pf, pw, po, B, HW, C, st()), verify=verify)

    @case("lpips_tap_bwd-" + tag, "aesr_lpips_tap_bwd")
    def build(leg, B=B, HW=HW, C=C):
        f, lw, d, gd = _tap_io(B, HW, C)
        # gd of the ABI is dL/dd[n] of the FINISHED distance (the 1/HW of aesr_lpips_finalize is applied inside the tap's backward)
        pf, pw, pg = leg.inp("f", f.detach().float()), leg.inp("lin_w", lw.float(), "param"), leg.inp("gd", gd.float())
        po = leg.out("gf0", B * HW * C)
        return dict(call=lambda: L_.aesr_lpips_tap_bwd(pf, pw, pg, po, B, HW, C, st()), verify=lambda: close(leg, "gf0", f.grad[:B], 1e-4))


@case("lpips_finalize", "aesr_lpips_finalize")
def build(leg):
    B, hws = 3, [35, 1, 100]
    g = gen(29)
    parts = [torch.rand(B, hip.LPIPS_NCH, generator=g) for _ in hws]
    ptrs = (ctypes.c_void_p * len(hws))(*[leg.inp("partial%d" % k, p).value for k, p in enumerate(parts)])
    po = leg.out("d", B)
    hw = hip.int_array(hws)

    def verify():
        want = sum(p.double().sum(1) / h for p, h in zip(parts, hws))
        np.testing.assert_allclose(leg.v("d").cpu().double().numpy(), want.numpy(), rtol=1e-5)
    return dict(call=lambda: L_.aesr_lpips_finalize(ptrs, hw, len(hws), po, B, st()), verify=verify)


# ---- BatchNorm (test_bn_groups_fwd_bwd: forward / running statistics 1e-5, backward 2e-5; test_bn_one_launch_equals_three_launches:
#      2e-6 / 5e-6 against the three-launch path, which is itself held to 1e-5 / 2e-5 against the reference -- the bounds used here) --------
def _bn_io(shape, nstart, mode, seed=30):
    N, H, W, C = shape
    G = len(nstart) - 1
    g = gen(seed, mode, *shape)
    y = F.leaky_relu(torch.randn(N, C, H, W, generator=g, dtype=f64) * 1.5 + 0.3, 0.01).requires_grad_(True)
    gam = torch.randn(C, generator=g, dtype=f64).requires_grad_(True)
    bet = torch.randn(C, generator=g, dtype=f64).requires_grad_(True)
    post = {0: lambda t: t, 1: lambda t: F.avg_pool2d(t, 2), 2: lambda t: F.interpolate(t, scale_factor=2, mode="nearest")}[mode]
    rm, rv = torch.zeros(C, dtype=f64), torch.ones(C, dtype=f64)
    outs, stats, sums = [], [], []
    for a, b in zip(nstart[:-1], nstart[1:]):
        yg = y[a:b]
        outs.append(post(F.batch_norm(yg, rm, rv, gam, bet, True, 0.1, 1e-5)))        # updates rm / rv group after group
        m, v = yg.detach().mean((0, 2, 3)), yg.detach().var((0, 2, 3), unbiased=False)
        istd = 1.0 / torch.sqrt(v + 1e-5)
        sc = gam.detach() * istd
        stats.append((m, istd, sc, bet.detach() - m * sc))
        sums.append(torch.stack([yg.detach().sum((0, 2, 3)), yg.detach().pow(2).sum((0, 2, 3))]))
    out = torch.cat(outs)
    st4 = [torch.stack([s[i] for s in stats]) for i in range(4)]           # mean, invstd, scale, shift as [G][C]
    counts = [float((b - a) * H * W) for a, b in zip(nstart[:-1], nstart[1:])]
    return types.SimpleNamespace(N=N, H=H, W=W, C=C, G=G, y=y, gam=gam, bet=bet, out=out, st4=st4, sums=torch.stack(sums), rm=rm, rv=rv, counts=counts,
                                 ns=hip.int_array(nstart), cnt=hip.double_array(counts), gen=g, mode=mode, nstart=nstart)


def _bn_running(leg, io):
    return (leg.inout("running_mean", torch.zeros(io.C)), leg.inout("running_var", torch.ones(io.C)),
            leg.inout("num_batches_tracked", torch.zeros(1, dtype=torch.int64)))


def _bn_stat_outs(leg, io):
    return [leg.out(n, io.G * io.C) for n in ("mean", "invstd", "scale", "shift")]


def _bn_verify_fwd(leg, io, with_out):
    for n, ref in zip(("mean", "invstd", "scale", "shift"), io.st4):
        close(leg, n, ref, 1e-5)
    close(leg, "running_mean", io.rm, 1e-5)
    close(leg, "running_var", io.rv, 1e-5)
    assert int(leg.v("num_batches_tracked")[0]) == io.G
    if with_out:
        close(leg, "out", nhwc(io.out.detach()), 1e-5)


BN_SHAPES = [((6, 33, 31, 32), [0, 4, 6]), ((3, 9, 9, 8), [0, 2, 3]), ((3, 2, 3, 8), [0, 2, 3]), ((9, 33, 47, 32), [0, 4, 7, 9]), ((1, 2, 3, 128), [0, 1]),
             ((4, 40, 40, 64), [0, 3, 4]), ((6, 81, 81, 64), [0, 4, 6]), ((5, 7, 5, 16), [0, 1, 2, 4, 5])]
for shape, nstart in BN_SHAPES:
    tag = "x".join(map(str, shape))

    @case("bn_stats-" + tag, "aesr_bn_stats")
    def build(leg, shape=shape, nstart=nstart):
        io = _bn_io(shape, nstart, 0)
        py = leg.inp("y", nhwc(io.y.detach().float()))
        pp, ps = leg.scratch("partial", io.G * hip.BN_NWG * 2 * io.C), leg.out("sums", io.G * 2 * io.C, dtype=f64)
        return dict(call=lambda: L_.aesr_bn_stats(py, pp, ps, io.H * io.W, io.C, io.G, io.ns, st()), verify=lambda: close(leg, "sums", io.sums, 1e-5))

    for train in (1, 0):
        @case("bn_finalize-%s-train%d" % (tag, train), "aesr_bn_finalize")
        def build(leg, shape=shape, nstart=nstart, train=train):
            io = _bn_io(shape, nstart, 0)
            ps = leg.inp("sums", io.sums)
            pg, pb = leg.inp("gamma", io.gam.detach().float(), "param"), leg.inp("beta", io.bet.detach().float(), "param")
            g = gen(31, *shape)
            rm0, rv0 = torch.randn(io.C, generator=g), torch.rand(io.C, generator=g) + 0.5
            if train:
                prm, prv, pn = _bn_running(leg, io)
            else:
                prm, prv = leg.inp("running_mean", rm0, "param"), leg.inp("running_var", rv0, "param")
                pn = leg.inp("num_batches_tracked", torch.zeros(1, dtype=torch.int64), "param")
            o = _bn_stat_outs(leg, io)

            def verify():
                if train:
                    _bn_verify_fwd(leg, io, False)
                else:           # eval: every group gets the running statistics
                    istd = 1.0 / torch.sqrt(rv0.double() + 1e-5)
                    sc = io.gam.detach().float().double() * istd
                    for n, ref in (("mean", rm0.double()), ("invstd", istd), ("scale", sc), ("shift", io.bet.detach().float().double() - rm0.double() * sc)):
                        close(leg, n, ref.repeat(io.G), 1e-5)
            return dict(call=lambda: L_.aesr_bn_finalize(ps, io.cnt, pg, pb, prm, prv, pn, *o, io.C, io.G, 0.1, 1e-5, train, 1, st()), verify=verify)

    @case("bn_stats_finalize-" + tag, "aesr_bn_stats_finalize")
    def build(leg, shape=shape, nstart=nstart):
        io = _bn_io(shape, nstart, 0)
        py, pp = leg.inp("y", nhwc(io.y.detach().float())), leg.scratch("partial", io.G * hip.BN_NWG * 2 * io.C)
        pg, pb = leg.inp("gamma", io.gam.detach().float(), "param"), leg.inp("beta", io.bet.detach().float(), "param")
        prm, prv, pn = _bn_running(leg, io)
        o = _bn_stat_outs(leg, io)
        return dict(call=lambda: L_.aesr_bn_stats_finalize(py, pp, io.cnt, pg, pb, prm, prv, pn, *o, io.H * io.W, io.C, io.G, io.ns, 0.1, 1e-5, 1, st()),
                    verify=lambda: _bn_verify_fwd(leg, io, False))

    for mode in (0, 1, 2):
        if mode == 1 and min(shape[1:3]) < 2:
            continue
        mtag = tag + "-m%d" % mode

        @case("bn_apply-" + mtag, "aesr_bn_apply")
        def build(leg, shape=shape, nstart=nstart, mode=mode):
            io = _bn_io(shape, nstart, mode)
            py = leg.inp("y", nhwc(io.y.detach().float()))
            psc, psh = leg.inp("scale", io.st4[2].float()), leg.inp("shift", io.st4[3].float())
            po = leg.out("out", io.out.numel())
            return dict(call=lambda: L_.aesr_bn_apply(py, psc, psh, po, io.N, io.H, io.W, io.C, mode, io.G, io.ns, st()),
                        verify=lambda: close(leg, "out", nhwc(io.out.detach()), 1e-5))

        @case("bn_finalize_apply-" + mtag, "aesr_bn_finalize_apply")
        def build(leg, shape=shape, nstart=nstart, mode=mode):
            io = _bn_io(shape, nstart, mode)
            assert L_.aesr_bn_fused_supported(io.C, io.G) == 1
            ps = leg.inp("sums", io.sums)
            pg, pb = leg.inp("gamma", io.gam.detach().float(), "param"), leg.inp("beta", io.bet.detach().float(), "param")
            prm, prv, pn = _bn_running(leg, io)
            o = _bn_stat_outs(leg, io)
            py, po = leg.inp("y", nhwc(io.y.detach().float())), leg.out("out", io.out.numel())
            return dict(call=lambda: L_.aesr_bn_finalize_apply(ps, io.cnt, pg, pb, prm, prv, pn, *o, py, po, io.N, io.H, io.W, io.C, mode, io.G, io.ns,
                                                               0.1, 1e-5, 1, st()), verify=lambda: _bn_verify_fwd(leg, io, True))

        def _bwd_io(shape=shape, nstart=nstart, mode=mode):
            io = _bn_io(shape, nstart, mode)
            gout = torch.randn(io.out.shape, generator=io.gen, dtype=f64)
            (io.out * gout).sum().backward()
            dpre = io.y.grad * torch.where(io.y.detach() > 0, 1.0, 0.01)
            xhat = [(io.y.detach()[a:b] - io.st4[0][k][None, :, None, None]) * io.st4[1][k][None, :, None, None]
                    for k, (a, b) in enumerate(zip(nstart[:-1], nstart[1:]))]
            adj = {0: lambda t: t, 1: lambda t: F.interpolate(t, scale_factor=2, mode="nearest") / 4,
                   2: lambda t: F.avg_pool2d(t, 2) * 4}[mode]           # g: the gradient w.r.t. the BN output seen through the pool / upsample
            gb = []
            for k, (a, b) in enumerate(zip(nstart[:-1], nstart[1:])):
                gg = adj(gout[a:b])
                if mode == 1:           # a dropped odd last row / column receives no gradient
                    full = torch.zeros_like(xhat[k])
                    full[:, :, :gg.shape[2], :gg.shape[3]] = gg
                    gg = full
                gb.append(torch.stack([gg.sum((0, 2, 3)), (gg * xhat[k]).sum((0, 2, 3))]))
            return io, gout, dpre, torch.stack(gb)

        def _bwd_inputs(leg, io, gout):
            return (leg.inp("gout", nhwc(gout.float())), leg.inp("y", nhwc(io.y.detach().float())), leg.inp("mean", io.st4[0].float()),
                    leg.inp("invstd", io.st4[1].float()), leg.inp("scale", io.st4[2].float()))

        def _bwd_verify(leg, io, dpre):
            close(leg, "dpre", nhwc(dpre), 2e-5)
            close(leg, "dgamma", io.gam.grad, 2e-5)
            close(leg, "dbeta", io.bet.grad, 2e-5)

        @case("bn_bwd_reduce-" + mtag, "aesr_bn_bwd_reduce")
        def build(leg, io_=_bwd_io, mode=mode):
            io, gout, dpre, bsums = io_()
            pg, py, pm, pi, _ = _bwd_inputs(leg, io, gout)
            pp, ps = leg.scratch("partial", io.G * hip.BN_NWG * 2 * io.C), leg.out("sums", io.G * 2 * io.C, dtype=f64)
            return dict(call=lambda: L_.aesr_bn_bwd_reduce(pg, py, pm, pi, pp, ps, io.N, io.H, io.W, io.C, mode, io.G, io.ns, st()),
                        verify=lambda: close(leg, "sums", bsums, 2e-5))

        @case("bn_bwd_apply-" + mtag, "aesr_bn_bwd_apply")
        def build(leg, io_=_bwd_io, mode=mode, bv=_bwd_verify, bi=_bwd_inputs):
            io, gout, dpre, bsums = io_()
            pg, py, pm, pi, psc = bi(leg, io, gout)
            ps = leg.inp("sums", bsums)
            pc = leg.scratch("coef", io.G * 2 * io.C)
            o1, o2, o3 = leg.out("dgamma", io.C, "param"), leg.out("dbeta", io.C, "param"), leg.out("dpre", io.y.numel())
            return dict(call=lambda: L_.aesr_bn_bwd_apply(pg, py, pm, pi, psc, ps, io.cnt, pc, o1, o2, o3, io.N, io.H, io.W, io.C, mode, 1, 0.01, io.G,
                                                          io.ns, st()), verify=lambda: bv(leg, io, dpre))

        @case("bn_bwd-" + mtag, "aesr_bn_bwd")
        def build(leg, io_=_bwd_io, mode=mode, bv=_bwd_verify, bi=_bwd_inputs):
            io, gout, dpre, bsums = io_()
            pg, py, pm, pi, psc = bi(leg, io, gout)
            pp, pc = leg.scratch("partial", io.G * hip.BN_NWG * 2 * io.C), leg.scratch("coef", io.G * 2 * io.C)
            o1, o2, o3 = leg.out("dgamma", io.C, "param"), leg.out("dbeta", io.C, "param"), leg.out("dpre", io.y.numel())
            return dict(call=lambda: L_.aesr_bn_bwd(pg, py, pm, pi, psc, pp, io.cnt, pc, o1, o2, o3, io.N, io.H, io.W, io.C, mode, 1, 0.01, io.G, io.ns,
                                                    st()), verify=lambda: bv(leg, io, dpre))

        if mode in (0, 1):
            @case("bn_fused1_fwd-" + mtag, "aesr_bn_fused1_fwd")
            def build(leg, shape=shape, nstart=nstart, mode=mode):
                io = _bn_io(shape, nstart, mode)
                fits = L_.aesr_bn_fused1_supported(io.N, io.H, io.W, io.C, mode, io.G, 0) == 1
                SEEN["bn_fused1"] += fits
                py, po = leg.inp("y", nhwc(io.y.detach().float())), leg.out("out", io.out.numel())
                pws = leg.scratch("workspace", L_.aesr_bn_fused1_workspace_floats(io.C, io.G))
                pbar = leg.state("barrier_state", torch.zeros(int(L_.aesr_bn_fused1_barrier_words()), dtype=torch.int32))
                pg, pb = leg.inp("gamma", io.gam.detach().float(), "param"), leg.inp("beta", io.bet.detach().float(), "param")
                prm, prv, pn = _bn_running(leg, io)
                o = _bn_stat_outs(leg, io)

                def verify():
                    _bn_verify_fwd(leg, io, True)
                    assert L_.aesr_bn_fused1_timeouts() == 0
                return dict(call=lambda: L_.aesr_bn_fused1_fwd(py, po, pws, pbar, io.cnt, pg, pb, prm, prv, pn, *o, io.N, io.H, io.W, io.C, mode, io.G,
                                                               io.ns, 0.1, 1e-5, 1, st()), verify=verify, expect_rc=0 if fits else 3)

            @case("bn_fused1_bwd-" + mtag, "aesr_bn_fused1_bwd")
            def build(leg, io_=_bwd_io, mode=mode, bv=_bwd_verify, bi=_bwd_inputs):
                io, gout, dpre, bsums = io_()
                fits = L_.aesr_bn_fused1_supported(io.N, io.H, io.W, io.C, mode, io.G, 1) == 1
                SEEN["bn_fused1"] += fits
                pg, py, pm, pi, psc = bi(leg, io, gout)
                pws = leg.scratch("workspace", L_.aesr_bn_fused1_workspace_floats(io.C, io.G))
                pbar = leg.state("barrier_state", torch.zeros(int(L_.aesr_bn_fused1_barrier_words()), dtype=torch.int32))
                pc = leg.scratch("coef", io.G * 2 * io.C)
                o1, o2, o3 = leg.out("dgamma", io.C, "param"), leg.out("dbeta", io.C, "param"), leg.out("dpre", io.y.numel())

                def verify():
                    bv(leg, io, dpre)
                    assert L_.aesr_bn_fused1_timeouts() == 0
                return dict(call=lambda: L_.aesr_bn_fused1_bwd(pg, py, pm, pi, psc, pws, pbar, io.cnt, pc, o1, o2, o3, io.N, io.H, io.W, io.C, mode, 1,
                                                               0.01, io.G, io.ns, st()), verify=verify, expect_rc=0 if fits else 3)


@case("bn_fused1-shared-barrier", ("aesr_bn_fused1_fwd", "aesr_bn_fused1_bwd"))
def build(leg):
    """One barrier state per NETWORK (include/aesr_hip.h): launches of different layers, forward and backward, back to back on one state,
    which is zeroed once and never again -- every member still matches its reference, and the whole sequence repeated on the used state
    gives the same bits (leg 3)."""
    members = [("bn_fused1_fwd-6x33x31x32-m1", (6, 33, 31, 32, 1, 2, 0)), ("bn_fused1_bwd-3x9x9x8-m0", (3, 9, 9, 8, 0, 2, 1)),
               ("bn_fused1_fwd-9x33x47x32-m0", (9, 33, 47, 32, 0, 3, 0)), ("bn_fused1_bwd-6x33x31x32-m1", (6, 33, 31, 32, 1, 2, 1)),
               ("bn_fused1_fwd-1x2x3x128-m0", (1, 2, 3, 128, 0, 1, 0)), ("bn_fused1_bwd-4x40x40x64-m1", (4, 40, 40, 64, 1, 2, 1))]
    by_id = {c.id: c for c in CASES}
    specs = [by_id[cid].build(SubLeg(leg, "%d." % k, shared=("barrier_state",))) for k, (cid, q) in enumerate(members)
             if L_.aesr_bn_fused1_supported(*q) == 1]
    assert len(specs) >= 2

    def call():
        for sp in specs:
            rc = sp["call"]()
            if rc:
                return rc
        return 0

    def verify():
        for sp in specs:
            sp["verify"]()
    return dict(call=call, verify=verify)


# ---- element-wise ops and losses (test_lerp_mse_act_adam: lerp bit-equal to the fp32 expression, mse 1e-6, act_bwd 1e-6, Adam 1e-6;
#      test_fused_lerp_decode_at_eval_patch_size: rtol 1e-6 / atol 1e-7; test_interleave_clamp: bit-equal; test_combined_mse_loss_block:
#      rtol 3e-7 / 1e-6; test_laploss_vs_oracle_nonsquare_and_full_size: loss 2e-6, gradient 1e-5) -----------------------------------------
AF, AT = torch.tensor([0.25, 0.5, 0.75]), torch.tensor([0.75, 0.5, 0.25])
for per in (4, 12, 1028, 8 * 5 * 4, 128 * 10 * 10):
    B = 3

    @case("lerp_fwd-%d" % per, "aesr_lerp_fwd")
    def build(leg, per=per, B=B):
        z = torch.randn(2 * B, per, generator=gen(32, per))
        pz, pa, pb, po = leg.inp("z", z), leg.inp("a_from", AF), leg.inp("a_to", AT), leg.out("zmix", B * per)
        return dict(call=lambda: L_.aesr_lerp_fwd(pz, pa, pb, po, B, per, st()),
                    verify=lambda: close(leg, "zmix", AF[:, None] * z[:B] + AT[:, None] * z[B:], None, "eq"))

    @case("lerp_bwd-%d" % per, "aesr_lerp_bwd")
    def build(leg, per=per, B=B):
        d = torch.randn(B, per, generator=gen(33, per))
        pd, pa, pb, po = leg.inp("dzmix", d), leg.inp("a_from", AF), leg.inp("a_to", AT), leg.out("dz", 2 * B * per)
        return dict(call=lambda: L_.aesr_lerp_bwd(pd, pa, pb, po, B, per, st()),
                    verify=lambda: close(leg, "dz", torch.cat([AF[:, None] * d, AT[:, None] * d]), None, "eq"))

    @case("lerp_cat_fwd-%d" % per, "aesr_lerp_cat_fwd")
    def build(leg, per=per, B=B):
        z = torch.randn(2 * B, per, generator=gen(34, per))
        pz, pa, pb, po = leg.inp("z", z), leg.inp("a_from", AF), leg.inp("a_to", AT), leg.out("zcat", 3 * B * per)
        return dict(call=lambda: L_.aesr_lerp_cat_fwd(pz, pa, pb, po, B, per, st()),
                    verify=lambda: close(leg, "zcat", torch.cat([z, AF[:, None] * z[:B] + AT[:, None] * z[B:]]), None, "eq"))

    @case("lerp_cat_bwd-%d" % per, "aesr_lerp_cat_bwd")
    def build(leg, per=per, B=B):
        g3 = torch.randn(3 * B, per, generator=gen(35, per))
        pg, pa, pb, po = leg.inp("g", g3), leg.inp("a_from", AF), leg.inp("a_to", AT), leg.out("dz", 2 * B * per)
        ref = lambda: torch.cat([g3[:B] + g3[2 * B:] * AF[:, None], g3[B:2 * B] + g3[2 * B:] * AT[:, None]])
        return dict(call=lambda: L_.aesr_lerp_cat_bwd(pg, pa, pb, po, B, per, st()), verify=lambda: close(leg, "dz", ref(), None, "eq"))

for Z, per, alphas, act in [(5, 480, [0.25, 0.5, 0.9], 1), (2, 4, [0.5], 0), (3, 1028, [i / 17.0 for i in range(1, 17)], 2)]:
    @case("lerp_multi-%dx%d-n%d" % (Z, per, len(alphas)), "aesr_lerp_multi")
    def build(leg, Z=Z, per=per, alphas=alphas, act=act):
        z = torch.randn(Z, per, generator=gen(36, Z, per))
        pz, po = leg.inp("z", z), leg.out("out", len(alphas) * (Z - 1) * per)
        fa = hip.float_array(alphas)

        def verify():
            ref = torch.cat([act_ref(float(np.float32(a)) * z[1:].double() + (1 - float(np.float32(a))) * z[:-1].double(), act) for a in alphas])
            assert torch.allclose(leg.v("out").cpu().double(), ref.reshape(-1), rtol=1e-6, atol=1e-7)
        return dict(call=lambda: L_.aesr_lerp_multi(pz, po, Z, per, fa, len(alphas), act, 0.01, st()), verify=verify)

for Z, n, per in [(2, 1, 36), (5, 0, 16), (7, 16, 60), (1, 4, 64), (30, 3, 4)]:
    @case("interleave_clamp-%dx%dx%d" % (Z, n, per), "aesr_interleave_clamp")
    def build(leg, Z=Z, n=n, per=per):
        g = gen(37, Z, n, per)
        orig = torch.rand(Z, per, generator=g) * 1.4 - 0.2
        synth = torch.rand(max(n * (Z - 1), 1), per, generator=g) * 1.4 - 0.2
        nn_ = n if Z > 1 else 0
        po_, ps = leg.inp("orig", orig), leg.inp("synth", synth)
        po = leg.out("out", ((Z - 1) * (nn_ + 1) + 1) * per)

        def verify():
            want = torch.full(((Z - 1) * (nn_ + 1) + 1, per), float("nan"))
            want[::nn_ + 1] = orig
            for k in range(nn_):
                want[k + 1::nn_ + 1] = synth.reshape(n, Z - 1, per)[k]
            close(leg, "out", want.clamp_(0, 1), None, "eq")
        return dict(call=lambda: L_.aesr_interleave_clamp(po_, ps, po, Z, n, per, 0.0, 1.0, st()), verify=verify)

N_TAILS = [1, 2, 3, 4, 1027, 4098, 24 * 160 * 160 + 3]           # n % 4 in {0, 1, 2, 3}, below one block and above
for n in N_TAILS:
    def _ab(n=n):
        g = gen(38, n)
        return torch.rand(n, generator=g), torch.rand(n, generator=g)

    for kind, fwd, bwd in (("mse", "aesr_mse_fwd", "aesr_mse_bwd"), ("l1", "aesr_l1_fwd", "aesr_l1_bwd")):
        @case("%s_fwd-%d" % (kind, n), fwd)
        def build(leg, n=n, ab=_ab, kind=kind, fwd=fwd):
            a, b = ab()
            pa, pb = leg.inp("a", a), leg.inp("b", b)
            pp, pl = leg.scratch("partial", hip.MSE_NPART, dtype=f64), leg.out("loss", 1)

            def verify():
                d = a.double() - b.double()
                ref = float((d * d).mean()) if kind == "mse" else float(d.abs().mean())
                tol = 1e-6 if kind == "mse" else 2e-6
                assert abs(float(leg.v("loss")[0]) - ref) <= tol * abs(ref), (float(leg.v("loss")[0]), ref)
            return dict(call=lambda: getattr(L_, fwd)(pa, pb, pp, pl, n, st()), verify=verify)

        @case("%s_bwd-%d" % (kind, n), bwd)
        def build(leg, n=n, ab=_ab, kind=kind, bwd=bwd):
            a, b = ab()
            pa, pb, pg, po = leg.inp("a", a), leg.inp("b", b), leg.inp("gloss", torch.tensor([0.7])), leg.out("da", n)

            def verify():
                d = a.double() - b.double()
                gl = float(np.float32(0.7))
                close(leg, "da", 2 * d * gl / n if kind == "mse" else torch.sign(d) * gl / n, 1e-6 if kind == "mse" else 1e-5)
            return dict(call=lambda: getattr(L_, bwd)(pa, pb, pg, po, n, st()), verify=verify)

    for act in (1, 3):
        @case("act_bwd-%d-a%d" % (n, act), "aesr_act_bwd")
        def build(leg, n=n, act=act):
            g = gen(39, n, act)
            y = torch.sigmoid(torch.randn(n, generator=g)) if act == 3 else F.leaky_relu(torch.randn(n, generator=g), 0.01)
            dout = torch.randn(n, generator=g)
            pd, py, po = leg.inp("dout", dout), leg.inp("y", y), leg.out("dpre", n)
            ref = lambda: dout.double() * (y.double() * (1 - y.double()) if act == 3 else torch.where(y > 0, 1.0, float(np.float32(0.01))).double())
            return dict(call=lambda: L_.aesr_act_bwd(pd, py, po, n, act, 0.01, st()), verify=lambda: close(leg, "dpre", ref(), 1e-6))

for N, M in [(3, 5), (2, 1000), (1, 1), (4, 1027), (2, 4096)]:
    @case("row_mean_fwd-%dx%d" % (N, M), "aesr_row_mean_fwd")
    def build(leg, N=N, M=M):
        x = torch.randn(N, M, generator=gen(40, N, M))
        px, po = leg.inp("x", x), leg.out("out", N)
        return dict(call=lambda: L_.aesr_row_mean_fwd(px, po, N, M, st()), verify=lambda: close(leg, "out", x.double().mean(1), 1e-6))

    @case("row_mean_bwd-%dx%d" % (N, M), "aesr_row_mean_bwd")
    def build(leg, N=N, M=M):
        g = torch.randn(N, generator=gen(41, N, M))
        pg, po = leg.inp("g", g), leg.out("dx", N * M)
        return dict(call=lambda: L_.aesr_row_mean_bwd(pg, po, N, M, st()),
                    verify=lambda: close(leg, "dx", (g.double() / M)[:, None].expand(N, M).contiguous(), 1e-6))

for sizes in [(1003, 517, 0), (5, 3, 2), (1, 1, 1), (4096, 2050, 1027)]:
    n1, n2, n3 = sizes

    def _m3(sizes=sizes):
        n1, n2, n3 = sizes
        g = gen(42, *sizes)
        return [torch.rand(n, generator=g) for n in (n1, n1, n2, n2, max(n3, 1), max(n3, 1))]

    @case("mse3_fwd-%dx%dx%d" % sizes, "aesr_mse3_fwd")
    def build(leg, sizes=sizes, m3=_m3):
        n1, n2, n3 = sizes
        a1, b1, a2, b2, a3, b3 = m3()
        # a1 and a2 are the two parts of ONE tensor, as ops.py passes flat and flat[n1:]: the second pointer is only 4-byte aligned when n1 is odd
        pa = leg.inp("a12", torch.cat([a1, a2]))
        pb1, pb2 = leg.inp("b1", b1), leg.inp("b2", b2)
        pa3, pb3 = (leg.inp("a3", a3), leg.inp("b3", b3)) if n3 else (None, None)
        plam = leg.inp("lam", torch.tensor([0.05]))
        pws = leg.state("workspace", torch.zeros(hip.MSE3_WS, dtype=f64))
        po = leg.out("out4", 4)

        def verify():
            m1, m2 = float(((a1.double() - b1.double()) ** 2).mean()), float(((a2.double() - b2.double()) ** 2).mean())
            m3_ = float(((a3.double() - b3.double()) ** 2).mean()) if n3 else 0.0
            lam = float(np.float32(0.05))
            np.testing.assert_allclose(leg.v("out4").cpu().numpy(), np.array([m1 + lam * m2, m1, lam * m2, m3_]), rtol=3e-7, atol=1e-12)

        def state_ok():           # "ws[3 * gridDim.x] is the ticket counter: zero before the first launch, left at zero"
            assert int(leg.v("workspace").view(torch.int64)[3 * 256]) == 0
        return dict(call=lambda: L_.aesr_mse3_fwd(pa, pb1, n1, leg.at("a12", n1), pb2, n2, pa3, pb3, n3, plam, pws, po, st()), verify=verify,
                    state_ok=state_ok)

    @case("mse3_bwd-%dx%dx%d" % sizes, "aesr_mse3_bwd")
    def build(leg, sizes=sizes, m3=_m3):
        n1, n2, n3 = sizes
        a1, b1, a2, b2, a3, b3 = m3()
        pa = leg.inp("a12", torch.cat([a1, a2]))
        pb1, pb2 = leg.inp("b1", b1), leg.inp("b2", b2)
        plam, pgl = leg.inp("lam", torch.tensor([0.05])), leg.inp("gloss", torch.tensor([0.7]))
        pd = leg.out("d12", n1 + n2)           # "d1, d2 may be the two parts of one tensor"

        def verify():
            lam, gl = float(np.float32(0.05)), float(np.float32(0.7))
            ref = torch.cat([(a1.double() - b1.double()) * (2 * gl / n1), (a2.double() - b2.double()) * (2 * gl * lam / n2)])
            close(leg, "d12", ref, 1e-6)
        return dict(call=lambda: L_.aesr_mse3_bwd(pa, pb1, n1, leg.at("a12", n1), pb2, n2, plam, pgl, pd, leg.at("d12", n1), st()), verify=verify)


def _adam_ref(p, grads, lr=1e-3, wd=0.01):
    pt = p.clone().double().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    outs = []
    for gr in grads:
        pt.grad = gr.clone().double()
        opt.step()
        outs.append(pt.detach().clone())
    return outs


for n in (1, 2, 3, 5, 1003, 5000, 70001, 1234567):
    @case("adam_step-%d" % n, "aesr_adam_step")
    def build(leg, n=n):
        g = gen(43, n)
        p, g1, g2 = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
        host = (ctypes.c_float * 8)()
        L_.aesr_adam_state_init(host, 0.0, 0.9, 0.999)
        state0 = torch.from_numpy(np.frombuffer(host, dtype=np.int32).copy()).view(f32)
        pp, pg = leg.inout("p", p), leg.inout("g", g1)
        pm, pv = leg.inout("exp_avg", torch.zeros(n)), leg.inout("exp_avg_sq", torch.zeros(n))
        ps = leg.state("state", state0)
        call = lambda zero_grad=1: L_.aesr_adam_step(pp, pg, pm, pv, ps, n, 1e-3, 0.9, 0.999, 1e-8, 0.01, zero_grad, st())
        refs = _adam_ref(p, [g1, g2])

        def verify():
            close(leg, "p", refs[0], 1e-6)
            assert float(leg.v("g").abs().max()) == 0.0           # zero_grad != 0 leaves g at zero

        def state_ok(steps=1):
            s = leg.v("state")
            assert float(s[0]) == steps and int(s.view(torch.int32)[3]) == 0           # the ticket counter is back at zero

        def reuse():
            """The second step on the same, not re-initialised state is the correct second step."""
            leg.v("g").copy_(g2.cuda())
            assert call(0) == 0
            torch.cuda.synchronize()
            close(leg, "p", refs[1], 1e-6)
            assert torch.equal(leg.v("g").cpu(), g2)           # zero_grad == 0: untouched
            state_ok(2)
        return dict(call=call, verify=verify, state_ok=state_ok, reuse=reuse)


# ---- Laplacian pyramid (test_blur_adjoint_and_down_up_are_transposes: blur 1e-6, down2 bit-equal) ------------------------------------------
K5 = (torch.outer(torch.tensor([1., 4, 6, 4, 1], dtype=f64), torch.tensor([1., 4, 6, 4, 1], dtype=f64)) / 256)[None, None]
for P, H, W in [(2, 9, 14), (1, 3, 3), (3, 7, 5), (1, 33, 130)]:
    tag = "%dx%dx%d" % (P, H, W)
    for adjoint in (0, 1):
        @case("lap_blur5-%s-adj%d" % (tag, adjoint), "aesr_lap_blur5")
        def build(leg, P=P, H=H, W=W, adjoint=adjoint):
            g = gen(44, P, H, W)
            x, add = torch.rand(P, H, W, generator=g), torch.rand(P, H, W, generator=g)
            px, pa, po = leg.inp("in", x), leg.inp("add", add), leg.out("out", P * H * W)

            def verify():
                xd = x.double().requires_grad_(True)
                blur = F.conv2d(F.pad(xd[:, None], (2, 2, 2, 2), mode="reflect"), K5)[:, 0]
                if adjoint:           # the transposed operator applied to x: the gradient of <G u, x> w.r.t. u
                    u = torch.zeros(P, H, W, dtype=f64, requires_grad=True)
                    (F.conv2d(F.pad(u[:, None], (2, 2, 2, 2), mode="reflect"), K5)[:, 0] * x.double()).sum().backward()
                    blur = u.grad
                close(leg, "out", add.double() + 4.0 * blur.detach(), 1e-6)
            return dict(call=lambda: L_.aesr_lap_blur5(px, pa, po, P, H, W, 4.0, adjoint, st()), verify=verify)

for P, H, W in [(2, 9, 14), (1, 3, 3), (3, 7, 5)]:
    @case("lap_blur5-noadd-%dx%dx%d" % (P, H, W), "aesr_lap_blur5")
    def build(leg, P=P, H=H, W=W):
        x = torch.rand(P, H, W, generator=gen(50, P, H, W))
        px, po = leg.inp("in", x), leg.out("out", P * H * W)
        ref = lambda: F.conv2d(F.pad(x.double()[:, None], (2, 2, 2, 2), mode="reflect"), K5)[:, 0]
        return dict(call=lambda: L_.aesr_lap_blur5(px, None, po, P, H, W, 1.0, 0, st()), verify=lambda: close(leg, "out", ref(), 1e-6))

for P, H, W in [(2, 9, 14), (1, 1, 1), (3, 7, 5), (2, 8, 12), (1, 33, 130)]:
    tag = "%dx%dx%d" % (P, H, W)

    @case("lap_down2-" + tag, "aesr_lap_down2")
    def build(leg, P=P, H=H, W=W):
        x = torch.rand(P, H, W, generator=gen(45, P, H, W))
        px, po = leg.inp("in", x), leg.out("out", P * ((H + 1) // 2) * ((W + 1) // 2))
        return dict(call=lambda: L_.aesr_lap_down2(px, po, P, H, W, st()), verify=lambda: close(leg, "out", x[:, ::2, ::2].contiguous(), None, "eq"))

    @case("lap_zero_insert2-" + tag, "aesr_lap_zero_insert2")
    def build(leg, P=P, H=H, W=W):
        h, w = (H + 1) // 2, (W + 1) // 2
        y = torch.rand(P, h, w, generator=gen(46, P, H, W))
        py, po = leg.inp("in", y), leg.out("out", P * H * W)

        def verify():
            z = torch.zeros(P, H, W)
            z[:, ::2, ::2] = y
            close(leg, "out", z, None, "eq")
        return dict(call=lambda: L_.aesr_lap_zero_insert2(py, po, P, h, w, H, W, st()), verify=verify)


# ---- batch assembly, metrics (tests/test_gpu_augment.py 2e-6; tests/test_gpu_metrics.py: SSIM 1e-9 abs, MSE 1e-9 rel, VIF 1e-10;
#      tests/test_gpu_long_axis.py: bitwise) ----------------------------------------------------------------------------------------------
@case("triplet_assemble", "aesr_triplet_assemble")
def build(leg):
    """Crops that reach into the zero padding on every side, every rotation, a second volume at an odd float offset inside `volumes`."""
    rs = np.random.RandomState(3)
    vols = [rs.rand(5, 13, 9).astype(np.float32), rs.rand(4, 20, 31).astype(np.float32)]
    offs = [0, vols[0].size]
    width = 12
    trip = [(0, 0, 4, 2, -2, -3, 0), (0, 1, 3, 2, 5, 1, 1), (1, 3, 0, 1, 10, 25, 2), (1, 2, 1, 3, -5, -4, 3), (0, 4, 4, 4, 0, 0, 2)]
    B = len(trip)
    descs = (hip.TripletDesc * B)()
    params = []
    for i, (vid, zf, zt, zb, oy, ox, k) in enumerate(trip):
        gain, cutoff = float(rs.uniform(2.5, 7.5)), float(rs.uniform(0.25, 0.75))
        Z, H, W = vols[vid].shape
        descs[i] = hip.TripletDesc(offs[vid], H, W, zf, zt, zb, oy, ox, k, gain, cutoff)
        params.append((np.float32(gain), np.float32(cutoff)))
    pv = leg.inp("volumes", torch.from_numpy(np.concatenate([v.reshape(-1) for v in vols])))
    pi, pb = leg.out("image", 2 * B * width * width), leg.out("between", B * width * width)

    def verify():
        img, btw = np.zeros((2 * B, width, width)), np.zeros((B, width, width))
        for i, (vid, zf, zt, zb, oy, ox, k) in enumerate(trip):
            Z, H, W = vols[vid].shape
            pad = np.zeros((Z, H + 2 * 32, W + 2 * 32))
            pad[:, 32:32 + H, 32:32 + W] = vols[vid]
            crop = pad[[zf, zt, zb], 32 + oy:32 + oy + width, 32 + ox:32 + ox + width]
            gain, cutoff = params[i]
            out = np.rot90(1 / (1 + np.exp(float(gain) * (float(cutoff) - crop))), k, (1, 2))
            img[i], img[B + i], btw[i] = out[0], out[1], out[2]
        close(leg, "image", torch.from_numpy(img), 2e-6, "abs")
        close(leg, "between", torch.from_numpy(btw), 2e-6, "abs")
    return dict(call=lambda: L_.aesr_triplet_assemble(pv, descs, B, width, pi, pb, st()), verify=verify)


for Z, H, W in [(3, 33, 47), (1, 7, 9), (4, 16, 16), (2, 5, 130)]:
    @case("ssim_mse-%dx%dx%d" % (Z, H, W), "aesr_ssim_mse")
    def build(leg, Z=Z, H=H, W=W):
        from oracle import step_oracle
        g = gen(47, Z, H, W)
        a = torch.rand(Z, H, W, generator=g)
        b = (a + 0.1 * torch.randn(Z, H, W, generator=g)).clamp(0, 1)
        win = 7 if min(H, W) >= 8 else 5
        pa, pb = leg.inp("a", a), leg.inp("b", b)
        pws = leg.scratch("workspace", L_.aesr_ssim_workspace_doubles(Z, H, W), dtype=f64)
        ps, pm = leg.out("ssim", Z, dtype=f64), leg.out("mse", Z, dtype=f64)

        def verify():
            for z in range(Z):
                assert abs(float(leg.v("ssim")[z]) - step_oracle.ssim(a[z], b[z], data_range=1.0, win=win)) < 1e-9
                ref_m = float(((a[z].double() - b[z].double()) ** 2).mean())
                assert abs(float(leg.v("mse")[z]) - ref_m) < 1e-9 * ref_m
        return dict(call=lambda: L_.aesr_ssim_mse(pa, pb, pws, ps, pm, Z, H, W, win, 1.0, 0.01, 0.03, st()), verify=verify)

for Z, H, W in [(2, 33, 47), (2, 9, 5), (1, 1, 1), (3, 28, 28)]:
    @case("vif_mscale-%dx%dx%d" % (Z, H, W), "aesr_vif_mscale")
    def build(leg, Z=Z, H=H, W=W):
        from oracle import vif_oracle as vo
        from evaluate.metrics import gaussian_kernel1d
        g = gen(48, Z, H, W)
        a = (torch.rand(Z, H, W, generator=g) * 1.3 - 0.15).clamp(0, 1)
        a[:, : H // 3, : W // 2] = 200.0 / 255.0
        b = (0.85 * a + 0.06 * torch.randn(Z, H, W, generator=g)).clamp(0, 1)
        if Z > 1:
            a[-1] = 0.0           # black reference slice: NaN
        ks = [gaussian_kernel1d((2 ** (4 - s + 1) + 1) / 5.0) for s in range(1, 5)]
        wts, rad = hip.double_array(np.concatenate([k[0] for k in ks])), hip.int_array([k[1] for k in ks])
        pa, pb = leg.inp("ref", a), leg.inp("dist", b)
        pws = leg.scratch("workspace", L_.aesr_vif_workspace_bytes(Z, H, W), dtype=torch.uint8)
        po = leg.out("vif", Z, dtype=f64)

        def verify():
            got = leg.v("vif").cpu().numpy()
            want = np.array([vo.vifp_mscale(vo.to_uint8(a[z].numpy()), vo.to_uint8(b[z].numpy())) for z in range(Z)])
            assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
            ok = ~np.isnan(want)
            assert (not ok.any()) or np.abs(got[ok] - want[ok]).max() < 1e-10, (got, want)
        return dict(call=lambda: L_.aesr_vif_mscale(pa, pb, pws, po, Z, H, W, wts, rad, 2.0, st()), verify=verify)

for Z, H, W in [(6, 40, 48), (10, 33, 47), (1, 7, 9), (3, 1, 5), (5, 12, 16), (65, 17, 130)]:
    for axis in (1, 2):
        @case("long_axis_views-%dx%dx%d-ax%d" % (Z, H, W, axis), "aesr_long_axis_views")
        def build(leg, Z=Z, H=H, W=W, axis=axis):
            g = gen(49, Z, H, W)
            ref, rec = torch.rand(Z, H, W, generator=g), torch.rand(Z, H, W, generator=g)
            ref[:, :min(3, H), :] = 0.0
            ref[:, :, W - min(4, W):] = 0.0
            ref[:, 0, :] = -0.0
            if H >= 2:
                ref[Z - 1, 1, W - 1] = 1e-30
            pr, pc = leg.inp("ref", ref), leg.inp("rec", rec)
            o1, o2 = leg.out("ref_view", Z * H * W), leg.out("rec_view", Z * H * W)
            ob = leg.out("black", H if axis == 1 else W, dtype=torch.uint8)

            def verify():
                wr, wc = torch.swapaxes(ref, 0, axis).contiguous(), torch.swapaxes(rec, 0, axis).contiguous()
                assert torch.equal(mg.bits(leg.v("ref_view")), mg.bits(wr)) and torch.equal(mg.bits(leg.v("rec_view")), mg.bits(wc))
                assert torch.equal(leg.v("black").cpu(), (wr == 0).flatten(1).all(1).to(torch.uint8))
            return dict(call=lambda: L_.aesr_long_axis_views(pr, pc, o1, o2, ob, Z, H, W, axis, st()), verify=verify)


# ---- the test -----------------------------------------------------------------------------------------------------------------------------
def covered_entries():
    return {e for c in CASES for e in c.entries}


def _run_leg(c, poison, sp=0, st_=0, may_refuse=False):
    leg = Leg(poison, sp, st_)
    spec = c.build(leg)
    torch.cuda.synchronize()
    leg.freeze()
    rc = spec["call"]()
    torch.cuda.synchronize()
    SEEN["legs"] += 1
    what = "%s [poison %s, param shift %d, tensor shift %d]" % (c.id, poison, sp, st_)
    mg.assert_guards_intact([b.g for b in leg.bufs.values()])
    for name, b in leg.bufs.items():
        if b.role == "in":
            mg.assert_unchanged(b.g.view, b.saved, "%s: %s" % (what, name))
    if rc != 0:
        msg = hip.last_error()
        unsupported = spec.get("expect_rc", 0) == rc           # a layer the entry point's own *_supported query turns down (AESR_ERR_UNSUPPORTED)
        assert may_refuse or unsupported, "%s: rc %d: %s" % (what, rc, msg)
        assert unsupported or "align" in msg.lower(), "%s: refused without naming the alignment: %r" % (what, msg)
        for name, b in leg.bufs.items():
            if b.role == "out":
                assert mg.poison_left(b.g.view, poison).numel() == b.g.view.numel(), "%s: refused, yet %s was written" % (what, name)
            elif b.role in ("inout", "state"):
                mg.assert_unchanged(b.g.view, b.saved, "%s: refused, yet %s" % (what, name))
        if not unsupported:
            SEEN["refused"].append(c.id)
        return None, spec
    for name, b in leg.bufs.items():
        if b.role == "out":
            left = mg.poison_left(b.g.view, poison)
            allowed = set(b.untouched or ())
            bad = [i for i in left.tolist() if i not in allowed]
            assert not bad, "%s: %d element(s) of %s never written, first %d, last %d" % (what, len(bad), name, bad[0], bad[-1])
    return leg, spec


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        diff = (a[k] != b[k]).nonzero().flatten()
        assert diff.numel() == 0, "%s: %s differs from leg 1 in %d element(s), first %d, last %d" % (what, k, diff.numel(), int(diff[0]), int(diff[-1]))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_guarded(c, monkeypatch):
    assert torch.cuda.is_available()
    leg_env.clear()
    for k, v in c.env.items():
        monkeypatch.setenv(k, str(v))
        leg_env[k] = str(v)
    # leg 1: NaN poison, aligned
    leg, spec = _run_leg(c, mg.POISON_NAN)
    if leg is None:           # the layer does not fit this entry point: it said so, and wrote nothing
        SEEN["ran"].add(c.id)
        return
    spec["verify"]()
    if "state_ok" in spec:
        spec["state_ok"]()
    want = leg.result_bits()
    SEEN["poisons"].add(mg.POISON_NAN)
    # leg 2: finite poison, aligned
    leg2, _ = _run_leg(c, mg.POISON_FINITE)
    _same_bits(leg2.result_bits(), want, c.id + " [finite poison]")
    SEEN["poisons"].add(mg.POISON_FINITE)
    # leg 3: state reuse
    if any(b.role == "state" for b in leg.bufs.values()):
        leg3, spec3 = _run_leg(c, mg.POISON_FINITE)
        if "reuse" in spec3:
            spec3["reuse"]()
        else:
            leg3.repoison()
            torch.cuda.synchronize()
            assert spec3["call"]() == 0
            torch.cuda.synchronize()
            mg.assert_guards_intact([b.g for b in leg3.bufs.values()])
            _same_bits(leg3.result_bits(), want, c.id + " [second call on the same state]")
            if "state_ok" in spec3:
                spec3["state_ok"]()
    # leg 4p: parameter-class pointers 4 bytes after a 16-byte boundary (and 8, 12: a slice of a flat buffer starts anywhere) -- must work
    if any(b.cls == "param" for b in leg.bufs.values()):
        for shift in (1, 2, 3):
            leg4, _ = _run_leg(c, mg.POISON_NAN, sp=shift)
            _same_bits(leg4.result_bits(), want, c.id + " [param pointers shifted by %d elements]" % shift)
    # leg 4t: tensor-class pointers shifted -- bit-identical, or refused by name with nothing written
    if any(b.cls == "tensor" for b in leg.bufs.values()):
        for shift in (1, 2, 3):
            leg5, _ = _run_leg(c, mg.POISON_NAN, st_=shift, may_refuse=True)
            if leg5 is not None:
                _same_bits(leg5.result_bits(), want, c.id + " [tensor pointers shifted by %d elements]" % shift)
    SEEN["ran"].add(c.id)


def test_helper_sees_planted_damage_on_the_device():
    """The checker on device memory: a guard word, an input element and an output element changed by THIS test through torch (inside the test's
    own allocation; no kernel is made to write out of range) are each reported."""
    g = mg.guarded(10, f32, "cuda", mg.POISON_NAN, 1, name="probe")
    assert g.view.data_ptr() % 16 == 4
    mg.assert_guards_intact([g])
    assert mg.poison_left(g.view, mg.POISON_NAN).numel() == 10
    off = g.front_bytes + g.payload_bytes
    g.backing[off:off + 4] = 0
    with pytest.raises(AssertionError, match="probe: back guard damaged, 1 word"):
        mg.assert_guards_intact([g])
    g.backing[g.front_bytes - 4:g.front_bytes] = 0
    assert [d[0] for d in mg.guard_damage(g)] == ["front", "back"]
    x = mg.guarded(8, f32, "cuda", torch.arange(8, dtype=f32), name="x")
    saved = mg.bits(x.view)
    x.view[3] = -1.0
    with pytest.raises(AssertionError, match="x: input modified, 1 element"):
        mg.assert_unchanged(x.view, saved, "x")


def test_every_path_was_guarded():
    """Module end: a planner change must not quietly drop a kernel out of this suite."""
    if len(SEEN["ran"]) != len(CASES):
        pytest.skip("only part of the case table ran in this process (%d of %d)" % (len(SEEN["ran"]), len(CASES)))
    assert SEEN["wino_fwd"] >= {1, 2, 3}, SEEN["wino_fwd"]
    assert SEEN["wino_dgrad"] >= {1, 2, 3}, SEEN["wino_dgrad"]
    assert SEEN["igemm_ksplit"] > 0 and SEEN["ring_ksplit"] > 0 and SEEN["bn_fused1"] > 0
    assert SEEN["poisons"] == {mg.POISON_NAN, mg.POISON_FINITE}
    assert L_.aesr_conv2d_wino_ring_timeouts() == 0 and L_.aesr_bn_fused1_timeouts() == 0
    print("\nmemguard: %d cases, %d legs; tensor-class 4-byte alignment refused by: %s" % (len(CASES), SEEN["legs"], sorted(set(SEEN["refused"])) or "none"))
