"""-m gpu: the Cout == 1 output convolution's backward in one pass (aesr_conv2d_cout1_bwd, include/aesr_hip_train.h; csrc/conv_thin.hip
thin_reduce_kernel<false, true> + thin_cout1_finish_kernel) against the three calls it replaces and against PyTorch-CPU autograd.

- Every shape x own activation {none (out = NULL), sigmoid} x mask {none, LeakyReLU 0.01, ReLU}: dx, dw and db start as NaN and none is left;
  ``torch.equal`` with aesr_act_bwd -> aesr_conv2d_cout1_wgrad + aesr_conv2d_cout1_dgrad_pre on the same inputs (the library is built with
  contraction off and the fused kernels keep the operation order of the unfused ones, so the bits must agree); rel-L2 < 1e-5 against autograd of
  act(conv2d(A, w, b, padding=1)), the bound of tests/test_gpu_kernels.py::test_cout1_conv_backward.
- The entry point between the guard bands of tests/memguard.py at its contractual sizes: NaN and 3e38 poisons in outputs and workspace, inputs
  unchanged, every pointer shifted by one element; refusals write nothing.
- Engine level: a decoder-shaped pass and the small trainer fixture with ``engine.FUSE_COUT1_BWD`` off and on, eagerly and in a captured
  step graph: gradients and final state ``torch.equal``.

GUARDED_ENTRIES and EXEMPT partition ``_hip.SIGNATURES_TRAIN`` (tests/test_abi.py checks that without a GPU)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memguard as mg

pytestmark = pytest.mark.gpu

GUARDED_ENTRIES = ("aesr_conv2d_cout1_bwd",)
EXEMPT = {"aesr_conv2d_cout1_bwd_workspace_floats": "host query"}
TOL = 1e-5                                           # test_cout1_conv_backward's bound
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
SHAPES = [(1, 1, 1, 4), (2, 12, 12, 8), (3, 37, 70, 16), (1, 9, 130, 64), (2, 5, 3, 256), (2, 24, 20, 32), (6, 160, 160, 32)]
GUARD_SHAPES = [(1, 1, 1, 4), (2, 12, 12, 8), (1, 9, 130, 64)]
OWN_ACTS = [ACT_NONE, ACT_SIGMOID]
MASKS = [(ACT_NONE, 0.0), (ACT_LRELU, 0.01), (ACT_RELU, 0.0)]


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=2)
def _inputs(shape, act, mask_act):
    """Seeded fp32 inputs (CPU, the device's layouts) and the fp64 autograd reference, made once per case and left unchanged."""
    N, H, W, cin = shape
    g = torch.Generator().manual_seed(1000 * cin + 10 * H + W + 3 * act + mask_act)
    h = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(1, cin, 3, 3, generator=g) / float(np.sqrt(9 * cin))
    b = torch.randn(1, generator=g)
    dout = torch.randn(N, 1, H, W, generator=g)
    A = F.relu(h) if mask_act == ACT_RELU else F.leaky_relu(h, 0.01)               # the saved input: the output of the activation in front
    pre = F.conv2d(A, w, b, padding=1)
    out = torch.sigmoid(pre) if act == ACT_SIGMOID else pre
    # reference: autograd in fp64 on the same fp32 values; the data gradient is taken at A (no mask) or in front of the mask activation
    h64, w64, b64 = h.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    A64 = (F.relu(h64) if mask_act == ACT_RELU else F.leaky_relu(h64, 0.01))
    if mask_act == ACT_NONE:
        A64 = A64.detach().requires_grad_(True)
    pre64 = F.conv2d(A64, w64, b64, padding=1)
    (torch.sigmoid(pre64) if act == ACT_SIGMOID else pre64).backward(dout.double())
    dx_ref = A64.grad if mask_act == ACT_NONE else h64.grad
    flipped = w.reshape(cin, 9).flip(1).t().contiguous()                            # wexp[t][ci] = W[0, ci, 8 - t]
    return dict(x=nhwc(A), dout=dout.reshape(N, H, W).contiguous(), out=out.reshape(N, H, W).contiguous(), flipped=flipped,
                dx_ref=nhwc(dx_ref), dw_ref=w64.grad, db_ref=b64.grad)


def _unfused(hip, d, shape, act, mask_act, mslope):
    """aesr_act_bwd -> aesr_conv2d_cout1_wgrad + aesr_conv2d_cout1_dgrad_pre: (dx, dw, db) on the device."""
    N, H, W, cin = shape
    L = hip.lib
    x, dout, out, fl = d["x"].cuda(), d["dout"].cuda(), d["out"].cuda(), d["flipped"].cuda()
    dpre = dout
    if act != ACT_NONE:
        dpre = torch.empty_like(dout)
        hip.check(L.aesr_act_bwd(hip.ptr(dout), hip.ptr(out), hip.ptr(dpre), dout.numel(), act, 0.0, hip.stream()), "aesr_act_bwd")
    dw, db = torch.full((1, cin, 3, 3), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    dx = torch.full((N, H, W, cin), float("nan"), device="cuda")
    ws = torch.empty(L.aesr_conv2d_cout1_workspace_floats(cin), device="cuda")
    hip.check(L.aesr_conv2d_cout1_wgrad(hip.ptr(x), hip.ptr(dpre), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), N, H, W, cin, hip.stream()), "wgrad")
    hip.check(L.aesr_conv2d_cout1_dgrad_pre(hip.ptr(dpre), hip.ptr(fl), hip.ptr(x) if mask_act != ACT_NONE else None, hip.ptr(dx), N, H, W, cin,
                                            mask_act, mslope, hip.stream()), "dgrad_pre")
    torch.cuda.synchronize()
    return dx, dw, db


@pytest.mark.parametrize("mask", MASKS, ids=["mask_none", "mask_lrelu", "mask_relu"])
@pytest.mark.parametrize("act", OWN_ACTS, ids=["act_none", "act_sigmoid"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fused_backward_equals_unfused_and_autograd(shape, act, mask):
    from superresolution_aniso_mri_amd import _hip as hip
    mask_act, mslope = mask
    N, H, W, cin = shape
    d = _inputs(shape, act, mask_act)
    L = hip.lib
    x, dout, fl = d["x"].cuda(), d["dout"].cuda(), d["flipped"].cuda()
    out = d["out"].cuda() if act != ACT_NONE else None
    dw, db = torch.full((1, cin, 3, 3), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    dx = torch.full((N, H, W, cin), float("nan"), device="cuda")
    nws = L.aesr_conv2d_cout1_bwd_workspace_floats(cin)
    assert nws == (512 + 1) * 10 * cin
    ws = torch.full((nws,), float("nan"), device="cuda")
    hip.check(L.aesr_conv2d_cout1_bwd(hip.ptr(x), hip.ptr(dout), hip.ptr(out), hip.ptr(fl), hip.ptr(dw), hip.ptr(db), hip.ptr(dx), hip.ptr(ws),
                                      N, H, W, cin, act, 0.0, mask_act, mslope, hip.stream()), "aesr_conv2d_cout1_bwd")
    torch.cuda.synchronize()
    for name, t in (("dx", dx), ("dw", dw), ("db", db)):
        assert not bool(torch.isnan(t).any()), "%s: NaN left" % name
    dx0, dw0, db0 = _unfused(hip, d, shape, act, mask_act, mslope)
    errs = (rel_l2(dx, d["dx_ref"]), rel_l2(dw, d["dw_ref"]), rel_l2(db, d["db_ref"]))
    print("%s act %d mask %d: rel-L2 vs autograd dx %.3g dw %.3g db %.3g" % ((shape, act, mask_act) + errs))
    assert torch.equal(dx, dx0), "dx differs from the unfused path in %d element(s)" % int((dx != dx0).sum())
    assert torch.equal(dw, dw0), "dw differs from the unfused path in %d element(s)" % int((dw != dw0).sum())
    assert torch.equal(db, db0), "db differs from the unfused path"
    assert max(errs) < TOL, errs


# ---- between guard bands ----------------------------------------------------------------------------------------------------------------
def _guarded_call(hip, d, shape, poison, shift, act=ACT_SIGMOID, mask_act=ACT_LRELU, mslope=0.01, cin_arg=None, n_arg=None, null_dx=False):
    N, H, W, cin = shape
    L = hip.lib
    ins = {k: mg.guarded(d[k].numel(), torch.float32, "cuda", d[k].reshape(-1), shift, k) for k in ("x", "dout", "out", "flipped")}
    outs = {"dw": mg.guarded(9 * cin, torch.float32, "cuda", poison, shift, "dw"), "db": mg.guarded(1, torch.float32, "cuda", poison, shift, "db"),
            "dx": mg.guarded(N * H * W * cin, torch.float32, "cuda", poison, shift, "dx"),
            "workspace": mg.guarded(L.aesr_conv2d_cout1_bwd_workspace_floats(cin), torch.float32, "cuda", poison, shift, "workspace")}
    for g in list(ins.values()) + list(outs.values()):
        assert g.view.data_ptr() % 16 == 4 * shift
    saved = {k: mg.bits(g.view) for k, g in ins.items()}
    p = lambda g: ctypes.c_void_p(g.view.data_ptr())            # noqa: E731
    torch.cuda.synchronize()
    rc = L.aesr_conv2d_cout1_bwd(p(ins["x"]), p(ins["dout"]), p(ins["out"]), p(ins["flipped"]), p(outs["dw"]), p(outs["db"]),
                                 None if null_dx else p(outs["dx"]), p(outs["workspace"]), N if n_arg is None else n_arg, H, W,
                                 cin if cin_arg is None else cin_arg, act, 0.0, mask_act, mslope, hip.stream())
    torch.cuda.synchronize()
    mg.assert_guards_intact(list(ins.values()) + list(outs.values()))
    for k, g in ins.items():
        mg.assert_unchanged(g.view, saved[k], k)
    return rc, outs


@pytest.mark.parametrize("shape", GUARD_SHAPES, ids=["x".join(map(str, s)) for s in GUARD_SHAPES])
def test_guard_bands_poisons_and_offset_pointers(shape):
    """NaN poison, finite poison, every pointer one element past a 16-byte boundary: guards intact, inputs unchanged, every output element
    written, the poisoned workspace never read before it is written (results bit-identical across the legs and equal to the unfused path)."""
    from superresolution_aniso_mri_amd import _hip as hip
    d = _inputs(shape, ACT_SIGMOID, ACT_LRELU)
    want = [mg.bits(t) for t in _unfused(hip, d, shape, ACT_SIGMOID, ACT_LRELU, 0.01)]
    for poison, shift in ((mg.POISON_NAN, 0), (mg.POISON_FINITE, 0), (mg.POISON_NAN, 1), (mg.POISON_FINITE, 1)):
        rc, outs = _guarded_call(hip, d, shape, poison, shift)
        assert rc == 0, hip.last_error()
        for k in ("dx", "dw", "db"):
            left = mg.poison_left(outs[k].view, poison)
            assert left.numel() == 0, "%s: %d element(s) never written, first %d [poison %s, shift %d]" % (k, left.numel(), int(left[0]), poison, shift)
        for k, w in zip(("dx", "dw", "db"), want):
            assert torch.equal(mg.bits(outs[k].view), w), "%s differs from the unfused path [poison %s, shift %d]" % (k, poison, shift)


def test_refusals_write_nothing():
    from superresolution_aniso_mri_amd import _hip as hip
    shape = (2, 12, 12, 8)
    d = _inputs(shape, ACT_SIGMOID, ACT_LRELU)
    for kwargs in (dict(cin_arg=12), dict(null_dx=True), dict(n_arg=0)):
        for poison in (mg.POISON_NAN, mg.POISON_FINITE):
            rc, outs = _guarded_call(hip, d, shape, poison, 0, **kwargs)
            assert rc == 1 and "aesr_conv2d_cout1_bwd" in hip.last_error(), (kwargs, rc, hip.last_error())
            for k, g in outs.items():
                assert mg.poison_left(g.view, poison).numel() == g.view.numel(), "%s: refused, yet %s was written" % (kwargs, k)


# ---- engine level -----------------------------------------------------------------------------------------------------------------------
class _Spy:
    """``engine.lib`` with the calls of a few entry points counted."""

    def __init__(self, lib, names):
        self._lib, self.calls = lib, {n: 0 for n in names}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in self.calls:
            def counted(*a, _fn=fn, _name=name):
                self.calls[_name] += 1
                return _fn(*a)
            return counted
        return fn


_WATCHED = ("aesr_conv2d_cout1_bwd", "aesr_act_bwd", "aesr_conv2d_cout1_wgrad", "aesr_conv2d_cout1_dgrad_pre")


@pytest.mark.parametrize("last_act", [torch.nn.Sigmoid, None], ids=["sigmoid", "linear"])
def test_engine_decoder_pass_switch_off_equals_switch_on(monkeypatch, last_act):
    """A decoder-shaped stack (3x3 convolutions + LeakyReLU, then Cin -> 1 + Sigmoid) through SequentialRunner.backward with the switch off and
    on from the same state: the input gradient and every parameter gradient bit-equal; the fused entry point ran on one leg only."""
    import torch.nn as nn
    from superresolution_aniso_mri_amd import engine
    torch.manual_seed(3)
    mods = [nn.Conv2d(8, 16, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(16, 16, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(16, 1, 3, padding=1)]
    if last_act is not None:
        mods.append(last_act())
    seq = nn.Sequential(*mods).cuda()
    N, H, W = 3, 21, 37
    x = torch.randn(N, H, W, 8, device="cuda")
    gout = torch.randn(N, H, W, 1, device="cuda")
    got = {}
    for on in (False, True):
        monkeypatch.setattr(engine, "FUSE_COUT1_BWD", on)
        spy = _Spy(engine.lib, _WATCHED)
        monkeypatch.setattr(engine, "lib", spy)
        runner = engine.SequentialRunner(seq)
        out, saved, steps = runner.forward(x, [0, N], True, True, fused=False)
        dx, grads = runner.backward(gout, saved, [0, N], N, True, steps=steps)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine, "lib", spy._lib)
        assert all(v is not None for v in grads.values()) and len(grads) == 6
        got[on] = (dx.clone(), {k: v.clone() for k, v in grads.items()}, dict(spy.calls))
    n_act = 1 if last_act is not None else 0
    assert got[False][2] == {"aesr_conv2d_cout1_bwd": 0, "aesr_act_bwd": n_act, "aesr_conv2d_cout1_wgrad": 1, "aesr_conv2d_cout1_dgrad_pre": 1}
    assert got[True][2] == {"aesr_conv2d_cout1_bwd": 1, "aesr_act_bwd": 0, "aesr_conv2d_cout1_wgrad": 0, "aesr_conv2d_cout1_dgrad_pre": 0}
    assert torch.equal(got[False][0], got[True][0]) and float(got[True][0].abs().max()) > 0
    for p in seq.parameters():
        assert torch.equal(got[False][1][p], got[True][1][p])


def test_trainer_steps_switch_off_equals_switch_on_eager_and_graphed(monkeypatch):
    """The small trainer fixture, three steps from the same state with the switch off and on, eagerly and with a captured step graph: the
    gradients of the first step, the logged losses and the final state are bit-equal on all four legs."""
    from test_gpu_step import GOLDEN, _batch, make_trainer
    from superresolution_aniso_mri_amd import engine
    rec = dict(np.load(os.path.join(GOLDEN, "step_k3_cardiac_mse.npz")))
    legs = {}
    for on in (False, True):
        for graphed in (False, True):
            monkeypatch.setattr(engine, "FUSE_COUT1_BWD", on)
            spy = _Spy(engine.lib, _WATCHED)
            monkeypatch.setattr(engine, "lib", spy)
            tr = make_trainer("cardiac_mse", rec)
            if graphed:
                tr.enable_step_graph(eager_steps=1)
            grads0 = None
            for step in range(3):
                tr.train(_batch(rec, step), keep_predictions=False)
                if step == 0:
                    grads0 = [p.grad.detach().clone() for p in tr.model.parameters()]
            torch.cuda.synchronize()
            monkeypatch.setattr(engine, "lib", spy._lib)
            assert (spy.calls["aesr_conv2d_cout1_bwd"] > 0) == on and (spy.calls["aesr_conv2d_cout1_dgrad_pre"] > 0) == (not on), spy.calls
            if graphed:
                assert len(tr._graphs) == 1
            legs[(on, graphed)] = (grads0, {k: v.detach().clone() for k, v in tr.model.state_dict().items()}, tr.losses["loss_ae"].floats())
    base = legs[(False, False)]
    for key, (grads0, state, losses) in legs.items():
        assert losses == base[2], key
        for a, b in zip(grads0, base[0]):
            assert torch.equal(a, b), key
        for k in state:
            assert torch.equal(state[k], base[1][k]), (key, k)
