"""-m gpu: every HIP kernel of libaesr_hip.so, called through the C ABI, against a PyTorch-CPU fp32 reference
of the same op on the same seeded inputs.  Tolerances are fp32 summation-order tolerances (the MFMA path is an
exact-fp32 fma chain): rel-L2 <= 1e-5 for forward ops, <= 1e-4 for long reductions (wgrad)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from superresolution_aniso_mri_amd import _hip
    assert torch.cuda.is_available()
    return _hip


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


_KEEP = []


def D(t):
    """Host tensor -> device tensor that stays alive until the test ends (kernels are asynchronous: a temporary
    whose only reference dies right after hip.ptr() could be recycled by the caching allocator before it is read)."""
    t = t.cuda() if not t.is_cuda else t
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_keepalive():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


CONV_CASES = [
    # N, H, W, Cin, Cout, KS, pad
    (2, 162, 162, 32, 32, 3, 1),     # enc.1/enc.3 of the ACDC model (odd size, 27x18 tiles)
    (3, 81, 81, 32, 64, 3, 1),
    (2, 40, 40, 64, 128, 3, 1),
    (2, 40, 40, 128, 128, 3, 1),
    (5, 10, 10, 64, 64, 3, 1),       # multi-image tiles (TI > 1)
    (2, 33, 35, 8, 16, 3, 1),        # channel counts below one MFMA block
    (1, 20, 20, 16, 1, 3, 1),        # Cout = 1 padded to 16 (output conv)
    (2, 17, 19, 16, 32, 1, 0),       # 1x1
    (1, 7, 7, 4, 8, 3, 1),
]


def _pack(hip, w, transpose):
    cout, cin, ks, _ = w.shape
    n = hip.lib.aesr_conv2d_packed_floats(cout, cin, ks, transpose)
    p = torch.empty(n, device="cuda")
    hip.check(hip.lib.aesr_conv2d_pack(hip.ptr(w), hip.ptr(p), cout, cin, ks, transpose, hip.stream()), "pack")
    return p


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("act", [0, 1, 3])
def test_conv_fwd(hip, case, act):
    N, H, W, Cin, Cout, KS, pad = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KS, KS, generator=g) / np.sqrt(Cin * KS * KS)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x, w, b, padding=pad)
    ref = {0: ref, 1: F.leaky_relu(ref, 0.01), 3: torch.sigmoid(ref)}[act]
    xd, wd, bd = nhwc(x).cuda(), w.cuda(), b.cuda()
    Ho, Wo = ref.shape[2:]
    out = torch.full((N, Ho, Wo, Cout), float("nan"), device="cuda")
    hip.check(hip.lib.aesr_conv2d_fwd(hip.ptr(xd), hip.ptr(D(_pack(hip, wd, 0))), hip.ptr(bd), hip.ptr(out), N, H, W, Cin, Cout,
                                      KS, pad, act, 0.01, hip.stream()), "conv_fwd")
    torch.cuda.synchronize()
    assert rel_l2(nchw(out), ref) < 1e-5


@pytest.mark.parametrize("case", [(23, 20, 20, 512, 512, 4), (11, 10, 10, 512, 512, 2), (5, 10, 10, 256, 128, 4), (3, 9, 11, 128, 64, 2)])
def test_conv_ksplit_workspace_paths(hip, case, monkeypatch):
    """Under-filled deep layers (VGG conv4/5 shapes): the workspace entry points split the input channels into extra work
    items + a fix-up pass.  Forward (bias + ReLU) and masked data gradient equal the unsplit kernels' results (1e-5)."""
    N, H, W, cin, cout, ks_forced = case
    monkeypatch.setenv("AESR_IGEMM_KSPLIT", str(ks_forced))
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(N, H, W, cin, generator=g).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).cuda()
    b = torch.randn(cout, generator=g).cuda()
    L = hip.lib
    pf, pb = _pack(hip, w, 0), _pack(hip, w, 1)
    ref = torch.empty(N, H, W, cout, device="cuda")
    hip.check(L.aesr_conv2d_fwd(hip.ptr(x), hip.ptr(pf), hip.ptr(b), hip.ptr(ref), N, H, W, cin, cout, 3, 1, 2, 0.0, hip.stream()), "fwd")
    nws = L.aesr_conv2d_workspace_floats(N, H, W, cin, cout, 3, 1)
    assert nws == ks_forced * N * H * W * cout
    ws = torch.empty(nws, device="cuda")
    out = torch.full_like(ref, float("nan"))
    hip.check(L.aesr_conv2d_fwd_ws(hip.ptr(x), hip.ptr(pf), hip.ptr(b), hip.ptr(out), hip.ptr(ws), N, H, W, cin, cout, 3, 1, 2, 0.0,
                                   hip.stream()), "fwd_ws")
    assert rel_l2(out, ref) < 1e-5
    dy = torch.randn(N, H, W, cout, generator=g).cuda()
    mask = torch.randn(N, H, W, cin, generator=g).cuda()
    dref = torch.empty(N, H, W, cin, device="cuda")
    hip.check(L.aesr_conv2d_dgrad(hip.ptr(dy), hip.ptr(pb), hip.ptr(mask), hip.ptr(dref), N, H, W, cin, cout, 3, 1, 2, 0.0, hip.stream()), "dgrad")
    nwd = L.aesr_conv2d_dgrad_workspace_floats(N, H, W, cin, cout, 3, 1)
    wsd = torch.empty(max(nwd, 1), device="cuda")
    dx = torch.full_like(dref, float("nan"))
    hip.check(L.aesr_conv2d_dgrad_ws(hip.ptr(dy), hip.ptr(pb), hip.ptr(mask), hip.ptr(dx), hip.ptr(wsd) if nwd else None, N, H, W, cin,
                                     cout, 3, 1, 2, 0.0, hip.stream()), "dgrad_ws")
    assert rel_l2(dx, dref) < 1e-5


def test_conv_ksplit_forced_after_the_unforced_plan(hip, monkeypatch):
    """AESR_IGEMM_KSPLIT takes effect on a shape the process has already planned without it: the unsplit kernels run first (and cache
    their plan), then the variable is set, the workspace queries ask for the two slabs and the workspace entry points run the split."""
    N, H, W, cin, cout = 2, 5, 5, 32, 32
    monkeypatch.delenv("AESR_IGEMM_KSPLIT", raising=False)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, W, cin, generator=g).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).cuda()
    b = torch.randn(cout, generator=g).cuda()
    dy = torch.randn(N, H, W, cout, generator=g).cuda()
    mask = torch.randn(N, H, W, cin, generator=g).cuda()
    L = hip.lib
    pf, pb = _pack(hip, w, 0), _pack(hip, w, 1)
    ref, dref = torch.empty(N, H, W, cout, device="cuda"), torch.empty(N, H, W, cin, device="cuda")
    hip.check(L.aesr_conv2d_fwd(hip.ptr(x), hip.ptr(pf), hip.ptr(b), hip.ptr(ref), N, H, W, cin, cout, 3, 1, 2, 0.0, hip.stream()), "fwd")
    hip.check(L.aesr_conv2d_dgrad(hip.ptr(dy), hip.ptr(pb), hip.ptr(mask), hip.ptr(dref), N, H, W, cin, cout, 3, 1, 2, 0.0, hip.stream()), "dgrad")
    assert L.aesr_conv2d_workspace_floats(N, H, W, cin, cout, 3, 1) == 0 and L.aesr_conv2d_dgrad_workspace_floats(N, H, W, cin, cout, 3, 1) == 0
    monkeypatch.setenv("AESR_IGEMM_KSPLIT", "2")
    assert L.aesr_conv2d_workspace_floats(N, H, W, cin, cout, 3, 1) == 3200 and L.aesr_conv2d_dgrad_workspace_floats(N, H, W, cin, cout, 3, 1) == 3200
    ws = torch.empty(3200, device="cuda")
    out, dx = torch.full_like(ref, float("nan")), torch.full_like(dref, float("nan"))
    hip.check(L.aesr_conv2d_fwd_ws(hip.ptr(x), hip.ptr(pf), hip.ptr(b), hip.ptr(out), hip.ptr(ws), N, H, W, cin, cout, 3, 1, 2, 0.0,
                                   hip.stream()), "fwd_ws")
    assert rel_l2(out, ref) < 1e-5
    hip.check(L.aesr_conv2d_dgrad_ws(hip.ptr(dy), hip.ptr(pb), hip.ptr(mask), hip.ptr(dx), hip.ptr(ws), N, H, W, cin, cout, 3, 1, 2, 0.0,
                                     hip.stream()), "dgrad_ws")
    assert rel_l2(dx, dref) < 1e-5


@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[4] % 4 == 0])
@pytest.mark.parametrize("masked", [False, True])
def test_conv_dgrad(hip, case, masked):
    N, H, W, Cin, Cout, KS, pad = case
    g = torch.Generator().manual_seed(7 + hash(case) % 1000)
    w = torch.randn(Cout, Cin, KS, KS, generator=g) / np.sqrt(Cout * KS * KS)
    Ho, Wo = H + 2 * pad - KS + 1, W + 2 * pad - KS + 1
    dy = torch.randn(N, Cout, Ho, Wo, generator=g)
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w, dy, padding=pad)
    xs = torch.randn(N, Cin, H, W, generator=g)
    if masked:
        ref = ref * torch.where(xs > 0, torch.ones_like(xs), torch.full_like(xs, 0.01))
    dx = torch.full((N, H, W, Cin), float("nan"), device="cuda")
    xsd = nhwc(xs).cuda() if masked else None
    hip.check(hip.lib.aesr_conv2d_dgrad(hip.ptr(D(nhwc(dy))), hip.ptr(D(_pack(hip, D(w), 1))), hip.ptr(xsd), hip.ptr(dx),
                                        N, H, W, Cin, Cout, KS, pad, 1 if masked else 0, 0.01, hip.stream()), "dgrad")
    torch.cuda.synchronize()
    assert rel_l2(nchw(dx), ref) < 1e-5


@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[4] % 4 == 0])
def test_conv_wgrad(hip, case):
    N, H, W, Cin, Cout, KS, pad = case
    g = torch.Generator().manual_seed(11 + hash(case) % 1000)
    x = torch.randn(N, Cin, H, W, generator=g)
    Ho, Wo = H + 2 * pad - KS + 1, W + 2 * pad - KS + 1
    dy = torch.randn(N, Cout, Ho, Wo, generator=g)
    ref_w = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, KS, KS), dy.double(), padding=pad)
    ref_b = dy.double().sum((0, 2, 3))
    dw = torch.full((Cout, Cin, KS, KS), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    ws = torch.empty(hip.lib.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, KS, pad), device="cuda")
    hip.check(hip.lib.aesr_conv2d_wgrad(hip.ptr(D(nhwc(x))), hip.ptr(D(nhwc(dy))), hip.ptr(dw), hip.ptr(db), hip.ptr(ws),
                                        N, H, W, Cin, Cout, KS, pad, hip.stream()), "wgrad")
    torch.cuda.synchronize()
    assert rel_l2(dw, ref_w) < 2e-5
    assert rel_l2(db, ref_b) < 2e-5


@pytest.mark.parametrize("cin,cout,ks,pad", [(1, 32, 1, 1), (1, 8, 1, 1), (3, 64, 3, 1), (2, 16, 3, 1)])
def test_smallcin_fwd_dgrad_wgrad(hip, cin, cout, ks, pad):
    N, H, W = 2, 21, 18
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x = torch.randn(N, cin, H, W, generator=g).requires_grad_(True)
    w = torch.randn(cout, cin, ks, ks, generator=g).requires_grad_(True)
    b = torch.randn(cout, generator=g).requires_grad_(True)
    ref = F.leaky_relu(F.conv2d(x, w, b, padding=pad), 0.01)
    Ho, Wo = ref.shape[2:]
    out = torch.empty((N, Ho, Wo, cout), device="cuda")
    L = hip.lib
    hip.check(L.aesr_conv2d_smallcin_fwd(hip.ptr(D(nhwc(x.detach()))), hip.ptr(D(w.detach())), hip.ptr(D(b.detach())), None,
                                         hip.ptr(out), N, H, W, cin, cout, ks, pad, 1, 0, 0.01, 0, 0, None, None, hip.stream()), "fwd")
    assert rel_l2(nchw(out), ref.detach()) < 1e-6
    # gradients of the pre-activation conv
    pre = F.conv2d(x, w, b, padding=pad)
    dy = torch.randn(pre.shape, generator=g)
    pre.backward(dy)
    dx = torch.empty((N, H, W, cin), device="cuda")
    hip.check(L.aesr_conv2d_smallcin_dgrad(hip.ptr(D(nhwc(dy))), hip.ptr(D(w.detach())), hip.ptr(dx), N, H, W, cin, cout, ks,
                                           pad, 0, None, hip.stream()), "dgrad")
    assert rel_l2(nchw(dx), x.grad) < 1e-5
    if ks == 1:
        dw, db = torch.empty_like(w, device="cuda"), torch.empty(cout, device="cuda")
        ws = torch.empty(L.aesr_small_wgrad_workspace_floats(cout * (cin + 1)), device="cuda")
        hip.check(L.aesr_conv2d_smallcin_wgrad(hip.ptr(D(nhwc(x.detach()))), hip.ptr(D(nhwc(dy))), hip.ptr(dw), hip.ptr(db),
                                               hip.ptr(ws), N, H, W, cin, cout, pad, hip.stream()), "wgrad")
        assert rel_l2(dw, w.grad) < 1e-5 and rel_l2(db, b.grad) < 1e-5


def test_smallcin_bcast_matches_scaling_layer(hip):
    """VGG conv1_1 on a 1-channel image with the LPIPS ScalingLayer (and the 2x-1 of perceptual.py) folded in."""
    N, H, W, cout = 2, 16, 20, 64
    g = torch.Generator().manual_seed(5)
    x = torch.rand(N, 1, H, W, generator=g).requires_grad_(True)
    w = torch.randn(cout, 3, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g) * 0.1
    shift = torch.tensor([-.030, -.088, -.188])[None, :, None, None]
    scale = torch.tensor([.458, .448, .450])[None, :, None, None]
    ref = F.relu(F.conv2d(((2 * x - 1) - shift) / scale, w, b, padding=1))
    ca = [2.0 / s for s in (.458, .448, .450)]
    cb = [(-1.0 - sh) / s for sh, s in zip((-.030, -.088, -.188), (.458, .448, .450))]
    out = torch.empty((N, H, W, cout), device="cuda")
    L = hip.lib
    hip.check(L.aesr_conv2d_smallcin_fwd(hip.ptr(D(x.detach().reshape(N, H, W, 1))), hip.ptr(D(w)), hip.ptr(D(b)), None,
                                         hip.ptr(out), N, H, W, 3, cout, 3, 1, 2, 0, 0.0, 0, 1, hip.float_array(ca),
                                         hip.float_array(cb), hip.stream()), "fwd")
    assert rel_l2(nchw(out), ref.detach()) < 1e-5
    dy = torch.randn(ref.shape, generator=g)
    pre = F.conv2d(((2 * x - 1) - shift) / scale, w, b, padding=1)
    pre.backward(dy)
    dx = torch.empty((N, H, W, 1), device="cuda")
    hip.check(L.aesr_conv2d_smallcin_dgrad(hip.ptr(D(nhwc(dy))), hip.ptr(D(w)), hip.ptr(dx), N, H, W, 3, cout, 3, 1, 1,
                                           hip.float_array(ca), hip.stream()), "dgrad")
    assert rel_l2(dx.reshape(N, 1, H, W), x.grad) < 1e-5


@pytest.mark.parametrize("shape", [(2, 24, 20, 32), (3, 37, 70, 16), (1, 9, 130, 64), (2, 160, 160, 32), (2, 12, 12, 8)])
def test_cout1_conv_backward(hip, shape):
    """Output conv Cin->1 (networks/acai_vanilla.py:98): data gradient (thin expand kernel, or the small-Cin kernel with
    the transpose flag for channel counts the thin kernels do not take) + weight/bias gradient."""
    N, H, W, cin = shape
    g = torch.Generator().manual_seed(9)
    h = torch.randn(N, cin, H, W, generator=g).requires_grad_(True)
    w = torch.randn(1, cin, 3, 3, generator=g).requires_grad_(True)
    b = torch.zeros(1, requires_grad=True)
    hl = F.leaky_relu(h, 0.01)
    out = F.conv2d(hl, w, b, padding=1)
    dy = torch.randn(out.shape, generator=g)
    out.backward(dy)
    L = hip.lib
    dx = torch.full((N, H, W, cin), float("nan"), device="cuda")
    if cin in (4, 8, 16, 32, 64, 128, 256):
        wsf = torch.empty(9 * cin, device="cuda")
        hip.check(L.aesr_conv2d_cout1_dgrad(hip.ptr(D(nhwc(dy))), hip.ptr(D(w.detach())), hip.ptr(D(nhwc(hl.detach()))), hip.ptr(dx),
                                            hip.ptr(wsf), N, H, W, cin, 1, 0.01, hip.stream()), "cout1 dgrad")
    else:
        hip.check(L.aesr_conv2d_smallcin_fwd(hip.ptr(D(nhwc(dy))), hip.ptr(D(w.detach())), None, hip.ptr(D(nhwc(hl.detach()))),
                                             hip.ptr(dx), N, H, W, 1, cin, 3, 1, 0, 1, 0.01, 1, 0, None, None, hip.stream()), "dgrad")
    assert rel_l2(nchw(dx), h.grad) < 1e-5
    dw, db = torch.empty((1, cin, 3, 3), device="cuda"), torch.empty(1, device="cuda")
    ws = torch.empty(L.aesr_conv2d_cout1_workspace_floats(cin), device="cuda")
    hip.check(L.aesr_conv2d_cout1_wgrad(hip.ptr(D(nhwc(hl.detach()))), hip.ptr(D(nhwc(dy))), hip.ptr(dw), hip.ptr(db),
                                        hip.ptr(ws), N, H, W, cin, hip.stream()), "wgrad")
    assert rel_l2(dw, w.grad) < 1e-5 and rel_l2(db, b.grad) < 1e-5


@pytest.mark.parametrize("shape", [(3, 21, 37, 32, 32, 1), (2, 160, 160, 32, 32, 1), (2, 8, 70, 16, 64, 1), (1, 30, 30, 48, 16, 0),
                                   (2, 5, 3, 32, 128, 2), (2, 34, 34, 8, 8, 1), (1, 20, 150, 8, 4, 1)])
def test_stem_folded_into_first_conv(hip, shape):
    """Conv2d(1,Cs,1,padding=p) -> Conv2d(Cs,C1,3,padding=1) -> LeakyReLU as ONE thin 1->C1 convolution
    (networks/acai_vanilla.py:51,55-56): forward and all four parameter gradients against the unfused PyTorch chain."""
    N, H, W, Cs, C1, p = shape
    g = torch.Generator().manual_seed(H * W)
    x = torch.rand(N, 1, H, W, generator=g)
    ws = (torch.randn(Cs, 1, 1, 1, generator=g)).requires_grad_(True)
    bs = (torch.randn(Cs, generator=g) * 0.3).requires_grad_(True)
    w1 = (torch.randn(C1, Cs, 3, 3, generator=g) / np.sqrt(9 * Cs)).requires_grad_(True)
    b1 = (torch.randn(C1, generator=g) * 0.1).requires_grad_(True)
    pre = F.conv2d(F.conv2d(x, ws, bs, padding=p), w1, b1, padding=1)
    ref = F.leaky_relu(pre, 0.01).detach()
    gout = torch.randn(pre.shape, generator=g)
    pre.backward(gout)
    L = hip.lib
    xd = D(x.reshape(N, H, W).contiguous())
    folded = torch.empty(L.aesr_stemconv_folded_floats(C1), device="cuda")
    dws, dbs, dw1, db1 = D(ws.detach()), D(bs.detach()), D(w1.detach()), D(b1.detach())
    hip.check(L.aesr_stemconv_fold(hip.ptr(dws), hip.ptr(dbs), hip.ptr(dw1), hip.ptr(folded), Cs, C1, hip.stream()), "fold")
    Ho, Wo = H + 2 * p, W + 2 * p
    out = torch.full((N, Ho, Wo, C1), float("nan"), device="cuda")
    hip.check(L.aesr_stemconv_fwd(hip.ptr(xd), hip.ptr(folded), hip.ptr(db1), hip.ptr(out), N, H, W, C1, p, 1, 0.01, hip.stream()),
              "stemconv fwd")
    assert rel_l2(nchw(out), ref) < 1e-5
    assert float((nchw(out).cpu() - ref.detach()).abs().max()) < 1e-4
    gws, gbs = torch.empty(Cs, device="cuda"), torch.empty(Cs, device="cuda")
    gw1, gb1 = torch.empty((C1, Cs, 3, 3), device="cuda"), torch.empty(C1, device="cuda")
    wsp = torch.empty(L.aesr_stemconv_workspace_floats(C1), device="cuda")
    hip.check(L.aesr_stemconv_wgrad(hip.ptr(xd), hip.ptr(D(nhwc(gout))), hip.ptr(dws), hip.ptr(dbs), hip.ptr(dw1), hip.ptr(gws),
                                    hip.ptr(gbs), hip.ptr(gw1), hip.ptr(gb1), hip.ptr(wsp), N, H, W, Cs, C1, p, hip.stream()),
              "stemconv wgrad")
    assert rel_l2(gws, ws.grad.reshape(-1)) < 2e-5 and rel_l2(gbs, bs.grad) < 2e-5
    assert rel_l2(gw1, w1.grad) < 2e-5 and rel_l2(gb1, b1.grad) < 2e-5


@pytest.mark.parametrize("shape", [(2, 24, 20, 32), (1, 160, 160, 32), (3, 9, 7, 8)])
def test_cout1_conv_forward_sigmoid(hip, shape):
    N, H, W, cin = shape
    g = torch.Generator().manual_seed(H)
    h = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(1, cin, 3, 3, generator=g) / np.sqrt(cin * 9)
    b = torch.randn(1, generator=g)
    ref = torch.sigmoid(F.conv2d(h, w, b, padding=1))
    out = torch.full((N, H, W, 1), float("nan"), device="cuda")
    hip.check(hip.lib.aesr_conv2d_cout1_fwd(hip.ptr(D(nhwc(h))), hip.ptr(D(w)), hip.ptr(D(b)), hip.ptr(out), N, H, W, cin, 3, 0.0,
                                            hip.stream()), "cout1_fwd")
    assert rel_l2(nchw(out), ref) < 1e-6


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 12, 16, 8), (3, 7, 5, 4), (1, 40, 40, 64), (2, 1, 1, 16), (2, 2, 3, 8)])
@pytest.mark.parametrize("masked", [False, True])
def test_resample2_fwd_bwd(hip, mode, shape, masked):
    """Stand-alone AvgPool2d(2) / nearest x2 / bilinear x2 (align_corners=False, networks/ae_standard.py:68), forward and
    backward (optionally fused with the LeakyReLU derivative of the producer) against ATen on the CPU."""
    N, H, W, C = shape
    if mode == 1 and (H < 2 or W < 2):
        pytest.skip("pooling needs H, W >= 2")
    g = torch.Generator().manual_seed(31 * H + W + mode)
    pre = torch.randn(N, C, H, W, generator=g).requires_grad_(True)
    x = F.leaky_relu(pre, 0.01) if masked else pre
    if mode == 1:
        ref = F.avg_pool2d(x, 2)
    elif mode == 2:
        ref = F.interpolate(x, scale_factor=2, mode="nearest")
    else:
        ref = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    gout = torch.randn(ref.shape, generator=g)
    ref.backward(gout)
    L = hip.lib
    xd = D(nhwc(x.detach()))
    out = torch.full((N, ref.shape[2], ref.shape[3], C), float("nan"), device="cuda")
    hip.check(L.aesr_resample2_fwd(hip.ptr(xd), hip.ptr(out), N, H, W, C, mode, hip.stream()), "resample fwd")
    assert rel_l2(nchw(out), ref.detach()) < 1e-6
    dx = torch.full((N, H, W, C), float("nan"), device="cuda")
    hip.check(L.aesr_resample2_bwd(hip.ptr(D(nhwc(gout))), hip.ptr(xd) if masked else None, hip.ptr(dx), N, H, W, C, mode,
                                   1 if masked else 0, 0.01, hip.stream()), "resample bwd")
    assert rel_l2(nchw(dx), pre.grad) < 1e-6


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(6, 33, 31, 32), (4, 40, 40, 64), (3, 9, 9, 8), (9, 80, 80, 32)])
def test_bn_groups_fwd_bwd(hip, mode, shape):
    """Two statistic groups (4+2 images etc.) == two independent nn.BatchNorm2d calls in sequence."""
    N, H, W, C = shape
    n0 = N - N // 3
    nstart = [0, n0, N]
    g = torch.Generator().manual_seed(N * H + C + mode)
    pre = torch.randn(N, C, H, W, generator=g)
    y = F.leaky_relu(pre, 0.01).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.normal_(generator=g)
        bn.bias.normal_(generator=g)
    post = {0: lambda t: t, 1: lambda t: F.avg_pool2d(t, 2), 2: lambda t: F.interpolate(t, scale_factor=2, mode="nearest")}[mode]
    bn.train()
    refs = [post(bn(y[a:b])) for a, b in zip(nstart[:-1], nstart[1:])]
    ref = torch.cat(refs)
    gout = torch.randn(ref.shape, generator=g)
    (refs[0] * gout[:n0]).sum().backward()             # gradients only through group 0
    L = hip.lib
    yd = nhwc(y.detach()).cuda()
    gam, bet = bn.weight.detach().cuda(), bn.bias.detach().cuda()
    rm, rv, nbt = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    G = 2
    partial = torch.empty(G * hip.BN_NWG * 2 * C, device="cuda")
    sums = torch.empty((G, 2, C), dtype=torch.float64, device="cuda")
    ns = hip.int_array(nstart)
    hip.check(L.aesr_bn_stats(hip.ptr(yd), hip.ptr(partial), hip.ptr(sums), H * W, C, G, ns, hip.stream()), "stats")
    counts = hip.double_array([n0 * H * W, (N - n0) * H * W])
    st = [torch.empty((G, C), device="cuda") for _ in range(4)]
    hip.check(L.aesr_bn_finalize(hip.ptr(sums), counts, hip.ptr(gam), hip.ptr(bet), hip.ptr(rm), hip.ptr(rv), hip.ptr(nbt),
                                 *[hip.ptr(t) for t in st], C, G, 0.1, 1e-5, 1, 1, hip.stream()), "finalize")
    Ho, Wo = ref.shape[2:]
    out = torch.empty((N, Ho, Wo, C), device="cuda")
    hip.check(L.aesr_bn_apply(hip.ptr(yd), hip.ptr(st[2]), hip.ptr(st[3]), hip.ptr(out), N, H, W, C, mode, G, ns, hip.stream()), "apply")
    assert rel_l2(nchw(out), ref.detach()) < 1e-5
    assert rel_l2(rm, bn.running_mean) < 1e-5 and rel_l2(rv, bn.running_var) < 1e-5 and int(nbt) == 2
    # backward through group 0 only (N = n0, G = 1), fused with the LeakyReLU derivative of the producer
    god = nhwc(gout[:n0]).cuda()
    ns1 = hip.int_array([0, n0])
    sums1 = torch.empty((1, 2, C), dtype=torch.float64, device="cuda")
    hip.check(L.aesr_bn_bwd_reduce(hip.ptr(god), hip.ptr(yd), hip.ptr(st[0]), hip.ptr(st[1]), hip.ptr(partial), hip.ptr(sums1), n0, H, W,
                                   C, mode, 1, ns1, hip.stream()), "bwd_reduce")
    coef = torch.empty((1, 2, C), device="cuda")
    dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dpre = torch.empty((n0, H, W, C), device="cuda")
    hip.check(L.aesr_bn_bwd_apply(hip.ptr(god), hip.ptr(yd), hip.ptr(st[0]), hip.ptr(st[1]), hip.ptr(st[2]), hip.ptr(sums1), counts,
                                  hip.ptr(coef), hip.ptr(dgam), hip.ptr(dbet), hip.ptr(dpre), n0, H, W, C, mode, 1, 0.01, 1, ns1,
                                  hip.stream()), "bwd_apply")
    mask = torch.where(y.detach()[:n0] > 0, 1.0, 0.01)
    assert rel_l2(nchw(dpre), y.grad[:n0] * mask) < 2e-5
    assert rel_l2(dgam, bn.weight.grad) < 2e-5 and rel_l2(dbet, bn.bias.grad) < 2e-5
    # the single-process composites (what the engine calls) give the same numbers
    rm2, rv2, nbt2 = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    st2 = [torch.full((G, C), float("nan"), device="cuda") for _ in range(4)]
    hip.check(L.aesr_bn_stats_finalize(hip.ptr(yd), hip.ptr(partial), counts, hip.ptr(gam), hip.ptr(bet), hip.ptr(rm2), hip.ptr(rv2),
                                       hip.ptr(nbt2), *[hip.ptr(t) for t in st2], H * W, C, G, ns, 0.1, 1e-5, 1, hip.stream()), "stats_finalize")
    coef2 = torch.full((1, 2, C), float("nan"), device="cuda")
    dgam2, dbet2 = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    dpre2 = torch.full((n0, H, W, C), float("nan"), device="cuda")
    hip.check(L.aesr_bn_bwd(hip.ptr(god), hip.ptr(yd), hip.ptr(st[0]), hip.ptr(st[1]), hip.ptr(st[2]), hip.ptr(partial), counts,
                            hip.ptr(coef2), hip.ptr(dgam2), hip.ptr(dbet2), hip.ptr(dpre2), n0, H, W, C, mode, 1, 0.01, 1, ns1,
                            hip.stream()), "bn_bwd")
    torch.cuda.synchronize()
    assert int(nbt2) == 2
    for got, want in zip(st2 + [rm2, rv2, coef2, dgam2, dbet2, dpre2], st + [rm, rv, coef, dgam, dbet, dpre]):
        assert rel_l2(got, want) < 2e-6
    # the data-parallel composite: finalize (from the sums) inside the apply launch -- the SAME numbers as finalize + apply, bit for bit
    assert L.aesr_bn_fused_supported(C, G) == 1
    rm3, rv3, nbt3 = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    st3 = [torch.full((G, C), float("nan"), device="cuda") for _ in range(4)]
    out3 = torch.full((N, Ho, Wo, C), float("nan"), device="cuda")
    hip.check(L.aesr_bn_finalize_apply(hip.ptr(sums), counts, hip.ptr(gam), hip.ptr(bet), hip.ptr(rm3), hip.ptr(rv3), hip.ptr(nbt3),
                                       *[hip.ptr(t) for t in st3], hip.ptr(yd), hip.ptr(out3), N, H, W, C, mode, G, ns, 0.1, 1e-5, 1, hip.stream()),
              "finalize_apply")
    torch.cuda.synchronize()
    assert int(nbt3) == 2 and torch.equal(out3, out) and torch.equal(rm3, rm) and torch.equal(rv3, rv)
    for got, want in zip(st3, st):
        assert torch.equal(got, want)


@pytest.mark.parametrize("mode", [0, 1])
def test_bn_tables_too_large_for_the_prologue(hip, mode):
    """G * C = 2048 > 1024: the finalize-inside-apply kernels have no room for their LDS tables.  aesr_bn_finalize_apply refuses (and
    writes nothing), aesr_bn_bwd_apply takes the separate bn_bwd_finalize launch and then bn_bwd_apply -- the one route through those two
    kernels with more than one group.  Both groups, forward and backward, against nn.BatchNorm2d evaluated in float64 on the CPU."""
    N, H, W, C, G = 4, 3, 3, 1024, 2
    nstart = [0, 2, 4]
    g = torch.Generator().manual_seed(7 + mode)
    y = F.leaky_relu(torch.randn(N, C, H, W, generator=g), 0.01)
    y64 = y.double().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.normal_(generator=g)
        bn.bias.normal_(generator=g)
    gam, bet = D(bn.weight.detach().clone()), D(bn.bias.detach().clone())
    bn = bn.double().train()
    post = (lambda t: F.avg_pool2d(t, 2)) if mode == 1 else (lambda t: t)
    ref = torch.cat([post(bn(y64[a:b])) for a, b in zip(nstart[:-1], nstart[1:])])       # group after group: the running statistics
    gout = torch.randn(ref.shape, generator=g)
    (ref * gout.double()).sum().backward()
    L = hip.lib
    assert L.aesr_bn_fused_supported(C, G) == 0
    yd, god = D(nhwc(y)), D(nhwc(gout))
    ns = hip.int_array(nstart)
    counts = hip.double_array([2 * H * W, 2 * H * W])
    partial = torch.empty(G * hip.BN_NWG * 2 * C, device="cuda")
    sums = torch.empty((G, 2, C), dtype=torch.float64, device="cuda")
    hip.check(L.aesr_bn_stats(hip.ptr(yd), hip.ptr(partial), hip.ptr(sums), H * W, C, G, ns, hip.stream()), "stats")
    Ho, Wo = ref.shape[2:]
    # the refusal: every output poisoned beforehand and untouched afterwards
    poison = [torch.full((G, C), 7.0, device="cuda") for _ in range(4)] + [torch.full((C,), 7.0, device="cuda") for _ in range(2)]
    pout, pnbt = torch.full((N, Ho, Wo, C), 7.0, device="cuda"), torch.full((), 7, dtype=torch.int64, device="cuda")
    rc = L.aesr_bn_finalize_apply(hip.ptr(sums), counts, hip.ptr(gam), hip.ptr(bet), hip.ptr(poison[4]), hip.ptr(poison[5]), hip.ptr(pnbt),
                                  *[hip.ptr(t) for t in poison[:4]], hip.ptr(yd), hip.ptr(pout), N, H, W, C, mode, G, ns, 0.1, 1e-5, 1, hip.stream())
    torch.cuda.synchronize()
    assert rc != 0 and "aesr_bn_finalize_apply" in hip.last_error()
    assert all(bool((t == 7.0).all()) for t in poison + [pout]) and int(pnbt) == 7
    # the three-launch sequence of the data-parallel path
    rm, rv, nbt = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    st = [torch.full((G, C), float("nan"), device="cuda") for _ in range(4)]
    hip.check(L.aesr_bn_finalize(hip.ptr(sums), counts, hip.ptr(gam), hip.ptr(bet), hip.ptr(rm), hip.ptr(rv), hip.ptr(nbt),
                                 *[hip.ptr(t) for t in st], C, G, 0.1, 1e-5, 1, 1, hip.stream()), "finalize")
    out = torch.full((N, Ho, Wo, C), float("nan"), device="cuda")
    hip.check(L.aesr_bn_apply(hip.ptr(yd), hip.ptr(st[2]), hip.ptr(st[3]), hip.ptr(out), N, H, W, C, mode, G, ns, hip.stream()), "apply")
    sums2 = torch.empty((G, 2, C), dtype=torch.float64, device="cuda")
    hip.check(L.aesr_bn_bwd_reduce(hip.ptr(god), hip.ptr(yd), hip.ptr(st[0]), hip.ptr(st[1]), hip.ptr(partial), hip.ptr(sums2), N, H, W, C,
                                   mode, G, ns, hip.stream()), "bwd_reduce")
    coef = torch.full((G, 2, C), float("nan"), device="cuda")
    dgam, dbet = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    dpre = torch.full((N, H, W, C), float("nan"), device="cuda")
    hip.check(L.aesr_bn_bwd_apply(hip.ptr(god), hip.ptr(yd), hip.ptr(st[0]), hip.ptr(st[1]), hip.ptr(st[2]), hip.ptr(sums2), counts,
                                  hip.ptr(coef), hip.ptr(dgam), hip.ptr(dbet), hip.ptr(dpre), N, H, W, C, mode, 1, 0.01, G, ns,
                                  hip.stream()), "bwd_apply")
    torch.cuda.synchronize()
    errs = dict(out=rel_l2(nchw(out), ref.detach()), running_mean=rel_l2(rm, bn.running_mean), running_var=rel_l2(rv, bn.running_var),
                dpre=rel_l2(nchw(dpre), y64.grad * torch.where(y64.detach() > 0, 1.0, 0.01)), dgamma=rel_l2(dgam, bn.weight.grad),
                dbeta=rel_l2(dbet, bn.bias.grad))
    print("bn_tables_too_large mode %d: %s" % (mode, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert int(nbt) == 2
    assert errs["out"] < 1e-5 and errs["running_mean"] < 1e-5 and errs["running_var"] < 1e-5
    assert errs["dpre"] < 2e-5 and errs["dgamma"] < 2e-5 and errs["dbeta"] < 2e-5


def test_lerp_mse_act_adam(hip):
    L = hip.lib
    g = torch.Generator().manual_seed(3)
    B, per = 3, 128 * 10 * 10
    z = torch.randn(2 * B, per, generator=g)
    af, at = torch.tensor([0.25, 0.5, 0.75]), torch.tensor([0.75, 0.5, 0.25])
    zm = torch.empty(B, per, device="cuda")
    hip.check(L.aesr_lerp_fwd(hip.ptr(D(z)), hip.ptr(D(af)), hip.ptr(D(at)), hip.ptr(zm), B, per, hip.stream()), "lerp")
    assert torch.equal(zm.cpu(), af[:, None] * z[:B] + at[:, None] * z[B:])
    d = torch.randn(B, per, generator=g)
    dz = torch.empty(2 * B, per, device="cuda")
    hip.check(L.aesr_lerp_bwd(hip.ptr(D(d)), hip.ptr(D(af)), hip.ptr(D(at)), hip.ptr(dz), B, per, hip.stream()), "lerp_bwd")
    assert torch.equal(dz.cpu(), torch.cat([af[:, None] * d, at[:, None] * d]))
    # the decoder-input form: [z | mix] in one pass and the folded gradient
    zc = torch.empty(3 * B, per, device="cuda")
    hip.check(L.aesr_lerp_cat_fwd(hip.ptr(D(z)), hip.ptr(D(af)), hip.ptr(D(at)), hip.ptr(zc), B, per, hip.stream()), "lerp_cat")
    assert torch.equal(zc.cpu(), torch.cat([z, af[:, None] * z[:B] + at[:, None] * z[B:]]))
    g3 = torch.randn(3 * B, per, generator=g)
    dz2 = torch.empty(2 * B, per, device="cuda")
    hip.check(L.aesr_lerp_cat_bwd(hip.ptr(D(g3)), hip.ptr(D(af)), hip.ptr(D(at)), hip.ptr(dz2), B, per, hip.stream()), "lerp_cat_bwd")
    assert torch.equal(dz2.cpu(), torch.cat([g3[:B] + g3[2 * B:] * af[:, None], g3[B:2 * B] + g3[2 * B:] * at[:, None]]))
    from superresolution_aniso_mri_amd import ops
    zz = torch.randn(2 * B, 8, 5, 4, generator=g).cuda().requires_grad_(True)
    cat = ops.lerp_cat(zz, 0.5, 0.5)
    assert cat.shape == (3 * B, 8, 5, 4) and torch.equal(cat[2 * B:], ops.lerp_mix(zz.detach(), 0.5, 0.5))
    (cat * torch.arange(3 * B, device="cuda").float()[:, None, None, None]).sum().backward()
    want = torch.cat([torch.arange(B) + 0.5 * (2 * B + torch.arange(B)), B + torch.arange(B) + 0.5 * (2 * B + torch.arange(B))]).float()
    assert torch.equal(zz.grad.cpu(), want[:, None, None, None].expand(2 * B, 8, 5, 4))
    a = torch.rand(24 * 160 * 160, generator=g).requires_grad_(True)
    b = torch.rand(24 * 160 * 160, generator=g)
    ref = F.mse_loss(a, b)
    ref.backward(torch.tensor(0.7))
    part, loss = torch.empty(hip.MSE_NPART, dtype=torch.float64, device="cuda"), torch.empty(1, device="cuda")
    hip.check(L.aesr_mse_fwd(hip.ptr(D(a.detach())), hip.ptr(D(b)), hip.ptr(part), hip.ptr(loss), a.numel(), hip.stream()), "mse")
    assert abs(float(loss) - float(ref)) < 1e-6 * float(ref)
    da = torch.empty(a.numel(), device="cuda")
    hip.check(L.aesr_mse_bwd(hip.ptr(D(a.detach())), hip.ptr(D(b)), hip.ptr(D(torch.tensor([0.7]))), hip.ptr(da), a.numel(),
                             hip.stream()), "mse_bwd")
    assert rel_l2(da, a.grad) < 1e-6
    y = torch.sigmoid(torch.randn(1000, generator=g))
    dout = torch.randn(1000, generator=g)
    dp = torch.empty(1000, device="cuda")
    hip.check(L.aesr_act_bwd(hip.ptr(D(dout)), hip.ptr(D(y)), hip.ptr(dp), 1000, 3, 0.0, hip.stream()), "act_bwd")
    assert rel_l2(dp, dout * y * (1 - y)) < 1e-6
    # Adam: 3 steps against torch.optim.Adam
    p = torch.randn(5000, generator=g)
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    pd, m, v = p.cuda(), torch.zeros(5000, device="cuda"), torch.zeros(5000, device="cuda")
    host = (ctypes.c_float * 8)()
    L.aesr_adam_state_init(host, 0.0, 0.9, 0.999)
    state = torch.from_numpy(np.frombuffer(host, dtype=np.int32).copy()).cuda().view(torch.float32)
    for k in range(3):
        gr = torch.randn(5000, generator=g)
        pt.grad = gr.clone()
        opt.step()
        gd = D(gr)
        hip.check(L.aesr_adam_step(hip.ptr(pd), hip.ptr(gd), hip.ptr(m), hip.ptr(v), hip.ptr(state), 5000, 1e-3, 0.9, 0.999, 1e-8,
                                   0.01, k % 2, hip.stream()), "adam")
        # zero_grad: the gradient buffer is left at zero (odd k) or untouched (even k); the step counter advances once per launch
        assert float(gd.abs().max()) == 0.0 if k % 2 else torch.equal(gd.cpu(), gr)
        assert float(state[0]) == k + 1 and state.view(torch.int32)[3].item() == 0
    # (rel-L2 1e-6 on parameters of size ~1 lets every update of ~1e-3 be 0.1 % off: tests/test_gpu_adam.py holds p, exp_avg and exp_avg_sq
    # of every step to 4 x torch's own fp32 error against fp64, which makes this bound redundant -- kept as the coarse first line)
    assert rel_l2(pd, pt.detach()) < 1e-6 and float(state[0]) == 3.0


def test_bad_arguments_fail_loudly(hip):
    L = hip.lib
    x = torch.zeros(16, device="cuda")
    rc = L.aesr_conv2d_fwd(hip.ptr(x), hip.ptr(x), None, hip.ptr(x), 1, 4, 4, 3, 8, 3, 1, 0, 0.0, hip.stream())
    assert rc != 0 and "multiple of 4" in hip.last_error()
    rc = L.aesr_lerp_fwd(hip.ptr(x), hip.ptr(x), hip.ptr(x), hip.ptr(x), 1, 6, hip.stream())
    assert rc != 0
    with pytest.raises(RuntimeError):
        hip.check(rc, "lerp")


# ---- Winograd F(2x2,3x3) form of the 3x3 / padding-1 convolutions (csrc/conv_wino.hip) -----------------------------------------
WINO_CASES = [
    # N, H, W, Cin, Cout
    (2, 162, 162, 32, 32),      # enc.1 / enc.3 of the ACDC model: 81x81 tiles, regions of 9x14 tiles
    (3, 81, 81, 32, 64),        # odd size: the last tile row / column is half outside the image
    (2, 40, 40, 128, 64),       # 8 chunks of input channels, two cout tiles
    (5, 10, 10, 64, 64),        # 5x5 tiles per image: several images per work item (TI > 1), idle waves
    (3, 7, 9, 16, 32),          # one chunk, partial tiles everywhere
    (1, 1, 1, 16, 32),          # a single pixel
    (2, 2, 3, 48, 96),          # Cin = 3 chunks, Cout = 3 cout tiles
    (1, 33, 130, 32, 32),       # wide image: regions that straddle the right border
    (3, 40, 40, 64, 128),       # resident-filter kernel with 16-cout workgroups (K side 64 channels, blocks tile the image exactly)
    (2, 16, 24, 48, 96),        # ... three chunks, six 16-cout tiles
    # ring kernel (conv_wino_ring.hip: K side of 64 and more channels where the filter is not resident)
    (2, 81, 81, 64, 64),        # 8 x 8 blocks tile 81 x 81 with 18 % padding: ring instead of the resident kernel; partial blocks at both borders
    (4, 20, 20, 128, 64),       # 10 x 10 tiles per image: blocks that are not 4 x 4 tiles
    (7, 10, 10, 128, 96),       # several images per block, image count not a multiple of it, three cout tiles
    (1, 40, 40, 256, 32),       # 16 chunks, one cout tile: fewer block groups than CUs
    (3, 10, 10, 512, 512),      # VGG conv5: 32 chunks x 16 cout tiles
    (2, 33, 47, 80, 160),       # 5 chunks, 5 cout tiles, odd sizes
]


def _pack_wino(hip, w, transpose):
    cout, cin = w.shape[:2]
    buf = torch.empty(hip.lib.aesr_conv2d_wino_packed_floats(cout, cin, transpose), device="cuda")
    job = (hip.PackJob * 1)(hip.PackJob(w.data_ptr(), buf.data_ptr(), cout, cin, 3, transpose))
    hip.check(hip.lib.aesr_conv2d_wino_pack_many(job, 1, hip.stream()), "wino_pack")
    return buf


@pytest.fixture(params=["planned", "ring"])
def streamed_kernel(request, monkeypatch):
    """Streamed Winograd layers on the kernel the launcher's cost estimates pick ("planned": AESR_WINO_RING=1, which keeps the first
    streamed kernel in the suite) and all on the ring kernel ("ring": the shipped default)."""
    monkeypatch.setenv("AESR_WINO_RING", "2" if request.param == "ring" else "1")
    return request.param


@pytest.mark.parametrize("case", WINO_CASES)
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_conv_wino_fwd(hip, case, act, streamed_kernel):
    """Forward with bias and every fused activation against an fp64 convolution (1e-5; measured 2-4e-7) and against the
    implicit-GEMM kernel of the same library."""
    N, H, W, Cin, Cout = case
    assert hip.lib.aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 0) == 1
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = {0: ref, 1: F.leaky_relu(ref, 0.01), 2: F.relu(ref), 3: torch.sigmoid(ref)}[act]
    xd, wd, bd = nhwc(x).cuda(), w.cuda(), b.cuda()
    out = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    hip.check(hip.lib.aesr_conv2d_wino_fwd(hip.ptr(xd), hip.ptr(D(_pack_wino(hip, wd, 0))), hip.ptr(bd), hip.ptr(out), N, H, W, Cin, Cout,
                                           act, 0.01, hip.stream()), "wino_fwd")
    out_i = torch.empty_like(out)
    hip.check(hip.lib.aesr_conv2d_fwd(hip.ptr(xd), hip.ptr(D(_pack(hip, wd, 0))), hip.ptr(bd), hip.ptr(out_i), N, H, W, Cin, Cout, 3, 1,
                                      act, 0.01, hip.stream()), "conv_fwd")
    torch.cuda.synchronize()
    assert rel_l2(nchw(out), ref) < 1e-5
    assert rel_l2(out, out_i) < 2e-6
    # no bias: the bias slot of the accumulators must start from zero
    out2 = torch.full_like(out, float("nan"))
    hip.check(hip.lib.aesr_conv2d_wino_fwd(hip.ptr(xd), hip.ptr(D(_pack_wino(hip, wd, 0))), None, hip.ptr(out2), N, H, W, Cin, Cout, 0, 0.0,
                                           hip.stream()), "wino_fwd")
    torch.cuda.synchronize()
    assert rel_l2(nchw(out2), F.conv2d(x.double(), w.double(), None, padding=1)) < 1e-5


@pytest.mark.parametrize("case", WINO_CASES)
@pytest.mark.parametrize("mask_act", [0, 1, 2])
def test_conv_wino_dgrad(hip, case, mask_act, streamed_kernel):
    """Data gradient (flipped / transposed filter) with the fused derivative mask of the producing activation."""
    N, H, W, Cout, Cin = case            # roles swapped so that the data-gradient constraints (Cout % 16, Cin % 32) hold
    assert hip.lib.aesr_conv2d_wino_supported(Cin, Cout, 3, 1, 1) == 1
    g = torch.Generator().manual_seed(3 + hash(case) % 1000)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cout * 9)
    dy = torch.randn(N, Cout, H, W, generator=g)
    xs = torch.randn(N, Cin, H, W, generator=g)            # saved activation output whose sign selects the derivative
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), padding=1)
    if mask_act == 1:
        ref = ref * torch.where(xs > 0, 1.0, 0.01).double()
    elif mask_act == 2:
        ref = ref * (xs > 0).double()
    dx = torch.full((N, H, W, Cin), float("nan"), device="cuda")
    hip.check(hip.lib.aesr_conv2d_wino_dgrad(hip.ptr(D(nhwc(dy))), hip.ptr(D(_pack_wino(hip, w.cuda(), 1))),
                                             hip.ptr(D(nhwc(xs))) if mask_act else None, hip.ptr(dx), N, H, W, Cin, Cout, mask_act, 0.01,
                                             hip.stream()), "wino_dgrad")
    torch.cuda.synchronize()
    assert rel_l2(nchw(dx), ref) < 1e-5


KSPLIT_CASES = [
    # N, H, W, Cin, Cout, forced split
    (2, 10, 10, 512, 64, 8),      # VGG conv5 of a small shard: 32 chunks in 8 splits of 4
    (3, 20, 12, 256, 96, 4),
    (1, 7, 9, 96, 32, 4),         # 6 chunks: 4 splits would leave one empty -> the launcher settles for 2
    (4, 40, 40, 128, 64, 2),
    (1, 5, 3, 64, 32, 2),
]


@pytest.mark.parametrize("case", KSPLIT_CASES)
def test_conv_wino_channel_split(hip, case, monkeypatch):
    """conv_wino_ring_f32 with its K side split over several work items + wino_split_reduce_kernel (aesr_conv2d_wino_fwd_ws / _dgrad_ws):
    forward with bias and LeakyReLU, data gradient with the ReLU mask, against fp64 (1e-5) and against the unsplit launch of the same
    kernel (2e-6: another summation order over the channels); a workspace that is too small means an unsplit launch, not an error."""
    N, H, W, Cin, Cout, S = case
    L = hip.lib
    monkeypatch.setenv("AESR_WINO_RING", "2")
    monkeypatch.setenv("AESR_RING_KSPLIT", str(S))
    g = torch.Generator().manual_seed(11 + hash(case) % 1000)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g)
    nws = L.aesr_conv2d_wino_workspace_floats(N, H, W, Cin, Cout, 0)
    assert nws >= 2 * N * H * W * Cout and nws % (N * H * W * Cout) == 0 and nws // (N * H * W * Cout) <= S
    ws = torch.full((nws,), float("nan"), device="cuda")
    xd, up = D(nhwc(x)), D(_pack_wino(hip, w.cuda(), 0))
    out, out1, out2 = (torch.full((N, H, W, Cout), float("nan"), device="cuda") for _ in range(3))
    hip.check(L.aesr_conv2d_wino_fwd_ws(hip.ptr(xd), hip.ptr(up), hip.ptr(b.cuda()), hip.ptr(out), hip.ptr(ws), nws, N, H, W, Cin, Cout, 1, 0.01,
                                        hip.stream()), "wino_fwd_ws")
    hip.check(L.aesr_conv2d_wino_fwd_ws(hip.ptr(xd), hip.ptr(up), hip.ptr(b.cuda()), hip.ptr(out1), None, 0, N, H, W, Cin, Cout, 1, 0.01,
                                        hip.stream()), "wino_fwd_ws(no workspace)")
    hip.check(L.aesr_conv2d_wino_fwd_ws(hip.ptr(xd), hip.ptr(up), hip.ptr(b.cuda()), hip.ptr(out2), hip.ptr(ws), N * H * W * Cout, N, H, W, Cin, Cout,
                                        1, 0.01, hip.stream()), "wino_fwd_ws(small workspace)")
    torch.cuda.synchronize()
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.01)
    assert rel_l2(nchw(out), ref) < 1e-5 and rel_l2(nchw(out1), ref) < 1e-5
    assert rel_l2(out, out1) < 2e-6 and not torch.equal(out, out1)          # really another summation order
    assert torch.equal(out1, out2)
    # data gradient (roles of the channel counts swapped), ReLU mask
    dy = torch.randn(N, Cin, H, W, generator=g)
    wt = torch.randn(Cin, Cout, 3, 3, generator=g) / np.sqrt(Cin * 9)      # a layer Cout -> Cin: K side of its data gradient = Cin channels
    xs = torch.randn(N, Cout, H, W, generator=g)
    nwd = L.aesr_conv2d_wino_workspace_floats(N, H, W, Cout, Cin, 1)
    assert nwd >= 2 * N * H * W * Cout
    wsd = torch.full((nwd,), float("nan"), device="cuda")
    dx = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    hip.check(L.aesr_conv2d_wino_dgrad_ws(hip.ptr(D(nhwc(dy))), hip.ptr(D(_pack_wino(hip, wt.cuda(), 1))), hip.ptr(D(nhwc(xs))), hip.ptr(dx), hip.ptr(wsd),
                                          nwd, N, H, W, Cout, Cin, 2, 0.0, hip.stream()), "wino_dgrad_ws")
    torch.cuda.synchronize()
    refd = torch.nn.grad.conv2d_input((N, Cout, H, W), wt.double(), dy.double(), padding=1) * (xs > 0).double()
    assert rel_l2(nchw(dx), refd) < 1e-5
    assert L.aesr_conv2d_wino_ring_timeouts() == 0


def test_conv_wino_channel_split_random_shapes(hip, monkeypatch):
    """30 seeded random small layers (odd sizes, channel counts that leave ragged splits, all-tail item lists): the split launch equals
    the unsplit launch of the same kernel to summation order, forward and data gradient, and both equal fp64."""
    L = hip.lib
    monkeypatch.setenv("AESR_WINO_RING", "2")
    rng = np.random.RandomState(7)
    g = torch.Generator().manual_seed(7)
    nsplit = 0
    for _ in range(30):
        N, H, W = int(rng.randint(1, 6)), int(rng.randint(3, 30)), int(rng.randint(3, 30))
        Cin, Cout = int(rng.choice([48, 64, 80, 96, 160, 256, 320])), int(rng.choice([32, 64, 96]))
        S = int(rng.choice([2, 4, 8, 16]))
        monkeypatch.setenv("AESR_RING_KSPLIT", str(S))
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
        b = torch.randn(Cout, generator=g)
        xd, up, bd = D(nhwc(x)), D(_pack_wino(hip, w.cuda(), 0)), b.cuda()
        nws = L.aesr_conv2d_wino_workspace_floats(N, H, W, Cin, Cout, 0)
        ws = torch.full((max(nws, 1),), float("nan"), device="cuda")
        out, out1 = (torch.full((N, H, W, Cout), float("nan"), device="cuda") for _ in range(2))
        hip.check(L.aesr_conv2d_wino_fwd_ws(hip.ptr(xd), hip.ptr(up), hip.ptr(bd), hip.ptr(out), hip.ptr(ws), nws, N, H, W, Cin, Cout, 2, 0.0, hip.stream()), "fwd_ws")
        hip.check(L.aesr_conv2d_wino_fwd_ws(hip.ptr(xd), hip.ptr(up), hip.ptr(bd), hip.ptr(out1), None, 0, N, H, W, Cin, Cout, 2, 0.0, hip.stream()), "fwd")
        # data gradient of a layer Cout -> Cin (its K side has Cin channels), LeakyReLU mask
        dy = torch.randn(N, Cin, H, W, generator=g)
        wt = torch.randn(Cin, Cout, 3, 3, generator=g) / np.sqrt(Cin * 9)
        xs = torch.randn(N, Cout, H, W, generator=g)
        dyd, upt, xsd = D(nhwc(dy)), D(_pack_wino(hip, wt.cuda(), 1)), D(nhwc(xs))
        nwd = L.aesr_conv2d_wino_workspace_floats(N, H, W, Cout, Cin, 1)
        wsd = torch.full((max(nwd, 1),), float("nan"), device="cuda")
        dx, dx1 = (torch.full((N, H, W, Cout), float("nan"), device="cuda") for _ in range(2))
        hip.check(L.aesr_conv2d_wino_dgrad_ws(hip.ptr(dyd), hip.ptr(upt), hip.ptr(xsd), hip.ptr(dx), hip.ptr(wsd), nwd, N, H, W, Cout, Cin, 1, 0.01, hip.stream()), "dgrad_ws")
        hip.check(L.aesr_conv2d_wino_dgrad_ws(hip.ptr(dyd), hip.ptr(upt), hip.ptr(xsd), hip.ptr(dx1), None, 0, N, H, W, Cout, Cin, 1, 0.01, hip.stream()), "dgrad")
        torch.cuda.synchronize()
        case = (N, H, W, Cin, Cout, S, nws // out.numel(), nwd // dx.numel())
        ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
        refd = torch.nn.grad.conv2d_input((N, Cout, H, W), wt.double(), dy.double(), padding=1) * torch.where(xs > 0, 1.0, 0.01).double()
        assert rel_l2(nchw(out), ref) < 1e-5 and rel_l2(nchw(out1), ref) < 1e-5, case
        assert rel_l2(nchw(dx), refd) < 1e-5 and rel_l2(nchw(dx1), refd) < 1e-5, case
        assert rel_l2(out, out1) < 2e-6 and rel_l2(dx, dx1) < 2e-6, case
        nsplit += (nws > 0) + (nwd > 0)
    assert nsplit >= 40                       # most of the 60 launches really ran split
    assert L.aesr_conv2d_wino_ring_timeouts() == 0


def test_conv_wino_channel_split_is_planned_for_small_deep_layers(hip):
    """Without any forcing: the launcher asks for slabs on the deep VGG layers of a small shard (few blocks x 512 channels) and on none of
    the layers of a full batch that fills the chip."""
    L = hip.lib
    assert L.aesr_conv2d_wino_workspace_floats(4, 10, 10, 512, 512, 0) > 0
    assert L.aesr_conv2d_wino_workspace_floats(2, 20, 20, 512, 512, 1) > 0
    assert L.aesr_conv2d_wino_workspace_floats(24, 160, 160, 64, 64, 0) == 0
    assert L.aesr_conv2d_wino_workspace_floats(36, 40, 40, 128, 128, 0) == 0
    assert L.aesr_conv2d_wino_workspace_floats(36, 160, 160, 32, 32, 0) == 0       # resident-filter kernel


def test_conv_wino_ring_kernel_selection_and_watchdog(hip, monkeypatch):
    """Layers with many K-side channels run on the ring kernel (kernel id 3); its arrival-counter watchdog never fired in this process;
    forced block shapes (every compile-time patch width of the kernel) give the same results as the planned ones."""
    L = hip.lib
    assert L.aesr_conv2d_wino_kernel(36, 40, 40, 128, 128, 3, 1, 0) == 3
    assert L.aesr_conv2d_wino_kernel(36, 162, 162, 32, 32, 3, 1, 0) == 2
    monkeypatch.setenv("AESR_WINO_RING", "2")           # every streamed layer on the ring kernel, whatever the cost estimates say
    assert L.aesr_conv2d_wino_kernel(36, 81, 81, 64, 64, 3, 1, 0) == 3
    g = torch.Generator().manual_seed(5)
    Cin, Cout, H, W = 128, 64, 18, 22
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g)
    up = D(_pack_wino(hip, w.cuda(), 0))
    # the plan is cached per (N, H, W, channels): a different image count per forced shape
    for n, shape in enumerate(["", "1,4,4", "1,3,5", "2,1,5", "2,2,4", "1,1,7", "4,1,4", "1,2,6", "1,5,3", "1,2,2"]):
        N = 3 + n
        if shape:
            monkeypatch.setenv("AESR_RING_SHAPE", shape)
        x = torch.randn(N, Cin, H, W, generator=g)
        ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.01)
        out = torch.full((N, H, W, Cout), float("nan"), device="cuda")
        hip.check(L.aesr_conv2d_wino_fwd(hip.ptr(D(nhwc(x))), hip.ptr(up), hip.ptr(b.cuda()), hip.ptr(out), N, H, W, Cin, Cout, 1, 0.01, hip.stream()),
                  "wino_fwd " + shape)
        torch.cuda.synchronize()
        assert rel_l2(nchw(out), ref) < 1e-5, shape
    monkeypatch.delenv("AESR_RING_SHAPE", raising=False)
    monkeypatch.delenv("AESR_WINO_RING", raising=False)
    assert L.aesr_conv2d_wino_ring_timeouts() == 0


def test_conv_wino_argument_errors(hip):
    L = hip.lib
    assert L.aesr_conv2d_wino_supported(8, 32, 3, 1, 0) == 0 and L.aesr_conv2d_wino_supported(32, 48, 3, 1, 0) == 0
    assert L.aesr_conv2d_wino_supported(32, 32, 1, 0, 0) == 0 and L.aesr_conv2d_wino_supported(32, 32, 3, 0, 0) == 0
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    out = torch.zeros(1, 4, 4, 32, device="cuda")
    rc = L.aesr_conv2d_wino_fwd(hip.ptr(x), hip.ptr(x), None, hip.ptr(out), 1, 4, 4, 8, 32, 0, 0.0, hip.stream())
    assert rc != 0 and "Cin" in hip.last_error()


@pytest.mark.parametrize("case", [(2, 162, 162, 32, 32), (3, 81, 81, 32, 64), (2, 40, 40, 128, 64), (5, 10, 10, 64, 64), (3, 7, 9, 32, 32),
                                  (1, 1, 1, 32, 32), (2, 2, 3, 64, 96), (1, 33, 130, 32, 32)])
def test_conv_wgrad_wino(hip, case):
    """3x3 / padding-1 layers with both channel counts multiples of 32 take the Winograd weight-gradient kernel
    (csrc/conv_wgrad_wino.hip) behind aesr_conv2d_wgrad: dW, db against fp64 (sums over up to 50k pixels: 2e-5)."""
    N, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(5 + hash(case) % 1000)
    x = torch.randn(N, Cin, H, W, generator=g)
    dy = torch.randn(N, Cout, H, W, generator=g)
    ref_w = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), dy.double(), padding=1)
    ref_b = dy.double().sum((0, 2, 3))
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    ws = torch.empty(hip.lib.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, 3, 1), device="cuda")
    hip.check(hip.lib.aesr_conv2d_wgrad(hip.ptr(D(nhwc(x))), hip.ptr(D(nhwc(dy))), hip.ptr(dw), hip.ptr(db), hip.ptr(ws),
                                        N, H, W, Cin, Cout, 3, 1, hip.stream()), "wgrad")
    torch.cuda.synchronize()
    assert rel_l2(dw, ref_w) < 2e-5
    assert rel_l2(db, ref_b) < 2e-5
    # twice the same call: bitwise identical (fixed-order slab reduction, no atomics)
    dw2 = torch.empty_like(dw)
    hip.check(hip.lib.aesr_conv2d_wgrad(hip.ptr(D(nhwc(x))), hip.ptr(D(nhwc(dy))), hip.ptr(dw2), hip.ptr(db), hip.ptr(ws),
                                        N, H, W, Cin, Cout, 3, 1, hip.stream()), "wgrad")
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize("case", [(3, 80, 80, 64, 32), (2, 160, 160, 32, 32), (2, 6, 10, 32, 64), (1, 2, 2, 32, 32), (2, 40, 40, 128, 64),
                                  (3, 24, 40, 64, 128), (2, 20, 12, 128, 128)])
def test_conv_wino_folded_upsample(hip, case, streamed_kernel):
    """nearest Upsample(x2) in front of a 3x3 convolution folded into the Winograd kernels (Decoder, networks/acai_vanilla.py:92-96):
    forward and weight gradient read the half-resolution tensor through (y/2, x/2); the data gradient stores the 2x2 block sums."""
    N, H, W, Cin, Cout = case              # H, W: the convolution's (upsampled) size
    L = hip.lib
    assert L.aesr_conv2d_wgrad_up2_supported(Cin, Cout) == 1
    g = torch.Generator().manual_seed(H + Cin)
    xh = torch.randn(N, Cin, H // 2, W // 2, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    dy = torch.randn(N, Cout, H, W, generator=g, dtype=torch.float64)
    xh.requires_grad_(True)
    w.requires_grad_(True)
    b.requires_grad_(True)
    xu = F.interpolate(xh, scale_factor=2, mode="nearest")
    ref = F.leaky_relu(F.conv2d(xu, w, b, padding=1), 0.01)
    pre = F.conv2d(xu, w, b, padding=1)
    pre.backward(dy)                          # gradients of the un-activated convolution wrt the half-resolution input / filter
    xd, wd, bd, dyd = D(nhwc(xh.detach().float())), D(w.detach().float()), D(b.detach().float()), D(nhwc(dy.float()))
    out = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    hip.check(L.aesr_conv2d_wino_fwd_up2(hip.ptr(xd), hip.ptr(D(_pack_wino(hip, wd, 0))), hip.ptr(bd), hip.ptr(out), N, H, W, Cin, Cout, 1,
                                         0.01, hip.stream()), "wino_fwd_up2")
    dxh = torch.full((N, H // 2, W // 2, Cin), float("nan"), device="cuda")
    hip.check(L.aesr_conv2d_wino_dgrad_sum2(hip.ptr(dyd), hip.ptr(D(_pack_wino(hip, wd, 1))), hip.ptr(dxh), N, H, W, Cin, Cout, hip.stream()),
              "wino_dgrad_sum2")
    dw = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    ws = torch.empty(L.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, 3, 1), device="cuda")
    hip.check(L.aesr_conv2d_wgrad_up2(hip.ptr(xd), hip.ptr(dyd), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), N, H, W, Cin, Cout, hip.stream()),
              "wgrad_up2")
    torch.cuda.synchronize()
    assert rel_l2(nchw(out), ref.detach()) < 1e-5
    assert rel_l2(nchw(dxh), xh.grad) < 1e-5
    assert rel_l2(dw, w.grad) < 2e-5
    assert rel_l2(db, b.grad) < 2e-5


# ---- BASELINE-size race screens ------------------------------------------------------------------------------------------
# The Winograd kernels order their LDS-DMA staging by hand (vmcnt + barrier); a misplaced wait shows as RARE wrong tiles that come and
# go with size and memory load (one did: conv_wgrad_wino_f32 read a tile before another wave's DMA had landed -- only at 36 images,
# never at the small sizes above).  Inputs with a large common-mode part (activations > 0, gradient ~ 1) make one stale tile
# visible at 1e-4; random inputs hide it below 1e-6.  Every call is made several times: results must be bitwise equal.
def _common_mode(shape, g, grad):
    t = torch.randn(shape, device="cuda", generator=g)
    return 1.0 + 1e-2 * t if grad else F.leaky_relu(t + 0.5, 0.01)


@pytest.mark.parametrize("case", [(36, 162, 162, 32, 32, 0), (36, 160, 160, 32, 32, 1), (36, 81, 81, 64, 64, 0), (36, 40, 40, 128, 128, 0)])
def test_conv_wgrad_wino_baseline_size_repeatable(hip, case):
    N, H, W, Cin, Cout, up2 = case
    L = hip.lib
    g = torch.Generator(device="cuda").manual_seed(11)
    x = _common_mode((N, H // 2, W // 2, Cin) if up2 else (N, H, W, Cin), g, False)
    dy = _common_mode((N, H, W, Cout), g, True)
    ws = torch.empty(L.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, 3, 1), device="cuda")
    outs = []
    for _ in range(4):
        dw = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
        db = torch.full((Cout,), float("nan"), device="cuda")
        if up2:
            hip.check(L.aesr_conv2d_wgrad_up2(hip.ptr(x), hip.ptr(dy), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), N, H, W, Cin, Cout, hip.stream()), "wgrad_up2")
        else:
            hip.check(L.aesr_conv2d_wgrad(hip.ptr(x), hip.ptr(dy), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), N, H, W, Cin, Cout, 3, 1, hip.stream()), "wgrad")
        torch.cuda.synchronize()
        outs.append((dw, db))
    for dw, db in outs[1:]:
        assert torch.equal(dw, outs[0][0]) and torch.equal(db, outs[0][1])
    xn = x.permute(0, 3, 1, 2).double()
    if up2:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    ref_w = torch.nn.grad.conv2d_weight(xn, (Cout, Cin, 3, 3), dy.permute(0, 3, 1, 2).double(), padding=1)
    assert float((outs[0][0].double() - ref_w).norm() / ref_w.norm()) < 2e-6
    assert float((outs[0][1].double() - dy.double().sum((0, 1, 2))).norm() / dy.double().sum((0, 1, 2)).norm()) < 2e-6


@pytest.mark.parametrize("case", [(36, 162, 162, 32, 32), (36, 160, 160, 32, 64), (36, 81, 81, 64, 64), (36, 80, 80, 64, 64), (36, 40, 40, 128, 128),
                                  (24, 80, 80, 128, 128), (24, 20, 20, 512, 512), (6, 40, 40, 128, 128)])
def test_conv_wino_baseline_size_repeatable(hip, case, streamed_kernel):
    """Forward (resident-filter kernel for Cin = 32, streamed kernel above) and masked data gradient at 36 images."""
    N, H, W, Cin, Cout = case
    L = hip.lib
    g = torch.Generator(device="cuda").manual_seed(13)
    x = _common_mode((N, H, W, Cin), g, False)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / np.sqrt(Cin * 9) + 0.02
    b = torch.randn(Cout, device="cuda", generator=g)
    ref = F.leaky_relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1), 0.01).permute(0, 2, 3, 1)
    uf, ub = D(_pack_wino(hip, w, 0)), D(_pack_wino(hip, w, 1))
    outs = []
    for _ in range(3):
        out = torch.full((N, H, W, Cout), float("nan"), device="cuda")
        hip.check(L.aesr_conv2d_wino_fwd(hip.ptr(x), hip.ptr(uf), hip.ptr(b), hip.ptr(out), N, H, W, Cin, Cout, 1, 0.01, hip.stream()), "wino_fwd")
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert float((outs[0].double() - ref).norm() / ref.norm()) < 2e-6
    if Cout % 16 == 0 and Cin % 32 == 0:
        dy = _common_mode((N, H, W, Cout), g, True)
        # data gradient of conv(x) wrt x for upstream gradient dy, then the derivative mask of the PRODUCING activation (x's)
        dref = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.permute(0, 3, 1, 2).double(), padding=1)
        dref = dref * torch.where(x.permute(0, 3, 1, 2) > 0, 1.0, 0.01).double()
        douts = []
        for _ in range(3):
            dx = torch.full((N, H, W, Cin), float("nan"), device="cuda")
            hip.check(L.aesr_conv2d_wino_dgrad(hip.ptr(dy), hip.ptr(ub), hip.ptr(x), hip.ptr(dx), N, H, W, Cin, Cout, 1, 0.01, hip.stream()), "wino_dgrad")
            torch.cuda.synchronize()
            douts.append(dx)
        assert torch.equal(douts[0], douts[1]) and torch.equal(douts[0], douts[2])
        assert float((douts[0].double() - dref.permute(0, 2, 3, 1)).norm() / dref.norm()) < 2e-6


@pytest.mark.parametrize("case", [(3, 160, 160, 32, 32), (2, 81, 81, 32, 64), (2, 37, 41, 32, 32), (1, 6, 6, 32, 64), (36, 160, 160, 32, 64),
                                  (30, 112, 112, 64, 64), (30, 56, 56, 128, 128), (30, 57, 55, 64, 128), (30, 28, 28, 128, 256), (30, 112, 112, 64, 32)])
@pytest.mark.parametrize("pool,act", [(0, 1), (1, 1), (1, 0), (0, 2)])
def test_conv_wino_eval_bn_epilogue(hip, case, pool, act):
    """Slice synthesis: convolution + LeakyReLU + eval-mode BatchNorm (+ AvgPool2d(2)) in one launch == the convolution followed by
    aesr_bn_apply, bit for bit (same per-element arithmetic and order), odd sizes included (the pooled output floors).  The
    resident-filter kernel (Cin = 32 here) and the ring kernel (the dHCP-size layers above it) carry the epilogue."""
    N, H, W, Cin, Cout = case
    L = hip.lib
    kind = L.aesr_conv2d_wino_kernel(N, H, W, Cin, Cout, 3, 1, 0)
    if Cin == 32:
        assert kind == 2 and L.aesr_conv2d_wino_fwd_bn_supported(N, H, W, Cin, Cout)
    elif not L.aesr_conv2d_wino_fwd_bn_supported(N, H, W, Cin, Cout):
        assert kind in (1, 3)       # 3: the ring kernel takes it only WITH a channel split, whose partial sums the epilogue cannot see
        pytest.skip("the planner gives this layer to the first streamed kernel (or a channel split), which has no such epilogue")
    g = torch.Generator(device="cuda").manual_seed(17 + pool)
    x = _common_mode((N, H, W, Cin), g, False)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / np.sqrt(Cin * 9) + 0.02
    b = torch.randn(Cout, device="cuda", generator=g)
    sc = torch.rand(Cout, device="cuda", generator=g) + 0.5
    sh = torch.randn(Cout, device="cuda", generator=g)
    uf = D(_pack_wino(hip, w, 0))
    mid = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    hip.check(L.aesr_conv2d_wino_fwd(hip.ptr(x), hip.ptr(uf), hip.ptr(b), hip.ptr(mid), N, H, W, Cin, Cout, act, 0.01, hip.stream()), "wino_fwd")
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    want = torch.full((N, Ho, Wo, Cout), float("nan"), device="cuda")
    ns = hip.int_array([0, N])
    hip.check(L.aesr_bn_apply(hip.ptr(mid), hip.ptr(sc), hip.ptr(sh), hip.ptr(want), N, H, W, Cout, hip.BN_POOL if pool else hip.BN_NONE, 1, ns,
                              hip.stream()), "apply")
    got = torch.full((N, Ho, Wo, Cout), float("nan"), device="cuda")
    for _ in range(2):
        got.fill_(float("nan"))
        hip.check(L.aesr_conv2d_wino_fwd_bn(hip.ptr(x), hip.ptr(uf), hip.ptr(b), hip.ptr(sc), hip.ptr(sh), hip.ptr(got), N, H, W, Cin, Cout, act, 0.01,
                                            pool, hip.stream()), "wino_fwd_bn")
        torch.cuda.synchronize()
        assert not torch.isnan(got).any()
        assert torch.equal(got, want)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)
    ref = F.leaky_relu(ref, 0.01) if act == 1 else (F.relu(ref) if act == 2 else ref)
    if pool:
        ref = F.avg_pool2d(ref, 2)
    ref = (ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]).permute(0, 2, 3, 1)
    assert float((got.double() - ref).norm() / ref.norm()) < 2e-6


@pytest.mark.parametrize("case", [(30, 3, 224, 224), (2, 1, 6, 6), (1, 4, 8, 8), (5, 0, 4, 4), (7, 16, 10, 6)])
def test_interleave_clamp(hip, case):
    """The super-resolved volume in one pass == n + 1 strided copies and a clamp (generate_hr_volumes.py:57-67), bit for bit."""
    from superresolution_aniso_mri_amd import ops
    Z, n, H, W = case
    g = torch.Generator(device="cuda").manual_seed(Z * 100 + n)
    orig = torch.rand(Z, H, W, device="cuda", generator=g) * 1.4 - 0.2
    synth = torch.rand(max(n * (Z - 1), 1), H, W, device="cuda", generator=g) * 1.4 - 0.2
    got = ops.interleave_clamp(orig, synth if n and Z > 1 else None, n)
    nn_ = n if Z > 1 else 0
    want = torch.full(((Z - 1) * (nn_ + 1) + 1, H, W), float("nan"), device="cuda")
    want[::nn_ + 1] = orig
    for k in range(nn_):
        want[k + 1::nn_ + 1] = synth.reshape(n, Z - 1, H, W)[k]
    want.clamp_(0, 1)
    assert got.shape == want.shape and torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.interleave_clamp(torch.rand(3, 4, 4, device="cuda"), torch.rand(5, 4, 4, device="cuda"), 2)
    assert hip.lib.aesr_interleave_clamp(hip.ptr(orig), hip.ptr(synth), hip.ptr(orig), Z, n, H * W, 0.0, 1.0, hip.stream()) != 0     # in place: refused


def test_conv_wino_eval_bn_epilogue_refuses_other_kernels(hip, monkeypatch):
    """The first streamed kernel and a channel-split layer have no such epilogue: the query says so and the call refuses instead of dropping the BatchNorm."""
    L = hip.lib
    monkeypatch.setenv("AESR_WINO_RING", "1")           # the cost-based choice of round 3 (the default puts every streamed layer on the ring kernel)
    cases = [c for c in [(2, 40, 40, 128, 128), (1, 81, 81, 64, 64), (3, 81, 81, 64, 64), (6, 40, 40, 128, 128), (1, 20, 20, 256, 256)]
             if not L.aesr_conv2d_wino_fwd_bn_supported(*c)]
    if not cases:
        pytest.skip("every candidate layer goes to a kernel with the epilogue under this planner setting")
    N, H, W, Cin, Cout = cases[0]
    assert L.aesr_conv2d_wino_kernel(N, H, W, Cin, Cout, 3, 1, 0) in (1, 3)     # 3: only with a channel split (workspace)
    x = torch.zeros(N * H * W * max(Cin, Cout), device="cuda")
    u = torch.zeros(16 * Cin * Cout, device="cuda")
    rc = L.aesr_conv2d_wino_fwd_bn(hip.ptr(x), hip.ptr(u), None, hip.ptr(x), hip.ptr(x), hip.ptr(x), N, H, W, Cin, Cout, 0, 0.0, 0, hip.stream())
    assert rc != 0
    assert not L.aesr_conv2d_wino_fwd_bn_supported(4, 16, 16, 24, 32)        # not a Winograd layer at all


@pytest.mark.parametrize("sizes", [(24 * 160 * 160, 12 * 160 * 160, 12 * 128 * 20 * 20), (1003, 517, 0), (5, 3, 2)])
def test_combined_mse_loss_block(hip, sizes):
    """aesr_mse3_fwd / _bwd (the loss block of the ae_combined step with MSE losses, one launch each) against torch in fp64;
    repeated calls are bitwise equal (fixed-order sums, the ticket counter is left at zero) and the autograd wrapper matches
    the term-by-term ops."""
    from superresolution_aniso_mri_amd import ops
    n1, n2, n3 = sizes
    g = torch.Generator(device="cuda").manual_seed(n1)
    a1, b1 = torch.rand(n1, device="cuda", generator=g), torch.rand(n1, device="cuda", generator=g)
    a2, b2 = torch.rand(n2, device="cuda", generator=g), torch.rand(n2, device="cuda", generator=g)
    a3, b3 = (torch.rand(n3, device="cuda", generator=g), torch.rand(n3, device="cuda", generator=g)) if n3 else (None, None)
    lam = torch.tensor([0.05], device="cuda")
    ws = torch.zeros(hip.MSE3_WS, dtype=torch.float64, device="cuda")
    outs = []
    for _ in range(3):
        out = torch.full((4,), float("nan"), device="cuda")
        hip.check(hip.lib.aesr_mse3_fwd(hip.ptr(a1), hip.ptr(b1), n1, hip.ptr(a2), hip.ptr(b2), n2, hip.ptr(a3), hip.ptr(b3), n3, hip.ptr(lam),
                                        hip.ptr(ws), hip.ptr(out), hip.stream()), "mse3_fwd")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    m1, m2 = float(((a1.double() - b1.double()) ** 2).mean()), float(((a2.double() - b2.double()) ** 2).mean())
    m3 = float(((a3.double() - b3.double()) ** 2).mean()) if n3 else 0.0
    want = np.array([m1 + 0.05 * m2, m1, 0.05 * m2, m3])
    np.testing.assert_allclose(outs[0].numpy(), want, rtol=3e-7, atol=1e-12)
    gl = torch.tensor([0.7], device="cuda")
    d = torch.full((n1 + n2,), float("nan"), device="cuda")
    hip.check(hip.lib.aesr_mse3_bwd(hip.ptr(a1), hip.ptr(b1), n1, hip.ptr(a2), hip.ptr(b2), n2, hip.ptr(lam), hip.ptr(gl), hip.ptr(d),
                                    hip.ptr(d[n1:]), hip.stream()), "mse3_bwd")
    ref = torch.cat([(a1.double() - b1.double()) * (2 * 0.7 / n1), (a2.double() - b2.double()) * (2 * 0.7 * 0.05 / n2)])
    assert rel_l2(d, ref) < 1e-6
    if n3 and n1 % 2 == 0:
        # the autograd wrapper on image-shaped tensors against the term-by-term ops (kwatsch/cardiac/trainer_ae.py path)
        B, H = 4, 12
        o3 = torch.rand(3 * B, 1, H, H, device="cuda", generator=g).requires_grad_(True)
        x, btw = torch.rand(2 * B, 1, H, H, device="cuda", generator=g), torch.rand(B, 1, H, H, device="cuda", generator=g)
        zm, zr = torch.rand(B, 8, 3, 3, device="cuda", generator=g), torch.rand(B, 8, 3, 3, device="cuda", generator=g)
        total, l1, l2, l3 = ops.combined_mse(o3, x, btw, zm, zr, lam.reshape(()))
        total.backward()
        o3r = o3.detach().clone().requires_grad_(True)
        t2 = ops.mse_loss(o3r[:2 * B], x) + lam.reshape(()) * ops.mse_loss(btw, o3r[2 * B:])
        t2.backward()
        assert abs(float(total) - float(t2)) <= 2e-7 * float(t2) and abs(float(l3) - float(ops.mse_loss(zm, zr))) <= 2e-7
        assert abs(float(l1) + float(l2) - float(total)) <= 1e-7
        assert rel_l2(o3.grad, o3r.grad) < 1e-6


def test_weight_prep_many_equals_the_separate_launches(hip):
    """aesr_weight_prep_many (csrc/prep.hip): implicit-GEMM packing, Winograd transform (both directions), the folded encoder stem and
    the flipped Cout == 1 filter of a whole step in ONE launch -- bitwise what aesr_conv2d_pack_many, aesr_conv2d_wino_pack_many,
    aesr_stemconv_fold and the flip inside aesr_conv2d_cout1_dgrad produce; more than 32 jobs span several launches."""
    g = torch.Generator().manual_seed(77)
    L = hip.lib
    jobs, checks = [], []

    def rnd(*shape):
        return D(torch.randn(*shape, generator=g))

    for k, (cout, cin, ks) in enumerate([(32, 32, 3), (64, 32, 3), (128, 64, 3), (16, 8, 3), (32, 12, 1), (64, 64, 3), (8, 4, 3)] * 3):
        w = rnd(cout, cin, ks, ks)
        for transpose in (0, 1):
            if (cin if not transpose else cout) % 4 == 0:
                n = L.aesr_conv2d_packed_floats(cout, cin, ks, transpose)
                got, want = D(torch.full((n,), float("nan"))), D(torch.empty(n))
                jobs.append(hip.PrepJob(w.data_ptr(), None, None, got.data_ptr(), hip.PREP_PACK, cout, cin, ks, transpose))
                one = (hip.PackJob * 1)(hip.PackJob(w.data_ptr(), want.data_ptr(), cout, cin, ks, transpose))
                hip.check(L.aesr_conv2d_pack_many(one, 1, hip.stream()), "pack")
                checks.append(("pack %d t%d" % (k, transpose), got, want))
            if ks == 3 and L.aesr_conv2d_wino_supported(cin, cout, 3, 1, transpose):
                got = D(torch.full((L.aesr_conv2d_wino_packed_floats(cout, cin, transpose),), float("nan")))
                jobs.append(hip.PrepJob(w.data_ptr(), None, None, got.data_ptr(), hip.PREP_WINO_PACK, cout, cin, 3, transpose))
                checks.append(("wino %d t%d" % (k, transpose), got, _pack_wino(hip, w, transpose)))
    # folded stem: Conv2d(1, 32, 1, padding=1) -> Conv2d(32, 32, 3, padding=1)
    ws, bs, w1 = rnd(32), rnd(32), rnd(32, 32, 3, 3)
    nf = L.aesr_stemconv_folded_floats(32)
    got, want = D(torch.full((nf,), float("nan"))), D(torch.empty(nf))
    jobs.append(hip.PrepJob(w1.data_ptr(), ws.data_ptr(), bs.data_ptr(), got.data_ptr(), hip.PREP_STEM_FOLD, 32, 32, 3, 0))
    hip.check(L.aesr_stemconv_fold(hip.ptr(ws), hip.ptr(bs), hip.ptr(w1), hip.ptr(want), 32, 32, hip.stream()), "fold")
    checks.append(("stem fold", got, want))
    # flipped Cout == 1 filter: wexp[t][ci] = W[0, ci, 8 - t]
    wc = rnd(1, 32, 3, 3)
    flipped = D(torch.full((9 * 32,), float("nan")))
    jobs.append(hip.PrepJob(wc.data_ptr(), None, None, flipped.data_ptr(), hip.PREP_COUT1_FLIP, 1, 32, 3, 0))
    assert len(jobs) > 64          # three launches of <= 32 jobs
    arr = (hip.PrepJob * len(jobs))(*jobs)
    hip.check(L.aesr_weight_prep_many(arr, len(jobs), hip.stream()), "prep_many")
    torch.cuda.synchronize()
    for what, a, b in checks:
        assert torch.equal(a, b), what
    assert torch.equal(flipped.cpu().reshape(9, 32), wc.cpu().reshape(32, 9).flip(1).t())
    # ... and the data gradient that takes it equals the one that flips for itself
    dy, ys = rnd(2, 20, 24, 1), rnd(2, 20, 24, 32)
    dx0, dx1, wsf = D(torch.empty(2, 20, 24, 32)), D(torch.empty(2, 20, 24, 32)), D(torch.empty(9 * 32))
    hip.check(L.aesr_conv2d_cout1_dgrad(hip.ptr(dy), hip.ptr(wc), hip.ptr(ys), hip.ptr(dx0), hip.ptr(wsf), 2, 20, 24, 32, hip.ACT_LRELU, 0.01, hip.stream()), "d0")
    hip.check(L.aesr_conv2d_cout1_dgrad_pre(hip.ptr(dy), hip.ptr(flipped), hip.ptr(ys), hip.ptr(dx1), 2, 20, 24, 32, hip.ACT_LRELU, 0.01, hip.stream()), "d1")
    assert torch.equal(dx0, dx1)
    bad = (hip.PrepJob * 1)(hip.PrepJob(wc.data_ptr(), None, None, flipped.data_ptr(), 9, 1, 32, 3, 0))
    assert L.aesr_weight_prep_many(bad, 1, hip.stream()) != 0 and "kind" in hip.last_error()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape,groups", [((6, 162, 162, 32), [0, 4, 6]), ((6, 81, 81, 64), [0, 4, 6]), ((3, 40, 40, 64), [0, 2, 3]),
                                          ((9, 33, 47, 32), [0, 4, 7, 9]), ((2, 7, 5, 8), [0, 2]), ((1, 2, 2, 128), [0, 1]),
                                          ((5, 80, 80, 32), [0, 5])])
def test_bn_one_launch_equals_three_launches(hip, mode, shape, groups):
    """aesr_bn_fused1_fwd / _bwd (csrc/bn_fused.hip: the layer resident in LDS, one grid barrier) against the three-launch composites the
    engine uses at larger batches (aesr_bn_stats_finalize + aesr_bn_apply, aesr_bn_bwd): same arithmetic per element, partial sums over
    other partitions -> statistics to fp64 rounding of the sums, results to fp32 rounding (2e-6), running statistics and the batch counter
    included; pooled and plain, 1-3 statistic groups, odd sizes (a last row / column the pooling leaves out), more units than workgroups
    and fewer; two calls on one barrier state (the counters are monotonic); repeatable bit for bit."""
    N, H, W, C = shape
    G = len(groups) - 1
    L = hip.lib
    if not L.aesr_bn_fused1_supported(N, H, W, C, mode, G, 1):
        pytest.skip("does not fit the one-launch form")
    g = torch.Generator().manual_seed(N * H + C + mode)
    y = D(F.leaky_relu(torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3, 0.01))
    gam, bet = D(torch.randn(C, generator=g)), D(torch.randn(C, generator=g))
    Ho, Wo = (H // 2, W // 2) if mode == 1 else (H, W)
    ns = hip.int_array(groups)
    counts = hip.double_array([float((groups[i + 1] - groups[i]) * H * W) for i in range(G)])
    bar = D(torch.zeros(int(L.aesr_bn_fused1_barrier_words()), dtype=torch.int32))

    ws_fwd = D(torch.empty(int(L.aesr_bn_fused1_workspace_floats(C, G))))

    def three(y=y):
        rm, rv, nbt = D(torch.zeros(C)), D(torch.ones(C)), D(torch.zeros((), dtype=torch.int64))
        st = [D(torch.full((G, C), float("nan"))) for _ in range(4)]
        partial = D(torch.empty(G * hip.BN_NWG * 2 * C))
        out = D(torch.full((N, Ho, Wo, C), float("nan")))
        hip.check(L.aesr_bn_stats_finalize(hip.ptr(y), hip.ptr(partial), counts, hip.ptr(gam), hip.ptr(bet), hip.ptr(rm), hip.ptr(rv), hip.ptr(nbt),
                                           *[hip.ptr(t) for t in st], H * W, C, G, ns, 0.1, 1e-5, 1, hip.stream()), "stats_finalize")
        hip.check(L.aesr_bn_apply(hip.ptr(y), hip.ptr(st[2]), hip.ptr(st[3]), hip.ptr(out), N, H, W, C, mode, G, ns, hip.stream()), "apply")
        return st, rm, rv, nbt, out

    def one(y=y):
        rm, rv, nbt = D(torch.zeros(C)), D(torch.ones(C)), D(torch.zeros((), dtype=torch.int64))
        st = [D(torch.full((G, C), float("nan"))) for _ in range(4)]
        ws = ws_fwd              # the SAME record buffer every call: a stale record of the previous call would show
        out = D(torch.full((N, Ho, Wo, C), float("nan")))
        hip.check(L.aesr_bn_fused1_fwd(hip.ptr(y), hip.ptr(out), hip.ptr(ws), hip.ptr(bar), counts, hip.ptr(gam), hip.ptr(bet), hip.ptr(rm), hip.ptr(rv),
                                       hip.ptr(nbt), *[hip.ptr(t) for t in st], N, H, W, C, mode, G, ns, 0.1, 1e-5, 1, hip.stream()), "fused fwd")
        return st, rm, rv, nbt, out

    st3, rm3, rv3, nbt3, out3 = three()
    st1, rm1, rv1, nbt1, out1 = one()
    torch.cuda.synchronize()
    assert L.aesr_bn_fused1_timeouts() == 0
    assert int(nbt1) == int(nbt3) == G
    for a, b, what in [(st1[0], st3[0], "mean"), (st1[1], st3[1], "invstd"), (st1[2], st3[2], "scale"), (st1[3], st3[3], "shift"),
                       (rm1, rm3, "running_mean"), (rv1, rv3, "running_var"), (out1, out3, "out")]:
        assert torch.isfinite(a).all(), what
        assert rel_l2(a, b) < 2e-6, what
    # backward through the leading groups (all but the last when there are several), LeakyReLU derivative of the producer folded in
    Gb = max(1, G - 1)
    nb = groups[Gb]
    nsb = hip.int_array(groups[:Gb + 1])
    cb = hip.double_array([float((groups[i + 1] - groups[i]) * H * W) for i in range(Gb)])
    gout = D(torch.randn(nb, Ho, Wo, C, generator=g))

    def bwd(fused):
        coef = D(torch.full((Gb, 2, C), float("nan")))
        dgam, dbet = D(torch.full((C,), float("nan"))), D(torch.full((C,), float("nan")))
        dpre = D(torch.full((nb, H, W, C), float("nan")))
        if fused:
            ws = D(torch.empty(int(L.aesr_bn_fused1_workspace_floats(C, Gb))))
            hip.check(L.aesr_bn_fused1_bwd(hip.ptr(gout), hip.ptr(y), hip.ptr(st3[0]), hip.ptr(st3[1]), hip.ptr(st3[2]), hip.ptr(ws), hip.ptr(bar), cb,
                                           hip.ptr(coef), hip.ptr(dgam), hip.ptr(dbet), hip.ptr(dpre), nb, H, W, C, mode, 1, 0.01, Gb, nsb, hip.stream()),
                      "fused bwd")
        else:
            partial = D(torch.empty(Gb * hip.BN_NWG * 2 * C))
            hip.check(L.aesr_bn_bwd(hip.ptr(gout), hip.ptr(y), hip.ptr(st3[0]), hip.ptr(st3[1]), hip.ptr(st3[2]), hip.ptr(partial), cb, hip.ptr(coef),
                                    hip.ptr(dgam), hip.ptr(dbet), hip.ptr(dpre), nb, H, W, C, mode, 1, 0.01, Gb, nsb, hip.stream()), "bn_bwd")
        return coef, dgam, dbet, dpre

    want = bwd(False)
    got = bwd(True)
    again = bwd(True)
    torch.cuda.synchronize()
    assert L.aesr_bn_fused1_timeouts() == 0
    for a, b, c, what in zip(got, want, again, ("coef", "dgamma", "dbeta", "dpre")):
        assert torch.isfinite(a).all(), what
        assert rel_l2(a, b) < 5e-6, what
        assert torch.equal(a, c), what              # fixed summation order: bitwise repeatable
    _, _, _, _, out1b = one()
    torch.cuda.synchronize()
    assert torch.equal(out1, out1b)
    # other data through the same record buffer and barrier state, back to back (the records cross the barrier as sc1 stores / loads
    # without fences: a record left over from the previous launch must never be read)
    for k in range(6):
        y2 = D(y * (0.5 + 0.25 * k) + (1.0 - 0.3 * k))
        a = one(y2)
        b = three(y2)
        torch.cuda.synchronize()
        # (shifted data: the variance is a difference of nearly equal fp32 partial sums, formed over other partitions in the two paths --
        # 4e-5 on a 4-pixel layer; a stale record would be an error of order 1)
        # (on the 4-pixel layer one channel's variance is 3e-4 of its mean square: 1e-3 in its invstd)
        tol2 = 2e-4 if N * H * W >= 64 else 5e-3
        assert rel_l2(a[4], b[4]) < tol2 and rel_l2(a[0][0], b[0][0]) < tol2 and rel_l2(a[0][1], b[0][1]) < tol2, k
    assert L.aesr_bn_fused1_timeouts() == 0
