"""-m gpu: train-mode BatchNorm + AvgPool2d(2) pooled once in the statistics pass (include/aesr_hip_bnpool.h; csrc/bn.hip: bn_stats_kernel_pool,
bn_apply_kernel_pooled, bn_bwd_reduce_kernel_pooled) against the three-launch route it replaces and against nn.BatchNorm2d + avg_pool2d in
float64 on the CPU.

- Bit for bit (``torch.equal``; the library is built with contraction off and both routes inline the same expressions of csrc/bn_math.h):
  m == aesr_bn_apply(y, scale = 1, shift = 0, POOL); out == aesr_bn_apply(y, the same scale / shift, POOL); dpre == the existing apply kernel's
  for the same coef; two calls agree.
- The per-channel sums are taken over windows instead of pixels: every statistic and ``out`` against aesr_bn_stats_finalize + aesr_bn_apply
  at rel-L2 < 2e-6, coef / dgamma / dbeta / dpre against aesr_bn_bwd at rel-L2 < 5e-6 -- the bounds of
  tests/test_gpu_kernels.py::test_bn_one_launch_equals_three_launches between two partitions of the same sums.
- Against the fp64 reference at the bounds of test_bn_groups_fwd_bwd: 1e-5 forward (running statistics included), 2e-5 backward.
- One window per group ([1, 2, 2, 128]): the window's mean IS the batch mean and every pixel carries the same gradient, so sum g * xhat and
  with it dgamma and the whole of dpre are zero in exact arithmetic (float64: 1e-16), and both routes return the rounding noise of their
  summands -- a relative error against that is the ratio of two noises (measured: 1.0 between the routes, for dgamma and for dpre).  Where the
  float64 result is below ONE fp32 rounding (2^-24) of the absolute sum of its summands, the same bound is taken relative to that absolute sum
  (``_close``); decided by the float64 reference and the number format alone.  Every other case and quantity keeps the plain rel-L2.
- The three launch entry points between the guard bands of tests/memguard.py at their contractual sizes; refusals write nothing.
- Engine level: one encoder block with ``engine.BN_POOL_ONCE`` off and on, eagerly and as a captured graph.

GUARDED_ENTRIES and EXEMPT partition ``_hip.SIGNATURES_BNPOOL`` (tests/test_abi.py checks that without a GPU)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import memguard as mg

pytestmark = pytest.mark.gpu

GUARDED_ENTRIES = ("aesr_bn_pool_stats_finalize", "aesr_bn_pool_apply", "aesr_bn_pool_bwd")
EXEMPT = {"aesr_bn_pool_supported": "host query"}
# ([N, H, W, C], group boundaries)
CASES = [((2, 2, 3, 4), (0, 2)),                 # one window per image and a column the pooling leaves out
         ((1, 2, 2, 128), (0, 1)),               # many channels
         ((3, 9, 9, 8), (0, 2, 3)),              # odd size, two groups
         ((6, 33, 31, 32), (0, 4, 6)),           # odd size, two groups
         ((4, 40, 40, 64), (0, 4)),              # even, one group
         ((12, 80, 80, 32), (0, 11, 12))]        # group 0: 17 600 windows > BN_NWG * PL = 16 384, the grid-stride loops wrap
GUARD_CASES = CASES[:4]
IDS = ["x".join(map(str, s)) for s, _ in CASES]
TOL_FWD, TOL_BWD = 2e-6, 5e-6                    # between two partitions of the sums (test_bn_one_launch_equals_three_launches)
TOL_REF_FWD, TOL_REF_BWD = 1e-5, 2e-5            # against the fp64 reference (test_bn_groups_fwd_bwd)
SLOPE, MOM, EPS = 0.01, 0.1, 1e-5


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _close(got, want, ref64, summands, tol):
    """rel-L2(got, want) < tol -- unless the exact result (``ref64``) lies below one fp32 rounding of the absolute sum of its summands, where no
    fp32 summation has a relative accuracy: then |got - want| < tol * |summands|.  -> (error, passed)"""
    cancelled = float(ref64.double().norm()) < 2.0 ** -24 * float(summands.double().norm())
    if not cancelled:
        e = rel_l2(got, want)
        return e, e < tol
    e = float((got.double().cpu().reshape(-1) - want.double().cpu().reshape(-1)).norm() / summands.double().norm())
    return e, e < tol


def _groups(groups, H, W):
    """(G, leading groups of the backward pass, their images, counts per group)"""
    G = len(groups) - 1
    Gb = max(1, G - 1)
    return G, Gb, groups[Gb], [float((groups[i + 1] - groups[i]) * H * W) for i in range(G)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, groups):
    """Seeded fp32 inputs (CPU, NHWC) and the fp64 reference: nn.BatchNorm2d group after group + avg_pool2d, gradients through the leading
    groups only, with the LeakyReLU derivative of the producer folded in.  Made once per case and left unchanged."""
    N, H, W, C = shape
    G, Gb, nb, _ = _groups(groups, H, W)
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W + C)
    y = F.leaky_relu(torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3, SLOPE)
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gout = torch.randn(nb, C, H // 2, W // 2, generator=g)
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gam)
        bn.bias.copy_(bet)
    y64 = y.double().requires_grad_(True)
    refs = [F.avg_pool2d(bn(y64[a:b]), 2) for a, b in zip(groups[:-1], groups[1:])]
    (torch.cat(refs[:Gb]) * gout.double()).sum().backward()
    mask = torch.where(y[:nb] > 0, 1.0, SLOPE).double()
    # sum over the leading groups of |g * xhat| per channel: the scale dgamma is summed at (g = gout / 4 on the pooled pixels, 0 on the rest)
    # ... and |scale| * (|g| + |k1| + |xhat * k2|) * act'(y) per element: the scale dpre = scale * (g - k1 - xhat * k2) * act'(y) is summed at
    dgam_abs, dpre_abs = torch.zeros(C, dtype=torch.float64), []
    for a, b in zip(groups[:Gb], groups[1:Gb + 1]):
        yg = y[a:b].double()
        mu, var = yg.mean((0, 2, 3), keepdim=True), yg.var((0, 2, 3), unbiased=False, keepdim=True)
        xh = (yg - mu) / torch.sqrt(var + EPS)
        gp = torch.zeros_like(yg)
        gp[:, :, :H // 2 * 2, :W // 2 * 2] = gout[a:b].double().repeat_interleave(2, 2).repeat_interleave(2, 3) / 4
        dgam_abs += (gp * xh).abs().sum((0, 2, 3))
        k1, k2 = gp.mean((0, 2, 3), keepdim=True), (gp * xh).mean((0, 2, 3), keepdim=True)
        scale = (gam.double().reshape(1, C, 1, 1) / torch.sqrt(var + EPS)).abs()
        dpre_abs.append(scale * (gp.abs() + k1.abs() + (xh * k2).abs()))
    dpre_abs = nhwc(torch.cat(dpre_abs) * mask)
    return dict(y=nhwc(y), gam=gam, bet=bet, gout=nhwc(gout), out_ref=nhwc(torch.cat(refs).detach()), rm_ref=bn.running_mean.clone(),
                rv_ref=bn.running_var.clone(), dpre_ref=nhwc(y64.grad[:nb] * mask), dgam_ref=bn.weight.grad.clone(), dbet_ref=bn.bias.grad.clone(),
                dgam_abs=dgam_abs, dpre_abs=dpre_abs)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _forward(hip, d, shape, groups, pooled):
    """-> dict(mean, invstd, scale, shift, rm, rv, nbt, out[, m]); every output starts as NaN"""
    N, H, W, C = shape
    G, _, _, counts = _groups(groups, H, W)
    L, p = hip.lib, hip.ptr
    y, gam, bet = d["y"].cuda(), d["gam"].cuda(), d["bet"].cuda()
    r = dict(mean=_nan(G, C), invstd=_nan(G, C), scale=_nan(G, C), shift=_nan(G, C), rm=torch.zeros(C, device="cuda"),
             rv=torch.ones(C, device="cuda"), nbt=torch.zeros((), dtype=torch.int64, device="cuda"), out=_nan(N, H // 2, W // 2, C))
    partial = _nan(G * hip.BN_NWG * 2 * C)
    ns, cnt = hip.int_array(groups), hip.double_array(counts)
    tabs = [p(r[k]) for k in ("mean", "invstd", "scale", "shift")]
    if pooled:
        r["m"] = _nan(N, H // 2, W // 2, C)
        hip.check(L.aesr_bn_pool_stats_finalize(p(y), p(r["m"]), p(partial), cnt, p(gam), p(bet), p(r["rm"]), p(r["rv"]), p(r["nbt"]), *tabs,
                                                N, H, W, C, G, ns, MOM, EPS, 1, hip.stream()), "aesr_bn_pool_stats_finalize")
        hip.check(L.aesr_bn_pool_apply(p(r["m"]), p(r["scale"]), p(r["shift"]), p(r["out"]), N, H // 2, W // 2, C, G, ns, hip.stream()),
                  "aesr_bn_pool_apply")
    else:
        hip.check(L.aesr_bn_stats_finalize(p(y), p(partial), cnt, p(gam), p(bet), p(r["rm"]), p(r["rv"]), p(r["nbt"]), *tabs, H * W, C, G, ns,
                                           MOM, EPS, 1, hip.stream()), "aesr_bn_stats_finalize")
        hip.check(L.aesr_bn_apply(p(y), p(r["scale"]), p(r["shift"]), p(r["out"]), N, H, W, C, hip.BN_POOL, G, ns, hip.stream()), "aesr_bn_apply")
    torch.cuda.synchronize()
    return r


def _backward(hip, d, shape, groups, st, m):
    """Backward through the leading groups from the tables ``st`` -> (coef, dgamma, dbeta, dpre); m given: the pooled-once route"""
    N, H, W, C = shape
    _, Gb, nb, counts = _groups(groups, H, W)
    L, p = hip.lib, hip.ptr
    y, gout = d["y"].cuda(), d["gout"].cuda()
    coef, dgam, dbet, dpre = _nan(Gb, 2, C), _nan(C), _nan(C), _nan(nb, H, W, C)
    partial = _nan(Gb * hip.BN_NWG * 2 * C)
    ns, cnt = hip.int_array(groups[:Gb + 1]), hip.double_array(counts[:Gb])
    if m is not None:
        hip.check(L.aesr_bn_pool_bwd(p(gout), p(y), p(m), p(st["mean"]), p(st["invstd"]), p(st["scale"]), p(partial), cnt, p(coef), p(dgam), p(dbet),
                                     p(dpre), nb, H, W, C, hip.ACT_LRELU, SLOPE, Gb, ns, hip.stream()), "aesr_bn_pool_bwd")
    else:
        hip.check(L.aesr_bn_bwd(p(gout), p(y), p(st["mean"]), p(st["invstd"]), p(st["scale"]), p(partial), cnt, p(coef), p(dgam), p(dbet), p(dpre),
                                nb, H, W, C, hip.BN_POOL, hip.ACT_LRELU, SLOPE, Gb, ns, hip.stream()), "aesr_bn_bwd")
    torch.cuda.synchronize()
    return coef, dgam, dbet, dpre


@pytest.mark.parametrize("shape,groups", CASES, ids=IDS)
def test_pooled_once_equals_three_launches_and_float64(shape, groups):
    from superresolution_aniso_mri_amd import _hip as hip
    N, H, W, C = shape
    G, Gb, nb, counts = _groups(groups, H, W)
    assert hip.lib.aesr_bn_pool_supported(N, H, W, C, G) == 1 and hip.lib.aesr_bn_pool_supported(nb, H, W, C, Gb) == 1
    d = _inputs(shape, groups)
    L, p = hip.lib, hip.ptr
    ns = hip.int_array(groups)
    y = d["y"].cuda()
    new, old = _forward(hip, d, shape, groups, True), _forward(hip, d, shape, groups, False)
    again = _forward(hip, d, shape, groups, True)
    assert int(new["nbt"]) == int(old["nbt"]) == G
    for k, t in new.items():
        assert bool(torch.isfinite(t).all()), "%s: NaN left" % k
        assert torch.equal(mg.bits(t), mg.bits(again[k])), "%s: two calls differ" % k
    # bit for bit: the means, and the apply for the same tables
    ones, zeros = torch.ones(G, C, device="cuda"), torch.zeros(G, C, device="cuda")
    m0, out0 = _nan(N, H // 2, W // 2, C), _nan(N, H // 2, W // 2, C)
    hip.check(L.aesr_bn_apply(p(y), p(ones), p(zeros), p(m0), N, H, W, C, hip.BN_POOL, G, ns, hip.stream()), "aesr_bn_apply")
    hip.check(L.aesr_bn_apply(p(y), p(new["scale"]), p(new["shift"]), p(out0), N, H, W, C, hip.BN_POOL, G, ns, hip.stream()), "aesr_bn_apply")
    torch.cuda.synchronize()
    assert torch.equal(new["m"], m0), "m differs from the pooled activation in %d element(s)" % int((new["m"] != m0).sum())
    assert torch.equal(new["out"], out0), "out differs from aesr_bn_apply in %d element(s)" % int((new["out"] != out0).sum())
    # the sums over windows against the sums over pixels, and both against float64
    for k in ("mean", "invstd", "scale", "shift", "rm", "rv", "out"):
        e = rel_l2(new[k], old[k])
        print("%s %s: pooled once vs three launches rel-L2 %.3g" % (shape, k, e))
        assert e < TOL_FWD, (k, e)
    errs = {k: rel_l2(new[k], d[r]) for k, r in (("out", "out_ref"), ("rm", "rm_ref"), ("rv", "rv_ref"))}
    print("%s forward vs float64: %s" % (shape, errs))
    assert max(errs.values()) < TOL_REF_FWD, errs

    # backward through the leading groups, from the pooled-once route's own tables
    got = _backward(hip, d, shape, groups, new, new["m"])
    want = _backward(hip, d, shape, groups, new, None)
    twice = _backward(hip, d, shape, groups, new, new["m"])
    for k, a, b, c in zip(("coef", "dgamma", "dbeta", "dpre"), got, want, twice):
        assert bool(torch.isfinite(a).all()), "%s: NaN left" % k
        assert torch.equal(mg.bits(a), mg.bits(c)), "%s: two calls differ" % k
        e, ok = rel_l2(a, b), rel_l2(a, b) < TOL_BWD
        if k in ("dgamma", "dpre"):
            e, ok = _close(a, b, d[{"dgamma": "dgam_ref", "dpre": "dpre_ref"}[k]], d[{"dgamma": "dgam_abs", "dpre": "dpre_abs"}[k]], TOL_BWD)
        print("%s %s: pooled once vs three launches rel-L2 %.3g" % (shape, k, e))
        assert ok, (k, e)
    errs = {"dbeta": rel_l2(got[2], d["dbet_ref"])}
    errs["dgamma"], ok1 = _close(got[1], d["dgam_ref"], d["dgam_ref"], d["dgam_abs"], TOL_REF_BWD)
    errs["dpre"], ok2 = _close(got[3], d["dpre_ref"], d["dpre_ref"], d["dpre_abs"], TOL_REF_BWD)
    print("%s backward vs float64: %s" % (shape, errs))
    assert ok1 and ok2 and max(errs.values()) < TOL_REF_BWD, errs
    # dpre for the SAME coef is the existing apply kernel's: sums = coef * M are exact in fp64 (24 + 18 bits) and divide back to coef
    coef = got[0]
    sums = coef.double() * torch.tensor(counts[:Gb], dtype=torch.float64, device="cuda").reshape(Gb, 1, 1)
    coef1, dgam1, dbet1, dpre1 = _nan(Gb, 2, C), _nan(C), _nan(C), _nan(nb, H, W, C)
    hip.check(L.aesr_bn_bwd_apply(p(d["gout"].cuda()), p(y), p(new["mean"]), p(new["invstd"]), p(new["scale"]), p(sums), hip.double_array(counts[:Gb]),
                                  p(coef1), p(dgam1), p(dbet1), p(dpre1), nb, H, W, C, hip.BN_POOL, hip.ACT_LRELU, SLOPE, Gb,
                                  hip.int_array(groups[:Gb + 1]), hip.stream()), "aesr_bn_bwd_apply")
    torch.cuda.synchronize()
    assert torch.equal(coef1, coef)
    assert torch.equal(dpre1, got[3]), "dpre differs from the existing kernel's in %d element(s)" % int((dpre1 != got[3]).sum())


# ---- between guard bands ----------------------------------------------------------------------------------------------------------------
def _p(g):
    return ctypes.c_void_p(g.view.data_ptr())


def _guarded_calls(hip, d, shape, groups, poison, shift, refuse=None):
    """The three entry points, every device buffer between guard bands.  refuse: (entry, argument, value) -- that call is expected to be
    refused and to leave its outputs poisoned.  -> the outputs of the three calls."""
    N, H, W, C = shape
    G, Gb, nb, counts = _groups(groups, H, W)
    Ho, Wo = H // 2, W // 2
    L = hip.lib
    f32 = torch.float32
    G_ = lambda n, fill, name, dt=f32: mg.guarded(n, dt, "cuda", fill, shift, name)            # noqa: E731
    ins = {k: G_(d[k].numel(), d[k].reshape(-1), k) for k in ("y", "gam", "bet", "gout")}
    fwd = {k: G_(G * C, poison, k) for k in ("mean", "invstd", "scale", "shift")}
    fwd.update(m=G_(N * Ho * Wo * C, poison, "m"), partial=G_(G * hip.BN_NWG * 2 * C, poison, "partial"))
    state = dict(rm=G_(C, torch.zeros(C), "running_mean"), rv=G_(C, torch.ones(C), "running_var"),
                 nbt=G_(1, torch.zeros(1, dtype=torch.int64), "nbt", torch.int64))
    app = dict(out=G_(N * Ho * Wo * C, poison, "out"))
    bwd = dict(partial_b=G_(Gb * hip.BN_NWG * 2 * C, poison, "partial_b"), coef=G_(Gb * 2 * C, poison, "coef"), dgamma=G_(C, poison, "dgamma"),
               dbeta=G_(C, poison, "dbeta"), dpre=G_(nb * H * W * C, poison, "dpre"))
    every = list(ins.values()) + list(fwd.values()) + list(state.values()) + list(app.values()) + list(bwd.values())
    for g in every:
        assert g.view.data_ptr() % 16 == (4 if g.view.element_size() == 4 else 8) * shift
    saved = {k: mg.bits(g.view) for k, g in ins.items()}
    ns, cnt = hip.int_array(groups), hip.double_array(counts)
    nsb, cntb = hip.int_array(groups[:Gb + 1]), hip.double_array(counts[:Gb])

    def args_of(entry, names, values):
        values = list(values)
        if refuse is not None and refuse[0] == entry:
            values[names.index(refuse[1])] = refuse[2]
        return values

    def run(entry, names, values, outs, frozen):
        """frozen: outputs of earlier calls that this call reads -- they must come back unchanged"""
        before = {k: mg.bits(g.view) for k, g in frozen.items()}
        torch.cuda.synchronize()
        rc = getattr(L, entry)(*args_of(entry, names, values))
        torch.cuda.synchronize()
        mg.assert_guards_intact(every)
        for k, g in ins.items():
            mg.assert_unchanged(g.view, saved[k], k)
        for k, g in frozen.items():
            mg.assert_unchanged(g.view, before[k], k)
        if refuse is not None and refuse[0] == entry:
            assert rc == 1 and entry in hip.last_error(), (refuse, rc, hip.last_error())
            for k, g in outs.items():
                assert mg.poison_left(g.view, poison).numel() == g.view.numel(), "%s: refused, yet %s was written" % (refuse, k)
            return False
        assert rc == 0, hip.last_error()
        for k, g in outs.items():
            left = mg.poison_left(g.view, poison)
            assert left.numel() == 0, "%s: %d element(s) never written, first %d [poison %s, shift %d]" % (k, left.numel(), int(left[0]), poison, shift)
        return True

    names = ["y", "m", "partial", "counts", "gamma", "beta", "running_mean", "running_var", "nbt", "mean", "invstd", "scale", "shift", "N", "H", "W",
             "C", "G", "nstart", "momentum", "eps", "update", "stream"]
    values = [_p(ins["y"]), _p(fwd["m"]), _p(fwd["partial"]), cnt, _p(ins["gam"]), _p(ins["bet"]), _p(state["rm"]), _p(state["rv"]), _p(state["nbt"]),
              _p(fwd["mean"]), _p(fwd["invstd"]), _p(fwd["scale"]), _p(fwd["shift"]), N, H, W, C, G, ns, MOM, EPS, 1, hip.stream()]
    if not run("aesr_bn_pool_stats_finalize", names, values, fwd, {}):
        assert int(state["nbt"].view[0]) == 0 and torch.equal(state["rm"].view.cpu(), torch.zeros(C)) and torch.equal(state["rv"].view.cpu(), torch.ones(C))
        return None
    assert int(state["nbt"].view[0]) == G
    names = ["m", "scale", "shift", "out", "N", "Ho", "Wo", "C", "G", "nstart", "stream"]
    values = [_p(fwd["m"]), _p(fwd["scale"]), _p(fwd["shift"]), _p(app["out"]), N, Ho, Wo, C, G, ns, hip.stream()]
    if not run("aesr_bn_pool_apply", names, values, app, fwd):
        return None
    names = ["gout", "y", "m", "mean", "invstd", "scale", "partial", "counts", "coef", "dgamma", "dbeta", "dpre", "N", "H", "W", "C", "act", "slope",
             "G", "nstart", "stream"]
    values = [_p(ins["gout"]), _p(ins["y"]), _p(fwd["m"]), _p(fwd["mean"]), _p(fwd["invstd"]), _p(fwd["scale"]), _p(bwd["partial_b"]), cntb,
              _p(bwd["coef"]), _p(bwd["dgamma"]), _p(bwd["dbeta"]), _p(bwd["dpre"]), nb, H, W, C, hip.ACT_LRELU, SLOPE, Gb, nsb, hip.stream()]
    if not run("aesr_bn_pool_bwd", names, values, bwd, {k: fwd[k] for k in ("m", "mean", "invstd", "scale")}):
        return None
    res = {k: g.view for k, g in list(fwd.items()) + list(app.items()) + list(bwd.items()) if not k.startswith("partial")}
    res.update(rm=state["rm"].view, rv=state["rv"].view)
    return res


@pytest.mark.parametrize("shape,groups", GUARD_CASES, ids=IDS[:len(GUARD_CASES)])
def test_guard_bands_poisons_and_offset_pointers(shape, groups):
    """NaN poison, finite poison, every pointer one element past a 16-byte boundary: guards intact, inputs unchanged, every output element
    written, the poisoned scratch never read before it is written (results bit-identical across the legs and equal to the plain calls)."""
    from superresolution_aniso_mri_amd import _hip as hip
    d = _inputs(shape, groups)
    plain = _forward(hip, d, shape, groups, True)
    plain.update(zip(("coef", "dgamma", "dbeta", "dpre"), _backward(hip, d, shape, groups, plain, plain["m"])))
    for poison, shift in ((mg.POISON_NAN, 0), (mg.POISON_FINITE, 0), (mg.POISON_NAN, 1), (mg.POISON_FINITE, 1)):
        res = _guarded_calls(hip, d, shape, groups, poison, shift)
        for k, t in res.items():
            assert torch.equal(mg.bits(t), mg.bits(plain[k])), "%s differs from the plain call [poison %s, shift %d]" % (k, poison, shift)


def test_refusals_write_nothing():
    from superresolution_aniso_mri_amd import _hip as hip
    shape, groups = CASES[2]
    d = _inputs(shape, groups)
    for k, (entry, arg, value) in enumerate((("aesr_bn_pool_stats_finalize", "C", 6), ("aesr_bn_pool_stats_finalize", "m", None), ("aesr_bn_pool_stats_finalize", "H", 1),
                              ("aesr_bn_pool_stats_finalize", "G", 5), ("aesr_bn_pool_apply", "C", 6), ("aesr_bn_pool_apply", "out", None),
                              ("aesr_bn_pool_apply", "N", 2), ("aesr_bn_pool_bwd", "C", 12), ("aesr_bn_pool_bwd", "dpre", None),
                              ("aesr_bn_pool_bwd", "W", 1), ("aesr_bn_pool_bwd", "G", 0), ("aesr_bn_pool_bwd", "act", 7))):
        poison = (mg.POISON_NAN, mg.POISON_FINITE)[k % 2]          # each entry point sees both
        assert _guarded_calls(hip, d, shape, groups, poison, 0, refuse=(entry, arg, value)) is None


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


_WATCHED = ("aesr_bn_pool_stats_finalize", "aesr_bn_pool_apply", "aesr_bn_pool_bwd", "aesr_bn_stats_finalize", "aesr_bn_apply", "aesr_bn_bwd")


def _block_pass(engine, runner, seq, x, gout, nstart):
    N = x.shape[0]
    out, saved, steps = runner.forward(x, nstart, True, True, fused=False)
    dx, grads = runner.backward(gout, saved, nstart, N, True, steps=steps)
    return [out, dx] + [grads[p] for p in seq.parameters()]


def test_engine_encoder_block_switch_off_equals_switch_on_eager_and_graphed(monkeypatch):
    """conv -> LReLU -> conv -> LReLU -> BatchNorm -> AvgPool2d(2) with 10 images in groups 7 + 3 (more than the one-launch form takes, so
    the three-launch route is the one replaced), odd size: the output, the input gradient and every parameter gradient with the switch off and
    on within the backward bound; with the switch on, the captured graph gives the eager bits, replay after replay.  Nothing non-linear sits
    behind the BatchNorm, so no LeakyReLU decision can depend on the moved statistics."""
    import torch.nn as nn
    from superresolution_aniso_mri_amd import engine
    torch.manual_seed(5)
    seq = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(16, 16, 3, padding=1), nn.LeakyReLU(0.01), nn.BatchNorm2d(16),
                        nn.AvgPool2d(2)).cuda().train()
    with torch.no_grad():
        seq[4].weight.normal_()
        seq[4].bias.normal_()
    N, H, W = 10, 21, 19
    nstart = [0, 7, 10]
    x = torch.randn(N, H, W, 8, device="cuda")
    gout = torch.randn(N, H // 2, W // 2, 16, device="cuda")
    got = {}
    for on in (False, True):
        monkeypatch.setattr(engine, "BN_POOL_ONCE", on)
        spy = _Spy(engine.lib, _WATCHED)
        monkeypatch.setattr(engine, "lib", spy)
        runner = engine.SequentialRunner(seq)
        res = _block_pass(engine, runner, seq, x, gout, nstart)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine, "lib", spy._lib)
        got[on] = ([t.clone() for t in res], dict(spy.calls))
    assert got[False][1] == {"aesr_bn_pool_stats_finalize": 0, "aesr_bn_pool_apply": 0, "aesr_bn_pool_bwd": 0, "aesr_bn_stats_finalize": 1,
                             "aesr_bn_apply": 1, "aesr_bn_bwd": 1}
    assert got[True][1] == {"aesr_bn_pool_stats_finalize": 1, "aesr_bn_pool_apply": 1, "aesr_bn_pool_bwd": 1, "aesr_bn_stats_finalize": 0,
                            "aesr_bn_apply": 0, "aesr_bn_bwd": 0}
    assert len(got[True][0]) == 2 + 6
    for k, (a, b) in enumerate(zip(got[True][0], got[False][0])):
        e = rel_l2(a, b)
        print("tensor %d: switch on vs off rel-L2 %.3g" % (k, e))
        assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0 and e < TOL_BWD, (k, e)
    # switch on: eager == captured graph, replay == replay
    monkeypatch.setattr(engine, "BN_POOL_ONCE", True)
    runner = engine.SequentialRunner(seq)
    eager = [t.clone() for t in _block_pass(engine, runner, seq, x, gout, nstart)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = _block_pass(engine, runner, seq, x, gout, nstart)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in res])
    for k, (a, b, c) in enumerate(zip(eager, replays[0], replays[1])):
        assert torch.equal(a, got[True][0][k]), k
        assert torch.equal(a, b), "tensor %d: the captured graph differs from the eager pass" % k
        assert torch.equal(b, c), "tensor %d: two replays differ" % k
