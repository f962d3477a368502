"""-m gpu: every route that takes train-mode BatchNorm batch statistics, on channels with |mean| >> spread (tests/bn_conditioning_util.py: the
inputs, the fp64 truth, the fp32 reference torch.native_batch_norm, the error measures and their bounds -- none taken from the code under test).

Routes (csrc/bn.hip, csrc/bn_fused.hip; modes none / pool / upsample where the route has them; every output starts as NaN):
  three     aesr_bn_stats -> aesr_bn_finalize -> aesr_bn_apply; the composite aesr_bn_stats_finalize gives the same bits
  sync      aesr_bn_stats -> aesr_bn_finalize_apply (SyncBN); and "two ranks on one device": aesr_bn_stats on each half of every group's images,
            the two fp64 sums added as the all-reduce does, finalized with the total count -- the sums of different ranks stay addable
  one       aesr_bn_fused1_fwd; a shape is skipped only where aesr_bn_fused1_supported says no, and ONE_LAUNCH_MUST_RUN may not be refused
  pooled    aesr_bn_pool_stats_finalize -> aesr_bn_pool_apply (odd shapes: the left-out row and column still count for the statistics)
and the backward pass of three / one / pooled from that route's own mean / invstd tables (aesr_bn_bwd, aesr_bn_fused1_bwd, aesr_bn_pool_bwd).
The backward reductions have no cancellation of their own; the assertions pin that.
Engine level: one encoder block (1x1 stem, 3x3 conv + LeakyReLU + BatchNorm + AvgPool) whose 3x3 conv has small weights and bias 10 -- the way a real channel
gets |mean| >> spread -- with ``engine.BN_POOL_ONCE`` off and on, against the same block in float64.

Before the sums were taken about a pivot (csrc/bn_math.h) every route failed here on invstd from r = |mean| / sigma ~ 8-32 up
(profiles/bn_conditioning.txt)."""
import pytest
import torch

import bn_conditioning_util as bc

pytestmark = pytest.mark.gpu

ONE_LAUNCH_MUST_RUN = ((2, 7, 5, 8), (9, 33, 47, 32), (4, 40, 40, 64))
MODE_CODE = {"none": 0, "pool": 1, "up": 2}


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _state(G, C):
    return dict(mean=_nan(G, C), invstd=_nan(G, C), scale=_nan(G, C), shift=_nan(G, C), rm=torch.zeros(C, device="cuda"),
                rv=torch.ones(C, device="cuda"), nbt=torch.zeros((), dtype=torch.int64, device="cuda"))


def _dev(shape, groups):
    d = bc.inputs(shape, groups)
    return bc.nhwc(d["y"]).cuda(), d["gam"].cuda(), d["bet"].cuda()


def _tabs(hip, r):
    return [hip.ptr(r[k]) for k in ("mean", "invstd", "scale", "shift")]


def _check(shape, groups, mode, got, what):
    """Every quantity of ``got`` within its bound; prints the worst error / bound per quantity, the whole table where one is over."""
    rows = bc.table(shape, groups, mode, got)
    worst = {}
    for q, g, k, r, er, e, b, ok in rows:
        if q not in worst or e / b > worst[q][0]:
            worst[q] = (e / b, k, r, er, e, b)
    print("%s %s %s: " % ("x".join(map(str, shape)), mode, what) +
          "; ".join("%s %.2g of its bound (class %d, r %.0f, e_ref %.1e, error %.1e)" % ((q,) + w[:5]) for q, w in worst.items()))
    assert not bc.failures(rows), "%s\n%s" % (what, bc.render(shape, groups, mode, rows))


def _forward(hip, route, shape, groups, mode):
    """-> dict(mean, invstd, scale, shift, rm, rv, nbt, out[, m])"""
    N, H, W, C = shape
    G, _, _, counts = bc.groups_of(groups, H, W)
    Ho, Wo = bc.out_dims(H, W, mode)
    L, p, code = hip.lib, hip.ptr, MODE_CODE[mode]
    y, gam, bet = _dev(shape, groups)
    r = _state(G, C)
    r["out"] = _nan(N, Ho, Wo, C)
    ns, cnt = hip.int_array(groups), hip.double_array(counts)
    partial = _nan(G * hip.BN_NWG * 2 * C)
    run = (p(r["rm"]), p(r["rv"]), p(r["nbt"]))
    if route in ("three", "sync", "sync2"):
        sums = torch.full((G, 2, C), float("nan"), dtype=torch.float64, device="cuda")
        if route == "sync2":
            # rank 0 takes the first half of every group's images (the larger one), rank 1 the rest: each its own launch, pivots and sums
            halves = [(a, (a + b + 1) // 2, b) for a, b in zip(groups[:-1], groups[1:])]
            total = torch.zeros_like(sums)
            for rank in (0, 1):
                spans = [(a, h) if rank == 0 else (h, b) for a, h, b in halves]
                yr = torch.cat([y[a:b] for a, b in spans]).contiguous()
                nsr = [0]
                for a, b in spans:
                    nsr.append(nsr[-1] + b - a)
                sr = torch.full_like(sums, float("nan"))
                hip.check(L.aesr_bn_stats(p(yr), p(partial), p(sr), H * W, C, G, hip.int_array(nsr), hip.stream()), "aesr_bn_stats")
                total += sr
            sums = total
        else:
            hip.check(L.aesr_bn_stats(p(y), p(partial), p(sums), H * W, C, G, ns, hip.stream()), "aesr_bn_stats")
        if route == "three":
            hip.check(L.aesr_bn_finalize(p(sums), cnt, p(gam), p(bet), *run, *_tabs(hip, r), C, G, bc.MOM, bc.EPS, 1, 1, hip.stream()), "aesr_bn_finalize")
            hip.check(L.aesr_bn_apply(p(y), p(r["scale"]), p(r["shift"]), p(r["out"]), N, H, W, C, code, G, ns, hip.stream()), "aesr_bn_apply")
        else:
            assert L.aesr_bn_fused_supported(C, G) == 1
            hip.check(L.aesr_bn_finalize_apply(p(sums), cnt, p(gam), p(bet), *run, *_tabs(hip, r), p(y), p(r["out"]), N, H, W, C, code, G, ns, bc.MOM,
                                               bc.EPS, 1, hip.stream()), "aesr_bn_finalize_apply")
    elif route == "composite":
        hip.check(L.aesr_bn_stats_finalize(p(y), p(partial), cnt, p(gam), p(bet), *run, *_tabs(hip, r), H * W, C, G, ns, bc.MOM, bc.EPS, 1, hip.stream()),
                  "aesr_bn_stats_finalize")
        hip.check(L.aesr_bn_apply(p(y), p(r["scale"]), p(r["shift"]), p(r["out"]), N, H, W, C, code, G, ns, hip.stream()), "aesr_bn_apply")
    elif route == "one":
        ws = _nan(int(L.aesr_bn_fused1_workspace_floats(C, G)))
        bar = torch.zeros(int(L.aesr_bn_fused1_barrier_words()), dtype=torch.int32, device="cuda")
        hip.check(L.aesr_bn_fused1_fwd(p(y), p(r["out"]), p(ws), p(bar), cnt, p(gam), p(bet), *run, *_tabs(hip, r), N, H, W, C, code, G, ns, bc.MOM,
                                       bc.EPS, 1, hip.stream()), "aesr_bn_fused1_fwd")
    elif route == "pooled":
        assert mode == "pool" and L.aesr_bn_pool_supported(N, H, W, C, G) == 1
        r["m"] = _nan(N, Ho, Wo, C)
        hip.check(L.aesr_bn_pool_stats_finalize(p(y), p(r["m"]), p(partial), cnt, p(gam), p(bet), *run, *_tabs(hip, r), N, H, W, C, G, ns, bc.MOM,
                                                bc.EPS, 1, hip.stream()), "aesr_bn_pool_stats_finalize")
        hip.check(L.aesr_bn_pool_apply(p(r["m"]), p(r["scale"]), p(r["shift"]), p(r["out"]), N, Ho, Wo, C, G, ns, hip.stream()), "aesr_bn_pool_apply")
    else:
        raise ValueError(route)
    torch.cuda.synchronize()
    assert int(r["nbt"]) == G
    return r


def _backward(hip, route, shape, groups, mode, st):
    """Backward through the leading groups from the tables ``st`` of the route -> dict(dgamma, dbeta, dpre)"""
    N, H, W, C = shape
    _, Gb, nb, counts = bc.groups_of(groups, H, W)
    L, p, code = hip.lib, hip.ptr, MODE_CODE[mode]
    y = _dev(shape, groups)[0]
    gout = bc.nhwc(bc.gradient(shape, groups, mode)).cuda()
    coef, dgam, dbet, dpre = _nan(Gb, 2, C), _nan(C), _nan(C), _nan(nb, H, W, C)
    ns, cnt = hip.int_array(groups[:Gb + 1]), hip.double_array(counts[:Gb])
    tabs = (p(st["mean"]), p(st["invstd"]), p(st["scale"]))
    if route == "one":
        ws = _nan(int(L.aesr_bn_fused1_workspace_floats(C, Gb)))
        bar = torch.zeros(int(L.aesr_bn_fused1_barrier_words()), dtype=torch.int32, device="cuda")
        hip.check(L.aesr_bn_fused1_bwd(p(gout), p(y), *tabs, p(ws), p(bar), cnt, p(coef), p(dgam), p(dbet), p(dpre), nb, H, W, C, code, hip.ACT_LRELU,
                                       bc.SLOPE, Gb, ns, hip.stream()), "aesr_bn_fused1_bwd")
    elif route == "pooled":
        partial = _nan(Gb * hip.BN_NWG * 2 * C)
        hip.check(L.aesr_bn_pool_bwd(p(gout), p(y), p(st["m"]), *tabs, p(partial), cnt, p(coef), p(dgam), p(dbet), p(dpre), nb, H, W, C, hip.ACT_LRELU,
                                     bc.SLOPE, Gb, ns, hip.stream()), "aesr_bn_pool_bwd")
    else:
        partial = _nan(Gb * hip.BN_NWG * 2 * C)
        hip.check(L.aesr_bn_bwd(p(gout), p(y), *tabs, p(partial), cnt, p(coef), p(dgam), p(dbet), p(dpre), nb, H, W, C, code, hip.ACT_LRELU, bc.SLOPE,
                                Gb, ns, hip.stream()), "aesr_bn_bwd")
    torch.cuda.synchronize()
    return dict(dgamma=dgam, dbeta=dbet, dpre=dpre)


def _stats(r):
    return dict(mean=r["mean"], invstd=r["invstd"], out=r["out"], rm=r["rm"], rv=r["rv"])


@pytest.mark.parametrize("shape,groups", bc.CASES, ids=bc.IDS)
def test_three_launches(shape, groups):
    from superresolution_aniso_mri_amd import _hip as hip
    for mode in bc.MODES:
        r = _forward(hip, "three", shape, groups, mode)
        _check(shape, groups, mode, _stats(r), "three launches")
        c = _forward(hip, "composite", shape, groups, mode)
        for k in ("mean", "invstd", "scale", "shift", "rm", "rv", "out"):
            assert torch.equal(r[k], c[k]), "%s: aesr_bn_stats_finalize differs from aesr_bn_stats + aesr_bn_finalize" % k
        _check(shape, groups, mode, _backward(hip, "three", shape, groups, mode, r), "aesr_bn_bwd")


@pytest.mark.parametrize("shape,groups", bc.CASES, ids=bc.IDS)
def test_syncbn_form_one_rank_and_two_ranks_on_one_device(shape, groups):
    from superresolution_aniso_mri_amd import _hip as hip
    for mode in bc.MODES:
        _check(shape, groups, mode, _stats(_forward(hip, "sync", shape, groups, mode)), "aesr_bn_finalize_apply")
    # the sums do not depend on the mode: the two ranks once
    _check(shape, groups, "none", _stats(_forward(hip, "sync2", shape, groups, "none")), "two ranks' sums added")


@pytest.mark.parametrize("shape,groups", bc.CASES, ids=bc.IDS)
def test_one_launch(shape, groups):
    from superresolution_aniso_mri_amd import _hip as hip
    N, H, W, C = shape
    G, Gb, nb, _ = bc.groups_of(groups, H, W)
    L = hip.lib
    ran = 0
    for mode in ("none", "pool"):
        if not L.aesr_bn_fused1_supported(N, H, W, C, MODE_CODE[mode], G, 0):
            assert shape not in ONE_LAUNCH_MUST_RUN, "%s %s: refused by aesr_bn_fused1_supported" % (shape, mode)
            continue
        ran += 1
        r = _forward(hip, "one", shape, groups, mode)
        assert L.aesr_bn_fused1_timeouts() == 0
        _check(shape, groups, mode, _stats(r), "aesr_bn_fused1_fwd")
        if not L.aesr_bn_fused1_supported(nb, H, W, C, MODE_CODE[mode], Gb, 1):
            assert shape not in ONE_LAUNCH_MUST_RUN, "%s %s: backward refused by aesr_bn_fused1_supported" % (shape, mode)
            print("%s %s: the backward pass does not fit the one-launch form" % (shape, mode))
            continue
        _check(shape, groups, mode, _backward(hip, "one", shape, groups, mode, r), "aesr_bn_fused1_bwd")
        assert L.aesr_bn_fused1_timeouts() == 0
    if not ran:
        pytest.skip("does not fit the one-launch form (aesr_bn_fused1_supported)")


@pytest.mark.parametrize("shape,groups", bc.CASES, ids=bc.IDS)
def test_pooled_once(shape, groups):
    from superresolution_aniso_mri_amd import _hip as hip
    r = _forward(hip, "pooled", shape, groups, "pool")
    _check(shape, groups, "pool", _stats(r), "pooled once")
    _check(shape, groups, "pool", _backward(hip, "pooled", shape, groups, "pool", r), "aesr_bn_pool_bwd")


# ---- engine level -----------------------------------------------------------------------------------------------------------------------
def _block(dtype):
    import torch.nn as nn
    torch.manual_seed(11)
    # (the engine runs the 3x3 convolution of a single-channel image only behind the network's 1x1 stem: the block starts with that stem)
    seq = nn.Sequential(nn.Conv2d(1, 32, 1), nn.Conv2d(32, 32, 3, padding=1), nn.LeakyReLU(0.01), nn.BatchNorm2d(32, eps=bc.EPS, momentum=bc.MOM),
                        nn.AvgPool2d(2)).train()
    with torch.no_grad():
        seq[1].weight.mul_(0.02)
        seq[1].bias.fill_(10.0)
        seq[3].weight.copy_(torch.where(torch.rand(32) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(32)))
        seq[3].bias.normal_()
    return seq.to(dtype)


def _block_cpu(dtype, x, gout):
    """The block on the CPU in ``dtype`` -> dict(out [N,Ho,Wo,C], rm, rv, dgamma, dbeta) and the activation entering the BatchNorm"""
    seq = _block(dtype)
    act = seq[2](seq[1](seq[0](bc.nchw(x).to(dtype))))
    out = seq[4](seq[3](act))
    (out * bc.nchw(gout).to(dtype)).sum().backward()
    return dict(out=bc.nhwc(out.detach()), rm=seq[3].running_mean.clone(), rv=seq[3].running_var.clone(), dgamma=seq[3].weight.grad.clone(),
                dbeta=seq[3].bias.grad.clone()), act.detach()


def _block_errors(got, t, act64, gam, gout):
    """The measures of bn_conditioning_util.errors, per channel, for the block (one group)"""
    C = act64.shape[1]
    mu, var = act64.mean((0, 2, 3)), act64.var((0, 2, 3), unbiased=False)
    iv = 1.0 / torch.sqrt(var + bc.EPS)
    xh = (act64 - mu.reshape(1, C, 1, 1)) * iv.reshape(1, C, 1, 1)
    gp = bc.nchw(gout).double().repeat_interleave(2, 2).repeat_interleave(2, 3) / 4
    got = {k: v.detach().double().cpu() for k, v in got.items()}
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    e = dict(out=((got["out"] - t["out"]) ** 2).mean((0, 1, 2)).sqrt() / gam.abs(), rmean=(got["rm"] - t["rm"]).abs() * iv,
             rvar=(got["rv"] / t["rv"] - 1.0).abs(), dgamma=(got["dgamma"] - t["dgamma"]).abs() / (gp * xh).abs().sum((0, 2, 3)),
             dbeta=(got["dbeta"] - t["dbeta"]).abs() / gp.abs().sum((0, 2, 3)))
    return e, mu.abs() * iv


def test_engine_encoder_block_with_a_large_bias(monkeypatch):
    """4 x 1 x 40 x 40 images, the 3x3 conv's weights x 0.02 and its bias 10: every channel enters the BatchNorm at 10 +- a few hundredths.  Output, running
    statistics, dgamma and dbeta against the block in float64, bounded per channel by the block in fp32 on the CPU and the number format."""
    from superresolution_aniso_mri_amd import engine
    g = torch.Generator().manual_seed(3)
    x, gout = torch.randn(4, 40, 40, 1, generator=g), torch.randn(4, 20, 20, 32, generator=g)
    t, act64 = _block_cpu(torch.float64, x, gout)
    ref, _ = _block_cpu(torch.float32, x, gout)
    gam = _block(torch.float64)[3].weight.detach()
    e_ref, r = _block_errors(ref, t, act64, gam, gout)
    assert float(r.min()) > 30.0, r                       # the case is what it claims to be
    # four images fit the one-launch form, which the engine prefers; with that form off (AESR_BN_FUSED=0) the switch chooses between the three
    # launches and the pooled-once route
    routes = set()
    for one_launch, on in ((True, False), (True, True), (False, False), (False, True)):
        monkeypatch.setenv("AESR_BN_FUSED", "1" if one_launch else "0")
        monkeypatch.setattr(engine, "BN_POOL_ONCE", on)
        calls, real = [], engine.lib

        class Spy:
            def __getattr__(self, name):
                if name.startswith("aesr_bn_") and name.endswith(("_fwd", "stats_finalize")):
                    calls.append(name)
                return getattr(real, name)

        monkeypatch.setattr(engine, "lib", Spy())
        seq = _block(torch.float32).cuda()
        runner = engine.SequentialRunner(seq)
        out, saved, steps = runner.forward(x.cuda(), [0, 4], True, True, fused=False)
        _, grads = runner.backward(gout.cuda(), saved, [0, 4], 4, True, steps=steps)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine, "lib", real)
        routes.update(calls)
        bn = seq[3]
        got = dict(out=out, rm=bn.running_mean, rv=bn.running_var, dgamma=grads[bn.weight], dbeta=grads[bn.bias])
        e, _ = _block_errors(got, t, act64, gam, gout)
        lines, bad = [], 0
        for q in e:
            for c in range(32):
                b = bc.bound(q, float(e_ref[q][c]), float(r[c]))
                ok = float(e[q][c]) <= b
                bad += not ok
                lines.append("  %-7s channel %2d r %7.1f e_ref %.2e error %.2e bound %.2e%s" % (q, c, float(r[c]), float(e_ref[q][c]), float(e[q][c]), b,
                                                                                              "" if ok else "  <-- over"))
        what = "one-launch form %s, BN_POOL_ONCE %s (%s)" % ("allowed" if one_launch else "off", on, ", ".join(calls))
        print("%s: worst error / bound %s" % (what, {q: "%.2g" % max(float(e[q][c]) / bc.bound(q, float(e_ref[q][c]), float(r[c])) for c in range(32))
                                                     for q in e}))
        assert not bad, "%s\n%s" % (what, "\n".join(lines))
    assert {"aesr_bn_stats_finalize", "aesr_bn_pool_stats_finalize"} <= routes, routes
