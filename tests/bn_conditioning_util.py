"""Train-mode BatchNorm on channels whose |mean| is large against their spread: inputs, the two evaluations that need no GPU, the error
measures and their bounds.  Shared by tests/test_bn_conditioning_reference.py (CPU) and tests/test_gpu_bn_conditioning.py (GPU).

Why: a variance taken as E[x^2] - E[x]^2 from fp32 sums about 0 loses (mean / sigma)^2 roundings; the variance itself does not depend on the
mean, so a sound fp32 algorithm owes the same handful of roundings at every ratio.  Every other BatchNorm test of the suite feeds
leaky_relu(randn)-like data with |mean| / sigma < 1 and cannot tell.

Inputs.  Channel c belongs to class c % 11 of CLASSES = (mean, sigma) pairs; y = mean_c + sigma_c * randn (seeded, formed in fp64, cast to
fp32: the fp32 values are the exact input of every evaluation).  gamma = +-(0.5 + rand), beta = randn; running statistics start at (0, 1),
momentum 0.1, eps 1e-5.  With C = 8 only the first eight classes occur.

Evaluations.
  truth(...)      nn.BatchNorm2d in fp64 on the CPU, group after group (as tests/test_gpu_bn_pool.py), then avg_pool2d / nearest upsample;
                  backward through the leading groups with the LeakyReLU(0.01) derivative of the producer folded in.
  reference(...)  torch.native_batch_norm in fp32 on the CPU (Welford statistics; it returns save_mean / save_invstd) and its autograd.
  restated(...)   numpy restatement of the library's statistics pass (csrc/bn.hip: bn_stats_kernel, 512 workgroups, PL = 256 / (C / 4) pixel
                  lanes, strided fp32 accumulation per thread, the lanes added into an fp32 partial, fp64 over the workgroups) with the sums taken
                  about 0 and the lanes added in fp32 (the scheme the library had) or about the group's pivot (the mean of eight of its pixels) and the lanes added in fp64
                  (the scheme it has), then the arithmetic of csrc/bn_math.h.

Errors, per group and channel, maxima over the channels of a class (iv64 = the truth's invstd, r = |mean64| * iv64):
  mean    |mean - mean64| * iv64                 invstd  |invstd / iv64 - 1|
  out     rms(out - out64) / |gamma_c|           rmean   |rm - rm64| * iv64             rvar  |rv / rv64 - 1|
  dgamma, dbeta, dpre: |error| (dpre: rms) over the absolute sum (dpre: rms) of the summands -- the rule of ``_close`` in
  tests/test_gpu_bn_pool.py.  The summands of dgamma are g * xhat; where xhat vanishes in exact arithmetic (the constant channel:
  sum |g * xhat64| < 2^-24 * sum |g|) no summand has a scale of its own and the error is taken against sum |g|, i.e. in units of xhat.
The running statistics and dgamma / dbeta exist once per channel, not per group: they take the largest iv64 and r of the groups.

Bounds, from the number format and the reference's own error e_ref (same class, shape, group), never from the code under test:
  invstd, rvar            max(16 * 2^-24, 4 * e_ref)                        a handful of roundings (sum, divide, sqrt, store) at any ratio
  mean, rmean, out        max(1e-5, 4 * max(e_ref, 2^-24 * (1 + r)))        1e-5: the suite's forward bound; the fp32 mean alone costs 2^-24 * r
  dgamma, dbeta, dpre     max(2e-5, 4 * max(e_ref, 2^-24 * (1 + r)))        2e-5: the suite's backward bound"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
CLASSES = ((0.0, 1.0), (0.5, 0.5), (2.0, 0.25), (-4.0, 0.5), (8.0, 0.25), (-3.2, 0.1), (12.8, 0.1), (-25.6, 0.05), (102.4, 0.05),
           (3.7, 0.0),            # constant: a dead or bias-only feature map
           (1.0, 1e-4))           # variance << eps
# ([N, H, W, C], group boundaries)
CASES = (((3, 9, 9, 8), (0, 2, 3)),
         ((2, 7, 5, 8), (0, 2)),
         ((6, 33, 31, 32), (0, 4, 6)),
         ((4, 40, 40, 64), (0, 4)),
         ((9, 33, 47, 32), (0, 4, 7, 9)),
         ((12, 80, 80, 32), (0, 11, 12)))          # the grid-stride loops of the statistics kernels wrap
IDS = ["x".join(map(str, s)) for s, _ in CASES]
MODES = ("none", "pool", "up")
SLOPE, MOM, EPS = 0.01, 0.1, 1e-5
FORWARD = ("mean", "invstd", "out", "rmean", "rvar")
BACKWARD = ("dgamma", "dbeta", "dpre")
NWG = 512                                          # workgroups of a statistics launch (_hip.BN_NWG)
PIVOT_N = 8                                        # pixels in a group's pivot (BN_PIVOT_N of csrc/bn_math.h)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def groups_of(groups, H, W):
    """(G, leading groups of the backward pass, their images, values per group)"""
    G = len(groups) - 1
    Gb = max(1, G - 1)
    return G, Gb, groups[Gb], [float((groups[i + 1] - groups[i]) * H * W) for i in range(G)]


def out_dims(H, W, mode):
    return {"none": (H, W), "pool": (H // 2, W // 2), "up": (2 * H, 2 * W)}[mode]


def _post(t, mode):
    if mode == "pool":
        return F.avg_pool2d(t, 2)
    if mode == "up":
        return F.interpolate(t, scale_factor=2, mode="nearest")
    return t


@functools.lru_cache(maxsize=None)
def inputs(shape, groups):
    """Seeded fp32 inputs on the CPU: y [N,C,H,W], gamma, beta.  Made once per case and left unchanged."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W + C)
    cls = torch.arange(C) % len(CLASSES)
    mu = torch.tensor([CLASSES[k][0] for k in cls], dtype=torch.float64).reshape(1, C, 1, 1)
    sd = torch.tensor([CLASSES[k][1] for k in cls], dtype=torch.float64).reshape(1, C, 1, 1)
    y = (mu + sd * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)).float()
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gam = sign * (0.5 + torch.rand(C, generator=g))
    bet = torch.randn(C, generator=g)
    return dict(y=y, gam=gam, bet=bet)


@functools.lru_cache(maxsize=None)
def gradient(shape, groups, mode):
    """The gradient w.r.t. the output of the leading groups, fp32 [nb,C,Ho,Wo]"""
    N, H, W, C = shape
    _, _, nb, _ = groups_of(groups, H, W)
    Ho, Wo = out_dims(H, W, mode)
    g = torch.Generator().manual_seed(7 + 1000 * N + 10 * H + W + C + MODES.index(mode))
    return torch.randn(nb, C, Ho, Wo, generator=g)


@functools.lru_cache(maxsize=None)
def truth(shape, groups, mode):
    """fp64 on the CPU.  -> dict: mean, iv, r [G,C]; out [N,Ho,Wo,C]; rm, rv [C]; dgamma, dbeta [C]; dpre [nb,H,W,C]; the absolute sums of
    the summands dgamma_abs, dbeta_abs [C], dpre_abs [nb,H,W,C]"""
    N, H, W, C = shape
    G, Gb, nb, _ = groups_of(groups, H, W)
    d = inputs(shape, groups)
    y, gam = d["y"], d["gam"].double()
    gout = gradient(shape, groups, mode).double()
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double().train()
    with torch.no_grad():
        bn.weight.copy_(d["gam"])
        bn.bias.copy_(d["bet"])
    y64 = y.double().requires_grad_(True)
    refs = [_post(bn(y64[a:b]), mode) for a, b in zip(groups[:-1], groups[1:])]
    (torch.cat(refs[:Gb]) * gout).sum().backward()
    mask = torch.where(y[:nb] > 0, 1.0, SLOPE).double()
    mean, iv = torch.zeros(G, C, dtype=torch.float64), torch.zeros(G, C, dtype=torch.float64)
    dgam_abs, dbet_abs, dpre_abs = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), []
    for k, (a, b) in enumerate(zip(groups[:-1], groups[1:])):
        yg = y[a:b].double()
        mu, var = yg.mean((0, 2, 3), keepdim=True), yg.var((0, 2, 3), unbiased=False, keepdim=True)
        mean[k], iv[k] = mu.reshape(C), (1.0 / torch.sqrt(var + EPS)).reshape(C)
        if k >= Gb:
            continue
        xh = (yg - mu) / torch.sqrt(var + EPS)
        # the gradient w.r.t. the BatchNorm output at full resolution
        if mode == "pool":
            gp = torch.zeros_like(yg)
            gp[:, :, :H // 2 * 2, :W // 2 * 2] = gout[a:b].repeat_interleave(2, 2).repeat_interleave(2, 3) / 4
        elif mode == "up":
            gp = F.avg_pool2d(gout[a:b], 2) * 4
        else:
            gp = gout[a:b]
        dgam_abs += (gp * xh).abs().sum((0, 2, 3))
        dbet_abs += gp.abs().sum((0, 2, 3))
        k1, k2 = gp.mean((0, 2, 3), keepdim=True), (gp * xh).mean((0, 2, 3), keepdim=True)
        scale = (gam.reshape(1, C, 1, 1) / torch.sqrt(var + EPS)).abs()
        dpre_abs.append(scale * (gp.abs() + k1.abs() + (xh * k2).abs()))
    # xhat == 0 in exact arithmetic: the summands of dgamma have no scale of their own
    dgam_abs = torch.where(dgam_abs < U * dbet_abs, dbet_abs, dgam_abs)
    return dict(mean=mean, iv=iv, r=mean.abs() * iv, out=nhwc(torch.cat(refs).detach()), rm=bn.running_mean.clone(), rv=bn.running_var.clone(),
                dgamma=bn.weight.grad.clone(), dbeta=bn.bias.grad.clone(), dpre=nhwc(y64.grad[:nb] * mask), dgamma_abs=dgam_abs,
                dbeta_abs=dbet_abs, dpre_abs=nhwc(torch.cat(dpre_abs) * mask))


@functools.lru_cache(maxsize=None)
def reference(shape, groups, mode):
    """torch.native_batch_norm in fp32 on the CPU, group after group, and its autograd.  -> dict as an evaluation under test (``errors``)"""
    N, H, W, C = shape
    G, Gb, nb, _ = groups_of(groups, H, W)
    d = inputs(shape, groups)
    y = d["y"].clone().requires_grad_(True)
    gam, bet = d["gam"].clone().requires_grad_(True), d["bet"].clone().requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    outs, means, ivs = [], [], []
    for a, b in zip(groups[:-1], groups[1:]):
        o, sm, siv = torch.native_batch_norm(y[a:b], gam, bet, rm, rv, True, MOM, EPS)
        outs.append(_post(o, mode))
        means.append(sm.detach())
        ivs.append(siv.detach())
    (torch.cat(outs[:Gb]) * gradient(shape, groups, mode)).sum().backward()
    mask = torch.where(d["y"][:nb] > 0, 1.0, SLOPE)
    return dict(mean=torch.stack(means), invstd=torch.stack(ivs), out=nhwc(torch.cat(outs).detach()), rm=rm, rv=rv, dgamma=gam.grad.clone(),
                dbeta=bet.grad.clone(), dpre=nhwc(y.grad[:nb] * mask))


# ---- the library's statistics pass, restated -----------------------------------------------------------------------------------------------
def _restated_sums(x, pivot):
    """x [P,C] fp32, the pixels of one group -> (sum, sum of squares) per channel in fp64, about 0, in the kernel's summation order"""
    P, C = x.shape
    PL = 256 // (C // 4)
    S = NWG * PL
    K = np.zeros(C, np.float32)
    if pivot:                                           # csrc/bn_math.h: bn_pivot_pixel, bn_pivot4
        K = x[min(P // (2 * PIVOT_N) + 17, P - 1)].copy()
        for j in range(1, PIVOT_N):
            K += x[min(((2 * j + 1) * P) // (2 * PIVOT_N) + 17 + 37 * j, P - 1)]
        K *= np.float32(1.0 / PIVOT_N)
    dv = (x - K).astype(np.float32)
    dv = np.concatenate([dv, np.zeros(((-P) % S, C), np.float32)]).reshape(-1, S, C)
    s, q = np.zeros((S, C), np.float32), np.zeros((S, C), np.float32)
    for it in range(dv.shape[0]):                       # a thread's strided pixels
        s += dv[it]
        q += dv[it] * dv[it]
    s, q = s.reshape(NWG, PL, C), q.reshape(NWG, PL, C)
    lanes = np.float64 if pivot else np.float32         # the lanes met in fp32 then; now in fp64, rounded once into the fp32 partial
    sp, qp = np.zeros((NWG, C), lanes), np.zeros((NWG, C), lanes)
    for k in range(PL):                                 # the workgroup's lanes, in order
        sp += s[:, k]
        qp += q[:, k]
    sp, qp = sp.astype(np.float32), qp.astype(np.float32)
    s0, q0, K = sp.astype(np.float64).sum(0), qp.astype(np.float64).sum(0), K.astype(np.float64)
    return s0 + P * K, q0 + 2.0 * K * s0 + P * K * K


def restated(shape, groups, pivot):
    """The forward pass without pooling in numpy, fp32 where the library is: statistics as ``_restated_sums``, then csrc/bn_math.h
    (bn_moments, bn_scale, bn_shift, bn_fwd_elem, bn_running_step).  -> dict(mean, invstd, out, rm, rv)"""
    N, H, W, C = shape
    d = inputs(shape, groups)
    x = nhwc(d["y"]).numpy()
    gam, bet = d["gam"].numpy(), d["bet"].numpy()
    f32 = np.float32
    rm, rv, means, ivs, outs = np.zeros(C, f32), np.ones(C, f32), [], [], []
    for a, b in zip(groups[:-1], groups[1:]):
        xg = x[a:b].reshape(-1, C)
        M = float(xg.shape[0])
        s0, s1 = _restated_sums(xg, pivot)
        mu = s0 / M
        var = np.maximum(s1 / M - mu * mu, 0.0)
        m, iv = mu.astype(f32), (1.0 / np.sqrt(var + float(f32(EPS)))).astype(f32)
        sc = gam * iv
        sh = bet - m * sc
        outs.append((xg * sc + sh).reshape(b - a, H, W, C))
        unb = var * M / (M - 1.0) if M > 1.0 else var
        rm = (f32(1) - f32(MOM)) * rm + f32(MOM) * m
        rv = (f32(1) - f32(MOM)) * rv + f32(MOM) * unb.astype(f32)
        means.append(m)
        ivs.append(iv)
    T = torch.from_numpy
    return dict(mean=T(np.stack(means)), invstd=T(np.stack(ivs)), out=T(np.concatenate(outs)), rm=T(rm), rv=T(rv))


# ---- errors and bounds -------------------------------------------------------------------------------------------------------------------
def errors(shape, groups, mode, got):
    """got: any of mean, invstd [G,C]; out [N,Ho,Wo,C]; rm, rv, dgamma, dbeta [C]; dpre [nb,H,W,C] (tensors on any device)
    -> {quantity: float64 [rows, C]} with one row per group (running statistics, dgamma, dbeta: one row)"""
    N, H, W, C = shape
    G, Gb, nb, _ = groups_of(groups, H, W)
    t = truth(shape, groups, mode)
    d = inputs(shape, groups)
    got = {k: torch.as_tensor(v).detach().double().cpu() for k, v in got.items()}
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), "%s: not finite" % k
    iv_top = t["iv"].max(0).values
    e = {}
    if "mean" in got:
        e["mean"] = (got["mean"] - t["mean"]).abs() * t["iv"]
    if "invstd" in got:
        e["invstd"] = (got["invstd"] / t["iv"] - 1.0).abs()
    if "out" in got:
        assert got["out"].shape == t["out"].shape, (got["out"].shape, t["out"].shape)
        diff = (got["out"] - t["out"]) ** 2
        e["out"] = torch.stack([diff[a:b].mean((0, 1, 2)).sqrt() for a, b in zip(groups[:-1], groups[1:])]) / d["gam"].double().abs()
    if "rm" in got:
        e["rmean"] = ((got["rm"] - t["rm"]).abs() * iv_top).reshape(1, C)
    if "rv" in got:
        e["rvar"] = (got["rv"] / t["rv"] - 1.0).abs().reshape(1, C)
    if "dgamma" in got:
        e["dgamma"] = ((got["dgamma"] - t["dgamma"]).abs() / t["dgamma_abs"]).reshape(1, C)
    if "dbeta" in got:
        e["dbeta"] = ((got["dbeta"] - t["dbeta"]).abs() / t["dbeta_abs"]).reshape(1, C)
    if "dpre" in got:
        assert got["dpre"].shape == t["dpre"].shape, (got["dpre"].shape, t["dpre"].shape)
        diff = (got["dpre"] - t["dpre"]) ** 2
        e["dpre"] = torch.stack([(diff[a:b].mean((0, 1, 2)) / (t["dpre_abs"][a:b] ** 2).mean((0, 1, 2))).sqrt()
                                 for a, b in zip(groups[:Gb], groups[1:Gb + 1])])
    return e


def bound(quantity, e_ref, r, ref_factor=4.0):
    if quantity in ("invstd", "rvar"):
        return max(16.0 * U, ref_factor * e_ref)
    floor = 1e-5 if quantity in FORWARD else 2e-5
    return max(floor, max(ref_factor * e_ref, 4.0 * U * (1.0 + r)))


def table(shape, groups, mode, got, ref_factor=4.0, ref_in_bound=True):
    """Rows (quantity, group or -1, class, r, e_ref, error under test, bound, within) for every quantity of ``got``, maxima over the channels of
    a class.  ref_in_bound False: the bound of the number format alone."""
    C = shape[3]
    t = truth(shape, groups, mode)
    e_ref = errors(shape, groups, mode, reference(shape, groups, mode))
    e_got = errors(shape, groups, mode, got)
    cls = torch.arange(C) % len(CLASSES)
    r_top = t["r"].max(0).values
    rows = []
    for q, eg in e_got.items():
        for row in range(eg.shape[0]):
            per_group = eg.shape[0] == t["r"].shape[0] and q not in ("rmean", "rvar", "dgamma", "dbeta")
            rr = t["r"][row] if per_group else r_top
            for k in sorted(set(cls.tolist())):
                sel = cls == k
                r, er, e = float(rr[sel].max()), float(e_ref[q][row][sel].max()), float(eg[row][sel].max())
                b = bound(q, er if ref_in_bound else 0.0, r, ref_factor)
                rows.append((q, row if per_group else -1, k, r, er, e, b, e <= b))
    return rows


def failures(rows):
    return [row for row in rows if not row[7]]


def render(shape, groups, mode, rows, only_failures=False):
    lines = ["%s groups %s mode %s" % ("x".join(map(str, shape)), list(groups), mode),
             "  quantity group class (mean, sigma)          r     e_ref     error     bound"]
    for q, g, k, r, er, e, b, ok in rows:
        if only_failures and ok:
            continue
        lines.append("  %-8s %5s %5d %-16s %8.1f  %8.2e  %8.2e  %8.2e%s" % (q, "all" if g < 0 else g, k, CLASSES[k], r, er, e, b, "" if ok else "  <-- over"))
    return "\n".join(lines)
