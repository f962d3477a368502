"""The Adam step (csrc/elementwise.hip: adam_step_kernel, ops.HipAdam): the fp64 restatement, the cases, the error measures and their bounds.
Shared by tests/test_adam_reference.py (CPU) and tests/test_gpu_adam.py (GPU).

Restatement.  ``adam64`` is torch's single-tensor Adam (not amsgrad, L2 weight decay added to the gradient) in float64:
    g += wd * p;   m = m + (g - m) * (1 - b1);   v = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** t;   bc2 = 1 - b2 ** t                     (Python doubles)
    p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
with per-step gradients and per-step (lr, betas, eps, wd), so schedules can be written down.  tests/test_adam_reference.py pins it against
``torch.optim.Adam`` in float64.

Cases.  Inputs are seeded, formed in float64 and cast to float32; the float32 values are the exact input of every evaluation.
p0 = 0.05 * randn, so an update of ~lr is well resolved in fp32.  The gradient of every 7th element is exactly 0 in all steps.
  regimes   unit: randn;  eps: 1e-9 * randn (eps = 1e-8 decides the step);  decades: 10^U{-12..3} per element, times randn;  huge: 1e15 * randn
            -- each for 3 and for 300 steps, without and with weight decay.  Gradients whose square leaves the fp32 range are out of scope.
  hyper     betas x eps x lr x wd of HYPER_GRID, 20 steps each, unit gradients.

Errors of an fp32 evaluation against the restatement, after a step:
  p   max |p - p64| / lr
  v   max |v / v64 - 1| where v64 >= 1e-30
  m   max |m - m64| / (largest |g + wd * p| the element has seen); an element that has seen none must hold m == 0 exactly
First step of a trainer.  With m = v = 0 the first Adam step is dp = -lr * g / (|g| + eps) whatever the betas (``first_step_check``).
Yardstick.  ``e_ref``: these errors for torch's own fp32 CPU Adam on identical inputs, as running maxima over the steps taken so far.
Bound of the kernel after step t: 4 * e_ref[t] (+ one fp32 ulp of p for p).  The factor covers roundings that legitimately differ from
torch's (fmaf for the weight decay, lr / bc1 in fp32, the association of (1 - b2) * g * g, a contracted b2 * v + ...): one rounding per
element per step each, the order of torch's own error.  Nothing here comes from the code under test."""
import functools
import itertools

import numpy as np
import torch

N_ARITH = 4099           # not a multiple of 4 or 256; one partial grid
N_STATE = 70001          # more elements than the launch has threads (128 workgroups of 256), with a tail
FACTOR = 4.0
V_FLOOR = 1e-30


def hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    return dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), wd=float(wd))


def adam64(p0, grads, hypers, m0=None, v0=None, t0=0):
    """Float64 Adam from step count ``t0``.  grads: one array per step; hypers: one ``hyper()`` per step (or one for all).
    Returns [(p, m, v, geff)] after every step, geff = the gradient the step used (g + wd * p)."""
    if isinstance(hypers, dict):
        hypers = [hypers] * len(grads)
    p = np.asarray(p0, dtype=np.float64).copy()
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, dtype=np.float64).copy()
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, dtype=np.float64).copy()
    out = []
    for k, (g, h) in enumerate(zip(grads, hypers)):
        t = t0 + k + 1
        b1, b2 = h["betas"]
        g = np.asarray(g, dtype=np.float64)
        if h["wd"] != 0.0:
            g = g + h["wd"] * p
        m = m + (g - m) * (1.0 - b1)
        v = b2 * v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        step_size = h["lr"] / bc1
        p = p + ((-step_size) * m) / (np.sqrt(v) / bc2 ** 0.5 + h["eps"])      # addcdiv_: (value * m) / denom
        out.append((p.copy(), m.copy(), v.copy(), g))
    return out


def torch_adam(p0, grads, hypers, dtype, m0=None, v0=None, t0=0):
    """``torch.optim.Adam`` (single-tensor) on the CPU in ``dtype`` on the same inputs.  Returns [(p, m, v)] as numpy arrays."""
    if isinstance(hypers, dict):
        hypers = [hypers] * len(grads)
    p = torch.nn.Parameter(torch.as_tensor(np.asarray(p0)).to(dtype).clone())
    h = hypers[0]
    opt = torch.optim.Adam([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["wd"], foreach=False)
    if t0 or m0 is not None:
        zero = torch.zeros_like(p.data)
        opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": zero.clone() if m0 is None else torch.as_tensor(np.asarray(m0)).to(dtype).clone(),
                        "exp_avg_sq": zero.clone() if v0 is None else torch.as_tensor(np.asarray(v0)).to(dtype).clone()}
    out = []
    for g, h in zip(grads, hypers):
        grp = opt.param_groups[0]
        grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"] = h["lr"], h["betas"], h["eps"], h["wd"]
        p.grad = torch.as_tensor(np.asarray(g)).to(dtype).clone()
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
REGIMES = ("unit", "eps", "decades", "huge")
HYPER_GRID = tuple(itertools.product(((0.9, 0.999), (0.5, 0.999), (0.0, 0.9)), (1e-8, 1e-3), (1e-3, 1e-5), (0.0, 0.01)))


def _cases():
    out = {}
    for regime, steps, wd in itertools.product(REGIMES, (3, 300), (0.0, 0.01)):
        out["%s-%d-wd%g" % (regime, steps, wd)] = dict(regime=regime, steps=steps, hyper=hyper(wd=wd), n=N_ARITH)
    for betas, eps, lr, wd in HYPER_GRID:
        out["hyper-b%g_%g-eps%g-lr%g-wd%g" % (betas + (eps, lr, wd))] = dict(regime="unit", steps=20, hyper=hyper(lr, betas, eps, wd), n=N_ARITH)
    return out


CASES = _cases()
CASE_IDS = tuple(CASES)


def gradients(regime, n, steps, gen):
    """[steps] float32 arrays; element i with i % 7 == 0 is exactly 0 in every step."""
    r = torch.randn(steps, n, generator=gen, dtype=torch.float64)
    if regime == "eps":
        r = r * 1e-9
    elif regime == "decades":
        r = r * 10.0 ** torch.randint(-12, 4, (n,), generator=gen).double()
    elif regime == "huge":
        r = r * 1e15
    elif regime != "unit":
        raise ValueError(regime)
    r[:, ::7] = 0.0
    return list(r.float().numpy())


@functools.lru_cache(maxsize=4)
def case_inputs(name):
    """(p0 float32, [gradients float32], hyper) of a case; the same arrays for every caller."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(1000 + CASE_IDS.index(name))
    p0 = (0.05 * torch.randn(c["n"], generator=gen, dtype=torch.float64)).float().numpy()
    return p0, gradients(c["regime"], c["n"], c["steps"], gen), c["hyper"]


# ---- error measures and bounds -------------------------------------------------------------------------------------------------------
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


class Scale:
    """Per-element largest |g + wd * p| seen so far (the scale of exp_avg), advanced step by step alongside a reference run."""

    def __init__(self, n, g0=None):
        self.gmax = np.zeros(n) if g0 is None else np.abs(np.asarray(g0, dtype=np.float64))

    def advance(self, geff):
        self.gmax = np.maximum(self.gmax, np.abs(geff))
        return self.gmax


def step_errors(got, ref, lr, gmax):
    """dict(p, v, m) of one step: ``got`` = (p, m, v) of an fp32 evaluation, ``ref`` = (p, m, v, ...) of adam64."""
    p, m, v = (np.asarray(a, dtype=np.float64) for a in got[:3])
    p64, m64, v64 = ref[:3]
    big = v64 >= V_FLOOR
    seen = gmax > 0
    dm = np.abs(m - m64)
    em = float((dm[seen] / gmax[seen]).max()) if seen.any() else 0.0
    if (dm[~seen] != 0).any():
        em = float("inf")
    return dict(p=float(np.abs(p - p64).max() / lr), v=float(np.abs(v[big] / v64[big] - 1.0).max()) if big.any() else 0.0, m=em,
                p_excess=float(((np.abs(p - p64) - ulp32(p64)) / lr).max()))


def run_errors(got_steps, ref_steps, hypers, g0=None):
    """Errors after every step and their running maxima: ([per step dict], [running max dict])."""
    if isinstance(hypers, dict):
        hypers = [hypers] * len(ref_steps)
    sc = Scale(len(ref_steps[0][0]), g0)
    per, run, cur = [], [], dict(p=0.0, v=0.0, m=0.0, p_excess=-float("inf"))
    for got, ref, h in zip(got_steps, ref_steps, hypers):
        e = step_errors(got, ref, h["lr"], sc.advance(ref[3]))
        cur = {k: max(cur[k], e[k]) for k in e}
        per.append(e)
        run.append(cur)
    return per, run


def e_ref(p0, grads, hypers, m0=None, v0=None, t0=0, g0=None):
    """The yardstick: torch's fp32 CPU Adam against the restatement on identical inputs.  Returns (ref_steps, [running max dict])."""
    ref = adam64(p0, grads, hypers, m0, v0, t0)
    return ref, run_errors(torch_adam(p0, grads, hypers, torch.float32, m0, v0, t0), ref, hypers, g0)[1]


@functools.lru_cache(maxsize=None)
def case_e_ref(name):
    """Final running maxima of ``e_ref`` for a case (small: kept for the whole session)."""
    p0, grads, h = case_inputs(name)
    return e_ref(p0, grads, h)[1][-1]


def check_against(got_steps, ref_steps, yard, hypers, what, g0=None):
    """Assert the bound FACTOR * yardstick (+ one ulp of p) after every step; returns the final running maxima of the errors."""
    per, run = run_errors(got_steps, ref_steps, hypers, g0)
    for t, (e, y) in enumerate(zip(per, yard)):
        assert e["p_excess"] <= FACTOR * y["p"], "%s step %d: p off by %.3e lr (+ulp), yardstick %.3e lr" % (what, t + 1, e["p_excess"], y["p"])
        assert e["v"] <= FACTOR * y["v"], "%s step %d: exp_avg_sq off by %.3e relative, yardstick %.3e" % (what, t + 1, e["v"], y["v"])
        assert e["m"] <= FACTOR * y["m"], "%s step %d: exp_avg off by %.3e of the gradient scale, yardstick %.3e" % (what, t + 1, e["m"], y["m"])
    return run[-1]


def report(what, err, yard):
    return "%-44s p %.2e lr (E_ref %.2e)  v %.2e (E_ref %.2e)  m %.2e (E_ref %.2e)" % (what, err["p"], yard["p"], err["v"], yard["v"], err["m"], yard["m"])


# ---- the first optimizer step of a trainer ------------------------------------------------------------------------------------------------
FIRST_STEP_SHARE = 0.75


def first_step_check(p0, p1, grad0, lr, eps, wd=0.0):
    """The first Adam step of a trainer, element by element: p1 - p0 against -lr * g / (|g| + eps) evaluated on a fixture's first gradients.
    p0, p1: {name: array} of EVERY trainable tensor before / after the step; grad0: the fixture's {name: array}.
    Compared wherever |g| >= 1e-3 * max |g| of its tensor and |g| >= 1e-6 -- a rounding-level difference between two evaluations of the
    gradient cannot flip the sign there; bound 0.02 lr + ulp(p).  At least FIRST_STEP_SHARE of every tensor's elements must be compared (asserted from
    the fixture), so a parameter that silently never trains fails.  Returns (smallest share, its tensor, largest error / lr)."""
    assert wd == 0.0, "the closed form holds without weight decay"
    assert set(p0) == set(p1) == set(grad0), sorted(set(p0) ^ set(grad0))
    low, worst = (2.0, ""), 0.0
    for k in sorted(p0):
        g = np.asarray(grad0[k], dtype=np.float64)
        a, b = np.asarray(p0[k], dtype=np.float64), np.asarray(p1[k], dtype=np.float64)
        assert g.shape == a.shape == b.shape, k
        keep = (np.abs(g) >= 1e-3 * np.abs(g).max()) & (np.abs(g) >= 1e-6)
        share = float(keep.mean())
        low = min(low, (share, k))
        assert share >= FIRST_STEP_SHARE, "%s: only %.3f of the fixture's gradient is large enough to be compared" % (k, share)
        err = np.abs((b - a) - (-lr * g / (np.abs(g) + eps)))
        bound = 0.02 * lr + np.maximum(ulp32(a), ulp32(b))
        bad = keep & (err > bound)
        assert not bad.any(), "%s: %d of %d compared elements off, the worst by %.3f lr (moved %.3e, expected %.3e)" % (
            k, int(bad.sum()), int(keep.sum()), float(err[keep].max() / lr), float((b - a).reshape(-1)[np.argmax(np.where(keep, err, 0))]),
            float((-lr * g / (np.abs(g) + eps)).reshape(-1)[np.argmax(np.where(keep, err, 0))]))
        worst = max(worst, float(err[keep].max() / lr))
    return low[0], low[1], worst
