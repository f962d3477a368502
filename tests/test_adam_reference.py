"""not-gpu: the fp64 restatement of Adam that tests/test_gpu_adam.py measures the HIP kernel with (tests/adam_util.py), pinned against
``torch.optim.Adam`` in float64 on every case, and the yardstick E_ref of every case: the error of torch's own fp32 CPU Adam against the
restatement on identical inputs.  The GPU test computes the same E_ref at run time; this file prints it (-s) and checks that it is a usable
yardstick (finite, and of the size fp32 roundings explain)."""
import numpy as np
import pytest
import torch

import adam_util as au


def _rel(a, b, scale):
    ok = scale > 0
    assert np.array_equal(a[~ok], b[~ok])
    return float((np.abs(a[ok] - b[ok]) / scale[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("name", au.CASE_IDS)
def test_restatement_is_torch_float64_adam(name):
    """1e-14 relative at every step of every case, each step taken from torch's own previous state, so that the figure is the step's and not
    the trajectory's: p against |p| + lr, exp_avg against the largest |g + wd * p| the element has seen (it cancels), exp_avg_sq against itself.
    Not bitwise: ATen's vectorised lerp_ / addcmul_ contract to fused multiply-adds, and lerp switches to ``end - (end - start) * (1 - w)``
    at w >= 0.5 -- a double-precision ulp either way (measured <= 4.6e-16; 9.2e-15 on the one element whose gradient all but cancels against wd * p).
    The two whole trajectories are compared as well, p against the largest |p| the element has had, exp_avg_sq against its largest value:
    measured <= 9.2e-15 but for beta1 = 0 with weight decay, 2.2e-14, where an element without a gradient of its own is driven through 0 in steps
    of lr and every step multiplies its relative error (x 3 per step seen) -- the conditioning of that trajectory, in any precision.  Held to
    1e-12: five orders below the fp32 errors the restatement measures."""
    p0, grads, h = au.case_inputs(name)
    ref = au.adam64(p0, grads, h)
    got = au.torch_adam(p0, grads, h, torch.float64)
    sc, local, whole, pmax, vmax = au.Scale(len(p0)), 0.0, 0.0, np.abs(p0).astype(np.float64), np.zeros(len(p0))
    prev = (p0.astype(np.float64), np.zeros(len(p0)), np.zeros(len(p0)))
    for t, ((p, m, v), (p64, m64, v64, geff)) in enumerate(zip(got, ref)):
        gmax, pmax, vmax = sc.advance(geff), np.maximum(pmax, np.abs(p64)), np.maximum(vmax, v64)
        whole = max(whole, _rel(p, p64, pmax), _rel(m, m64, gmax), _rel(v, v64, vmax))
        p1, m1, v1, _ = au.adam64(prev[0], grads[t:t + 1], h, prev[1], prev[2], t0=t)[0]
        local = max(local, _rel(p, p1, np.abs(p1) + h["lr"]), _rel(m, m1, gmax), _rel(v, v1, v1))
        prev = (p, m, v)
    print("%-44s restatement vs torch float64: step %.2e  trajectory %.2e" % (name, local, whole))
    assert local <= 1e-14 and whole <= 1e-12


def test_restatement_with_a_schedule_and_from_a_later_step():
    """Per-step hyper-parameters (lr, betas, eps and wd all change) and a start at step 99 999 with given moments."""
    gen = torch.Generator().manual_seed(5)
    n = 257
    p0 = (0.05 * torch.randn(n, generator=gen, dtype=torch.float64)).float().numpy()
    grads = au.gradients("unit", n, 6, gen)
    hypers = [au.hyper(1e-3 * (1 + k), (0.9 - 0.1 * (k // 3), 0.999 - 0.01 * (k // 2)), 10.0 ** (-8 + k), 0.01 * (k % 2)) for k in range(6)]
    m0, v0 = 0.1 * np.random.RandomState(0).randn(n), 0.5 + np.random.RandomState(1).rand(n)
    for t0, m, v in ((0, None, None), (99999, m0, v0)):
        ref = au.adam64(p0, grads, hypers, m, v, t0)
        got = au.torch_adam(p0, grads, hypers, torch.float64, m, v, t0)
        for (p, mm, vv), r in zip(got, ref):
            np.testing.assert_allclose(p, r[0], rtol=1e-14, atol=1e-17)
            np.testing.assert_allclose(mm, r[1], rtol=0, atol=1e-14)
            np.testing.assert_allclose(vv, r[2], rtol=1e-14)


@pytest.mark.parametrize("name", au.CASE_IDS)
def test_e_ref(name):
    """Prints E_ref.  A yardstick must be finite; torch's fp32 Adam owes a handful of roundings per element per step, so after T steps
    p is within (T + 1) * 2^-20 lr + T ulp(p) (every step rounds m / denom, the product and the sum: ~3 * 2^-24 of a step of <= ~3 lr, and p
    once) and, without weight decay, exp_avg_sq within (T + 2) * 2^-22 and exp_avg within (T + 2) * 2^-22 of the gradient scale -- loose ceilings that only catch a
    yardstick gone wrong, e.g. a restatement that drifted from torch."""
    p0, grads, h = au.case_inputs(name)
    ref, yard = au.e_ref(p0, grads, h)
    y, T = yard[-1], len(grads)
    print("E_ref " + name.ljust(44) + " p %.3e lr   v %.3e   m %.3e" % (y["p"], y["v"], y["m"]))
    assert y == au.case_e_ref(name)
    assert all(np.isfinite(list(e.values())).all() for e in yard)
    assert all(a[k] <= b[k] for a, b in zip(yard, yard[1:]) for k in a)            # running maxima
    ulp_p = float(au.ulp32(np.abs(np.stack([r[0] for r in ref])).max())) / h["lr"]
    assert y["p"] <= (T + 1) * 2.0 ** -20 + T * ulp_p
    if h["wd"] == 0.0:         # (with weight decay the gradient is g + wd * p: where that is small, p's absolute error shows in v and m)
        assert y["v"] <= (T + 2) * 2.0 ** -22 and y["m"] <= (T + 2) * 2.0 ** -22


def test_error_measures_see_what_they_should():
    """The measures on planted errors: a wrong eps placement, a bias correction one step off and a non-zero exp_avg where no gradient ever was."""
    p0, grads, h = au.case_inputs("eps-3-wd0")
    ref, yard = au.e_ref(p0, grads, h)
    f32 = au.torch_adam(p0, grads, h, torch.float32)
    assert au.check_against(f32, ref, yard, h, "torch fp32")["p"] == yard[-1]["p"]
    off = au.adam64(p0, grads, h, t0=1)
    with pytest.raises(AssertionError, match="p off"):
        au.check_against([tuple(a.astype(np.float32) for a in s[:3]) for s in off], ref, yard, h, "t off by one")
    bad = [(p, m.copy(), v) for p, m, v in f32]
    bad[1][1][0] = 1e-30
    with pytest.raises(AssertionError, match="exp_avg off by inf"):
        au.check_against(bad, ref, yard, h, "planted exp_avg")


def test_first_step_check_on_planted_steps():
    """``first_step_check`` passes the exact first step in fp32 and fails a tensor that never trains, a step of the wrong size and a missing tensor."""
    rs = np.random.RandomState(3)
    g = {"a.weight": rs.randn(8, 4, 3, 3) * 1e-2, "a.bias": rs.randn(8) * 1e-4}
    g["a.weight"].reshape(-1)[::9] *= 1e-5                                             # a ninth of it below the comparison threshold
    p0 = {k: (0.05 * rs.randn(*v.shape)).astype(np.float32) for k, v in g.items()}
    lr, eps = 1e-3, 1e-8
    p1 = {k: (p0[k].astype(np.float64) - lr * g[k] / (np.abs(g[k]) + eps)).astype(np.float32) for k in g}
    share, where, worst = au.first_step_check(p0, p1, g, lr, eps)
    assert where == "a.weight" and 0.85 < share < 0.9 and worst < 1e-4
    with pytest.raises(AssertionError, match="a.bias"):
        au.first_step_check(p0, dict(p1, **{"a.bias": p0["a.bias"]}), g, lr, eps)
    with pytest.raises(AssertionError, match="off, the worst by 0.03"):
        au.first_step_check(p0, {k: (p0[k] + 0.97 * (p1[k] - p0[k])).astype(np.float32) for k in g}, g, lr, eps)
    with pytest.raises(AssertionError):
        au.first_step_check({"a.bias": p0["a.bias"]}, {"a.bias": p1["a.bias"]}, g, lr, eps)
    with pytest.raises(AssertionError, match="large enough"):
        au.first_step_check(p0, p1, dict(g, **{"a.bias": g["a.bias"] * np.where(np.arange(8) < 3, 1e-4, 1.0)}), lr, eps)
