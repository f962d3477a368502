"""-m gpu: the Adam step -- ``adam_step_kernel`` through the C ABI (aesr_adam_step / aesr_adam_state_init) and ``ops.HipAdam`` as a
``torch.optim.Adam`` -- against the fp64 restatement of tests/adam_util.py, which tests/test_adam_reference.py pins to torch's float64 Adam.

Bounds (adam_util): after every step p, exp_avg and exp_avg_sq are within 4 x E_ref of the restatement (p: plus one fp32 ulp of p), E_ref being
the error of torch's own fp32 CPU Adam on identical inputs, computed here at run time.  Bitwise where the arithmetic leaves no freedom: an element
with g = m = v = 0 and no weight decay keeps p, m and v; the ``zero_grad`` flag leaves g untouched / exactly 0; 1000 launches back to back leave the
32 bytes of device state that ``aesr_adam_state_init(1000)`` writes; a run resumed from ``state_init`` and a HipAdam reloaded from its own
``state_dict`` continue as the one that was never stopped.

Out of scope: gradients whose square leaves the fp32 range (|g| > ~1.8e19).  There the kernel's ((1 - b2) * g) * g and ATen's addcmul_ need
not associate alike and overflow at different |g|; the largest gradients used are 1e15 * randn.

Kernel cases: n = 4099 (no multiple of 4 or 256, one partial grid) for arithmetic, n = 70 001 (every workgroup of the capped grid strides, with a
tail) for the state and the ticket counter.  HipAdam cases: four parameters of unequal shapes, both AESR_LAZY_ZERO settings, gradients that are
exact in fp32 (a loss linear in the parameters), so the restatement sees the very gradients the optimizer saw.
Measured figures and the mutants these tests were run against: profiles/adam_parity.txt."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import adam_util as au

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from superresolution_aniso_mri_amd import _hip
    assert torch.cuda.is_available()
    return _hip


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def host_state(hip, t, betas):
    """The 8 words ``aesr_adam_state_init`` writes for an optimizer that has taken ``t`` steps."""
    host = (ctypes.c_float * 8)()
    hip.lib.aesr_adam_state_init(host, float(t), float(betas[0]), float(betas[1]))
    return np.frombuffer(host, dtype=np.int32).copy()


def dev_state(hip, t, betas):
    return torch.from_numpy(host_state(hip, t, betas)).cuda().view(torch.float32)


def run_kernel(hip, p0, grads, hypers, m0=None, v0=None, t0=0, flags=None, state=None):
    """``len(grads)`` launches of aesr_adam_step, none synchronised.  Returns ([(p, m, v)] after every launch, g buffers after every launch,
    the 8 state words at the end)."""
    if isinstance(hypers, dict):
        hypers = [hypers] * len(grads)
    n, T = len(p0), len(grads)
    p = torch.from_numpy(np.asarray(p0, dtype=np.float32)).cuda()
    m = torch.zeros(n, device="cuda") if m0 is None else torch.from_numpy(np.asarray(m0, dtype=np.float32)).cuda()
    v = torch.zeros(n, device="cuda") if v0 is None else torch.from_numpy(np.asarray(v0, dtype=np.float32)).cuda()
    g = torch.from_numpy(np.stack(grads)).cuda()
    state = dev_state(hip, t0, hypers[0]["betas"]) if state is None else state
    out = torch.empty(T, 3, n, device="cuda")
    for k, h in enumerate(hypers):
        hip.check(hip.lib.aesr_adam_step(hip.ptr(p), hip.ptr(g[k]), hip.ptr(m), hip.ptr(v), hip.ptr(state), n, h["lr"], h["betas"][0], h["betas"][1],
                                         h["eps"], h["wd"], 0 if flags is None else flags[k], hip.stream()), "adam")
        out[k, 0], out[k, 1], out[k, 2] = p, m, v
    out = out.cpu().numpy()
    return [(out[k, 0], out[k, 1], out[k, 2]) for k in range(T)], g.cpu().numpy(), state.view(torch.int32).cpu().numpy()


# ---- 2. the kernel through the C ABI ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", au.CASE_IDS)
def test_kernel_vs_fp64(hip, name):
    p0, grads, h = au.case_inputs(name)
    ref, yard = au.e_ref(p0, grads, h)
    got, g_after, state = run_kernel(hip, p0, grads, h)
    per, run = au.run_errors(got, ref, h)
    print(au.report("kernel " + name, run[-1], yard[-1]) + "  p beyond its ulp %.2e lr" % max(run[-1]["p_excess"], 0.0))
    au.check_against(got, ref, yard, h, name)
    assert np.array_equal(bits(g_after), bits(np.stack(grads)))                   # zero_grad = 0: the gradients are read only
    assert np.array_equal(state, host_state(hip, len(grads), h["betas"]))
    if h["wd"] == 0.0:
        # g = 0 in every step, m = v = 0: nothing may move, bit for bit (denom = eps, m / denom = 0)
        for p, m, v in got:
            assert np.array_equal(bits(p[::7]), bits(p0[::7])) and not bits(m[::7]).any() and not bits(v[::7]).any()


def test_zero_grad_flag(hip):
    """0 leaves g bitwise untouched, 1 leaves exact zeros (+0), alternating over 6 steps; the step itself does not depend on the flag."""
    gen = torch.Generator().manual_seed(77)
    p0 = (0.05 * torch.randn(au.N_ARITH, generator=gen, dtype=torch.float64)).float().numpy()
    grads = au.gradients("unit", au.N_ARITH, 6, gen)
    h = au.hyper(wd=0.01)
    flags = [0, 1, 0, 1, 1, 0]
    got, g_after, _ = run_kernel(hip, p0, grads, h, flags=flags)
    plain, _, _ = run_kernel(hip, p0, grads, h)
    for k, f in enumerate(flags):
        if f:
            assert not bits(g_after[k]).any(), k
        else:
            assert np.array_equal(bits(g_after[k]), bits(grads[k])), k
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[k], plain[k])), k
    ref, yard = au.e_ref(p0, grads, h)
    au.check_against(got, ref, yard, h, "zero_grad flag")


def _ulps32(x, want):
    want32 = np.float32(want)
    return abs(float(np.float32(x)) - want) / float(np.spacing(want32))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("t", [0, 1, 9, 999, 99999])
def test_state_init(hip, t, betas):
    s = host_state(hip, t, betas)
    f, d = s.view(np.float32), s.view(np.float64)
    assert float(f[0]) == float(t) and s[3] == 0
    assert _ulps32(f[1], 1.0 - betas[0] ** (t + 1)) <= 1.0 and _ulps32(f[2], (1.0 - betas[1] ** (t + 1)) ** 0.5) <= 1.0
    for got, b in zip(d[2:4], betas):
        assert abs(got - b ** (t + 1)) <= 1e-10 * b ** (t + 1), (got, b ** (t + 1))


def test_1000_launches_back_to_back(hip):
    """The ticket counter and the state advance 1000 times with nothing between the launches: every one of the 32 bytes equals
    ``state_init(1000)`` -- the same chain of double multiplications -- and the counter is back at 0."""
    gen = torch.Generator().manual_seed(78)
    n, h = au.N_STATE, au.hyper()
    p0, g = 0.05 * torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    p, g = p0.cuda(), g.cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = dev_state(hip, 0, h["betas"])
    for _ in range(1000):
        hip.check(hip.lib.aesr_adam_step(hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(state), n, h["lr"], h["betas"][0], h["betas"][1],
                                         h["eps"], h["wd"], 0, hip.stream()), "adam")
    got = state.view(torch.int32).cpu().numpy()
    assert got[3] == 0
    assert np.array_equal(got, host_state(hip, 1000, h["betas"])), (got, host_state(hip, 1000, h["betas"]))
    # a constant gradient: m = (1 - b1^t) g and v = (1 - b2^t) g^2, so EVERY step moves an element by lr * g / (|g| + eps).  1000 roundings of a
    # p below 1.3 (<= 6e-8 each) and 1000 steps good to 1e-6 lr: 1e-4 -- a tenth of the one step a dropped launch or element would be short of
    want = p0.double() - 1000 * h["lr"] * g.double().cpu() / (g.double().cpu().abs() + h["eps"])
    assert float((p.double().cpu() - want).abs().max()) <= 1e-4


def test_step_100000(hip):
    """One step from ``state_init(99 999)`` with moments of a plausible size, against the restatement at t = 100 000 (beta2^t = 3.5e-44:
    the bias corrections have long been 1, which a power kept in fp32 or a step count off by a few would not show -- the state does)."""
    gen = torch.Generator().manual_seed(79)
    n, h = au.N_STATE, au.hyper(wd=0.01)
    p0 = (0.05 * torch.randn(n, generator=gen, dtype=torch.float64)).float().numpy()
    m0 = (0.3 * torch.randn(n, generator=gen, dtype=torch.float64)).float().numpy()
    v0 = (0.2 + torch.rand(n, generator=gen, dtype=torch.float64)).float().numpy()
    grads = au.gradients("unit", n, 1, gen)
    ref, yard = au.e_ref(p0, grads, h, m0, v0, 99999, g0=np.abs(m0))
    got, _, state = run_kernel(hip, p0, grads, h, m0, v0, 99999)
    run = au.check_against(got, ref, yard, h, "t = 100000", g0=np.abs(m0))
    print(au.report("kernel t=100000", run, yard[-1]))
    assert np.array_equal(state, host_state(hip, 100000, h["betas"]))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
def test_resume_is_bitwise(hip, betas):
    """40 steps straight through = 25 steps, the state replaced by ``state_init(25)``, 15 more steps."""
    gen = torch.Generator().manual_seed(80)
    n, h = au.N_STATE, au.hyper(betas=betas, wd=0.01)
    p0 = (0.05 * torch.randn(n, generator=gen, dtype=torch.float64)).float().numpy()
    grads = au.gradients("unit", n, 40, gen)
    straight, _, s_straight = run_kernel(hip, p0, grads, h)
    first, _, s25 = run_kernel(hip, p0, grads[:25], h)
    assert np.array_equal(s25, host_state(hip, 25, betas))
    p25, m25, v25 = first[-1]
    rest, _, s_resumed = run_kernel(hip, p25, grads[25:], h, m25, v25, t0=25)
    for k, (a, b) in enumerate(zip(straight, first + rest)):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), k
    assert np.array_equal(s_straight, s_resumed)


# ---- 3. HipAdam as a torch.optim.Adam ---------------------------------------------------------------------------------------------------
SHAPES = ((3, 5, 3, 3), (7,), (1,), (64, 33))
NUMEL = sum(int(np.prod(s)) for s in SHAPES)


def _split(flat):
    out, off = [], 0
    for s in SHAPES:
        k = int(np.prod(s))
        out.append(flat[off:off + k].reshape(s))
        off += k
    return out


def _flat(arrays):
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays])


class Rig:
    """Four CUDA parameters under a HipAdam, seeded exact-in-fp32 gradient tables, and the record of every step taken."""

    def __init__(self, monkeypatch, lazy, h=None, seed=0, steps=8, p0=None):
        from superresolution_aniso_mri_amd import ops
        monkeypatch.setenv("AESR_LAZY_ZERO", lazy)
        self.h = au.hyper(wd=0.01) if h is None else h
        gen = torch.Generator().manual_seed(200 + seed)
        drawn = (0.05 * torch.randn(NUMEL, generator=gen, dtype=torch.float64)).float().numpy()
        self.p0 = drawn if p0 is None else np.asarray(p0, dtype=np.float32)          # (the gradient tables depend on the seed alone)
        self.params = [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in _split(self.p0)]
        self.opt = ops.HipAdam(self.params, lr=self.h["lr"], betas=self.h["betas"], eps=self.h["eps"], weight_decay=self.h["wd"])
        assert self.opt.lazy_zero == (lazy != "0")
        # two tables of gradients per step: [step][parameter]
        self.C = [[[torch.from_numpy(a.copy()).cuda() for a in _split(g)] for g in au.gradients("unit", NUMEL, steps, gen)] for _ in range(2)]
        self.got, self.grads, self.hypers = [], [], []

    def state(self):
        return tuple(t.detach().cpu().numpy().copy() for t in (self.opt.flat_p, self.opt.flat_m, self.opt.flat_v))

    def autograd(self, i, table, k):
        """The gradient table[k][i] reaches parameter i through stock autograd: a loss linear in the parameter, ordinary torch ops."""
        (self.params[i] * self.C[table][k][i]).sum().backward()

    def engine_write(self, i, table, k):
        """... the engine's way: the destination from the engine's ``SequentialRunner._grad_dst``, written directly; a temporary goes back to autograd, which adds it."""
        from superresolution_aniso_mri_amd.engine import SequentialRunner
        p, grads = self.params[i], {}
        dst = SequentialRunner._grad_dst(p, grads)
        dst.copy_(self.C[table][k][i])
        if grads[p] is not None:
            assert grads[p] is dst and dst.data_ptr() != p.grad.data_ptr()
            p.grad.add_(grads[p])
        return grads[p] is None

    def step(self, expected):
        """opt.step(); ``expected``: the gradient of every parameter as float32 arrays (None = exactly zero)."""
        g = self.opt.param_groups[0]
        self.hypers.append(au.hyper(g["lr"], g["betas"], g["eps"], g["weight_decay"]))
        self.opt.step()
        exp = [np.zeros(s, dtype=np.float32) if e is None else np.asarray(e, dtype=np.float32) for e, s in zip(expected, SHAPES)]
        for i, (p, e) in enumerate(zip(self.params, exp)):
            assert p.grad.data_ptr() == self.opt.flat_g.data_ptr() + 4 * sum(int(np.prod(s)) for s in SHAPES[:i])
            assert np.array_equal(bits(p.grad), bits(e)), "parameter %d: the step did not see the gradient it was given" % i
        self.grads.append(_flat(exp))
        self.got.append(self.state())

    def check(self, what, start=None):
        """Every recorded step against the restatement AND against a stock float64 CPU torch.optim.Adam driven with the same gradients."""
        p0, m0, v0, t0 = (self.p0, None, None, 0) if start is None else start
        g0 = None if m0 is None else np.abs(m0)
        ref, yard = au.e_ref(p0, self.grads, self.hypers, m0, v0, t0, g0=g0)
        run = au.check_against(self.got, ref, yard, self.hypers, what, g0=g0)
        stock = au.torch_adam(p0, self.grads, self.hypers, torch.float64, m0, v0, t0)
        au.check_against(self.got, [s + (r[3],) for s, r in zip(stock, ref)], yard, self.hypers, what + " (stock float64)", g0=g0)
        print(au.report("HipAdam " + what, run, yard[-1]))


def _cpu(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hipadam_gradients_by_plain_autograd(monkeypatch, lazy):
    """zero_grad(); loss.backward(); step() with a loss of ordinary torch ops, five times, gradients different each time."""
    rig = Rig(monkeypatch, lazy)
    for k in range(5):
        rig.opt.zero_grad()
        sum((p * c).sum() for p, c in zip(rig.params, rig.C[0][k])).backward()
        for p, c in zip(rig.params, rig.C[0][k]):
            assert np.array_equal(bits(p.grad), bits(c)), "step %d: autograd added onto what zero_grad() had declared zero" % k
        rig.step([_cpu(c) for c in rig.C[0][k]])
    rig.check("plain autograd lazy=" + lazy)


@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hipadam_mixed_provenance(monkeypatch, lazy):
    """In one step: a parameter written the engine's way, one accumulated by autograd, one differentiated twice (direct write then autograd's +=
    on even steps, autograd first and the engine second on odd ones), one not reached at all (exactly zero).  Roles rotate over 4 steps."""
    rig = Rig(monkeypatch, lazy)
    for k in range(4):
        rig.opt.zero_grad()
        expected = [None] * 4
        for i in range(4):
            role = (i + k) % 4
            c0, c1 = rig.C[0][k][i], rig.C[1][k][i]
            if role == 0:
                assert rig.engine_write(i, 0, k), "a freshly zeroed gradient must be written in place"
                expected[i] = _cpu(c0)
            elif role == 1:
                rig.autograd(i, 0, k)
                expected[i] = _cpu(c0)
            elif role == 2:
                if k % 2 == 0:
                    assert rig.engine_write(i, 0, k)
                    rig.autograd(i, 1, k)
                else:
                    rig.autograd(i, 1, k)
                    assert not rig.engine_write(i, 0, k), "a direct write would drop what autograd has added"
                expected[i] = _cpu(c0 + c1)
        rig.step(expected)
    rig.check("mixed provenance lazy=" + lazy)


@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hipadam_gradient_tensors_replaced(monkeypatch, lazy):
    """``p.grad = tensor`` / ``p.grad = None`` between zero_grad() and step() act as the given values / as zeros; afterwards p.grad is the view of
    flat_g again (Rig.step asserts it); zero_grad(set_to_none=True) keeps the views."""
    rig = Rig(monkeypatch, lazy)
    views = [p.grad.data_ptr() for p in rig.params]
    for k in range(3):
        rig.opt.zero_grad(set_to_none=True)
        assert [p.grad.data_ptr() if p.grad is not None else None for p in rig.params] == views
        rig.autograd(0, 0, k)
        rig.autograd(3, 0, k)
        rig.params[1].grad = rig.C[1][k][1].clone()
        rig.params[2].grad = None
        if k == 2:                      # and one whose replaced tensor is then accumulated onto by autograd
            rig.params[3].grad = rig.C[1][k][3].clone()
            rig.autograd(3, 0, k)
        e3 = _cpu(rig.C[0][k][3]) if k < 2 else _cpu(rig.C[1][k][3] + rig.C[0][k][3])
        rig.step([_cpu(rig.C[0][k][0]), _cpu(rig.C[1][k][1]), None, e3])
    rig.check("gradient tensors replaced lazy=" + lazy)


@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hipadam_schedules(monkeypatch, lazy):
    """CosineAnnealingLR(opt, 6) over 6 steps on HipAdam and on a stock optimizer; betas assigned between steps 3 and 4 (the next step uses
    beta_new ** t, as torch does); weight decay changed between steps."""
    rig = Rig(monkeypatch, lazy, au.hyper(lr=2e-3, wd=0.0))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(rig.opt, 6)
    twin = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=2e-3)
    twin_sched = torch.optim.lr_scheduler.CosineAnnealingLR(twin, 6)
    for k in range(6):
        if k == 2:
            rig.opt.param_groups[0]["weight_decay"] = 0.01
        if k == 3:
            rig.opt.param_groups[0]["betas"] = (0.8, 0.99)
        if k == 5:
            rig.opt.param_groups[0]["weight_decay"] = 0.0
        assert rig.opt.param_groups[0]["lr"] == twin.param_groups[0]["lr"]
        rig.opt.zero_grad()
        sum((p * c).sum() for p, c in zip(rig.params, rig.C[0][k])).backward()
        rig.step([_cpu(c) for c in rig.C[0][k]])
        sched.step()
        twin.step()
        twin_sched.step()
    assert [h["betas"] for h in rig.hypers] == [(0.9, 0.999)] * 3 + [(0.8, 0.99)] * 3
    assert len({h["lr"] for h in rig.hypers}) == 6 and [h["wd"] for h in rig.hypers] == [0.0, 0.0, 0.01, 0.01, 0.01, 0.0]
    rig.check("schedules lazy=" + lazy)


def _run(rig, first, count):
    for k in range(first, first + count):
        rig.opt.zero_grad()
        sum((p * c).sum() for p, c in zip(rig.params, rig.C[0][k])).backward()
        rig.step([_cpu(c) for c in rig.C[0][k]])


@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hipadam_checkpoint_into_stock_adam(monkeypatch, lazy):
    """After 5 steps HipAdam's state_dict loads into a stock Adam (step == 5, the moments of this step); both continue for 3 steps."""
    rig = Rig(monkeypatch, lazy)
    _run(rig, 0, 5)
    sd = copy.deepcopy(rig.opt.state_dict())
    assert [float(s["step"]) for s in sd["state"].values()] == [5.0] * 4
    p5, m5, v5 = rig.state()
    cpu_params = [torch.nn.Parameter(torch.from_numpy(a.copy()).double()) for a in _split(p5)]
    stock = torch.optim.Adam(cpu_params, lr=1.0, foreach=False)
    stock.load_state_dict(sd)
    assert stock.param_groups[0]["lr"] == rig.h["lr"] and stock.param_groups[0]["weight_decay"] == rig.h["wd"]
    assert np.array_equal(_flat([_cpu(stock.state[p]["exp_avg"]) for p in cpu_params]), m5.astype(np.float64))
    assert np.array_equal(_flat([_cpu(stock.state[p]["exp_avg_sq"]) for p in cpu_params]), v5.astype(np.float64))
    rig.got, rig.grads, rig.hypers = [], [], []
    _run(rig, 5, 3)
    stock_steps = []
    for k in range(5, 8):
        for p, c in zip(cpu_params, rig.C[0][k]):
            p.grad = c.cpu().double()
        stock.step()
        stock_steps.append((_flat([_cpu(p) for p in cpu_params]),) + tuple(_flat([_cpu(stock.state[p][key]) for p in cpu_params]) for key in ("exp_avg", "exp_avg_sq")))
    assert [float(stock.state[p]["step"]) for p in cpu_params] == [8.0] * 4
    ref, yard = au.e_ref(p5, rig.grads, rig.hypers, m5, v5, 5, g0=np.abs(m5))
    au.check_against(rig.got, [s + (r[3],) for s, r in zip(stock_steps, ref)], yard, rig.hypers, "the stock Adam that loaded the checkpoint", g0=np.abs(m5))
    rig.check("continued beside a stock Adam lazy=" + lazy, start=(p5, m5, v5, 5))


@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hipadam_loads_a_stock_checkpoint(monkeypatch, lazy):
    """A stock fp32 Adam's state_dict, saved at step 5 with moments of its own, loaded into a fresh HipAdam, which then continues."""
    h = au.hyper(wd=0.01)
    gen = torch.Generator().manual_seed(300)
    p0 = (0.05 * torch.randn(NUMEL, generator=gen, dtype=torch.float64)).float().numpy()
    early = au.gradients("unit", NUMEL, 5, gen)
    cpu_params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in _split(p0)]
    stock = torch.optim.Adam(cpu_params, lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["wd"], foreach=False)
    for g in early:
        for p, a in zip(cpu_params, _split(g)):
            p.grad = torch.from_numpy(a.copy())
        stock.step()
    sd = copy.deepcopy(stock.state_dict())
    p5 = _flat([_cpu(p) for p in cpu_params])
    m5, v5 = (_flat([_cpu(stock.state[p][key]) for p in cpu_params]) for key in ("exp_avg", "exp_avg_sq"))
    assert np.abs(m5).min() > 0 and v5.min() > 0
    rig = Rig(monkeypatch, lazy, h, p0=p5)
    rig.opt.load_state_dict(sd)
    assert np.array_equal(bits(rig.opt.flat_m), bits(m5)) and np.array_equal(bits(rig.opt.flat_v), bits(v5))
    assert float(rig.opt.state_dict()["state"][0]["step"]) == 5.0
    _run(rig, 0, 3)
    assert float(rig.opt.state_dict()["state"][3]["step"]) == 8.0
    rig.check("loaded from a stock Adam lazy=" + lazy, start=(p5, m5, v5, 5))


@pytest.mark.parametrize("lazy", ["1", "0"])
def test_hipadam_reloaded_continues_bitwise(monkeypatch, lazy):
    """Save, load into a new HipAdam, continue: bit for bit the HipAdam that was never stopped -- parameters, moments and the 32 bytes of
    device state -- and again after a second save."""
    h = au.hyper(betas=(0.8, 0.99), wd=0.01)
    a = Rig(monkeypatch, lazy, h, steps=11)
    first = 0
    for count in (5, 2):
        _run(a, first, count)
        first += count
        sd = copy.deepcopy(a.opt.state_dict())
        b = Rig(monkeypatch, lazy, h, steps=11, p0=a.state()[0])
        b.opt.load_state_dict(sd)
        assert a.opt.state[a.params[0]]["exp_avg"].data_ptr() == a.opt.flat_m.data_ptr()            # saving detached no view
        assert b.opt.state[b.params[0]]["exp_avg"].data_ptr() == b.opt.flat_m.data_ptr()
        a.got = []
        _run(a, first, 2)
        _run(b, first, 2)
        for k, (x, y) in enumerate(zip(a.got, b.got)):
            assert all(np.array_equal(bits(u), bits(w)) for u, w in zip(x, y)), (first, k)
        assert np.array_equal(_cpu(a.opt.dev_state.view(torch.int32)), _cpu(b.opt.dev_state.view(torch.int32)))
        first += 2
    assert first == 11 and float(a.opt.state_dict()["state"][0]["step"]) == 11.0
