"""-m gpu: the prologue and epilogue of conv_wgrad_wino_f32 (csrc/conv_wgrad_wino.hip) in its default form against the earlier one that
AESR_WGRAD_WINO_LEAN=0 keeps selectable, through aesr_conv2d_wgrad / aesr_conv2d_wgrad_up2 with forced plans (AESR_WGRAD_WINO_TILE,
AESR_WGRAD_WINO_S: read on every call, part of the plan-cache key).

The library reads AESR_WGRAD_WINO_LEAN once per process, so the other form runs in ONE child process (this file as a script) that computes
every case and leaves dw / db in a file; each test compares its own result with it bit for bit.  On every case, in both processes:
- dw and db between the guard bands of tests/memguard.py, as are x, dy and the slab workspace; outputs and workspace start as NaN poison:
  guards intact, inputs unchanged, no output element left unwritten;
- rel-L2 against the fp64 CPU conv2d weight gradient within WGRAD_BOUND, the bound of tests/test_gpu_kernels.py::test_conv_wgrad_wino.

Cases: workgroups with exactly 1, 2, 3 and 4 tile visits (one tile: both look-ahead tiles are past the end) and launches that mix k and
k + 1 visits; both tile shapes (8x16 has a wave that issues no X DMA); several (ci, co) chunks, where the bias gradient comes from the
ci chunk 0 alone; 128 -> 128 with one slab; odd sizes whose last tile rows and columns hang over the image; the folded Upsample(x2)."""
import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WGRAD_BOUND = 2e-5              # tests/test_gpu_kernels.py::test_conv_wgrad_wino: "dW, db against fp64 (sums over up to 50k pixels: 2e-5)"
TILES = ((16, 8), (8, 16))


def _cases():
    out = []
    for th, tw in TILES:
        t = "%dx%d" % (th, tw)
        for k in (1, 2, 3, 4):      # one slab, k tiles side by side: exactly k visits
            H, W = (16, 8 * k) if th == 16 else (8, 16 * k)
            out.append(("visits%d-%s" % (k, t), (1, H, W, 32, 32, 0), (th, tw), 1))
        out.append(("visits4443-%s" % t, (1, 40, 40, 32, 32, 0), (th, tw), 4))          # 15 tiles
        out.append(("visits332-%s" % t, (2, 32, 16, 32, 32, 0), (th, tw), 3))           # 8 tiles
        out.append(("chunks64to32-%s" % t, (1, 24, 24, 64, 32, 0), (th, tw), 2))
        out.append(("chunks32to64-%s" % t, (1, 24, 24, 32, 64, 0), (th, tw), 2))
        out.append(("128to128-S1-%s" % t, (1, 16, 16, 128, 128, 0), (th, tw), 1))
        out.append(("odd41-%s" % t, (1, 41, 41, 32, 32, 0), (th, tw), 0))                # S = 0: the planner's
        out.append(("odd81-%s" % t, (1, 81, 81, 32, 32, 0), (th, tw), 0))
        out.append(("up2-16-%s" % t, (1, 16, 16, 32, 32, 1), (th, tw), 1))
        out.append(("up2-40-%s" % t, (1, 40, 40, 64, 32, 1), (th, tw), 4))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _io(shape):
    """Seeded fp32 inputs in the device's layout (CPU) and the fp64 reference, made once per shape and left unchanged."""
    N, H, W, Cin, Cout, up2 = shape
    g = torch.Generator().manual_seed(7 + 1000 * Cin + 10 * H + W + up2)
    x = torch.randn((N, Cin, H // 2, W // 2) if up2 else (N, Cin, H, W), generator=g)
    dy = torch.randn(N, Cout, H, W, generator=g)
    xr = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up2 else x.double()
    ref_w = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, 3, 3), dy.double(), padding=1)
    ref_b = dy.double().sum((0, 2, 3))
    return x.permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous(), ref_w, ref_b


class _forced_plan:
    def __init__(self, tile, S):
        self.env = {"AESR_WGRAD_WINO_TILE": "%d,%d" % tile, "AESR_WGRAD_WINO_S": str(S) if S else None}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(hip, case, calls=1):
    """The guarded call(s) of one case: (dw, db) on the CPU, one pair per call; every assertion that needs no second process."""
    import memguard as mg
    name, shape, tile, S = case
    N, H, W, Cin, Cout, up2 = shape
    L = hip.lib
    x, dy, ref_w, ref_b = _io(shape)
    with _forced_plan(tile, S):
        nws = L.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, 3, 1)
        assert nws > 0 and nws % (10 * Cin * Cout) == 0
        if S:
            assert nws == S * 10 * Cin * Cout, "the forced slab count was not honoured"
        ins = {"x": mg.guarded(x.numel(), torch.float32, "cuda", x.reshape(-1), 0, "x"),
               "dy": mg.guarded(dy.numel(), torch.float32, "cuda", dy.reshape(-1), 0, "dy")}
        outs = {"dw": mg.guarded(Cout * Cin * 9, torch.float32, "cuda", mg.POISON_NAN, 0, "dw"),
                "db": mg.guarded(Cout, torch.float32, "cuda", mg.POISON_NAN, 0, "db"),
                "workspace": mg.guarded(nws, torch.float32, "cuda", mg.POISON_NAN, 0, "workspace")}
        saved = {k: mg.bits(g.view) for k, g in ins.items()}
        p = lambda g: ctypes.c_void_p(g.view.data_ptr())            # noqa: E731
        results = []
        for _ in range(calls):
            torch.cuda.synchronize()
            if up2:
                rc = L.aesr_conv2d_wgrad_up2(p(ins["x"]), p(ins["dy"]), p(outs["dw"]), p(outs["db"]), p(outs["workspace"]), N, H, W, Cin, Cout, hip.stream())
            else:
                rc = L.aesr_conv2d_wgrad(p(ins["x"]), p(ins["dy"]), p(outs["dw"]), p(outs["db"]), p(outs["workspace"]), N, H, W, Cin, Cout, 3, 1,
                                         hip.stream())
            assert rc == 0, (name, hip.last_error())
            torch.cuda.synchronize()
            mg.assert_guards_intact(list(ins.values()) + list(outs.values()))
            for k, g in ins.items():
                mg.assert_unchanged(g.view, saved[k], k)
            for k in ("dw", "db"):
                left = mg.poison_left(outs[k].view, mg.POISON_NAN)
                assert left.numel() == 0, "%s %s: %d element(s) never written, first %d" % (name, k, left.numel(), int(left[0]))
            dw, db = outs["dw"].view.cpu().clone().reshape(Cout, Cin, 3, 3), outs["db"].view.cpu().clone()
            ew, eb = rel_l2(dw, ref_w), rel_l2(db, ref_b)
            print("%s: rel-L2 against fp64 dw %.3g db %.3g" % (name, ew, eb))
            assert ew < WGRAD_BOUND and eb < WGRAD_BOUND, (name, ew, eb)
            results.append((dw, db))
    return results


@pytest.fixture(scope="module")
def hip():
    from superresolution_aniso_mri_amd import _hip
    assert torch.cuda.is_available()
    return _hip


@pytest.fixture(scope="module")
def other_form(tmp_path_factory):
    """dw / db of every case from a process that runs the AESR_WGRAD_WINO_LEAN=0 instantiation (it makes the same assertions there)."""
    out = str(tmp_path_factory.mktemp("wgrad_lean") / "lean0.pt")
    env = dict(os.environ, AESR_WGRAD_WINO_LEAN="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "the AESR_WGRAD_WINO_LEAN=0 process failed:\n" + r.stdout[-3000:] + r.stderr[-3000:]
    return torch.load(out)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_default_form_equals_lean0_bitwise(hip, other_form, case):
    (dw, db), = run_case(hip, case)
    dw0, db0 = other_form[case[0]]
    assert torch.equal(dw.view(torch.int32), dw0.view(torch.int32)), "dw differs from AESR_WGRAD_WINO_LEAN=0 in %d element(s)" % int((dw != dw0).sum())
    assert torch.equal(db.view(torch.int32), db0.view(torch.int32)), "db differs from AESR_WGRAD_WINO_LEAN=0 in %d element(s)" % int((db != db0).sum())


@pytest.mark.parametrize("tile", TILES, ids=["16x8", "8x16"])
def test_twice_on_the_same_buffers(hip, tile):
    """The slab workspace (and every other buffer) is reused by the second call: identical results."""
    (dw1, db1), (dw2, db2) = run_case(hip, ("twice-%dx%d" % tile, (2, 32, 16, 64, 32, 0), tile, 3), calls=2)
    assert torch.equal(dw1.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db1.view(torch.int32), db2.view(torch.int32))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from superresolution_aniso_mri_amd import _hip as _lib
    torch.save({c[0]: run_case(_lib, c)[0] for c in CASES}, sys.argv[1])
