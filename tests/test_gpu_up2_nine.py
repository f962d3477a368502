"""-m gpu: the nine-position Winograd forms of the two convolutions behind a nearest Upsample(x2) (csrc/conv_wino_res.hip and
csrc/conv_wgrad_wino.hip, NINE; AESR_WINO_UP2_NINE=0 keeps the 16-position instantiations selectable), through the C ABI.

A Winograd tile of an upsampled image has rows 1, 2 and columns 1, 2 of its 4 x 4 patch equal, so V = B^T d B is exactly +0 at the 7
positions 4 i + j with i == 2 or j == 2, and the 2x2-summing data gradient gives those positions weight 0.  What is checked:
- forward (aesr_conv2d_wino_fwd_up2) and weight gradient (aesr_conv2d_wgrad_up2): EQUAL AS BITS to the library's 16-position path on the
  explicitly upsampled tensor (aesr_conv2d_wino_fwd / aesr_conv2d_wgrad on repeat_interleave(x_half): the same shape, hence the same
  plan and kernel family), in this process;
- data gradient (aesr_conv2d_wino_dgrad_sum2): rel-L2 against fp64 autograd through F.interpolate(nearest) + conv2d on the CPU below
  DGRAD_BOUND per case, and over all cases the root-sum-square of those errors not above that of the 16-position form, which ONE child
  process (this file as a script, AESR_WINO_UP2_NINE=0: the library reads it once per process) computes on the same inputs;
- one BASELINE-size case (36 x 160 x 160, 32 -> 32) per direction, twice on the same buffers: bit-equal runs (the hand-ordered DMA waits
  of these kernels once raced at 36 images only), forward and weight gradient also bit-equal to the 16-position reference.
Outputs and workspaces start as NaN before every call."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DGRAD_BOUND = 1e-5              # tests/test_gpu_kernels.py::test_conv_wino_folded_upsample holds aesr_conv2d_wino_dgrad_sum2 to it
RES, RING = 2, 3                # aesr_conv2d_wino_kernel: resident filter / filter ring

# (N, H, W, Cin, Cout), H x W the convolution's (upsampled) size, and the kernel that serves the layer
FWD_CASES = [((1, 4, 4, 16, 32), RES),          # smaller than a block, one chunk
             ((2, 8, 8, 32, 32), RES),          # exactly one block, two chunks
             ((3, 12, 20, 32, 64), RES),        # ragged blocks on both axes, two cout tiles
             ((1, 40, 40, 64, 32), RES),        # 16-cout workgroups: three positions interleaved
             ((1, 16, 16, 128, 32), RING)]      # the ring kernel: all 16 positions, must still agree
# the same with the K side swapped: dy has Cout channels, so (1, 40, 40, 32, 64) is the 16-cout data gradient
DGRAD_CASES = [((N, H, W, Cout, Cin), k) for (N, H, W, Cin, Cout), k in FWD_CASES]
WGRAD_CASES = [(1, 4, 4, 32, 32),               # less than a tile
               (2, 16, 8, 32, 32),              # exactly one tile (16x8; two rows of the 8x16 grid, half filled)
               (3, 20, 12, 32, 64),             # ragged
               (1, 36, 24, 64, 32)]             # two ci blocks, several tiles per workgroup
TILES = ((16, 8), (8, 16))
BASELINE = (36, 160, 160, 32, 32)


def _id(shape):
    return "x".join(str(v) for v in shape)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _assert_bits(a, b, what):
    assert not torch.isnan(a).any(), "%s: element(s) never written" % what
    assert _bits_equal(a, b), "%s differs from the 16-position reference in %d element(s)" % (what, int((a.view(torch.int32) != b.view(torch.int32)).sum()))


def _up(xh):
    """[N, H/2, W/2, C] -> the nearest-upsampled [N, H, W, C] tensor, explicitly"""
    return xh.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()


def _pack(hip, w, transpose):
    cout, cin = w.shape[:2]
    buf = torch.empty(hip.lib.aesr_conv2d_wino_packed_floats(cout, cin, transpose), device="cuda")
    job = (hip.PackJob * 1)(hip.PackJob(w.data_ptr(), buf.data_ptr(), cout, cin, 3, transpose))
    hip.check(hip.lib.aesr_conv2d_wino_pack_many(job, 1, hip.stream()), "wino_pack")
    return buf


def _device_inputs(shape, seed):
    """x_half, filter, (non-zero) bias and dy of a case, generated on the device"""
    N, H, W, Cin, Cout = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    xh = torch.randn(N, H // 2, W // 2, Cin, device="cuda", generator=g)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / math.sqrt(Cin * 9)
    b = torch.randn(Cout, device="cuda", generator=g) + 0.25
    dy = torch.randn(N, H, W, Cout, device="cuda", generator=g)
    return xh, w, b, dy


class _forced_tile:
    def __init__(self, tile):
        self.value = "%d,%d" % tile

    def __enter__(self):
        self.saved = os.environ.get("AESR_WGRAD_WINO_TILE")
        os.environ["AESR_WGRAD_WINO_TILE"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("AESR_WGRAD_WINO_TILE", None)
        if self.saved is not None:
            os.environ["AESR_WGRAD_WINO_TILE"] = self.saved


@pytest.fixture(scope="module")
def hip():
    from superresolution_aniso_mri_amd import _hip
    assert torch.cuda.is_available()
    return _hip


# ---- forward ----------------------------------------------------------------------------------------------------------------
def _forward(hip, shape, act, calls=1):
    """out of aesr_conv2d_wino_fwd_up2 (one per call, same buffers) and of aesr_conv2d_wino_fwd on the upsampled input"""
    N, H, W, Cin, Cout = shape
    L = hip.lib
    xh, w, b, _ = _device_inputs(shape, 11 + H + Cin)
    up = _pack(hip, w, 0)
    out, outs = _nan(N, H, W, Cout), []
    for _ in range(calls):
        out.fill_(float("nan"))
        hip.check(L.aesr_conv2d_wino_fwd_up2(_p(xh), _p(up), _p(b), _p(out), N, H, W, Cin, Cout, act, 0.01, hip.stream()), "wino_fwd_up2")
        torch.cuda.synchronize()
        outs.append(out.clone())
    xu, ref = _up(xh), _nan(N, H, W, Cout)
    hip.check(L.aesr_conv2d_wino_fwd(_p(xu), _p(up), _p(b), _p(ref), N, H, W, Cin, Cout, act, 0.01, hip.stream()), "wino_fwd")
    torch.cuda.synchronize()
    assert not torch.isnan(ref).any()
    return outs, ref


@pytest.mark.parametrize("act", [0, 1], ids=["none", "lrelu"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[_id(c[0]) for c in FWD_CASES])
def test_forward_equals_16_positions_bitwise(hip, case, act):
    shape, kind = case
    N, H, W, Cin, Cout = shape
    assert hip.lib.aesr_conv2d_wino_kernel(N, H, W, Cin, Cout, 3, 1, 0) == kind
    (out,), ref = _forward(hip, shape, act)
    _assert_bits(out, ref, "out")


def test_forward_baseline_size_twice(hip):
    (o1, o2), ref = _forward(hip, BASELINE, 1, calls=2)
    assert _bits_equal(o1, o2), "two runs on the same buffers differ"
    _assert_bits(o1, ref, "out")


# ---- weight gradient --------------------------------------------------------------------------------------------------------
def _wgrad(hip, shape, tile, calls=1):
    """(dw, db) of aesr_conv2d_wgrad_up2 (one pair per call, same buffers) and of aesr_conv2d_wgrad on the upsampled input"""
    N, H, W, Cin, Cout = shape
    L = hip.lib
    xh, _, _, dy = _device_inputs(shape, 23 + H + Cin)
    with _forced_tile(tile):
        nws = L.aesr_conv2d_wgrad_workspace_floats(N, H, W, Cin, Cout, 3, 1)
        assert nws > 0
        dw, db, ws, res = _nan(Cout, Cin, 3, 3), _nan(Cout), _nan(nws), []
        for _ in range(calls):
            for t in (dw, db, ws):
                t.fill_(float("nan"))
            hip.check(L.aesr_conv2d_wgrad_up2(_p(xh), _p(dy), _p(dw), _p(db), _p(ws), N, H, W, Cin, Cout, hip.stream()), "wgrad_up2")
            torch.cuda.synchronize()
            res.append((dw.clone(), db.clone()))
        xu, rw, rb = _up(xh), _nan(Cout, Cin, 3, 3), _nan(Cout)
        ws.fill_(float("nan"))
        hip.check(L.aesr_conv2d_wgrad(_p(xu), _p(dy), _p(rw), _p(rb), _p(ws), N, H, W, Cin, Cout, 3, 1, hip.stream()), "wgrad")
        torch.cuda.synchronize()
    assert not torch.isnan(rw).any() and not torch.isnan(rb).any()
    return res, (rw, rb)


@pytest.mark.parametrize("tile", TILES, ids=["16x8", "8x16"])
@pytest.mark.parametrize("shape", WGRAD_CASES, ids=[_id(c) for c in WGRAD_CASES])
def test_wgrad_equals_16_positions_bitwise(hip, shape, tile):
    ((dw, db),), (rw, rb) = _wgrad(hip, shape, tile)
    _assert_bits(dw, rw, "dw")
    _assert_bits(db, rb, "db")


@pytest.mark.parametrize("tile", TILES, ids=["16x8", "8x16"])
def test_wgrad_twice_on_the_same_buffers(hip, tile):
    ((dw1, db1), (dw2, db2)), (rw, rb) = _wgrad(hip, (3, 20, 12, 32, 64), tile, calls=2)
    assert _bits_equal(dw1, dw2) and _bits_equal(db1, db2), "two runs on the same buffers differ"
    _assert_bits(dw2, rw, "dw")
    _assert_bits(db2, rb, "db")


@pytest.mark.parametrize("tile", TILES, ids=["16x8", "8x16"])
def test_wgrad_baseline_size_twice(hip, tile):
    ((dw1, db1), (dw2, db2)), (rw, rb) = _wgrad(hip, BASELINE, tile, calls=2)
    assert _bits_equal(dw1, dw2) and _bits_equal(db1, db2), "two runs on the same buffers differ"
    _assert_bits(dw1, rw, "dw")
    _assert_bits(db1, rb, "db")


# ---- data gradient ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dgrad_io(shape):
    """Seeded CPU inputs in the device's layout and the fp64 reference dx_half [N, H/2, W/2, Cin]; made once per shape, left unchanged."""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(5 + 100 * Cin + H + W)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    dy = torch.randn(N, Cout, H, W, generator=g)
    xh = torch.zeros(N, Cin, H // 2, W // 2, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.interpolate(xh, scale_factor=2, mode="nearest"), w.double(), None, padding=1).backward(dy.double())
    return w, dy.permute(0, 2, 3, 1).contiguous(), xh.grad.permute(0, 2, 3, 1).contiguous()


def _dgrad(lib_mod, shape, calls=1):
    N, H, W, Cin, Cout = shape
    w, dy, _ = _dgrad_io(shape)
    wd, dyd = w.cuda(), dy.cuda()
    upt = _pack(lib_mod, wd, 1)
    dx, res = _nan(N, H // 2, W // 2, Cin), []
    for _ in range(calls):
        dx.fill_(float("nan"))
        lib_mod.check(lib_mod.lib.aesr_conv2d_wino_dgrad_sum2(_p(dyd), _p(upt), _p(dx), N, H, W, Cin, Cout, lib_mod.stream()), "wino_dgrad_sum2")
        torch.cuda.synchronize()
        assert not torch.isnan(dx).any(), "dx_half: element(s) never written"
        res.append(dx.cpu())
    return res


def _rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def sixteen_position_dgrad(tmp_path_factory):
    """dx_half of every data-gradient case from a process that runs the AESR_WINO_UP2_NINE=0 instantiations"""
    out = str(tmp_path_factory.mktemp("up2_nine") / "nine0.pt")
    env = dict(os.environ, AESR_WINO_UP2_NINE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "the AESR_WINO_UP2_NINE=0 process failed:\n" + r.stdout[-3000:] + r.stderr[-3000:]
    return torch.load(out)


def test_dgrad_sum2_against_fp64_and_the_16_position_form(hip, sixteen_position_dgrad):
    """Per case rel-L2 against fp64 below DGRAD_BOUND; over all cases the root-sum-square of the errors is not above the 16-position
    form's (three terms that cancel in exact arithmetic only are gone)."""
    new, old = [], []
    print("rel-L2 of dx_half against fp64 autograd:  case (N,H,W,Cin,Cout)  kernel  nine positions  16 positions")
    for shape, kind in DGRAD_CASES:
        N, H, W, Cin, Cout = shape
        assert hip.lib.aesr_conv2d_wino_kernel(N, H, W, Cin, Cout, 3, 1, 1) == kind
        ref = _dgrad_io(shape)[2]
        (dx,) = _dgrad(hip, shape)
        e9, e16 = _rel_l2(dx, ref), _rel_l2(sixteen_position_dgrad[_id(shape)], ref)
        print("  %-18s %-5s %.4e %.4e" % (_id(shape), "res" if kind == RES else "ring", e9, e16))
        new.append(e9)
        old.append(e16)
    rss9, rss16 = math.sqrt(sum(e * e for e in new)), math.sqrt(sum(e * e for e in old))
    print("  %-18s %-5s %.4e %.4e" % ("root-sum-square", "", rss9, rss16))
    assert all(e < DGRAD_BOUND for e in new), new
    assert rss9 <= rss16, (rss9, rss16)


def test_dgrad_sum2_baseline_size_twice(hip):
    N, H, W, Cin, Cout = BASELINE
    _, w, _, dy = _device_inputs(BASELINE, 31)
    upt = _pack(hip, w, 1)
    dx, res = _nan(N, H // 2, W // 2, Cin), []
    for _ in range(2):
        dx.fill_(float("nan"))
        hip.check(hip.lib.aesr_conv2d_wino_dgrad_sum2(_p(dy), _p(upt), _p(dx), N, H, W, Cin, Cout, hip.stream()), "wino_dgrad_sum2")
        torch.cuda.synchronize()
        res.append(dx.clone())
    assert not torch.isnan(res[0]).any(), "dx_half: element(s) never written"
    assert _bits_equal(res[0], res[1]), "two runs on the same buffers differ"


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from superresolution_aniso_mri_amd import _hip as _lib
    torch.save({_id(shape): _dgrad(_lib, shape)[0] for shape, _ in DGRAD_CASES}, sys.argv[1])
