"""not gpu: the in-plane resampling step against the reference's own results (tests/golden/inplane.npz, written by
tests/make_golden_inplane.py from datasets/common.py:157-206 of the reference).

- A numpy restatement of the arithmetic, kept in this file (``restate``): scipy's separable Gaussian with the ``reflect`` boundary, each
  1-D pass in double and stored as float32, then the order-1 zoom with its coordinates in double and mode ``constant`` -- reproduces every
  fixture case within 1e-7 (6e-8 was measured for such a restatement against scipy, plus the rounding of the last store).  It shares no
  code with the package: the package's host tables are checked against it.
- The host tables (``datasets.common.zoom_tables``) predict the dead lines of the quirk cases and none elsewhere.
- Host-side argument checks of the C entry points, and the CLI's refusal of ``--resample`` on a ``.npy`` volume without ``--spacing``."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-7
QUIRK = {"d_quirk": (True, True), "d_quirk224": (True, True)}      # tag -> (last row dead, last column dead)


def fixture():
    fx = dict(np.load(os.path.join(HERE, "golden", "inplane.npz")))
    return fx, [str(t) for t in fx["tags"]]


def case_input(fx, tag):
    """float32 input of a case: images are stored as uint16 counts of 1/1024, labels as int64."""
    x = fx[tag + "/in"]
    return x.astype(np.float32) if bool(fx[tag + "/labels"]) else (x / 1024.0).astype(np.float32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _blur_axis(x, axis, sigma):
    """One pass of scipy.ndimage.gaussian_filter1d on float32 data: double accumulation in scipy's order, stored as float32."""
    r = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    w = w / w.sum()
    n = x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r, r)
    xp = np.pad(x.astype(np.float64), pad, mode="symmetric")          # d c b a | a b c d
    take = lambda s: np.take(xp, np.arange(s, s + n), axis=axis)      # noqa: E731
    acc = take(r) * w[r]
    for j in range(r, 0, -1):
        acc = acc + (take(r - j) + take(r + j)) * w[r + j]
    return acc.astype(np.float32)


def _axis_table(n, n_out):
    step = (n - 1) / (n_out - 1) if n_out > 1 else 1.0
    c = np.arange(n_out, dtype=np.float64) * np.float64(step)
    dead = c > n - 1
    i0 = np.floor(c).astype(np.int64)
    t = c - np.floor(c)
    i0[dead], t[dead] = 0, 0.0
    return i0, np.minimum(i0 + 1, n - 1), t, dead


def restate(x, spacing, new_spacing, do_blur=True, clamp_edges=False):
    """x float32 [..., H, W] -> float32 [..., Ho, Wo]"""
    zoom = np.array(list(spacing)[-2:], np.float64) / np.array(list(new_spacing)[-2:], np.float64)
    H, W = x.shape[-2:]
    if do_blur:
        x = _blur_axis(x, x.ndim - 2, 0.25 / zoom[0])
        x = _blur_axis(x, x.ndim - 1, 0.25 / zoom[1])
    Ho, Wo = int(round(H * zoom[0])), int(round(W * zoom[1]))
    y0, y1, ty, dy = _axis_table(H, Ho)
    x0, x1, tx, dx = _axis_table(W, Wo)
    if clamp_edges:
        y0[dy], y1[dy], x0[dx], x1[dx] = H - 1, H - 1, W - 1, W - 1
    xd = x.astype(np.float64)
    ty_, tx_ = ty[:, None], tx[None, :]
    out = (xd[..., y0[:, None], x0[None, :]] * (1 - ty_) * (1 - tx_) + xd[..., y0[:, None], x1[None, :]] * (1 - ty_) * tx_
           + xd[..., y1[:, None], x0[None, :]] * ty_ * (1 - tx_) + xd[..., y1[:, None], x1[None, :]] * ty_ * tx_)
    if not clamp_edges:
        out[..., dy, :] = 0.0
        out[..., :, dx] = 0.0
    return out.astype(np.float32)


def test_restatement_reproduces_the_reference():
    fx, tags = fixture()
    assert len(tags) == 16 and "a_full" in tags and "g_4d" in tags
    worst = 0.0
    for tag in tags:
        x, want = case_input(fx, tag), fx[tag + "/out"]
        got = restate(x, fx[tag + "/spacing"], fx[tag + "/new_spacing"], do_blur=bool(fx[tag + "/do_blur"]))
        assert got.shape == want.shape, (tag, got.shape, want.shape)
        if bool(fx[tag + "/labels"]):
            assert want.dtype == np.int64 and np.array_equal(np.round(got).astype(np.int64), want), tag
            continue
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print("%-18s %s max |restatement - reference| = %.3g" % (tag, want.shape, err))
        worst = max(worst, err)
        assert err <= TOL, (tag, err)


def test_fixture_is_what_the_issue_asked_for():
    fx, tags = fixture()
    assert fx["a_full/in"].shape == (1, 216, 256) and fx["a_full/out"].shape == (1, 241, 286)
    assert fx["d_quirk/out"].shape == (2, 42, 30) and fx["d_quirk224/out"].shape == (1, 224, 23)
    assert fx["g_4d/in"].shape == (3, 4, 40, 48) and fx["g_4d/out"].ndim == 4
    assert fx["e_tiny_identity/out"].shape == fx["e_tiny_identity/in"].shape == (2, 13, 9)
    assert os.path.getsize(os.path.join(HERE, "golden", "inplane.npz")) < 1 << 20
    for tag in tags:
        if not bool(fx[tag + "/labels"]):
            assert fx[tag + "/in"].dtype == np.uint16 and fx[tag + "/in"].max() <= 1024 and fx[tag + "/out"].dtype == np.float32


def test_host_tables_predict_the_dead_lines():
    from superresolution_aniso_mri_amd.datasets import common as dc
    fx, tags = fixture()
    for tag in tags:
        want = fx[tag + "/out"]
        H, W = fx[tag + "/in"].shape[-2:]
        zoom = dc.zoom_factors(fx[tag + "/spacing"], fx[tag + "/new_spacing"])
        Ho, Wo = dc.out_size(H, zoom[0]), dc.out_size(W, zoom[1])
        assert (Ho, Wo) == want.shape[-2:], tag
        row, col = QUIRK.get(tag, (False, False))
        assert dc.dead_lines(H, Ho).tolist() == ([Ho - 1] if row else []), tag
        assert dc.dead_lines(W, Wo).tolist() == ([Wo - 1] if col else []), tag
        if not bool(fx[tag + "/labels"]):
            flat = want.reshape((-1,) + want.shape[-2:])
            assert bool((flat[:, -1, :] == 0).all()) == row and bool((flat[:, :, -1] == 0).all()) == col, tag
        # the package's tables are the restatement's
        for n, n_out in ((H, Ho), (W, Wo)):
            i0, t = dc.zoom_tables(n, n_out)
            r0, _, rt, rdead = _axis_table(n, n_out)
            assert np.array_equal(i0 < 0, rdead) and np.array_equal(i0[~rdead], r0[~rdead]) and np.array_equal(t[~rdead], rt[~rdead])
            c0, ct = dc.zoom_tables(n, n_out, clamp_edges=True)
            assert np.array_equal(c0[~rdead], i0[~rdead]) and (c0[rdead] == n - 1).all() and (ct[rdead] == 0).all()
    # the examples of the module docstring
    for n, sp, n_out, dead in ((229, 1.37, 224, True), (243, 1.25, 217, True), (222, 0.7, 111, True), (216, 1.25, 193, False),
                               (256, 1.5625, 286, False), (224, 1.4, 224, False)):
        assert dc.out_size(n, sp / 1.4) == n_out and (dc.dead_lines(n, n_out).size == 1) == dead, (n, sp)


def test_gaussian_weights_are_scipys():
    scipy_filters = pytest.importorskip("scipy.ndimage._filters")
    from superresolution_aniso_mri_amd.datasets import common as dc
    for zoom in (1.5625 / 1.4, 1.4 / 1.5625, 0.5, 0.125, 2.5, 1.0, 1.37 / 1.4):
        sigma = 0.25 / zoom
        w, r = dc.gaussian_weights(sigma)
        assert r == int(4.0 * sigma + 0.5) and w.shape == (2 * r + 1,)
        assert np.array_equal(w, scipy_filters._gaussian_kernel1d(sigma, 0, r))


def test_out_size_is_pythons_round():
    from superresolution_aniso_mri_amd import _hip
    f = _hip.lib.aesr_inplane_out_size
    rs = np.random.RandomState(5)
    for n in list(range(1, 40)) + [216, 224, 229, 243, 256, 319]:
        for zoom in [0.5, 1.5, 2.5, 0.25, 0.75, 1.0] + list(rs.uniform(0.12, 3.0, 20)) + [s / 1.4 for s in (0.7, 1.25, 1.37, 1.5625, 1.68)]:
            want = int(round(n * float(zoom)))
            assert f(n, float(zoom)) == (want if want >= 1 else 0), (n, zoom)
    assert f(5, 0.5) == 2 and f(7, 0.5) == 4 and f(3, 0.5) == 2          # 2.5 -> 2, 3.5 -> 4, 1.5 -> 2: halves to even
    assert f(0, 1.0) == 0 and f(5, 0.0) == 0 and f(5, float("nan")) == 0 and f(5, float("inf")) == 0 and f(2 ** 30, 4.0) == 0
    assert _hip.lib.aesr_inplane_workspace_bytes(0, 5) == 0 and _hip.lib.aesr_inplane_workspace_bytes(241, 286) % 8 == 0


def test_entry_point_checks_its_arguments_on_the_host():
    """Argument and limit checks run before anything touches the device: callable without a GPU; nothing is dereferenced on the device."""
    from superresolution_aniso_mri_amd import _hip
    from superresolution_aniso_mri_amd.datasets import common as dc
    call = _hip.lib.aesr_inplane_resample
    D = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_hip.DP)       # noqa: E731
    I = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_hip.IP)         # noqa: E731, E741
    fake = ctypes.c_void_p(4096)                                                     # never dereferenced: every call below is refused first
    H, W, zoom = 20, 24, 0.5
    Ho, Wo = dc.out_size(H, zoom), dc.out_size(W, zoom)
    iy, ty = dc.zoom_tables(H, Ho)
    ix, tx = dc.zoom_tables(W, Wo)
    w, r = dc.gaussian_weights(0.25 / zoom)
    ok = [fake, fake, fake, 2, H, W, Ho, Wo, D(w), r, D(w), r, I(iy), D(ty), I(ix), D(tx), 1, None]

    def rc(**over):
        names = ["inp", "out", "ws", "N", "H", "W", "Ho", "Wo", "wy", "ry", "wx", "rx", "iy", "ty", "ix", "tx", "blur", "stream"]
        args = list(ok)
        for k, v in over.items():
            args[names.index(k)] = v
        return call(*args)

    assert rc(inp=None) == 1 and "null" in _hip.last_error()
    assert rc(N=0) == 1 and rc(Ho=0) == 1 and rc(wy=None) == 1
    assert rc(ws=ctypes.c_void_p(4100)) == 1 and "align" in _hip.last_error()
    # radius 9: zoom 0.11 -> sigma 2.27 -> int(9.59) = 9
    w9, r9 = dc.gaussian_weights(0.25 / 0.11)
    assert r9 == 9
    assert rc(wy=D(w9), ry=r9) == 3 and "8" in _hip.last_error() and "radius" in _hip.last_error()
    assert rc(wx=D(w9), rx=r9) == 3
    w_bad = w.copy()
    w_bad[0] *= 2
    assert rc(wy=D(w_bad)) == 1 and "symmetric" in _hip.last_error()
    bad = iy.copy()
    bad[3] = H                                  # past the last row
    assert rc(iy=I(bad)) == 1 and "row table" in _hip.last_error()
    bad = ix.copy()
    bad[0] = -1                                 # only the last line may be dead
    assert rc(ix=I(bad)) == 1 and "column table" in _hip.last_error()
    bad = ix.copy()
    bad[2], bad[3] = bad[3], bad[2] - 1         # decreasing
    assert rc(ix=I(bad)) == 1
    tb = tx.copy()
    tb[1] = 1.5
    assert rc(tx=D(tb)) == 1
    # a table whose taps are so far apart that even a one-row tile's footprint exceeds the LDS
    Hbig = 1 << 14
    far_y = np.array([0, Hbig - 2], np.int32)
    far_x = np.arange(0, Hbig, Hbig // 8, dtype=np.int32)
    assert call(fake, fake, fake, 1, Hbig, Hbig, 2, 8, None, 0, None, 0, I(far_y), D(np.zeros(2)), I(far_x), D(np.zeros(8)), 0, None) == 3
    assert "LDS" in _hip.last_error()


def test_python_interface_rejects_what_is_not_built():
    import torch
    from datasets.common import apply_2d_zoom_3d, apply_2d_zoom_4d
    from superresolution_aniso_mri_amd.datasets import common as dc
    assert apply_2d_zoom_3d is dc.apply_2d_zoom_3d and apply_2d_zoom_4d is dc.apply_2d_zoom_4d       # the root shim
    x = np.zeros((2, 8, 8), np.float32)
    with pytest.raises(NotImplementedError, match="order"):
        apply_2d_zoom_3d(x, (8, 1.5, 1.5), (1.4, 1.4), order=3)
    with pytest.raises(ValueError, match="3-D"):
        apply_2d_zoom_3d(x[0], (1.5, 1.5), (1.4, 1.4))
    with pytest.raises(ValueError, match="4-D"):
        apply_2d_zoom_4d(x, (1.5, 1.5), (1.4, 1.4))
    with pytest.raises(ValueError, match="zoom"):
        apply_2d_zoom_3d(x, (8, 0.0, 1.5), (1.4, 1.4))
    with pytest.raises(RuntimeError, match="GPU"):
        apply_2d_zoom_3d(torch.zeros(2, 8, 8), (1.5, 1.5), (1.4, 1.4))          # a CPU tensor: no fallback


def test_cli_refuses_resample_of_npy_without_spacing(tmp_path, capsys):
    from superresolution_aniso_mri_amd import generate_hr_volumes
    data = tmp_path / "vols"
    data.mkdir()
    np.save(str(data / "v.npy"), np.zeros((3, 8, 8), np.float32))
    with pytest.raises(SystemExit) as e:
        generate_hr_volumes.main(["--exper_dir=" + str(tmp_path / "none"), "--model_nbr=1", "--data_input_dir=" + str(data),
                                  "--output_dir=" + str(tmp_path / "out"), "--resample"])
    assert e.value.code != 0
    assert "--spacing" in capsys.readouterr().err
    assert not (tmp_path / "out").exists() or not list((tmp_path / "out").iterdir())
