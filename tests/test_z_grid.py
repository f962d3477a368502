"""The through-plane grid of a target slice spacing (evaluate/z_grid.py) and the command-line arguments around it: host code only.

The grid's rule is stated in that module; here it is held to the integer grid it generalises (the seven commensurate cases: J, gaps,
originals, and alphas that are ``np.linspace``'s once cast to fp32, the precision the kernels take them in), to three non-commensurate
tables worked out by hand, to its invariants, its snapping and every refusal."""
import numpy as np
import pytest

from superresolution_aniso_mri_amd.evaluate.z_grid import MAX_PER_GAP, target_grid

COMMENSURATE = [(10, 4), (8, 3), (9.6, 5), (10, 6), (5, 1), (7, 6), (10, 15)]
TABLES = [((5, 10, 1.4), 29, [8, 7, 7, 7]), ((4, 8, 1.25), 20, [7, 6, 7]), ((3, 10, 1.5625), 13, [7, 6])]


@pytest.mark.parametrize("s,n", COMMENSURATE)
def test_commensurate_spacing_is_the_integer_grid(s, n):
    Z = 5
    g = target_grid(Z, s, s / (n + 1))
    assert g.J == (Z - 1) * (n + 1) + 1 == len(g.gap) == len(g.alpha) == len(g.is_original)
    want = np.linspace(0, 1, n + 2)[1:-1].astype(np.float32)
    assert len(g.gap_alphas) == Z - 1
    for al in g.gap_alphas:
        assert np.array_equal(np.asarray(al, dtype=np.float64).astype(np.float32), want)
    j = np.arange(g.J)
    assert np.array_equal(g.is_original, j % (n + 1) == 0) and g.is_original[-1]
    assert np.array_equal(g.gap, np.minimum(j // (n + 1), Z - 2))
    assert np.array_equal(g.source[g.is_original], np.arange(Z)) and (g.source[~g.is_original] == -1).all()
    assert g.alpha[-1] == 1.0 and g.num_synthesised == (Z - 1) * n


@pytest.mark.parametrize("case,J,per_gap", TABLES)
def test_non_commensurate_tables(case, J, per_gap):
    Z, s, d = case
    g = target_grid(Z, s, d)
    assert g.J == J
    # slices per gap, the originals counted with the gap they open (the last slice, if an original, with the last gap)
    assert [int((g.gap == i).sum()) for i in range(Z - 1)] == per_gap
    assert [len(a) for a in g.gap_alphas] == [c - int(g.is_original[g.gap == i].sum()) for i, c in enumerate(per_gap)]
    assert g.is_original[0] and g.source[0] == 0
    for i, al in enumerate(g.gap_alphas):
        assert al == sorted(al) and all(0.0 < a < 1.0 for a in al)
        assert np.allclose(np.asarray(al) + i, g.position[(g.gap == i) & ~g.is_original], rtol=0, atol=1e-12)


@pytest.mark.parametrize("Z,s,d", [c for c, _, _ in TABLES] + [(5, s, s / (n + 1)) for s, n in COMMENSURATE] + [(7, 6.3, 0.9), (2, 5.0, 4.999)])
def test_invariants(Z, s, d):
    g = target_grid(Z, s, d)
    assert g.position[0] == 0.0 and (np.diff(g.position) > 0).all() and g.position[-1] <= Z - 1
    assert (g.alpha >= 0).all() and (g.alpha <= 1).all() and (g.gap >= 0).all() and (g.gap <= max(Z - 2, 0)).all()
    assert np.allclose(g.position, np.arange(g.J) * d / s, rtol=0, atol=1e-6)
    assert (g.J - 1) * d <= (Z - 1) * s * (1 + 1e-6) and g.J * d > (Z - 1) * s * (1 - 1e-6)      # the next slice would lie beyond the last
    assert sum(len(a) for a in g.gap_alphas) == g.num_synthesised == int((~g.is_original).sum())


def test_snapping_to_input_slices():
    g = target_grid(4, 10, 10 / 3)          # 3 * (10 / 3) / 10 is not 1 in floating point everywhere: every third slice IS an input slice
    assert g.J == 10 and [len(a) for a in g.gap_alphas] == [2, 2, 2]
    assert np.array_equal(np.flatnonzero(g.is_original), [0, 3, 6, 9]) and np.array_equal(g.source[g.is_original], [0, 1, 2, 3])
    assert np.array_equal(g.position[g.is_original], [0.0, 1.0, 2.0, 3.0])
    g = target_grid(3, 1.0, 0.1)            # 0.1 * 10 etc.
    assert g.J == 21 and [len(a) for a in g.gap_alphas] == [9, 9] and g.is_original[-1]


def test_one_and_two_slices():
    g = target_grid(1, 10, 1.4)
    assert g.J == 1 and g.is_original.tolist() == [True] and g.source.tolist() == [0] and g.gap_alphas == [] and g.num_synthesised == 0
    g = target_grid(2, 10, 1.4)
    assert g.J == 8 and g.gap.tolist() == [0] * 8 and [len(a) for a in g.gap_alphas] == [7] and g.is_original.tolist() == [True] + [False] * 7
    g = target_grid(2, 10, 10)
    assert g.J == 2 and g.is_original.all() and g.source.tolist() == [0, 1] and g.alpha.tolist() == [0.0, 1.0] and g.gap_alphas == [[]]


def test_refusals():
    with pytest.raises(ValueError, match="Z="):
        target_grid(0, 10, 1.4)
    with pytest.raises(ValueError, match="target_spacing_z.*down-sampling"):
        target_grid(5, 1.4, 10)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="^spacing_z"):
            target_grid(5, bad, 1.4)
        with pytest.raises(ValueError, match="^target_spacing_z"):
            target_grid(5, 10, bad)
    assert MAX_PER_GAP == 16
    assert [len(a) for a in target_grid(3, 17.0, 1.0).gap_alphas] == [16, 16]          # s / d = 17: the most there is
    with pytest.raises(ValueError, match="target_spacing_z.*aesr_lerp_multi"):
        target_grid(3, 17.5, 1.0)
    with pytest.raises(ValueError, match="aesr_lerp_multi"):
        target_grid(2, 10, 0.5)


# ---- the command line: arguments only, nothing touches a device ----------------------------------------------------------------------
def test_cli_argument_errors(tmp_path, capsys):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    base = ["--exper_dir=" + str(tmp_path / "exp"), "--data_input_dir=" + str(tmp_path), "--output_dir=" + str(tmp_path / "out")]
    with pytest.raises(SystemExit):
        ghv.parse_args(base + ["--target_spacing_z=1.4", "--isotropic"])
    assert "not allowed with" in capsys.readouterr().err
    for target in (["--target_spacing_z=1.4"], ["--isotropic"]):
        with pytest.raises(SystemExit):
            ghv.parse_args(base + target + ["--num_interpolations=6"])
        assert "--num_interpolations" in capsys.readouterr().err
    for method in ("lanczos", "bspline"):
        with pytest.raises(ValueError, match="aesr_z_expand takes integer factors only"):
            ghv.main(base + ["--method=" + method, "--target_spacing_z=1.4"])
    np.save(str(tmp_path / "vol0.npy"), np.zeros((5, 8, 8), dtype=np.float32))
    with pytest.raises(SystemExit):           # refused when the files are known, before any model is loaded
        ghv.main(base + ["--target_spacing_z=1.4"])
    assert "--spacing_z" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ghv.main(base + ["--isotropic", "--spacing_z=10", "--method=linear"])
    assert "--spacing Y X" in capsys.readouterr().err


def test_cli_defaults_are_the_integer_grid():
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    _, args = ghv.parse_args(["--exper_dir=e", "--data_input_dir=d"])
    assert args.num_interpolations == 6 and not args.on_grid and args.target_spacing_z is None and not args.isotropic
    _, args = ghv.parse_args(["--exper_dir=e", "--data_input_dir=d", "--num_interpolations=3"])
    assert args.num_interpolations == 3 and not args.on_grid
    _, args = ghv.parse_args(["--exper_dir=e", "--data_input_dir=d", "--target_spacing_z=1.4"])
    assert args.num_interpolations is None and args.on_grid and args.target_spacing_z == 1.4
    _, args = ghv.parse_args(["--method=nearest", "--output_dir=o", "--data_input_dir=d", "--isotropic"])
    assert args.num_interpolations is None and args.on_grid and args.isotropic


def test_isotropic_target_takes_the_smaller_in_plane_spacing(capsys):
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    assert ghv.isotropic_target((1.5625, 1.5625), "v.nii") == 1.5625 and capsys.readouterr().out == ""
    assert ghv.isotropic_target((1.5625, 1.25), "v.nii") == 1.25
    out = capsys.readouterr().out
    assert "v.nii" in out and "not square" in out and "1.25" in out


def test_grid_arguments_of_the_volume_functions():
    from superresolution_aniso_mri_amd import generate_hr_volumes as ghv
    from superresolution_aniso_mri_amd.evaluate import common as ec
    import torch
    g = target_grid(3, 10, 1.4)
    with pytest.raises(ValueError, match="alpha_range"):
        ghv.create_super_volume(None, torch.zeros(3, 8, 8), [0.5], grid=g)
    with pytest.raises(ValueError, match="alpha_range"):
        ec.create_super_volume(None, torch.zeros(3, 8, 8), alpha_range=[0.5], grid=g)
    with pytest.raises(ValueError, match="downsample_steps"):
        ec.create_super_volume(None, torch.zeros(3, 8, 8), downsample_steps=2, grid=g)
    with pytest.raises(ValueError, match="num_interpolations"):
        ghv.upsample_volume(None, np.zeros((3, 8, 8), dtype=np.float32), 6, grid=g)
    with pytest.raises(ValueError, match="integer factors only"):
        ghv.expand_volume_on_grid(np.zeros((3, 8, 8), dtype=np.float32), g, "lanczos")
    with pytest.raises(ValueError, match="3 slices"):
        ghv.expand_volume_on_grid(np.zeros((4, 8, 8), dtype=np.float32), g, "linear")
