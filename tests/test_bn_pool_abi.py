"""No GPU: the entry points of include/aesr_hip_bnpool.h (BatchNorm + AvgPool2d(2) pooled once) on the host; tests/test_abi.py checks the
header against ``_hip.SIGNATURES_BNPOOL``.

- ``aesr_bn_pool_supported`` on both sides of each of its limits;
- argument refusals come before anything touches the device: non-zero, the function's name in the message."""
import ctypes


def test_supported_on_both_sides_of_each_limit():
    from superresolution_aniso_mri_amd import _hip
    ok = _hip.lib.aesr_bn_pool_supported
    assert ok(36, 162, 162, 32, 2) == 1 and ok(36, 81, 81, 64, 2) == 1 and ok(10, 33, 31, 32, 2) == 1
    # channels: a multiple of 4, C / 4 a divisor of 256 (the kernels' lane layout, as the other BatchNorm launches), at most 1024
    assert ok(2, 4, 4, 4, 1) == 1 and ok(2, 4, 4, 1024, 1) == 1 and ok(2, 4, 4, 128, 1) == 1
    assert ok(2, 4, 4, 0, 1) == 0 and ok(2, 4, 4, 6, 1) == 0 and ok(2, 4, 4, 30, 1) == 0 and ok(2, 4, 4, 2048, 1) == 0 and ok(2, 4, 4, -4, 1) == 0
    assert ok(2, 4, 4, 12, 1) == 0 and ok(2, 4, 4, 1028, 1) == 0
    # at least one window
    assert ok(2, 2, 2, 8, 1) == 1 and ok(2, 1, 2, 8, 1) == 0 and ok(2, 2, 1, 8, 1) == 0 and ok(2, 0, 4, 8, 1) == 0
    # groups: 1 .. 4 (BnGroups), none of them empty
    assert ok(4, 4, 4, 8, 4) == 1 and ok(4, 4, 4, 8, 5) == 0 and ok(4, 4, 4, 8, 0) == 0 and ok(4, 4, 4, 8, -1) == 0
    assert ok(3, 4, 4, 8, 4) == 0 and ok(0, 4, 4, 8, 1) == 0
    # 32-bit pixel indices: N * H * W < 2^31
    assert ok(2, 32768, 32767, 8, 1) == 1 and ok(2, 32768, 32768, 8, 1) == 0 and ok(1 << 20, 2, 1024, 8, 1) == 0
    assert ok(32768, 256, 256, 8, 1) == 0 and ok(32767, 256, 256, 8, 1) == 1


def _refused(call, fname, names, ok, bad):
    from superresolution_aniso_mri_amd import _hip
    for name, value in bad:
        args = list(ok)
        args[names.index(name)] = value
        rc = call(*args)
        assert rc == 1 and fname in _hip.last_error(), (fname, name, value, rc, _hip.last_error())


def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    L = _hip.lib
    fake = ctypes.c_void_p(4096)
    ns, cnt = _hip.int_array([0, 2, 3]), _hip.double_array([2.0 * 81, 81.0])
    groups = [("G", 0), ("G", 5), ("G", -1), ("nstart", None), ("nstart", _hip.int_array([0, 3, 3])), ("nstart", _hip.int_array([1, 2, 3])),
              ("nstart", _hip.int_array([0, 2, 4])), ("nstart", _hip.int_array([0, 3, 2]))]
    names = ["y", "m", "partial", "counts", "gamma", "beta", "running_mean", "running_var", "nbt", "mean", "invstd", "scale", "shift",
             "N", "H", "W", "C", "G", "nstart", "momentum", "eps", "update", "stream"]
    ok = [fake, fake, fake, cnt] + [fake] * 9 + [3, 9, 9, 8, 2, ns, 0.1, 1e-5, 1, None]
    bad = [(n, None) for n in ("y", "m", "partial", "counts", "gamma", "beta", "mean", "invstd", "scale", "shift")]
    bad += [("C", 6), ("C", 0), ("C", 12), ("C", 2048), ("H", 1), ("W", 1), ("H", 0), ("N", 0), ("N", 4)] + groups
    _refused(L.aesr_bn_pool_stats_finalize, "aesr_bn_pool_stats_finalize", names, ok, bad)

    names = ["m", "scale", "shift", "out", "N", "Ho", "Wo", "C", "G", "nstart", "stream"]
    ok = [fake] * 4 + [3, 4, 4, 8, 2, ns, None]
    bad = [(n, None) for n in ("m", "scale", "shift", "out")] + [("C", 6), ("C", 12), ("Ho", 0), ("Wo", 0), ("Wo", -3), ("N", 0), ("N", 2)] + groups
    _refused(L.aesr_bn_pool_apply, "aesr_bn_pool_apply", names, ok, bad)

    names = ["gout", "y", "m", "mean", "invstd", "scale", "partial", "counts", "coef", "dgamma", "dbeta", "dpre", "N", "H", "W", "C", "act", "slope",
             "G", "nstart", "stream"]
    ok = [fake] * 7 + [cnt] + [fake] * 4 + [3, 9, 9, 8, _hip.ACT_LRELU, 0.01, 2, ns, None]
    bad = [(n, None) for n in names[:12]] + [("C", 6), ("C", 12), ("H", 1), ("W", 1), ("N", 0), ("N", 5), ("act", 4), ("act", -1)] + groups
    _refused(L.aesr_bn_pool_bwd, "aesr_bn_pool_bwd", names, ok, bad)
