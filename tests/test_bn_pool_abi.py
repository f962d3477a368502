"""No GPU: the BatchNorm + AvgPool2d(2) pool-once header of libaesr_hip.so (include/aesr_hip_bnpool.h, ``_hip.SIGNATURES_BNPOOL``).

- the header == the table == the library's exports, with the argument types as bound; disjoint from every other header and table;
- ``GUARDED_ENTRIES`` and ``EXEMPT`` of tests/test_gpu_bn_pool.py partition the table, and only the ``_supported`` query is exempt;
- ``aesr_bn_pool_supported`` on both sides of each of its limits;
- argument refusals come before anything touches the device: non-zero, the function's name in the message."""
import ctypes
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"aesr_bn_pool_supported", "aesr_bn_pool_stats_finalize", "aesr_bn_pool_apply", "aesr_bn_pool_bwd"}


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(aesr_[a-z0-9_]+)\s*\(", hdr))


def test_header_table_and_exports_agree():
    from superresolution_aniso_mri_amd import _hip
    declared = _declared("aesr_hip_bnpool.h")
    assert declared == set(_hip.SIGNATURES_BNPOOL) == NAMES
    others = set()
    tables = [k for k in vars(_hip) if k.startswith("SIGNATURES") and k != "SIGNATURES_BNPOOL"]
    assert len(tables) >= 8
    for k in tables:
        others |= set(getattr(_hip, k))
    headers = [os.path.basename(h) for h in glob.glob(os.path.join(ROOT, "include", "*.h")) if not h.endswith("aesr_hip_bnpool.h")]
    assert len(headers) >= 8
    for h in headers:
        others |= _declared(h)
    assert not declared & others
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in declared:
        assert getattr(lib, name, None) is not None, "%s is declared in include/aesr_hip_bnpool.h but not exported" % name
        res, args = _hip.SIGNATURES_BNPOOL[name]
        assert getattr(_hip.lib, name).argtypes == args and getattr(_hip.lib, name).restype == res
    # the C declarations, argument by argument
    P, I, F, IP, DP = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, _hip.IP, _hip.DP
    assert _hip.SIGNATURES_BNPOOL["aesr_bn_pool_supported"] == (I, [I] * 5)
    assert _hip.SIGNATURES_BNPOOL["aesr_bn_pool_stats_finalize"] == (I, [P, P, P, DP] + [P] * 9 + [I] * 5 + [IP, F, F, I, P])
    assert _hip.SIGNATURES_BNPOOL["aesr_bn_pool_apply"] == (I, [P] * 4 + [I] * 5 + [IP, P])
    assert _hip.SIGNATURES_BNPOOL["aesr_bn_pool_bwd"] == (I, [P] * 7 + [DP] + [P] * 4 + [I] * 5 + [F, I, IP, P])


def test_guard_band_cases_and_exemptions_partition_the_bnpool_abi():
    """The rule of tests/test_memguard_host.py::test_case_table_and_exemptions_partition_the_abi for this table."""
    import test_gpu_bn_pool as tg
    from superresolution_aniso_mri_amd import _hip
    covered, exempt, names = set(tg.GUARDED_ENTRIES), set(tg.EXEMPT), set(_hip.SIGNATURES_BNPOOL)
    assert not (covered & exempt) and covered | exempt == names, (sorted(names - covered - exempt), sorted((covered | exempt) - names))
    for name, reason in tg.EXEMPT.items():
        assert reason and name.endswith("_supported"), "%s is a launch entry point: it needs a case, not an exemption" % name
    assert exempt == {"aesr_bn_pool_supported"}
    assert callable(tg.test_guard_bands_poisons_and_offset_pointers) and callable(tg.test_refusals_write_nothing)
    assert set(tg.GUARD_CASES) <= set(tg.CASES)


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
