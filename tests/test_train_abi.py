"""No GPU: the fourth header of libaesr_hip.so (include/aesr_hip_train.h, ``_hip.SIGNATURES_TRAIN``).

- the header == the table == the library's exports, with the argument types as bound; disjoint from the three other headers and tables;
- ``GUARDED_ENTRIES`` and ``EXEMPT`` of tests/test_gpu_cout1_bwd.py partition the table, and only the ``_floats`` query is exempt;
- the workspace query is (512 + 1) * 10 * Cin;
- argument refusals come before anything touches the device: non-zero, the function's name in the message."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("aesr_hip.h", "aesr_hip_preproc.h", "aesr_hip_dataprep.h")
THIN_CHANNELS = (4, 8, 16, 32, 64, 128, 256)


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(aesr_[a-z0-9_]+)\s*\(", hdr))


def test_train_header_table_and_exports_agree():
    from superresolution_aniso_mri_amd import _hip
    declared = _declared("aesr_hip_train.h")
    assert declared == set(_hip.SIGNATURES_TRAIN) == {"aesr_conv2d_cout1_bwd", "aesr_conv2d_cout1_bwd_workspace_floats"}
    others = set(_hip.SIGNATURES) | set(_hip.SIGNATURES_PREPROC) | set(_hip.SIGNATURES_DATAPREP)
    for h in OTHER_HEADERS:
        others |= _declared(h)
    assert not declared & others
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in declared:
        assert getattr(lib, name, None) is not None, "%s is declared in include/aesr_hip_train.h but not exported" % name
        res, args = _hip.SIGNATURES_TRAIN[name]
        assert getattr(_hip.lib, name).argtypes == args and getattr(_hip.lib, name).restype == res
    # the C declaration, argument by argument: 8 pointers, 5 ints, float, int, float, stream
    P = ctypes.c_void_p
    assert _hip.SIGNATURES_TRAIN["aesr_conv2d_cout1_bwd"] == (ctypes.c_int, [P] * 8 + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_float, P])
    assert _hip.SIGNATURES_TRAIN["aesr_conv2d_cout1_bwd_workspace_floats"] == (ctypes.c_size_t, [ctypes.c_int])


def test_guard_band_cases_and_exemptions_partition_the_train_abi():
    """The rule of tests/test_memguard_host.py::test_case_table_and_exemptions_partition_the_abi for the fourth table."""
    import test_gpu_cout1_bwd as tg
    from superresolution_aniso_mri_amd import _hip
    covered, exempt, names = set(tg.GUARDED_ENTRIES), set(tg.EXEMPT), set(_hip.SIGNATURES_TRAIN)
    assert not (covered & exempt) and covered | exempt == names, (sorted(names - covered - exempt), sorted((covered | exempt) - names))
    for name, reason in tg.EXEMPT.items():
        assert reason and name.endswith("_floats"), "%s is a launch entry point: it needs a case, not an exemption" % name
    assert covered == {"aesr_conv2d_cout1_bwd"}
    assert callable(tg.test_guard_bands_poisons_and_offset_pointers) and callable(tg.test_refusals_write_nothing)
    assert set(tg.GUARD_SHAPES) <= set(tg.SHAPES)


def test_workspace_query():
    from superresolution_aniso_mri_amd import _hip
    f = _hip.lib.aesr_conv2d_cout1_bwd_workspace_floats
    for cin in THIN_CHANNELS:
        assert f(cin) == (512 + 1) * 10 * cin
    assert f(0) == 0 and f(-4) == 0


def test_entry_point_checks_its_arguments_on_the_host():
    """Every refusal comes before anything touches the device: callable without a GPU; the pointers below are never dereferenced."""
    from superresolution_aniso_mri_amd import _hip
    call = _hip.lib.aesr_conv2d_cout1_bwd
    fake = ctypes.c_void_p(4096)
    names = ["x", "dout", "out", "w_flipped", "dw", "db", "dx", "workspace", "N", "H", "W", "Cin", "act", "slope", "mask_act", "mask_slope", "stream"]
    ok = [fake] * 8 + [2, 12, 12, 8, _hip.ACT_SIGMOID, 0.0, _hip.ACT_LRELU, 0.01, None]
    bad = [("x", None), ("dout", None), ("out", None), ("w_flipped", None), ("dw", None), ("db", None), ("dx", None), ("workspace", None),
           ("N", 0), ("H", 0), ("W", -1), ("Cin", 12), ("Cin", 0), ("Cin", 512), ("Cin", 24), ("act", 4), ("mask_act", -1)]
    for name, value in bad:
        args = list(ok)
        args[names.index(name)] = value
        rc = call(*args)
        assert rc == 1 and "aesr_conv2d_cout1_bwd" in _hip.last_error(), (name, value, rc, _hip.last_error())
    assert "Cin=12" in (call(*[12 if n == "Cin" else v for n, v in zip(names, ok)]) and _hip.last_error())
