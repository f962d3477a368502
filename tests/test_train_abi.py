"""No GPU: the entry points of include/aesr_hip_train.h on the host (tests/test_abi.py checks the header against ``_hip.SIGNATURES_TRAIN``).

- the workspace query is (512 + 1) * 10 * Cin;
- argument refusals come before anything touches the device: non-zero, the function's name in the message."""
import ctypes

THIN_CHANNELS = (4, 8, 16, 32, 64, 128, 256)


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
