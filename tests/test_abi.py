"""No GPU: the C ABI of libaesr_hip.so, stated once.  For every header of ``_hip.HEADERS``: the header's declarations == its table == the
library's exports == what ``_load()`` bound, with every parameter and return type of the table checked against the C prototype; no name in two
headers or tables; the recorded symbol list (tests/golden/abi_symbols.json) unchanged; the ctypes structures and the mirrored constants against
their ``typedef struct`` / ``#define``; and the guard-band cases and exemptions of the header's GPU test module partition its table."""
import ctypes
import glob
import importlib
import json
import os
import re

import pytest

import abi_util as au
from superresolution_aniso_mri_amd import _hip

CSRC = os.path.join(au.ROOT, "superresolution_aniso_mri_amd", "csrc")


def _tables():
    """name of the table in _hip -> table, for every SIGNATURES* dict of the module"""
    return {k: v for k, v in vars(_hip).items() if k.startswith("SIGNATURES")}


# ---- names ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", list(_hip.HEADERS))
def test_header_table_exports_and_binding_agree(header):
    table = _hip.HEADERS[header]
    declared = au.declared(header)
    assert declared == set(table), declared ^ set(table)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name, (res, args) in table.items():
        assert getattr(lib, name, None) is not None, "%s is declared in include/%s but not exported" % (name, header)
        assert getattr(_hip.lib, name).restype == res and getattr(_hip.lib, name).argtypes == args, name


def test_no_name_is_declared_or_listed_twice():
    assert au.headers() == sorted(_hip.HEADERS), "include/*.h and _hip.HEADERS differ"
    tables = _tables()
    assert sorted(map(id, tables.values())) == sorted(map(id, _hip.HEADERS.values())), "a SIGNATURES* table of _hip is not in HEADERS, or is in it twice"
    # whatever it is called: a module-level dict of (restype, [argtypes]) pairs is a table of entry points, and HEADERS has every one
    for k, v in vars(_hip).items():
        if isinstance(v, dict) and v and all(isinstance(e, tuple) and len(e) == 2 and isinstance(e[1], list) for e in v.values()):
            assert any(v is t for t in _hip.HEADERS.values()), "_hip.%s is a table of entry points that is not in HEADERS" % k
    for what, sets in (("declared in", {h: au.declared(h) for h in au.headers()}), ("listed in", {k: set(t) for k, t in tables.items()})):
        seen = {}
        for where, names in sets.items():
            for name in names:
                assert name not in seen, "%s is %s %s and %s" % (name, what, seen[name], where)
                seen[name] = where


def test_the_abi_is_the_recorded_one():
    """The ABI does not shrink (or grow) unnoticed: a symbol that comes or goes changes tests/golden/abi_symbols.json in the same commit."""
    want = json.load(open(os.path.join(au.ROOT, "tests", "golden", "abi_symbols.json")))
    assert {h: sorted(t) for h, t in _hip.HEADERS.items()} == want


# ---- types ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", list(_hip.HEADERS))
def test_bound_types_are_the_prototypes(header):
    """Every return type and every parameter of every symbol, by the rule of abi_util.compatible: no exception list."""
    table, protos = _hip.HEADERS[header], au.prototypes(header)
    assert set(protos) == set(table)
    for name, (ret, params) in protos.items():
        res, args = table[name]
        assert ret in au.RETURNS and au.RETURNS[ret] is res, "%s returns %s, bound as %s" % (name, ret, res)
        assert len(args) == len(params), "%s takes %d arguments, %d are bound" % (name, len(params), len(args))
        for i, ((ctype, pname), bound) in enumerate(zip(params, args)):
            assert au.compatible(ctype, bound, _hip), "%s: argument %d, %s %s, is bound as %s" % (name, i, ctype, pname, bound)


def test_structures_are_the_headers():
    found = {}
    for header in _hip.HEADERS:
        found.update(au.structs(header))
    assert set(found) == set(au.STRUCTS)
    for cname, pyname in au.STRUCTS.items():
        fields = getattr(_hip, pyname)._fields_
        assert [f[0] for f in fields] == [n for _, n in found[cname]], cname
        for (ctype, fname), (_, bound) in zip(found[cname], fields):
            want = ctypes.c_void_p if ctype.endswith("*") else au.SCALARS[ctype]
            assert bound is want, "%s.%s is %s in the header, %s in _hip.%s" % (cname, fname, ctype, bound, pyname)
    assert ctypes.sizeof(_hip.TripletDesc) == 48


# ---- constants -----------------------------------------------------------------------------------------------------------------------
# (_hip name, header, #define).  Not here, because they mirror a definition of csrc/ that no public header states: ACT_* (the enum of
# csrc/aesr_common.h), REDUCE_MAX_JOBS (csrc/aesr_kernels.h) and SEG_MIN_CLASSES / SEG_MAX_CLASSES (the limits written out in
# csrc/seg_head.hip).
MIRRORED = ([(n, "aesr_hip.h", "AESR_" + n) for n in (
    "PREP_PACK", "PREP_WINO_PACK", "PREP_STEM_FOLD", "PREP_COUT1_FLIP", "RS_POOL", "RS_NEAREST", "RS_BILINEAR", "BN_NONE", "BN_POOL", "BN_UP",
    "BN_NWG", "LPIPS_NCH", "MSE_NPART", "MSE3_WS", "P2P_HANDLE_BYTES", "P2P_SLOTS", "COMM_ID_BYTES", "COMM_F32", "COMM_F64", "COMM_SUM", "COMM_MAX")]
            + [(n, "aesr_hip_baselines.h", "AESR_" + n) for n in ("ZX_ALIGN_ITK", "ZX_ALIGN_GRID", "ZX_CLAMP", "ZX_MIRROR", "ZX_MAX_FACTOR",
                                                                     "ZX_MAX_TAPS")]
            + [(n, "aesr_hip_reslice.h", "AESR_" + n) for n in ("RESLICE_NEAREST", "RESLICE_LINEAR")]
            + [(n, "aesr_hip_surface.h", "AESR_" + n) for n in ("SURFACE_MAX_CLASSES", "SURFACE_COUNTS", "SURFACE_MAX_W")]
            + [(n, "aesr_hip_components.h", "AESR_" + n) for n in ("COMPONENTS_MAX_CLASSES", "COMPONENTS_COLUMNS", "COMPONENTS_MAX_PER_CLASS")]
            + [(n, "aesr_hip_shape.h", "AESR_" + n) for n in ("SHAPE_MAX_CLASSES", "SHAPE_MAX_W")]
            + [(n, "aesr_hip_reslice_taps.h", "AESR_" + n) for n in ("TAPS_BSPLINE3", "TAPS_LANCZOS", "TAPS_COSINE", "TAPS_MIN_RADIUS", "TAPS_MAX_RADIUS")])
# integer #defines of the headers that _hip has no use for
NOT_MIRRORED = {"AESR_ABI_VERSION", "AESR_ERR_ARG", "AESR_ERR_HIP", "AESR_ERR_UNSUPPORTED", "AESR_MSE3_NPART", "AESR_P2P_REC_BYTES"}


def test_mirrored_constants_are_the_headers():
    defs = {h: au.defines(h) for h in _hip.HEADERS}
    for name, header, define in MIRRORED:
        assert getattr(_hip, name) == defs[header][define], (name, header, define)
    every = {d for h in defs for d in defs[h]}
    assert every == {d for _, _, d in MIRRORED} | NOT_MIRRORED, "an integer #define of include/ is neither mirrored in _hip nor listed as unused"
    # values that callers outside the package rely on
    assert (_hip.RESLICE_NEAREST, _hip.RESLICE_LINEAR) == (0, 1) and (_hip.RS_POOL, _hip.RS_NEAREST, _hip.RS_BILINEAR) == (1, 2, 3)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
# header -> (GPU test module, exact set of exempt names, guard-band tests that must exist, (subset, superset) attributes of the module).
# Every name of the header's table is the subject of a guard-band case of that module (its covered_entries(), else its GUARDED_ENTRIES) or
# exempt for a stated reason; an exemption is a pure host query -- a launch entry point needs a case.  The main header's exemptions are given
# by rule (MAIN_*) instead of by name.
GUARDS = {
    "aesr_hip.h": ("test_gpu_memguard", None, ("test_guarded", "test_every_path_was_guarded"), ()),
    "aesr_hip_preproc.h": ("test_gpu_inplane", {"aesr_inplane_out_size", "aesr_inplane_workspace_bytes"},
                           ("test_guard_bands_poisons_and_offset_pointers",), ()),
    "aesr_hip_dataprep.h": ("test_gpu_brain", {"aesr_thick_slices_out_slices", "aesr_thick_slices_store_bytes"},
                            ("test_thick_slices_guard_bands_poisons_and_offset_pointers", "test_assemble_raw_guard_bands_and_poisons"), ()),
    "aesr_hip_train.h": ("test_gpu_cout1_bwd", {"aesr_conv2d_cout1_bwd_workspace_floats"},
                         ("test_guard_bands_poisons_and_offset_pointers", "test_refusals_write_nothing"), (("GUARD_SHAPES", "SHAPES"),)),
    "aesr_hip_baselines.h": ("test_gpu_z_expand", {"aesr_z_expand_out_slices", "aesr_z_expand_store_bytes", "aesr_bspline_coef_bytes"},
                             ("test_z_expand_guard_bands_poisons_and_offset_pointers", "test_prefilter_guard_bands_poisons_and_offset_pointers"), ()),
    "aesr_hip_reslice.h": ("test_gpu_reslice", set(),
                           ("test_affine_guard_bands_poisons_and_offset_pointers", "test_grid_guard_bands_poisons_and_offset_pointers"), ()),
    "aesr_hip_seg.h": ("test_gpu_multichannel", {"aesr_softmax_dice_workspace_floats"}, ("test_guard_bands_poisons_and_offset_pointers",), ()),
    "aesr_hip_surface.h": ("test_gpu_seg_metrics", {"aesr_surface_workspace_bytes"}, ("test_guard_bands_poisons_and_shifted_pointers",), ()),
    "aesr_hip_bnpool.h": ("test_gpu_bn_pool", {"aesr_bn_pool_supported"},
                          ("test_guard_bands_poisons_and_offset_pointers", "test_refusals_write_nothing"), (("GUARD_CASES", "CASES"),)),
    "aesr_hip_labelprep.h": ("test_gpu_labelled", set(), ("test_guard_bands_poisons_and_offset_pointers", "test_refusals_write_nothing"), ()),
    "aesr_hip_components.h": ("test_gpu_components", {"aesr_components_workspace_bytes"}, ("test_guard_bands_poisons_and_shifted_pointers",), ()),
    "aesr_hip_shape.h": ("test_gpu_shape_interp", {"aesr_shape_workspace_bytes"}, ("test_guard_bands_poisons_and_shifted_pointers",), ()),
    "aesr_hip_reslice_taps.h": ("test_gpu_reslice_taps", set(),
                                ("test_taps_guard_bands_poisons_and_offset_pointers", "test_prefilter_guard_bands_poisons_and_offset_pointers"), ()),
}
MAIN_HOST_SUFFIXES = ("_supported", "_floats", "_bytes", "_words", "_doubles", "_kernel", "_timeouts")
MAIN_HOST_NAMES = ("aesr_version", "aesr_last_error_string", "aesr_adam_state_init")


def test_every_header_has_a_guard_band_row():
    assert set(GUARDS) == set(_hip.HEADERS)


@pytest.mark.parametrize("header", list(_hip.HEADERS))
def test_guard_band_cases_and_exemptions_partition_the_table(header):
    module, exact, tests, subsets = GUARDS[header]
    tg = importlib.import_module(module)
    covered = tg.covered_entries() if hasattr(tg, "covered_entries") else set(tg.GUARDED_ENTRIES)
    exempt, names = set(tg.EXEMPT), set(_hip.HEADERS[header])
    assert not (covered & exempt), sorted(covered & exempt)
    assert covered | exempt == names, (sorted(names - covered - exempt), sorted((covered | exempt) - names))
    assert all(tg.EXEMPT.values()), "an exemption without a reason"
    if exact is not None:
        assert exempt == exact, "%s: only %s may be exempt; a launch entry point needs a case, not an exemption" % (module, sorted(exact))
    else:
        for name in exempt:          # only pure host queries and the entry points that need a peer or a communicator
            peer = name.startswith(("aesr_comm_", "aesr_p2p_")) or (name.startswith("aesr_bn_fused1_") and name.endswith("_p2p"))
            assert peer or name.endswith(MAIN_HOST_SUFFIXES) or name in MAIN_HOST_NAMES, "%s is a launch entry point: it needs a case, not an exemption" % name
        assert len(covered) >= 70
        assert len({c.id for c in tg.CASES}) == len(tg.CASES)
    for t in tests:
        assert callable(getattr(tg, t)), (module, t)
    for sub, sup in subsets:
        assert set(getattr(tg, sub)) <= set(getattr(tg, sup)), (module, sub, sup)


# ---- the build -----------------------------------------------------------------------------------------------------------------------
def test_the_build_lists_every_header_and_source():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hdrs = re.search(r"^HDRS = (.*)$", mk, flags=re.M).group(1).split()
    assert {h for h in hdrs if h.startswith("../../include/")} == {"../../include/" + h for h in _hip.HEADERS}
    assert {h for h in hdrs if "/" not in h} == {os.path.basename(h) for h in glob.glob(os.path.join(CSRC, "*.h"))}
    assert re.search(r"^build/%\.o: %\.hip \$\(HDRS\)$", mk, flags=re.M) and re.search(r"^build/asan/%\.o: %\.hip \$\(HDRS\)$", mk, flags=re.M)
    srcs = re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert sorted(srcs) == sorted(os.path.basename(s) for s in glob.glob(os.path.join(CSRC, "*.hip")))
