"""The engine's launches against the stored dump (scripts/launch_dump.py): every library call of small forward / backward, train / eval,
single-process and data-parallel passes -- its entry point, its scalars, its tensors by symbol, its host arrays, its profiler record -- equals,
line by line, what the engine did before its routes were gathered into one function per step kind.  No device is needed: the library is
replaced by a recorder."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_launches.txt")


def test_engine_makes_the_stored_launches():
    spec = importlib.util.spec_from_file_location("launch_dump", os.path.join(ROOT, "scripts", "launch_dump.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got = tool.dump().split("\n")
    want = open(GOLDEN).read().split("\n")
    case = None
    for k, (g, w) in enumerate(zip(got, want)):
        if w.startswith("===="):
            case = w
        assert g == w, "line %d of the dump, in %s:\n  stored: %s\n  now:    %s" % (k + 1, case, w, g)
    assert len(got) == len(want), "the dump has %d lines, the stored one %d" % (len(got), len(want))
    assert len(want) > 2000 and want[-2].startswith("==== 55 cases reach the 41 launching entry points")


class _Event:
    """stands in for torch.cuda.Event: remembers whether it was recorded; elapsed_time of an unrecorded event raises, as the real one does"""

    def __init__(self, enable_timing=False):
        self.recorded = False

    def record(self, stream=None):
        self.recorded = True

    def elapsed_time(self, other):
        if not (self.recorded and other.recorded):
            raise RuntimeError("event was not recorded")
        return 0.5


def _stub_events(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)


def test_profiler_records_close_by_token_and_an_open_one_is_skipped(monkeypatch):
    """Nested records close the record they were opened as, and summary() leaves out a record whose end event was never recorded instead
    of raising."""
    from superresolution_aniso_mri_amd import engine
    _stub_events(monkeypatch)
    prof = engine.KernelProfiler()
    outer = prof.begin("bn_fwd", 0.0, 100.0)
    inner = prof.begin("conv_igemm_f32", 8.0)
    prof.end(outer)                                  # out of order: the inner record stays open
    assert outer[4].recorded and not inner[4].recorded
    lost = prof.begin("bn_bwd", 0.0, 7.0)            # never closed
    prof.end(inner)
    assert [r[0] for r in prof.records] == ["bn_fwd", "conv_igemm_f32", "bn_bwd"] and not lost[4].recorded
    assert prof.summary() == {"bn_fwd": {"launches": 1, "flops": 0.0, "bytes": 100.0, "ms": 0.5},
                              "conv_igemm_f32": {"launches": 1, "flops": 8.0, "bytes": 0.0, "ms": 0.5}}


def test_profiled_block_and_launch_close_their_record_when_the_call_raises(monkeypatch):
    """An exception between begin and end (a callback inside the bn_fwd / bn_bwd block, a call the library refuses) still closes the record."""
    import pytest
    from superresolution_aniso_mri_amd import engine
    _stub_events(monkeypatch)
    prof = engine.KernelProfiler()
    monkeypatch.setattr(engine, "PROFILER", prof)
    with pytest.raises(ValueError):
        with engine.profiled("bn_fwd", 0.0, 12.0):
            raise ValueError("sync_bn failed")

    class Refusing:
        aesr_act_bwd = staticmethod(lambda *a: 1)
        aesr_last_error_string = staticmethod(lambda: b"refused")

    monkeypatch.setattr(engine, "lib", Refusing())
    monkeypatch.setattr(engine, "stream", lambda: None)
    with pytest.raises(RuntimeError, match=r"aesr_act_bwd\(last layer\) failed \(code 1\)"):
        engine.launch("aesr_act_bwd", None, 4, kind="act_bwd", nbytes=48.0, what="aesr_act_bwd(last layer)")
    assert [(r[0], r[4].recorded) for r in prof.records] == [("bn_fwd", True), ("act_bwd", True)]
    assert prof.summary() == {"bn_fwd": {"launches": 1, "flops": 0.0, "bytes": 12.0, "ms": 0.5},
                              "act_bwd": {"launches": 1, "flops": 0.0, "bytes": 48.0, "ms": 0.5}}
