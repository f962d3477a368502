"""not gpu: the guard-band helper (tests/memguard.py) on CPU tensors against tiny pure-Python "kernels" with planted violations --
the evidence that the checker of tests/test_gpu_memguard.py can fail.  No GPU kernel is ever made to write out of range."""
import pytest
import torch

import memguard as mg


def _neighbour(view, offset):
    """Element `offset` relative to the start of view, inside view's own backing allocation (what a stray pointer of a kernel reaches)."""
    return torch.as_strided(view, (1,), (1,), view.storage_offset() + offset)


def kernel_ok(x, out):
    out.copy_(x * 2)


def kernel_past_end(x, out):
    out.copy_(x * 2)
    _neighbour(out, out.numel())[0] = 1.0


def kernel_before_start(x, out):
    out.copy_(x * 2)
    _neighbour(out, -1)[0] = 1.0


def kernel_writes_input(x, out):
    out.copy_(x * 2)
    x[x.numel() // 2] += 1.0


def _run(kernel, n, dtype, fill, shift):
    x = mg.guarded(n, dtype, "cpu", torch.arange(n, dtype=dtype), shift, name="x")
    out = mg.guarded(n, dtype, "cpu", fill, shift, name="out")
    saved = mg.bits(x.view)
    kernel(x.view, out.view)
    return x, out, saved


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("fill", [mg.POISON_NAN, mg.POISON_FINITE])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 64])
def test_correct_kernel_passes(n, dtype, fill, shift):
    x, out, saved = _run(kernel_ok, n, dtype, fill, shift)
    assert out.view.data_ptr() % 16 == (0 if shift == 0 else out.view.element_size())
    mg.assert_guards_intact([x, out])
    mg.assert_unchanged(x.view, saved, "x")
    assert mg.poison_left(out.view, fill).numel() == 0
    assert torch.equal(out.view, torch.arange(n, dtype=dtype) * 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shift", [0, 1])
def test_store_past_the_end_is_reported(dtype, shift):
    x, out, saved = _run(kernel_past_end, 7, dtype, mg.POISON_NAN, shift)
    with pytest.raises(AssertionError, match=r"out: back guard damaged, [12] word\(s\), first at word offset 0"):
        mg.assert_guards_intact([x, out])
    mg.assert_guards_intact([x])
    assert [d[0] for d in mg.guard_damage(out)] == ["back"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shift", [0, 1])
def test_store_before_the_start_is_reported(dtype, shift):
    x, out, saved = _run(kernel_before_start, 7, dtype, mg.POISON_FINITE, shift)
    with pytest.raises(AssertionError, match=r"out: front guard damaged, [12] word\(s\), first at word offset 1"):
        mg.assert_guards_intact([x, out])
    assert [d[0] for d in mg.guard_damage(out)] == ["front"]


def test_modified_input_is_reported():
    x, out, saved = _run(kernel_writes_input, 9, torch.float32, mg.POISON_NAN, 0)
    mg.assert_guards_intact([x, out])
    with pytest.raises(AssertionError, match=r"x: input modified, 1 element\(s\), first at 4, last at 4"):
        mg.assert_unchanged(x.view, saved, "x")


def test_unwritten_output_elements_are_found_under_both_poisons():
    for fill in (mg.POISON_NAN, mg.POISON_FINITE):
        for dtype in (torch.float32, torch.float64, torch.uint8):
            out = mg.guarded(6, dtype, "cpu", fill, name="out")
            out.view[:4] = 1
            assert mg.poison_left(out.view, fill).tolist() == [4, 5]
    # a NaN the kernel computed itself is not the poison
    out = mg.guarded(3, torch.float32, "cpu", mg.POISON_NAN)
    out.view.fill_(float("nan"))
    assert mg.poison_left(out.view, mg.POISON_NAN).numel() == 0


def test_guard_sizes_and_byte_buffers():
    g = mg.guarded(5, torch.uint8, "cpu", mg.POISON_NAN, shift_elems=1, name="black")
    assert g.view.data_ptr() % 16 == 4
    assert g.guard_words("front").numel() >= mg.GUARD_ELEMS and g.guard_words("back")[0].numel() >= mg.GUARD_ELEMS
    mg.assert_guards_intact([g])
    _neighbour(g.view, 5)[0] = 0              # the byte right after a 5-byte payload
    with pytest.raises(AssertionError, match="black: back guard damaged"):
        mg.assert_guards_intact([g])
    empty = mg.guarded(0, torch.float32, "cpu", mg.POISON_NAN)
    assert empty.view.numel() == 0
    mg.assert_guards_intact([empty])


