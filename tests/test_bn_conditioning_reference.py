"""The bounds of tests/bn_conditioning_util.py are neither vacuous nor flaky -- shown without a GPU:

- the fp32 reference (torch.native_batch_norm on the CPU) alone is within every bound of the number format, i.e. with its own error taken out
  of the bound altogether -- so e_ref never is what makes a bound wide, and the weaker statement (the factor 4 replaced by 1 wherever e_ref
  enters) holds with it;
- a numpy restatement of the statistics pass with fp32 one-pass sums about 0 -- what the library did -- violates the invstd bound for every
  class with r >= 128 at every shape;
- the same restatement with the sums about the group's pivot, the mean of eight of its pixels -- what csrc/bn.hip and csrc/bn_fused.hip do (csrc/bn_math.h) -- is within
  all bounds of the forward pass."""
import pytest

import bn_conditioning_util as bc


@pytest.mark.parametrize("shape,groups", bc.CASES, ids=bc.IDS)
def test_reference_alone_is_within_the_bounds_of_the_number_format(shape, groups):
    for mode in bc.MODES:
        rows = bc.table(shape, groups, mode, bc.reference(shape, groups, mode), ref_in_bound=False)
        assert {r[0] for r in rows} == set(bc.FORWARD + bc.BACKWARD)
        assert not bc.failures(rows), "\n" + bc.render(shape, groups, mode, rows)
        # ... and, as stated: within max(floor, 1 * e_ref) -- implied, kept as the statement the GPU test's factor 4 is measured against
        assert not bc.failures(bc.table(shape, groups, mode, bc.reference(shape, groups, mode), ref_factor=1.0))


@pytest.mark.parametrize("shape,groups", bc.CASES, ids=bc.IDS)
def test_sums_about_zero_lose_invstd_and_sums_about_a_pivot_do_not(shape, groups):
    about_zero = bc.table(shape, groups, "none", bc.restated(shape, groups, pivot=False))
    text = "\n" + bc.render(shape, groups, "none", about_zero)
    # (the constant channel has r = 1170 too, but its sums about 0 are sums of one number: exact by luck at some shapes, 0.29 off at others)
    big = [r for r in about_zero if r[0] == "invstd" and r[3] >= 128.0 and bc.CLASSES[r[2]][1] > 0.0]
    assert len({r[2] for r in big}) >= 2, text               # the classes with r >= 128 that C = 8 has: (12.8, 0.1), (-25.6, 0.05)
    assert all(not r[7] for r in big), text
    pivot = bc.table(shape, groups, "none", bc.restated(shape, groups, pivot=True))
    assert {r[0] for r in pivot} == set(bc.FORWARD)
    assert not bc.failures(pivot), "\n" + bc.render(shape, groups, "none", pivot)
