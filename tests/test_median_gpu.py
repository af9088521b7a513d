"""-m gpu: the median-filter kernels (csrc/kernels/median.h) on the MI355X through MedianFilter / median_filter / MedianSmooth(d) against the
reference's own outputs (tests/golden/median.npz), bit for bit -- a selection has no rounding -- with NaN exactly where the reference has NaN.
Every case runs twice and has to give identical bits; the path the host chooses is asserted per case (tests/median_cases.py)."""
import pytest

import median_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GROUPS = ("small", "unit", "fast3d", "fast2d", "fast-r011", "func", "smooth", "2d", "1d", "radii", "general", "passes", "nonfinite")


@pytest.mark.parametrize("group", GROUPS)
def test_golden_cases_bit_identical_to_the_reference(group):
    paths = mc.case_golden(DEV, lambda cid: cid.startswith(group))
    assert paths, group
    print(group, "paths taken", sorted(paths))


def test_both_kernels_ran():
    assert mc.case_golden(DEV, lambda cid: cid in ("fast3d-5x65x17-normal", "general-10x19x21-r2")) == {mc.FAST, mc.GENERAL}


def test_median_api():
    mc.case_api(DEV)
