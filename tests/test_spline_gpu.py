"""-m gpu: the spline-order resampling kernels (csrc/kernels/spline.h) on the MI355X through ops.spline_prefilter / ops.spline_resample and through
Spacing(d) / SpatialResample / Resample / lazy resampling with an integer `mode`, against scipy's and the reference's own outputs
(tests/golden/spline.npz) under the acceptance rule of tests/spline_cases.py.  Every case runs twice and has to give identical bits."""
import pytest

import spline_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("group", ("pre-o2", "pre-o3", "pre-o4", "pre-o5"))
def test_prefilter_against_scipy(group):
    assert sc.case_prefilter(DEV, lambda cid: cid.startswith(group)) > 0


@pytest.mark.parametrize("group", ("ops-o0", "ops-o1", "ops-o2", "ops-o3", "ops-o4", "ops-o5"))
def test_sampler_against_scipy(group):
    assert sc.case_samples(DEV, lambda cid: cid.startswith(group)) > 0


@pytest.mark.parametrize("group", ("spacing-", "sresample-", "exact-", "resample-", "lazy-", "inverse-", "spacingd-"))
def test_transforms_against_the_reference(group):
    assert sc.case_transforms(DEV, lambda cid: cid.startswith(group)) > 0


def test_spline_api():
    sc.case_api(DEV)
