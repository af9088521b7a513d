"""-m gpu: the bilateral-filter kernels (csrc/kernels/bilateral.h) on the MI355X through monai_amd._C.bilateral_filter against the reference's own
outputs (tests/golden/bilateral*.npz) with the tolerances of tests/bilateral_cases.py: float32 within twice the reference's own float32 error, float64
within the a-priori bound, NaN exactly where the reference has NaN.  Every case runs twice and has to give identical bits; the kernel the host chooses
is asserted per case.  The ratio |ours - ref64| / e_ref is printed per group (run with -s)."""
import pytest
import torch

import bilateral_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("group", bc.GROUPS)
def test_golden_cases_within_the_reference_error(group):
    cases = [c for c in bc.golden_cases() if c["id"].split("-")[0] == group]
    assert cases, group
    worst = bc.check_cases(DEV, cases)
    print(group, "worst |ours - ref64| / e_ref per kernel (1 tile, 2 generic):", {k: round(v, 2) for k, v in sorted(worst.items())})


def test_large_volumes_and_both_kernels_ran():
    """40 x 41 x 42 at sigma 2 (11 taps) and sigma 3 (15 taps) on the tile kernel, sigma 3 in float64 on the generic kernel"""
    worst = bc.check_cases(DEV, bc.gpu_cases())
    assert set(worst) == {bc.TILE, bc.GENERIC}
    print("large volumes, worst ratio per kernel:", {k: round(v, 2) for k, v in sorted(worst.items())})


def test_autograd_half_and_non_contiguous():
    from monai_amd import _C, ops
    from monai_amd.networks.layers import BilateralFilter

    x = torch.from_numpy(bc.inputs(next(c for c in bc.golden_cases() if c["id"] == "chan-c2")).copy()).to(DEV)
    xg = x.clone().requires_grad_()
    y = BilateralFilter.apply(xg, 1.0, 1.5, False)
    assert torch.equal(y, ops.bilateral_filter(x, 1.0, 1.5))
    y.sum().backward()
    assert torch.equal(xg.grad, ops.bilateral_filter(torch.ones_like(x), 1.0, 1.5))
    h = x.half()
    assert torch.equal(_C.bilateral_filter(h, 1.0, 1.5, False), ops.bilateral_filter(h.float(), 1.0, 1.5).half())
    xt = x.transpose(3, 4)
    assert torch.equal(ops.bilateral_filter(xt, 1.0, 1.5), ops.bilateral_filter(xt.contiguous(), 1.0, 1.5))
    with pytest.raises(RuntimeError, match="fast_approx=False"):
        BilateralFilter.apply(x)
