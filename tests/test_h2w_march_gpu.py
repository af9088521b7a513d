"""-m gpu: the split march of conv3d_k3_h2w_kernel (csrc/kernels/conv3d_wino_h2.h) on the MI355X, over the launches of tests/h2w_march_cases.py -- every split into
generic head blocks, steady blocks and generic tail blocks, two chunks with halo planes inside the volume, borders on every side.  Against the fp64 convolution through
the shared parity cases with their own tolerances (NaN-prefilled outputs: a plane a block forgot shows), accumulating form == old + plain form bitwise, pooled maxima
and minima == MaxPool3d(2) of the output bitwise (the pooling exchange and the two uniform-descriptor stores run only here, the emulator has its own exchange), and
every launch reproducible to the bit.  The bits themselves are pinned on the CPU: tests/test_h2w_march_bits_emu.py."""
import pytest
import torch
import torch.nn.functional as F

import h2w_finish_cases as hc
import h2w_march_cases as mc
import kernel_cases as kc
from monai_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [c[0] for c in mc.CASES]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_native_lib():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from monai_amd import _lib

    assert _lib.lib().path.endswith("libmonai_amd.so")


@pytest.mark.parametrize("cname,form,n,cin,cout,dims", mc.CASES, ids=IDS)
def test_against_fp64(cname, form, n, cin, cout, dims):
    cfg = ops.conv3d_k3_h2w_config()
    if form == "pool":
        kc.case_conv3d_pool(DEV, n, cin, cout, dims, cfg=cfg)      # output and records == the plain form's, maxima / minima == MaxPool3d(2), bitwise
    elif form == "acc":
        kc.case_conv3d_accumulate(DEV, n, cin, cout, dims, cfg=cfg)
    else:
        kc.case_conv3d(DEV, cfg, n, cin, cout, dims, fused_stats=True)


@pytest.mark.parametrize("cname,form,n,cin,cout,dims", mc.CASES, ids=IDS)
def test_forms_agree_and_repeat(cname, form, n, cin, cout, dims):
    """two launches of the case's form: no NaN left, the same bits; accumulating == old + plain, one fp32 addition per voxel; pooled == MaxPool3d(2) of the output"""
    a = hc.run_case(DEV, form, n, cin, cout, dims)
    b = hc.run_case(DEV, form, n, cin, cout, dims)
    assert sorted(a) == sorted(b)
    for k in a:
        assert not bool(a[k].isnan().any()), k
        assert torch.equal(a[k], b[k]), k
    if form == "acc":
        plain = hc.run_case(DEV, "plain", n, cin, cout, dims)["out"]
        old = hc.inputs(4100 + cout + dims[0] + dims[2], n, cin, cout, dims, with_old=True)[4]
        assert torch.equal(a["out"], old + plain)
    if form == "pool":
        plain = hc.run_case(DEV, "plain", n, cin, cout, dims)
        assert torch.equal(a["out"], plain["out"]) and torch.equal(a["stats"], plain["stats"])
        assert torch.equal(a["pool_max"], F.max_pool3d(a["out"], 2)) and torch.equal(a["pool_min"], -F.max_pool3d(-a["out"], 2))
