"""-m gpu: the finishing step of conv3d_k3_h2w_kernel (csrc/kernels/conv3d_wino_h2.h) with whole 64-byte output rows per lane quad, on the MI355X: every lane
loads, adds and stores ITS piece (accumulating identity, bitwise), no piece is left out (NaN-prefilled outputs through the shared parity cases), and a launch
is reproducible to the bit (the statistics leaves are merged in one fixed tree).  The bits themselves are pinned on the CPU: tests/test_h2w_finish_bits_emu.py."""
import pytest
import torch

import h2w_finish_cases as hc
import kernel_cases as kc
from monai_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_native_lib():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from monai_amd import _lib

    assert _lib.lib().path.endswith("libmonai_amd.so")


def _launch(x, nrm, packed, b, out, accumulate=False):
    cfg = ops.conv3d_k3_h2w_config()
    stats = torch.full((out.shape[0], out.shape[1], ops.conv3d_k3_stat_tiles(cfg, *out.shape[2:]), 3), float("nan"), device=DEV)
    ops.conv3d_k3(cfg, x, nrm, packed, b, out, stats, accumulate=accumulate)
    return stats


# 2 x 2 regions with borders on every side, two cout groups, two samples | two z-chunks of one region
@pytest.mark.parametrize("n,cin,cout,dims", [(2, 32, 64, (5, 8, 32)), (1, 32, 32, (24, 4, 16))])
def test_accumulating_form_adds_its_own_piece(n, cin, cout, dims):
    """acc_out == old + plain_out, one fp32 addition per voxel, bitwise: a lane that loads or stores another lane's piece fails here;
    and a second launch of either form on the same input gives the same output and the same statistics records, bit for bit"""
    x, w, b, nrm, old = hc.inputs(900 + cout + dims[0], n, cin, cout, dims, with_old=True)
    x, b, nrm = x.to(DEV), b.to(DEV), nrm.to(DEV)
    packed = ops.conv3d_k3_pack(ops.conv3d_k3_h2w_config(), w.to(DEV))
    plain = torch.full((n, cout) + tuple(dims), float("nan"), device=DEV)
    st_plain = _launch(x, nrm, packed, b, plain)
    assert not bool(plain.isnan().any()) and not bool(st_plain.isnan().any())
    acc = old.clone().to(DEV)
    st_acc = _launch(x, nrm, packed, b, acc, accumulate=True)
    assert torch.equal(acc.cpu(), old + plain.cpu())
    assert not bool(st_acc.isnan().any())

    plain2 = torch.full_like(plain, float("nan"))
    st_plain2 = _launch(x, nrm, packed, b, plain2)
    assert torch.equal(plain2, plain) and torch.equal(st_plain2, st_plain)
    acc2 = old.clone().to(DEV)
    st_acc2 = _launch(x, nrm, packed, b, acc2, accumulate=True)
    assert torch.equal(acc2, acc) and torch.equal(st_acc2, st_acc)


def test_no_piece_left_out_plain_and_pooling():
    """NaN-prefilled outputs, statistics, pooled maxima and minima through the shared parity cases: two samples, two cout groups, 2 x 2 regions, even depth"""
    cfg = ops.conv3d_k3_h2w_config()
    kc.case_conv3d(DEV, cfg, 2, 32, 64, (4, 8, 32), fused_stats=True)
    kc.case_conv3d_pool(DEV, 2, 32, 64, (4, 8, 32), cfg=cfg)


def test_pooling_form_is_reproducible():
    """two launches of the pooling form on the same input: bit-equal output, statistics, maxima and minima"""
    a = hc.run_case(DEV, "pool", 2, 32, 64, (4, 8, 32))
    b = hc.run_case(DEV, "pool", 2, 32, 64, (4, 8, 32))
    assert sorted(a) == sorted(b) == ["out", "pool_max", "pool_min", "stats"]
    for k in a:
        assert not bool(a[k].isnan().any()) and torch.equal(a[k], b[k]), k
