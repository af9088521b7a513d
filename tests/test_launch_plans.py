"""-m "not gpu": the launch plan of every network engine -- which entry points a forward calls, in which order, with which configuration ids, shapes, strides
and null / non-null buffers -- is pinned to text fixtures (tests/golden/launch_plans/<network>.txt).  Nothing is launched (tests/launch_trace.py); configuration
selection is host arithmetic of the product library, so this is the plan the MI355X runs: a network that silently drops off a fast kernel, loses a fused
epilogue or re-packs its weights every forward fails here.  Two consecutive `forward_into` calls of a batch of 2 at the benchmark's window (96^3, one input
channel) per network; `python tests/test_launch_plans.py` rewrites the fixtures (do that only for a change that is MEANT to move launches)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PLANS = os.path.join(HERE, "golden", "launch_plans")
SECOND = "== second forward =="


def _make(name: str):
    """-> (network, input shape): the six networks of bench.py's NETS as bench.py constructs them, a BatchNorm UNet and a 2-D BasicUNet on one 96 x 96 plane"""
    import bench
    from monai_amd.networks.nets import BasicUNet, UNet

    if name in bench.NETS:
        return bench.build_net(name, 96, "cpu"), (2, 1, 96, 96, 96)
    torch.manual_seed(1)
    if name == "unet_batchnorm":
        return UNet(spatial_dims=3, in_channels=1, out_channels=5, channels=(16, 32, 64, 128, 256), strides=(2, 2, 2, 2), num_res_units=2, norm="batch").eval(), (2, 1, 96, 96, 96)
    return BasicUNet(spatial_dims=2, in_channels=1, out_channels=5).eval(), (2, 1, 96, 96)


NAMES = ("basicunet", "unet", "dynunet", "segresnet", "unetr", "swinunetr", "unet_batchnorm", "basicunet_2d")


def _trace(name: str) -> list:
    from launch_trace import launch_trace
    from monai_amd import config

    with launch_trace() as lines, config.conv_algo_scope("auto"):
        net, shape = _make(name)
        x = torch.zeros(shape)
        out = torch.empty((shape[0], 5) + shape[2:])
        net.forward_into(x, out)
        lines.append(SECOND)
        net.forward_into(x, out)
    return list(lines)


@pytest.mark.parametrize("name", NAMES)
def test_launch_plan(name):
    lines = _trace(name)
    with open(os.path.join(PLANS, name + ".txt")) as f:
        want = f.read().splitlines()
    assert len(lines) == len(want), (len(lines), len(want))
    for i, (a, b) in enumerate(zip(lines, want)):
        assert a == b, f"launch {i}: {a!r} != {b!r}"
    second = lines[lines.index(SECOND) + 1:]
    assert len(second) > 10
    repacked = [ln for ln in second if "_pack_" in ln.split(" ", 1)[0]]
    assert not repacked, repacked       # the per-parameter-version cache holds: no weight is packed again by the second forward


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.makedirs(PLANS, exist_ok=True)
    for nm in NAMES:
        with open(os.path.join(PLANS, nm + ".txt"), "w") as f:
            f.write("\n".join(_trace(nm)) + "\n")
