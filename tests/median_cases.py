"""Shared cases of the median filter (MedianSmooth(d), MedianFilter, median_filter, ops.median_filter) and of the kernels under them
(monai_amd/csrc/kernels/median.h); tests/test_median_emu.py runs them on the SIMT emulator, tests/test_median_gpu.py on the MI355X.

Every case is compared with the output of the reference's own classes on the CPU, stored as bits in tests/golden/median.npz
(tests/golden/make_golden_median.py, which also requires scipy.ndimage.median_filter(mode="nearest") to agree on every finite case); the inputs are
regenerated here from seeds.  A median is a selection: finite inputs have NO tolerance.  Where the reference's output is NaN (a window that holds
+-inf or NaN: the one-hot convolution multiplies it by 0) the output has to be NaN as well -- payload and sign are not compared.

Shapes: the register path (radius 1 in y and x, 0 or 1 in z) stages tiles of 16 (x) x 64 (y) x 4 (z) outputs in 3-D and 16 x 256 in 2-D; the
cases sit one below, at and one above those extents, and at two tiles plus a remainder.  The general path picks its own 256-output box per
radius; its cases use odd sizes above one box."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "median.npz")
FAST, GENERAL = 1, 2


def data(kind: str, shape, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "ties":                   # six values, negatives among them
        return rng.choice(np.array([-7.0, -2.0, 0.0, 1.0, 3.0, 250.0], np.float32), size=shape)
    if kind == "normal":
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    if kind == "negzero":                # -0.0 is the median of many windows, among negative neighbours and among positive ones
        a = rng.choice(np.array([-3.0, -0.0, -0.0, -0.0, 2.0], np.float32), size=shape)
        a.reshape(-1)[: a.size // 3] = np.where(a.reshape(-1)[: a.size // 3] > 0, np.float32(-1.0), a.reshape(-1)[: a.size // 3])
        return a
    if kind == "ones":
        return np.ones(shape, np.float32)
    raise KeyError(kind)


def _case(cid, via, shape, sd, radius, kind, passes=1, poke=None):
    return {"id": cid, "via": via, "shape": tuple(shape), "sd": sd, "radius": radius, "kind": kind, "passes": passes, "poke": poke}


def golden_cases():
    c = []
    # volumes smaller than the window (the reference's own test shapes and radii): clamped many times over
    c.append(_case("small-2x3x5-r124", "filter", (1, 1, 2, 3, 5), 3, [1, 2, 4], "normal"))
    c.append(_case("small-4x3x2-r321", "filter", (1, 1, 4, 3, 2), 3, [3, 2, 1], "ties"))
    c.append(_case("small-2x3x5-r124-ones", "filter", (1, 1, 2, 3, 5), 3, [1, 2, 4], "ones"))
    # unit axes
    c.append(_case("unit-1x1x7-r1", "filter", (1, 1, 1, 7), 3, 1, "normal"))
    c.append(_case("unit-1x9x1-r1", "filter", (1, 1, 9, 1), 3, 1, "normal"))
    c.append(_case("unit-1x9x1-r2", "filter", (1, 1, 9, 1), 3, 2, "ties"))
    # the register path around its tile extents (4 x 64 x 16), and two tiles plus a remainder on every axis; W % 4 == 0 takes the 16-byte stores
    for shape, kind in (((3, 63, 15), "normal"), ((4, 64, 16), "ties"), ((5, 65, 17), "normal"), ((9, 131, 38), "ties"), ((4, 64, 36), "negzero")):
        c.append(_case("fast3d-%dx%dx%d-%s" % (shape + (kind,)), "filter", (1,) + shape, 3, 1, kind))
    for shape, kind in (((255, 15), "normal"), ((256, 16), "ties"), ((257, 17), "ties"), ((520, 38), "ties")):
        c.append(_case("fast2d-%dx%d-%s" % (shape + (kind,)), "filter", (1,) + shape, 2, 1, kind))
    c.append(_case("fast-r011-6x70x37", "filter", (1, 6, 70, 37), 3, [0, 1, 1], "normal"))
    # n > 1
    c.append(_case("func-2x3x7x8x9-k3", "func", (2, 3, 7, 8, 9), 3, 1, "normal"))
    c.append(_case("func-2x3x7x8x9-k535", "func", (2, 3, 7, 8, 9), 3, [2, 1, 2], "ties"))
    c.append(_case("smooth-3ch-6x10x11-r1", "smooth", (3, 6, 10, 11), 3, 1, "normal"))
    c.append(_case("smooth-3ch-6x10x11-r2", "smooth", (3, 6, 10, 11), 3, 2, "ties"))
    c.append(_case("smoothd-2ch-9x70-r1", "smoothd", (2, 9, 70), 2, 1, "normal"))
    c.append(_case("smoothd-2ch-9x10-r01", "smoothd", (2, 9, 10), 2, [0, 1], "ties"))
    # 2-D and 1-D
    c.append(_case("2d-12x13-r21", "filter", (2, 12, 13), 2, [2, 1], "normal"))
    c.append(_case("1d-40-r1", "filter", (2, 3, 40), 1, 1, "normal"))
    c.append(_case("1d-300-r3", "filter", (2, 300), 1, 3, "ties"))
    # radii on one volume, all three kinds of data
    for radius in (1, 2, 3, [1, 2, 3], [0, 1, 1]):
        for kind in ("ties", "normal", "negzero"):
            rid = "".join(str(r) for r in radius) if isinstance(radius, list) else str(radius)
            c.append(_case("radii-9x10x11-r%s-%s" % (rid, kind), "filter", (1, 9, 10, 11), 3, radius, kind))
    c.append(_case("general-10x19x21-r2", "filter", (1, 10, 19, 21), 3, 2, "normal"))
    # repeated passes
    c.append(_case("passes2-5x9x11-r1", "filter", (2, 5, 9, 11), 3, 1, "normal", passes=2))
    c.append(_case("passes2-5x9x11-r121", "filter", (1, 5, 9, 11), 3, [1, 2, 1], "ties", passes=2))
    c.append(_case("passes3-9x70-r1", "filter", (1, 9, 70), 2, 1, "normal", passes=3))
    # one non-finite value in an otherwise finite volume, at a corner and in the interior, on both paths
    for name, value in (("pinf", np.inf), ("ninf", -np.inf), ("nan", np.nan)):
        for where, at in (("corner", (0, 0, 0, 0)), ("interior", (0, 3, 4, 5)), ("far", (0, 5, 8, 9))):
            for radius in (1, 2):
                c.append(_case("nonfinite-%s-%s-r%d" % (name, where, radius), "filter", (1, 6, 9, 10), 3, radius, "normal", poke=(at, value)))
    return c


_inputs_cache: dict = {}


def inputs(case) -> np.ndarray:
    cid = case["id"]
    if cid not in _inputs_cache:
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % 100003
        a = data(case["kind"], case["shape"], seed).copy()
        if case["poke"] is not None:
            a[case["poke"][0]] = case["poke"][1]
        a.setflags(write=False)
        _inputs_cache[cid] = a
    return _inputs_cache[cid]


def radius3(case):
    sd, r = case["sd"], case["radius"]
    r = list(r) if isinstance(r, list) else [r] * sd
    return [0] * (3 - sd) + r


def expected_path(case) -> int:
    """the kernel the host has to choose: the register network for radius 1 in y and x and 0 or 1 in z, the bisection kernel otherwise"""
    rz, ry, rx = radius3(case)
    return FAST if (rx == 1 and ry == 1 and rz <= 1) else GENERAL


def run_case(layers, transforms, case, dev):
    """the case's output from `layers` / `transforms`: the reference's monai.networks.layers / monai.transforms, or the product's"""
    x = torch.from_numpy(inputs(case).copy()).to(dev)
    before = x.clone()
    via, r, sd = case["via"], case["radius"], case["sd"]
    if via == "filter":
        out = layers.MedianFilter(r, spatial_dims=sd)(x, number_of_passes=case["passes"]) if case["passes"] != 1 else layers.MedianFilter(r, spatial_dims=sd)(x)
    elif via == "func":
        k = [2 * v + 1 for v in r] if isinstance(r, list) else 2 * r + 1
        out = layers.median_filter(x, kernel_size=k, spatial_dims=sd)
    elif via == "smooth":
        out = transforms.MedianSmooth(radius=r)(x)
    else:
        out = transforms.MedianSmoothd(keys="img", radius=r)({"img": x, "other": 1})
        assert out["other"] == 1
        out = out["img"]
    assert torch.equal(x.cpu().view(torch.int32), before.cpu().view(torch.int32)), "the input was modified"
    return out


_golden_cache: dict = {}


def golden():
    if not _golden_cache:
        with np.load(GOLDEN) as z:
            _golden_cache.update({k: z[k] for k in z.files})
    return _golden_cache


def same_as_reference(got: np.ndarray, want_bits: np.ndarray) -> bool:
    """NaN exactly where the reference has NaN, the reference's bits everywhere else"""
    want = want_bits.view(np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want_bits[~nan]))


def case_golden(dev, select) -> set:
    """every golden case whose id `select` accepts: the reference's output, twice with the same bits, on the path the host is expected to choose;
    returns the paths taken"""
    import monai_amd.networks.layers as layers
    import monai_amd.transforms as transforms
    from monai_amd import ops

    g = golden()
    assert json.loads(str(g["manifest"])) == [c["id"] for c in golden_cases()], "tests/golden/median.npz is stale: run make_golden_median.py"
    paths = set()
    for case in golden_cases():
        if not select(case["id"]):
            continue
        path = ops.median_filter_path(case["shape"][len(case["shape"]) - case["sd"]:], radius3(case)[3 - case["sd"]:])
        assert path == expected_path(case), (case["id"], path)
        paths.add(path)
        outs = [run_case(layers, transforms, case, dev) for _ in range(2)]
        a, b = (torch.as_tensor(o).cpu().numpy() for o in outs)
        assert a.dtype == np.float32 and a.shape == case["shape"], (case["id"], a.dtype, a.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ("not the same bits twice", case["id"])
        assert same_as_reference(a, g[case["id"]]), (case["id"], int((a.view(np.uint32) != g[case["id"]]).sum()))
        assert not np.signbit(a[a == 0]).any(), ("a selected zero is +0.0", case["id"])
    return paths


def case_api(dev) -> None:
    import pytest
    import monai_amd.networks.layers as layers
    import monai_amd.transforms as ours
    from monai_amd import ops
    from monai_amd._fallback import UnsupportedOnDevice
    from monai_amd.data.meta_tensor import MetaTensor

    f = layers.MedianFilter([1, 2, 4])
    assert tuple(f.radius) == (1, 2, 4) and list(f.window) == [3, 5, 9] and f.spatial_dims == 3 and isinstance(f, torch.nn.Module)
    k = f.kernel
    assert k.shape == (135, 1, 3, 5, 9) and k.dtype == torch.float32 and torch.equal(k.reshape(135, 135), torch.eye(135))
    assert tuple(layers.MedianFilter(2, spatial_dims=2).radius) == (2, 2)
    with pytest.raises(ValueError):
        layers.MedianFilter([3, 2])
    with pytest.raises(TypeError, match="Input type is not a torch.Tensor"):
        layers.median_filter(np.zeros((3, 3, 3), np.float32))
    x = torch.from_numpy(data("normal", (2, 5, 6, 7), 5)).to(dev)
    want = layers.MedianFilter(1)(x)
    assert type(want) is torch.Tensor and want.dtype == torch.float32 and want.shape == x.shape
    # the function form: default 3 x 3 x 3, an explicit box kernel, the public op
    for got in (layers.median_filter(x), layers.median_filter(x, kernel=layers.MedianFilter(1).kernel), ops.median_filter(x, 1),
                ops.median_filter(x, [1, 1, 1], spatial_dims=3, passes=1), layers.MedianFilter(1)(x, number_of_passes=1)):
        assert torch.equal(got, want)
    assert torch.equal(ops.median_filter(x, 1, passes=2), layers.MedianFilter(1)(want))
    assert layers.MedianFilter(1)(x, number_of_passes=0) is x
    # what is not on the HIP path says so (and goes to the reference where MONAI is importable)
    with pytest.raises(NotImplementedError, match="one-hot box kernel"):
        layers.median_filter(x, kernel=torch.ones(27, 1, 3, 3, 3))
    with pytest.raises(NotImplementedError, match="kernel sizes"):
        layers.median_filter(x, kernel_size=(3, 4, 3))
    with pytest.raises(NotImplementedError, match="convolution arguments"):
        layers.median_filter(x, dilation=2)
    for bad in (x.double(), x.half(), x.to(torch.int32)):
        with pytest.raises(UnsupportedOnDevice):
            ops.median_filter(bad, 1)
        with pytest.raises(UnsupportedOnDevice):
            layers.MedianFilter(1)(bad)
    with pytest.raises(UnsupportedOnDevice, match="window of 441 values"):
        ops.median_filter(x, [4, 3, 3])
    with pytest.raises(UnsupportedOnDevice, match="spatial_dims"):
        ops.median_filter(x, 1, spatial_dims=4)
    with pytest.raises(ValueError):
        ops.median_filter(x, [1, 1])
    with pytest.raises(ValueError):
        ops.median_filter(x, [1, -1, 1])
    # MedianSmooth(d): float32 out of any real input, MetaTensor in / MetaTensor out with meta and applied operations kept
    s = ours.MedianSmooth(radius=1)
    assert s.radius == 1 and ours.MedianSmooth().radius == 1
    assert torch.equal(s(x), layers.MedianFilter(1, spatial_dims=3)(x))
    xi = (x * 0.1).to(torch.int16)
    assert s(xi).dtype == torch.float32 and torch.equal(s(xi), s(xi.to(torch.float32)))
    m = MetaTensor(x.clone(), meta={"affine": torch.eye(4), "name": "case"}, applied_operations=[{"class": "Earlier"}])
    out = s(m)
    assert isinstance(out, MetaTensor) and out.meta["name"] == "case" and torch.equal(torch.as_tensor(out.meta["affine"]), torch.eye(4))
    assert out.applied_operations == [{"class": "Earlier"}] and torch.equal(out.as_tensor(), s(x)) and torch.equal(m.as_tensor(), x)
    assert ours.MedianSmoothD is ours.MedianSmoothDict is ours.MedianSmoothd
    d = ours.MedianSmoothd(keys=("img", "absent"), radius=[1, 1, 1], allow_missing_keys=True)({"img": x, "n": 3})
    assert set(d) == {"img", "n"} and d["n"] == 3 and torch.equal(d["img"], s(x)) and isinstance(ours.MedianSmoothd("img", 1).converter, ours.MedianSmooth)
    with pytest.raises(KeyError, match="was missing in the data and allow_missing_keys==False"):
        ours.MedianSmoothd(keys=("img", "absent"), radius=1)({"img": x})
    with pytest.raises(ValueError):
        ours.MedianSmooth(radius=[1, 1])(x)          # three spatial axes
