"""Shared cases of spline-order resampling (integer `mode` of Spacing(d) / SpatialResample / Resample / lazy resampling, ops.spline_prefilter /
ops.spline_resample) and of the kernels under them (monai_amd/csrc/kernels/spline.h); tests/test_spline_emu.py runs them on the SIMT emulator,
tests/test_spline_gpu.py on the MI355X.

Expected values come from tests/golden/spline.npz (tests/golden/make_golden_spline.py): the fp32 output bits of the reference's own classes on the
CPU -- which the script requires to be the fp32 cast of scipy.ndimage.map_coordinates on the reference's dense grid -- of scipy.ndimage.map_coordinates
itself for the kernel-level cases, and scipy.ndimage.spline_filter's float64 output for the prefilter.  Inputs and coordinates are regenerated from seeds.

Acceptance per voxel: |out - golden| <= spacing32(|golden|) + 2^-36 max|input| -- both sides are fp64 computations rounded once to fp32, so they differ
by at most one fp32 step; the floor is fp64 round-off (2^-53) with 2^17 of headroom for operation count, filter gain and coordinate round-off, still
2^13 below fp32's epsilon.  Prefilter outputs use the floor alone.  Every case runs twice and has to give identical bits.

A last-bit coordinate difference flips a voxel at three kinds of points: order 0 at half-integers, `constant` at 0 and n - 1, `grid-constant` at the pad
extent.  On cases whose coordinates are not exact the golden file carries a mask of the voxels whose reference coordinate lies within 1e-9 of such a
point (at most 0.1 % of a case, asserted when the file is made); they are left out.  The exact-coordinate cases leave nothing out.

Shapes: a line of at most 48 samples takes the closed-form start of the half-sample-symmetric prefilter, a longer one the 48-sample warm-up: lines of
2, 3, 5, 13, 48, 49 and 150 samples; odd shapes such as 5 x 65 x 17; 2-D images; 1 and 3 channels."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "spline.npz")
MODES = ("reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap")
FLOOR = 2.0 ** -36


def _seed(cid: str) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % 100003


def data(shape, seed: int) -> np.ndarray:
    a = (np.random.default_rng(seed).standard_normal(shape) * 100).astype(np.float32)
    a.setflags(write=False)
    return a


def rot(deg_z: float, shear: float = 0.0) -> np.ndarray:
    """4 x 4: rotation about the first axis by deg_z, then a shear of the last axis by the second"""
    t = np.deg2rad(deg_z)
    r = np.eye(4)
    r[1, 1], r[1, 2], r[2, 1], r[2, 2] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    s = np.eye(4)
    s[2, 1] = shear
    return r @ s


# ------------------------------------------------------------------------------------------------------------------ kernel-level cases
def prefilter_cases():
    c = []
    for order in (2, 3, 4, 5):
        for mode in MODES:
            c.append({"id": "pre-o%d-%s-3x13x5" % (order, mode), "shape": (1, 3, 13, 5), "order": order, "mode": mode, "rank": 3})
    for order, mode in ((3, "reflect"), (5, "mirror"), (4, "grid-wrap"), (5, "reflect")):
        c.append({"id": "pre-o%d-%s-2x150x3" % (order, mode), "shape": (1, 2, 150, 3), "order": order, "mode": mode, "rank": 3})
    c.append({"id": "pre-o5-nearest-2d-150x3", "shape": (1, 1, 150, 3), "order": 5, "mode": "nearest", "rank": 2})
    c.append({"id": "pre-o3-nearest-2d-9x6", "shape": (3, 1, 9, 6), "order": 3, "mode": "nearest", "rank": 2})
    for order, mode in ((3, "reflect"), (5, "grid-mirror")):
        c.append({"id": "pre-o%d-%s-49x2x48" % (order, mode), "shape": (1, 49, 2, 48), "order": order, "mode": mode, "rank": 3})
    c.append({"id": "pre-o3-grid-constant-2d-9x6", "shape": (3, 1, 9, 6), "order": 3, "mode": "grid-constant", "rank": 2})
    c.append({"id": "pre-o5-wrap-2d-9x6", "shape": (3, 1, 9, 6), "order": 5, "mode": "wrap", "rank": 2})
    return c


PRE_CROP = 3


def prefilter_crop(case, coef: np.ndarray) -> np.ndarray:
    """what the golden file holds of a case's coefficients: everything, except for the 3-D cases of the padding modes (24 more samples per axis: 230 KB
    each), of which it holds the image's own box and PRE_CROP samples of the pad around it -- the pad out to its end is compared on the 2-D cases, and
    sampled at the pad extent by the kernel-level cases"""
    if case["rank"] == 2 or case["mode"] not in ("nearest", "grid-constant"):
        return coef
    lo = 12 - PRE_CROP
    return coef[:, lo:coef.shape[1] - lo, lo:coef.shape[2] - lo, lo:coef.shape[3] - lo]


def sample_cases():
    """ops.spline_resample on a dense fp64 grid against scipy.ndimage.map_coordinates: every order x every mode, random coordinates up to four periods
    outside, half-integer coordinates (exact: nothing left out), one far point per sign"""
    c = []
    for order in range(6):
        for mode in MODES:
            c.append({"id": "ops-o%d-%s-5x13x7" % (order, mode), "shape": (2, 5, 13, 7), "order": order, "mode": mode, "rank": 3, "npts": (300, 160)})
    for order, mode in ((3, "reflect"), (3, "nearest"), (5, "grid-constant"), (2, "wrap"), (0, "constant"), (1, "grid-wrap")):
        c.append({"id": "ops-o%d-%s-2d-9x6" % (order, mode), "shape": (3, 1, 9, 6), "order": order, "mode": mode, "rank": 2, "npts": (300, 200)})
    for order, mode in ((3, "mirror"), (5, "reflect"), (4, "nearest")):
        c.append({"id": "ops-o%d-%s-2x3x150" % (order, mode), "shape": (1, 2, 3, 150), "order": order, "mode": mode, "rank": 3, "npts": (300, 200)})
    return c


def sample_coords(case):
    """(coords [3, n] fp64, exact [n] bool): the first block random, the second on half-integers (exact in every implementation), then two far points"""
    rng = np.random.default_rng(_seed(case["id"]) + 7)
    shape = case["shape"][1:]
    nr, ne = case["npts"]
    co = np.stack([rng.uniform(-3.2 * n, 4.2 * n, nr) for n in shape])
    ex = np.stack([rng.integers(-6 * n - 2, 8 * n + 2, ne) * 0.5 for n in shape])
    # the boundary points themselves, in every combination with interior points
    for a, n in enumerate(shape):
        k = min(ne, 12)
        ex[a, :k] = np.resize(np.array([0.0, n - 1.0, -0.5, n - 0.5, -1.0, float(n), 0.5, n - 1.5, -12.0, n + 11.0, -12.5, n + 11.5]), k)
    far = np.stack([np.array([1.0e6 + 0.25, -1.0e6 - 0.25]) for _ in shape])
    co = np.concatenate([co, ex, far], axis=1)
    if case["rank"] == 2:
        co[0] = 0.0
    exact = np.zeros(co.shape[1], bool)
    exact[nr:nr + ne] = True
    return co, exact


def near_discontinuity(co, shape, order, mode, rank, tol=1e-9):
    """voxels whose coordinate lies within `tol` of a point where the result jumps: order 0 at half-integers, `constant` at 0 and n - 1 (any order),
    `grid-constant` at the extent of the (padded) support"""
    hit = np.zeros(co.shape[1], bool)
    for a in range(3 - rank, 3):
        x, n = co[a], shape[a]
        if order == 0:
            hit |= np.abs(x - np.floor(x) - 0.5) < tol
        if mode == "constant":
            hit |= (np.abs(x) < tol) | (np.abs(x - (n - 1)) < tol)
        if mode == "grid-constant":
            pad = 12 if order > 1 else 0
            for edge in (-pad - (order + 1) / 2.0, n - 1 + pad + (order + 1) / 2.0):
                hit |= np.abs(x - edge) < tol
    return hit


# ------------------------------------------------------------------------------------------------------------------ transform-level cases
def transform_cases():
    c = []

    def add(cid, via, shape, order, pad, **kw):
        d = {"id": cid, "via": via, "shape": tuple(shape), "order": order, "pad": pad, "ac": False, "dtype": None, "exact": False}
        d.update(kw)
        c.append(d)

    iso = np.diag([1.3, 0.7, 1.1, 1.0])
    # Spacing: up- and down-sampling by non-dyadic ratios, both align_corners, every order at least once, the grid_sample padding names
    # (`constant` is left to the rotated SpatialResample cases: an axis-aligned resampling puts whole output planes on index 0 or n - 1, where a last-bit
    # difference of the coordinate decides between the value and 0 -- in the reference too)
    for order, pad, ac in ((3, "border", False), (3, "border", True), (0, "border", False), (1, "reflection", False), (2, "nearest", True), (4, "mirror", False),
                           (5, "grid-wrap", False), (3, "grid-constant", False), (3, "reflect", True), (5, "wrap", False), (2, "grid-mirror", False)):
        add("spacing-o%d-%s-ac%d-5x23x9" % (order, pad, ac), "spacing", (1, 5, 23, 9), order, pad, ac=ac, affine=iso,
            pixdim=(1.0, 1.3, 0.9) if order else (0.93, 1.37, 0.81))      # order 0: no output plane on a half-integer coordinate
    add("spacing-o3-border-5x65x17", "spacing", (1, 5, 65, 17), 3, "border", affine=iso, pixdim=(1.0, 1.3, 0.9))
    add("spacing-o3-border-3ch-13x9x11", "spacing", (3, 13, 9, 11), 3, "border", affine=iso, pixdim=(1.0, 1.0, 1.0))
    add("spacing-o3-border-150x3x2", "spacing", (1, 150, 3, 2), 3, "border", affine=np.diag([0.7, 1.0, 1.0, 1.0]), pixdim=(2.1, 1.0, 1.0))
    add("spacing-o5-reflect-49x48x2", "spacing", (1, 49, 48, 2), 5, "reflect", affine=np.diag([1.3, 1.3, 1.0, 1.0]), pixdim=(2.0, 2.0, 1.0))
    add("spacing-o3-border-2d-33x21", "spacing", (2, 33, 21), 3, "border", affine=np.diag([1.3, 0.7, 1.0, 1.0]), pixdim=(1.0, 1.0))
    add("spacing-o3-border-f32-7x23x9", "spacing", (1, 7, 23, 9), 3, "border", affine=iso, pixdim=(1.0, 1.0, 1.0), dtype="float32")
    add("spacing-o1-border-f32-7x23x9", "spacing", (1, 7, 23, 9), 1, "border", affine=iso, pixdim=(1.0, 1.0, 1.0), dtype="float32", ac=True)
    # SpatialResample: rotation and shear, 3-D and 2-D
    src = rot(0.0) @ np.diag([1.3, 0.7, 1.1, 1.0])
    dst = rot(25.0, 0.2) @ np.diag([1.0, 1.0, 1.0, 1.0])
    dst[:3, 3] = (-1.5, 4.0, -3.0)
    for order, pad, ac in ((3, "border", False), (3, "reflection", True), (5, "zeros", False), (0, "border", False), (2, "grid-wrap", True), (4, "wrap", False),
                           (1, "grid-constant", False), (3, "mirror", False), (0, "constant", False), (3, "zeros", True)):
        add("sresample-o%d-%s-ac%d-5x13x17" % (order, pad, ac), "sresample", (1, 5, 13, 17), order, pad, ac=ac, affine=src, dst=dst, size=(7, 12, 15))
    t2 = np.deg2rad(-17.0)
    dst2 = np.array([[np.cos(t2), -np.sin(t2), 2.0], [np.sin(t2), np.cos(t2), -1.0], [0, 0, 1.0]]) @ np.diag([0.8, 1.25, 1.0])
    add("sresample-o3-border-2d-13x20", "sresample", (2, 13, 20), 3, "border", affine=np.eye(3), dst=dst2, size=(16, 18))
    add("sresample-o3-zeros-2d-ac1-13x20", "sresample", (2, 13, 20), 3, "zeros", ac=True, affine=np.eye(3), dst=dst2, size=(16, 18))
    # exact coordinates: index = 0.5 o - (1, 2, 1.5) lands on integers and half-integers, on 0 and n - 1 of every axis, before and after the volume;
    # nothing is left out (several periods outside: the half-integer block of the kernel-level cases)
    half = np.diag([0.5, 0.5, 0.5, 1.0])
    half[:3, 3] = (-1.0, -2.0, -1.5)
    for order in range(6):
        for pad in MODES:
            add("exact-o%d-%s-3x5x4" % (order, pad), "sresample", (1, 3, 5, 4), order, pad, affine=np.eye(4), dst=half, size=(8, 14, 10), exact=True)
    shift = np.eye(4)
    shift[:3, 3] = (-3.0, 2.0, -40.0)
    add("exact-shift-o3-border-5x13x7", "sresample", (1, 5, 13, 7), 3, "border", affine=np.eye(4), dst=shift, size=(9, 13, 60), exact=True)
    # Resample with an explicit grid: norm_coords / align_corners in all four combinations, 3-D and 2-D, an fp32 grid
    for nc_, ac in ((True, False), (True, True), (False, False), (False, True)):
        add("resample-o3-nearest-nc%d-ac%d-6x9x8" % (nc_, ac), "resample", (2, 6, 9, 8), 3, "nearest", ac=ac, norm=nc_, gshape=(5, 11, 7))
    add("resample-o2-reflection-2d-9x8", "resample", (2, 9, 8), 2, "reflection", norm=True, gshape=(11, 7))
    add("resample-o5-grid-mirror-6x9x8", "resample", (1, 6, 9, 8), 5, "grid-mirror", norm=True, gshape=(5, 11, 7))
    add("resample-o0-border-6x9x8", "resample", (1, 6, 9, 8), 0, "border", norm=True, gshape=(5, 11, 7))
    # lazy: Spacing(lazy) then SpatialPad(lazy), executed once with the spline order as an override; equal to ...
    add("lazy-o3-border-6x20x9", "lazy", (1, 6, 20, 9), 3, "border", affine=iso, pixdim=(1.0, 1.0, 1.0), size=(10, 16, 12))
    add("lazy-o0-border-6x20x9", "lazy", (1, 6, 20, 9), 0, "border", affine=iso, pixdim=(0.93, 1.37, 0.81), size=(10, 16, 12))
    # inverse of a Spacing made with an integer mode
    add("inverse-o3-border-5x21x8", "inverse", (1, 5, 21, 8), 3, "border", affine=iso, pixdim=(1.0, 1.0, 1.0))
    add("inverse-o2-reflection-ac1-5x21x8", "inverse", (1, 5, 21, 8), 2, "reflection", ac=True, affine=iso, pixdim=(1.0, 1.0, 1.0))
    # Spacingd with per-key modes
    add("spacingd-o3-nearest-5x21x8", "spacingd", (1, 5, 21, 8), 3, "border", affine=iso, pixdim=(1.0, 1.0, 1.0))
    return c


_inputs_cache: dict = {}


def inputs(case) -> np.ndarray:
    cid = case["id"]
    if cid not in _inputs_cache:
        _inputs_cache[cid] = data(case["shape"], _seed(cid))
    return _inputs_cache[cid]


def resample_grid(case) -> np.ndarray:
    """the explicit grid of a `resample` case: a rotated, scaled, slightly warped centred grid (fp64), partly outside the image"""
    rng = np.random.default_rng(_seed(case["id"]) + 3)
    gs = case["gshape"]
    sr = len(gs)
    axes = np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in gs], indexing="ij")
    g = np.stack(axes)
    t = np.deg2rad(20.0)
    m = np.eye(sr)
    m[-2:, -2:] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
    g = np.tensordot(m * 1.15, g, axes=1) + rng.uniform(-0.3, 0.3, g.shape)
    if not case["norm"]:          # already normalised to [-1, 1] (and beyond)
        g = g / np.array([(n - 1) / 2.0 for n in case["shape"][1:]]).reshape((sr,) + (1,) * sr) * 1.1
    return np.concatenate([g, np.ones((1,) + tuple(gs))])


class Namespace:
    """the transforms under test: the reference's (monai.*) when the goldens are made, the product's in the tests"""

    def __init__(self, which: str):
        if which == "reference":
            import monai.transforms as t
            from monai.data import MetaTensor
            from monai.transforms.lazy.functional import apply_pending
        else:
            import monai_amd.transforms as t
            from monai_amd.data.meta_tensor import MetaTensor
            from monai_amd.transforms.lazy import apply_pending
        self.t, self.MetaTensor, self.apply_pending = t, MetaTensor, apply_pending


def run_transform(ns: Namespace, case, dev, dtype_override="case"):
    """the case's output(s) as a list of tensors / MetaTensors"""
    t = ns.t
    x = torch.from_numpy(inputs(case).copy()).to(dev)
    dt = case["dtype"] if dtype_override == "case" else dtype_override
    dtype = {None: np.float64, "float32": np.float32, "float64": np.float64}[dt]
    via, order, pad, ac = case["via"], case["order"], case["pad"], case["ac"]
    if via == "resample":
        g = torch.from_numpy(resample_grid(case)).to(dev)
        if case.get("grid32"):
            g = g.float()
        return [t.Resample(mode=order, padding_mode=pad, norm_coords=case["norm"], align_corners=ac, dtype=dtype)(x, grid=g)]
    img = ns.MetaTensor(x, affine=torch.as_tensor(case["affine"], dtype=torch.float64))
    if via == "spacing":
        return [t.Spacing(pixdim=case["pixdim"], mode=order, padding_mode=pad, align_corners=ac, dtype=dtype)(img)]
    if via == "sresample":
        return [t.SpatialResample(mode=order, padding_mode=pad, align_corners=ac, dtype=dtype)(img, dst_affine=torch.as_tensor(case["dst"], dtype=torch.float64),
                                                                                              spatial_size=case["size"])]
    if via == "lazy":
        y = t.Spacing(pixdim=case["pixdim"], lazy=True)(img)
        y = t.SpatialPad(spatial_size=case["size"], lazy=True)(y)
        assert len(y.pending_operations) == 2
        out = ns.apply_pending(y, overrides={"mode": order, "padding_mode": pad})
        return [out[0] if isinstance(out, tuple) else out]
    if via == "inverse":
        tr = t.Spacing(pixdim=case["pixdim"], mode=order, padding_mode=pad, align_corners=ac, dtype=dtype)
        fwd = tr(img)
        return [fwd, tr.inverse(fwd)]
    if via == "spacingd":
        lab = ns.MetaTensor((x > 0).to(torch.float32), affine=torch.as_tensor(case["affine"], dtype=torch.float64))
        d = t.Spacingd(keys=["image", "label"], pixdim=case["pixdim"], mode=(order, "nearest"), padding_mode=(pad, "border"))({"image": img, "label": lab})
        return [d["image"], d["label"]]
    raise KeyError(via)


# ------------------------------------------------------------------------------------------------------------------ checks
_golden_cache: dict = {}


def golden():
    if not _golden_cache:
        with np.load(GOLDEN) as z:
            _golden_cache.update({k: z[k] for k in z.files})
        ids = [c["id"] for c in prefilter_cases() + sample_cases() + transform_cases()]
        assert json.loads(str(_golden_cache["manifest"])) == ids, "tests/golden/spline.npz is stale: run make_golden_spline.py"
    return _golden_cache


def close(got: np.ndarray, want_bits: np.ndarray, scale: float, skip=None) -> tuple:
    """(ok, worst excess in units of the tolerance, voxels compared) under the acceptance rule of the module docstring"""
    want = want_bits.view(np.float32).astype(np.float64)
    tol = np.spacing(np.abs(want_bits.view(np.float32))).astype(np.float64) + FLOOR * scale
    err = np.abs(got.astype(np.float64) - want)
    nan = np.isnan(want)
    keep = ~nan if skip is None else (~nan & ~skip)
    ok = np.array_equal(np.isnan(got), nan) and bool((err[keep] <= tol[keep]).all())
    return ok, float((err[keep] / tol[keep]).max()) if keep.any() else 0.0, int(keep.sum())


def _mask(g, cid, n):
    key = cid + ":skip"
    return np.unpackbits(g[key])[:n].astype(bool) if key in g else None


def case_prefilter(dev, select) -> int:
    from monai_amd import ops

    g, n = golden(), 0
    for case in prefilter_cases():
        if not select(case["id"]):
            continue
        x = inputs(case)
        outs = [ops.spline_prefilter(torch.from_numpy(x.copy()).to(dev), case["order"], case["mode"], rank=case["rank"]).cpu().numpy() for _ in range(2)]
        want = g[case["id"]]
        full = (x.shape[0],) + tuple(n + (24 if case["mode"] in ("nearest", "grid-constant") and a >= 3 - case["rank"] else 0) for a, n in enumerate(x.shape[1:]))
        assert outs[0].shape == full, (case["id"], outs[0].shape, full)
        outs = [prefilter_crop(case, o) for o in outs]
        assert outs[0].dtype == np.float64 and outs[0].shape == want.shape, (case["id"], outs[0].shape, want.shape)
        assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), ("not the same bits twice", case["id"])
        err = float(np.abs(outs[0] - want).max())
        print(case["id"], "max error %.3g, bound %.3g" % (err, FLOOR * float(np.abs(x).max())))
        assert err <= FLOOR * float(np.abs(x).max()), (case["id"], err)
        n += 1
    return n


def case_samples(dev, select) -> int:
    from monai_amd import ops

    g, n = golden(), 0
    for case in sample_cases():
        if not select(case["id"]):
            continue
        x = inputs(case)
        co, exact = sample_coords(case)
        grid = torch.from_numpy(co.reshape(3, 1, 1, -1).copy()).to(dev)
        outs = [ops.spline_resample(torch.from_numpy(x.copy()).to(dev), case["order"], case["mode"], coords=grid, rank=case["rank"]).cpu().numpy().reshape(x.shape[0], -1)
                for _ in range(2)]
        assert outs[0].dtype == np.float32
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), ("not the same bits twice", case["id"])
        skip = near_discontinuity(co, case["shape"][1:], case["order"], case["mode"], case["rank"]) & ~exact
        assert skip.mean() <= 0.001, (case["id"], skip.mean())
        ok, worst, cnt = close(outs[0], g[case["id"]], float(np.abs(x).max()), np.broadcast_to(skip, outs[0].shape))
        print(case["id"], "worst error / tolerance %.3g over %d values" % (worst, cnt))
        assert ok, (case["id"], worst)
        n += 1
    return n


def case_transforms(dev, select) -> int:
    g, n = golden(), 0
    ns = Namespace("product")
    for case in transform_cases():
        if not select(case["id"]):
            continue
        cid = case["id"]
        x = inputs(case)
        runs = [run_transform(ns, case, dev) for _ in range(2)]
        for k, (a, b) in enumerate(zip(*runs)):
            key = cid if k == 0 else "%s:%d" % (cid, k)
            an, bn = torch.as_tensor(a).cpu().numpy(), torch.as_tensor(b).cpu().numpy()
            want = g[key]
            assert an.dtype == np.float32 and an.shape == want.shape, (key, an.dtype, an.shape, want.shape)
            assert np.array_equal(an.view(np.uint32), bn.view(np.uint32)), ("not the same bits twice", key)
            if cid.startswith("spacingd") and k == 1:          # the label: the nearest-neighbour kernel that was there before
                assert np.array_equal(an.view(np.uint32), want), key
                continue
            if case["dtype"] == "float32":
                # the reference computes its grid in float32 here; the product's float64 coordinates lie inside the reference's own float32 / float64 spread,
                # of which the golden file holds a one-sided measurement: twice that
                spread = float(g[cid + ":spread"])
                err = float(np.abs(an.astype(np.float64) - want.view(np.float32)).max())
                print(key, "max error %.3g, reference spread %.3g" % (err, spread))
                assert err <= 2.0 * spread, (key, err, spread)
                continue
            skip = _mask(g, key, an.size)
            assert not (case["exact"] and skip is not None)
            ok, worst, cnt = close(an.reshape(-1), want.reshape(-1), float(np.abs(x).max()), skip)
            print(key, "worst error / tolerance %.3g over %d of %d values" % (worst, cnt, an.size))
            assert ok, (key, worst)
            if hasattr(a, "affine") and (key + ":affine") in g:
                assert np.allclose(np.asarray(a.affine.cpu(), dtype=np.float64), g[key + ":affine"], rtol=0, atol=1e-12), key
        n += 1
    return n


def case_api(dev) -> None:
    """what the feature adds on the public surface, and what stays refused"""
    import pytest
    import monai_amd.transforms as ours
    from monai_amd import ops
    from monai_amd._fallback import UnsupportedOnDevice
    from monai_amd.data.meta_tensor import MetaTensor

    x = torch.from_numpy(data((1, 6, 20, 9), 11).copy()).to(dev)
    aff = torch.diag(torch.tensor([1.3, 0.7, 1.1, 1.0], dtype=torch.float64))
    img = MetaTensor(x, affine=aff, applied_operations=[{"class": "Earlier"}])
    tr = ours.Spacing(pixdim=(1.0, 1.0, 1.0), mode=3, padding_mode="border")
    out = tr(img)
    assert isinstance(out, MetaTensor) and out.dtype == torch.float32 and tuple(out.shape) == (1, 8, 14, 10)
    assert torch.allclose(torch.as_tensor(out.meta["affine"]).cpu(), torch.eye(4, dtype=torch.float64), atol=1e-12)
    rec = out.applied_operations[-1]
    assert len(out.applied_operations) == 2 and rec["class"] == "SpatialResample" and tuple(rec["orig_size"]) == (6, 20, 9)
    assert rec["extra_info"]["mode"] == 3 and rec["extra_info"]["padding_mode"] == "border" and rec["extra_info"]["align_corners"] is False
    assert rec["extra_info"]["dtype"] == "float64" and torch.equal(rec["extra_info"]["src_affine"].cpu(), aff)
    back = tr.inverse(out)
    assert tuple(back.shape) == (1, 6, 20, 9) and len(back.applied_operations) == 1
    # an int-valued enum and a digit string select the same branch; grid_sample padding names map onto scipy's
    import enum

    class Order(enum.IntEnum):
        THREE = 3

    for mode, pad in ((Order.THREE, "nearest"), ("3", "border")):
        assert torch.equal(ours.Spacing(pixdim=(1.0, 1.0, 1.0), mode=mode, padding_mode=pad)(img).as_tensor(), out.as_tensor())
    assert not torch.equal(ours.Spacing(pixdim=(1.0, 1.0, 1.0), mode=1, padding_mode="border")(img).as_tensor(), out.as_tensor())
    # the unchanged-affine shortcut stays in front
    same = ours.Spacing(pixdim=(1.3, 0.7, 1.1), mode=3)(img)
    assert torch.equal(same.as_tensor(), x)
    # the public ops: a 3 x 4 index matrix and a dense grid give the same result; the prefilter alone
    m = np.zeros((3, 4))
    m[:, :3], m[:, 3] = np.diag([0.5, 1.25, 0.75]), (0.25, -1.0, 0.5)
    a = ops.spline_resample(x, 3, "mirror", out_size=(7, 9, 8), m=m.reshape(-1))
    oz, oy, ox = np.meshgrid(np.arange(7.0), np.arange(9.0), np.arange(8.0), indexing="ij")
    grid = np.stack([0.5 * oz + 0.25, 1.25 * oy - 1.0, 0.75 * ox + 0.5])
    b = ops.spline_resample(x, 3, "mirror", coords=torch.from_numpy(grid).to(dev))
    c = ops.spline_resample(x, 3, "mirror", coords=torch.from_numpy(np.stack([oz, oy, ox])).to(dev), scale=(0.5, 1.25, 0.75), offset=(0.25, -1.0, 0.5))
    assert a.dtype == torch.float32 and tuple(a.shape) == (1, 7, 9, 8) and torch.equal(a, b) and torch.equal(a, c)
    assert ops.spline_prefilter(x, 3, "nearest").shape == (1, 30, 44, 33) and ops.spline_prefilter(x, 3, "mirror").dtype == torch.float64
    # a non-finite coordinate writes NaN, the others are untouched
    bad = torch.from_numpy(grid.copy())
    bad[1, 2, 3, 4] = float("nan")
    bad[0, 0, 0, 0] = float("inf")
    d = ops.spline_resample(x, 3, "mirror", coords=bad.to(dev)).cpu()
    nan = torch.isnan(d)
    assert int(nan.sum()) == 2 and nan[0, 2, 3, 4] and nan[0, 0, 0, 0] and torch.equal(d[~nan], a.cpu()[~nan])
    # channel groups: a workspace bound below one group's coefficients changes nothing
    x3 = torch.from_numpy(data((3, 6, 20, 9), 12).copy()).to(dev)
    whole = ops.spline_resample(x3, 3, "nearest", out_size=(7, 9, 8), m=m.reshape(-1))
    saved = ops.SPLINE_WORKSPACE_BYTES
    ops.SPLINE_WORKSPACE_BYTES = 30 * 44 * 33 * 8 + 1
    try:
        assert torch.equal(ops.spline_resample(x3, 3, "nearest", out_size=(7, 9, 8), m=m.reshape(-1)), whole)
    finally:
        ops.SPLINE_WORKSPACE_BYTES = saved
    # argument errors
    for order in (6, -1):
        with pytest.raises(RuntimeError, match="spline order not supported"):
            ops.spline_resample(x, order, "mirror", out_size=(7, 9, 8), m=m.reshape(-1))
    with pytest.raises(RuntimeError, match="spline order not supported"):
        ops.spline_prefilter(x, 7, "mirror")
    with pytest.raises(RuntimeError, match="no prefilter"):
        ops.spline_prefilter(x, 1, "mirror")
    with pytest.raises(ValueError, match="padding"):
        ops.spline_resample(x, 3, "edge", out_size=(7, 9, 8), m=m.reshape(-1))
    with pytest.raises(ValueError, match="Unsupported padding_mode"):
        ours.Spacing(pixdim=(1.0, 1.0, 1.0), mode=3, padding_mode="edge")(img)
    with pytest.raises(ValueError, match="Unsupported padding_mode"):
        ours.Resample(mode=3, padding_mode="edge")(x, grid=torch.from_numpy(np.concatenate([grid, grid[:1]])).to(dev))
    with pytest.raises(ValueError, match="Unsupported mode"):
        ours.Spacing(pixdim=(1.0, 1.0, 1.0), mode=6)(img)          # not a spline order: the grid_sample branch refuses it, as in the reference
    with pytest.raises(NotImplementedError, match="1-D"):
        ours.Resample(mode=3)(x[0, 0, 0][None], grid=torch.zeros(2, 5, dtype=torch.float64).to(dev))
    with pytest.raises(NotImplementedError, match="1-D"):
        ours.SpatialResample(mode=3)(MetaTensor(x[0, 0, 0][None], affine=torch.eye(2, dtype=torch.float64)), dst_affine=torch.diag(torch.tensor([2.0, 1.0])).double(),
                                     spatial_size=(4,))
    # other dtypes are still refused (and go to the reference where it is importable)
    for other in (x.double(), x.half(), (x * 0.1).to(torch.int16)):
        with pytest.raises(UnsupportedOnDevice):
            ours.Spacing(pixdim=(1.0, 1.0, 1.0), mode=3)(MetaTensor(other, affine=aff))
        with pytest.raises(UnsupportedOnDevice):
            ours.Resample(mode=3)(other, grid=torch.from_numpy(np.concatenate([grid, grid[:1]])).to(dev))
        with pytest.raises(UnsupportedOnDevice):
            ops.spline_resample(other, 3, "mirror", out_size=(7, 9, 8), m=m.reshape(-1))
