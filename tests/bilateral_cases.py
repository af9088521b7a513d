"""Shared cases of the exact bilateral filter (monai_amd._C.bilateral_filter, ops.bilateral_filter, BilateralFilter) and of the kernels under it
(monai_amd/csrc/kernels/bilateral.h); tests/test_bilateral_emu.py runs them on the SIMT emulator, tests/test_bilateral_gpu.py on the MI355X.

Every case is compared with the outputs of the reference's own ``bilateral_filter`` (monai/csrc/filtering/bilateral/bilateralfilter_cpu.cpp) on the CPU,
stored in tests/golden/bilateral*.npz by tests/golden/make_golden_bilateral.py: ``ref32`` (the bits of its float32 output) and ``ref64`` (its float64
output for the same float32 values).  The inputs are regenerated here from seeds.

Tolerances (max abs over the output, NaN exactly where the reference has NaN):
  float32   |ours - ref64| <= 2 e_ref + 2 * 2^-24 * max|x|, e_ref = max |ref32 - ref64| -- the reference's own float32 distance from its float64 output.
            The kernel adds the same positive terms in float32 in another order and takes exp2 from the hardware where the reference calls libm: two error
            sources of the reference's kind and size, hence twice its error, plus one float32 step each for the final division and the un-scaling.
  float64   |ours - ref64| <= (2 K^dims + 8) * 2^-53 * max|x|: the a-priori bound for a quotient of two recursive sums with positive weights.
  float16   equals the float32 result of the up-cast input rounded to half, exactly.
Every case runs twice and has to give the same bits.

Tile shapes (bilateral_plan of csrc/capi.hip; a function of the window, the channel count and of which axes have extent 1): K = 5, C = 1 stages
16 (x) x 8 (y) x 8 (z) outputs in 3-D, 64 x 16 in 2-D and 1024 in 1-D; the tile-extent cases sit one below, at and one above those extents on every
axis, and at two tiles plus a remainder.  The tile path takes float32 with at most 4 channels whose staged tile fits 63 KiB (3-D windows up to 15 taps
at C = 1, 2-D windows up to 31 taps at C = 4, every 1-D window at C <= 4); everything else (float64, more channels, larger windows) is the generic kernel's."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden")
TILE, GENERIC = 1, 2
WINDOW_RULE = ((0.2, 1), (0.3, 3), (0.6, 3), (0.61, 5), (0.8, 5), (1.2, 7), (2.2, 11))      # spatial sigma -> K by the float32 rule
GROUPS = ("window", "small", "unit", "tile3d", "tile2d", "tile1d", "win3d", "win2d", "win1d", "chan", "color", "generic", "f64", "nonfinite")


def _case(cid, shape, ss, cs, path, scale=1.0, f64=False, poke=None, file="bilateral"):
    return {"id": cid, "shape": tuple(shape), "ss": ss, "cs": cs, "path": path, "scale": scale, "f64": f64, "poke": poke, "file": file}


def golden_cases():
    c = []
    # the window rule: the three sigmas whose K a double-precision product gets wrong (0.2, 0.6, 2.2) among them; sigma 0.2 is the identity
    for ss, k in WINDOW_RULE:
        c.append(_case("window-s%s-k%d" % (ss, k), (1, 1, 14, 15), ss, 0.7, TILE if k > 1 else GENERIC))      # one tap: nothing to stage
    # volumes smaller than the window: clamped many times over
    c.append(_case("small-2x3x5-s1", (1, 1, 2, 3, 5), 1.0, 0.8, TILE))
    c.append(_case("small-4x3x2-s1.4", (1, 1, 4, 3, 2), 1.4, 0.8, TILE))
    # unit axes
    c.append(_case("unit-1x1x7", (1, 1, 1, 1, 7), 1.0, 0.8, TILE))
    c.append(_case("unit-1x9x1", (1, 1, 1, 9, 1), 1.0, 0.8, TILE))
    c.append(_case("unit-9x1x1", (1, 1, 9, 1, 1), 1.0, 0.8, TILE))
    # tile extents (16 x 8 x 8, 64 x 16, 1024 at K = 5, C = 1): one below, at, one above, two tiles and a remainder
    for shape in ((7, 7, 15), (8, 8, 16), (9, 9, 17), (19, 18, 35)):
        c.append(_case("tile3d-%dx%dx%d" % shape, (1, 1) + shape, 1.0, 0.8, TILE))
    for shape in ((15, 63), (16, 64), (17, 65), (35, 131)):
        c.append(_case("tile2d-%dx%d" % shape, (1, 1) + shape, 1.0, 0.8, TILE))
    for n in (1023, 1024, 1025, 2051):
        c.append(_case("tile1d-%d" % n, (1, 1, n), 1.0, 0.8, TILE))
    # every 3-D window of the tile path at C = 1 (3 ... 15 taps), 2-D windows up to 25 taps at C = 4, 1-D windows up to 255 taps
    for ss, k in ((0.6, 3), (1.4, 7), (1.8, 9), (2.2, 11), (3.0, 15)):
        c.append(_case("win3d-k%d" % k, (1, 1, 9, 10, 18), ss, 0.8, TILE))
    for ss, k, ch in ((1.8, 9, 2), (2.6, 13, 3), (3.4, 17, 1), (4.2, 21, 4), (5.0, 25, 4)):
        c.append(_case("win2d-k%d-c%d" % (k, ch), (1, ch, 20, 40), ss, 0.8, TILE))
    for ss, k, ch in ((3.0, 15, 1), (12.6, 63, 3), (25.4, 127, 1), (51.0, 255, 4)):
        c.append(_case("win1d-k%d-c%d" % (k, ch), (1, ch, 300), ss, 0.8, TILE))
    # channels: the colour distance is joint over the channels; batch items and channels hold different data
    for ch in (1, 2, 3, 4, 5, 16):
        c.append(_case("chan-c%d" % ch, (2, ch, 5, 6, 9), 1.0, 1.5, TILE if ch <= 4 else GENERIC))
    c.append(_case("chan-2d-c3", (2, 3, 17, 19), 1.0, 1.5, TILE))
    # colour-sigma regimes on data x 100: almost every weight underflows, mixed, a pure Gaussian
    for cs in (0.05, 30.0, 1e4):
        c.append(_case("color-cs%g" % cs, (1, 1, 6, 9, 10), 1.0, cs, TILE, scale=100.0))
        c.append(_case("color-cs%g-c5" % cs, (1, 5, 9, 10), 1.0, cs, GENERIC, scale=100.0))
    # the issue's larger windows: 13 taps in 3-D (the tile still fits), 2-D with 5 channels (generic), 1-D with 255 taps; a window past the tile's reach
    c.append(_case("generic-3d-s2.6", (1, 1, 14, 15, 16), 2.6, 0.8, TILE))
    c.append(_case("generic-2d-s5-c5", (1, 5, 12, 13), 5.0, 0.8, GENERIC))
    c.append(_case("generic-1d-s51", (1, 1, 300), 51.0, 0.8, TILE))
    c.append(_case("generic-3d-s3.4", (1, 1, 6, 7, 20), 3.4, 0.8, GENERIC))       # 17 taps: the staged tile would not fit
    c.append(_case("generic-2d-s7-c4", (1, 4, 12, 40), 7.0, 0.8, GENERIC))        # 35 taps at 4 channels: the same
    # float64: always the generic kernel
    c.append(_case("f64-3d-s2.6", (1, 1, 14, 15, 16), 2.6, 0.8, GENERIC, f64=True))
    c.append(_case("f64-2d-s5-c5", (1, 5, 12, 13), 5.0, 0.8, GENERIC, f64=True))
    c.append(_case("f64-1d-s51", (1, 1, 300), 51.0, 0.8, GENERIC, f64=True))
    c.append(_case("f64-3d-s1-c2", (2, 2, 5, 6, 9), 1.0, 1.5, GENERIC, f64=True))
    # one non-finite value in an otherwise finite 3-D volume, on both paths
    for name, value in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        for where, at in (("corner", (0, 0, 0, 0, 0)), ("interior", (0, 0, 3, 4, 5))):
            c.append(_case("nonfinite-%s-%s-tile" % (name, where), (1, 1, 6, 9, 10), 1.0, 0.8, TILE, poke=(at, value)))
            c.append(_case("nonfinite-%s-%s-generic" % (name, where), (1, 5, 5, 7, 8), 1.0, 0.8, GENERIC, poke=(at, value)))
    for case in c:      # two golden files, each well under the size limit for a committed file
        if case["id"].split("-")[0] in ("chan", "color", "generic", "f64", "nonfinite"):
            case["file"] = "bilateral_2"
    return c


def gpu_cases():
    """run on the MI355X only: their goldens cost the reference's CPU code seconds"""
    return [_case("gpu-40x41x42-s2", (1, 1, 40, 41, 42), 2.0, 0.8, TILE, file="bilateral_gpu_s2"),
            _case("gpu-40x41x42-s3", (1, 1, 40, 41, 42), 3.0, 0.8, TILE, file="bilateral_gpu_s3"),
            _case("gpu-40x41x42-s3-f64", (1, 1, 40, 41, 42), 3.0, 0.8, GENERIC, f64=True, file="bilateral_gpu_s3")]


def all_cases():
    return golden_cases() + gpu_cases()


_inputs_cache: dict = {}


def inputs(case) -> np.ndarray:
    """float32 values (the float64 cases run on exactly these values)"""
    cid = case["id"][:-4] if case["id"].endswith("-f64") and case["id"].startswith("gpu") else case["id"]
    if cid not in _inputs_cache:
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % 100003
        a = (np.random.default_rng(seed).standard_normal(case["shape"]) * case["scale"]).astype(np.float32)
        if case["poke"] is not None:
            a[case["poke"][0]] = case["poke"][1]
        a.setflags(write=False)
        _inputs_cache[cid] = a
    return _inputs_cache[cid]


def golden_key(case) -> str:
    return "gpu-40x41x42-s3" if case["id"] == "gpu-40x41x42-s3-f64" else case["id"]


_golden_cache: dict = {}


def golden(file: str):
    if file not in _golden_cache:
        with np.load(os.path.join(GOLDEN_DIR, file + ".npz")) as z:
            _golden_cache[file] = {k: z[k] for k in z.files}
    return _golden_cache[file]


def window(ss: float) -> int:
    """K by the reference's rule, the product in float32"""
    return int(np.ceil(np.float32(5.0) * np.float32(ss))) | 1


def bound(case, ref32: np.ndarray, ref64: np.ndarray):
    """(tolerance, e_ref) of the case"""
    x = inputs(case)
    xmax = float(np.abs(x[np.isfinite(x)]).max())
    ok = ~np.isnan(ref64)
    e_ref = float(np.abs(ref32[ok].astype(np.float64) - ref64[ok]).max()) if ok.any() else 0.0
    if case["f64"]:
        return (2 * window(case["ss"]) ** (len(case["shape"]) - 2) + 8) * 2.0 ** -53 * xmax, e_ref
    return 2 * e_ref + 2 * 2.0 ** -24 * xmax, e_ref


def run(case, dev) -> torch.Tensor:
    from monai_amd import _C

    x = torch.from_numpy(inputs(case).copy())
    x = (x.double() if case["f64"] else x).to(dev)
    before = x.clone()
    out = _C.bilateral_filter(x, case["ss"], case["cs"], False)
    assert torch.equal(x.cpu().view(torch.int64 if case["f64"] else torch.int32), before.cpu().view(torch.int64 if case["f64"] else torch.int32)), "the input was modified"
    return out


def check_cases(dev, cases) -> dict:
    """the cases against the reference, twice with the same bits, each on the kernel it names; returns {path: worst |ours - ref64| / e_ref of the float32
    cases} (printed per group by the tests)"""
    from monai_amd import ops

    worst: dict = {}
    for case in cases:
        cid = case["id"]
        g = golden(case["file"])
        assert cid in json.loads(str(g["manifest"])) or golden_key(case) in json.loads(str(g["manifest"])), "tests/golden/%s.npz is stale: run make_golden_bilateral.py" % case["file"]
        ref32, ref64 = g[golden_key(case) + "/ref32"].view(np.float32), g[golden_key(case) + "/ref64"]
        dtype = torch.float64 if case["f64"] else torch.float32
        path = ops.bilateral_filter_path(case["shape"][2:], case["shape"][1], case["ss"], dtype)
        assert path == case["path"], (cid, "kernel", path, "expected", case["path"])
        a, b = (run(case, dev).cpu().numpy() for _ in range(2))
        assert a.dtype == (np.float64 if case["f64"] else np.float32) and a.shape == case["shape"], (cid, a.dtype, a.shape)
        assert a.tobytes() == b.tobytes(), ("not the same bits twice", cid)
        nan = np.isnan(ref32)
        assert np.array_equal(np.isnan(a), nan), (cid, "NaN where the reference has none, or the reverse", int(np.isnan(a).sum()), int(nan.sum()))
        if case["poke"] is not None:
            assert nan.any() and not nan.all(), cid
        tol, e_ref = bound(case, ref32, ref64)
        err = float(np.abs(a[~nan].astype(np.float64) - ref64[~nan]).max())
        ratio = err / e_ref if e_ref > 0 else 0.0
        print("%-34s %s K=%-3d err %.3e  e_ref %.3e  ratio %.2f  bound %.3e" % (cid, "tile   " if path == TILE else "generic", window(case["ss"]), err, e_ref, ratio, tol))
        if not case["f64"]:
            worst[path] = max(worst.get(path, 0.0), ratio)
        else:
            worst.setdefault(path, 0.0)
        assert err <= tol, (cid, err, tol, e_ref)
        if window(case["ss"]) == 1:
            assert a.tobytes() == inputs(case).astype(a.dtype).tobytes(), (cid, "a window of one tap is the identity, bit for bit")
    return worst
