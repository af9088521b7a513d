"""Cases shared by the emulator and the GPU tests of the surface metrics (HausdorffDistanceMetric, SurfaceDistanceMetric, SurfaceDiceMetric), the
mask-edge kernel and the exact Euclidean distance transform (csrc/kernels/edt.h), and by the golden generator
(tests/golden/make_golden_surface.py), which runs `run_all` on the real reference."""
import os
import warnings

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the smallest shapes at which these kernels can go wrong: one voxel, odd sizes, 2-D, an axis past one wave and one 256-thread workgroup both as the
# scanned (contiguous) axis and as the column axis, rows of more than one 64-lane trip, more than 256 columns
SHAPES = [(1, 1, 1), (3, 5, 7), (4, 4), (12, 13), (17, 16, 15), (5, 3, 300), (300, 3, 5), (2, 70, 66)]
SPACED_SHAPES = [(3, 5, 7), (12, 13), (17, 16, 15)]
REDUCTIONS = ("none", "mean", "sum", "mean_batch", "sum_batch", "mean_channel", "sum_channel")
SQRT2 = float(np.float32(np.sqrt(2)))
THRESHOLDS = (0.0, 1.0, SQRT2)
EPS32 = 2.0 ** -23


def _tag(shape):
    return "x".join(str(v) for v in shape)


def blobs(shape, seed):
    """box-filtered uniform noise thresholded at its 65th percentile: blob-like, touching the borders"""
    r = np.random.default_rng(seed).random(shape)
    pad = np.pad(r, 1, mode="edge")
    s = np.zeros(shape)
    for off in np.ndindex(*([3] * len(shape))):
        s += pad[tuple(slice(o, o + n) for o, n in zip(off, shape))]
    return s > np.percentile(s, 65)


def mask_pairs(shape):
    """(prediction, truth) bool masks of the issue's list, in a fixed order"""
    z = np.zeros(shape, bool)
    last = tuple(n - 1 for n in shape)
    mid = tuple(n // 2 for n in shape)
    single, corner0, corner1, both = z.copy(), z.copy(), z.copy(), z.copy()
    single[mid] = True
    corner0[(0,) * len(shape)] = True
    corner1[last] = True
    both[(0,) * len(shape)] = both[last] = True
    plane, line = z.copy(), z.copy()
    plane[mid[0]] = True                                   # a full plane (a full row in 2-D)
    line[mid[:-1]] = True                                  # a full line along the contiguous axis
    col = z.copy()
    col[(slice(None),) + mid[1:]] = True                   # a full line along the first axis
    checker = (np.indices(shape).sum(0) % 2).astype(bool)
    return [
        ("single", single, corner1), ("corners", corner0, corner1), ("both_corners", both, single), ("full", np.ones(shape, bool), blobs(shape, 11)),
        ("plane_line", plane, line), ("line_col", line, col), ("checker", checker, ~checker), ("blobs", blobs(shape, 12), blobs(shape, 13)),
        ("pred_empty", z, blobs(shape, 14)), ("truth_empty", blobs(shape, 15), z), ("both_empty", z, z),
    ]


def batch(shape, dtype=torch.float32):
    """every mask pair of `shape` as one batch: two-channel one-hot tensors [B, 2, *shape] (background, foreground)"""
    pairs = mask_pairs(shape)
    p = np.stack([np.stack([~a, a]) for _, a, _ in pairs])
    y = np.stack([np.stack([~b, b]) for _, _, b in pairs])
    return torch.from_numpy(p).to(dtype), torch.from_numpy(y).to(dtype)


def labels5(shape, seed):
    """a 5-class label map of nested / adjacent blobs, [1, 1, *shape] uint8"""
    lab = np.zeros(shape, np.uint8)
    for c in range(1, 5):
        lab[blobs(shape, seed + c)] = c
    return torch.from_numpy(lab)[None, None]


def onehot(lab, k, dtype=torch.float32):
    return torch.zeros((lab.shape[0], k) + tuple(lab.shape[2:]), dtype=dtype).scatter_(1, lab.long(), 1).contiguous()


def spacing_of(shape):
    return [0.8, 1.25, 2.5][-len(shape):]


# ---------------------------------------------------------------------------------------------------------------- EDT against brute force
def edt_images(shape):
    """C channels whose ZERO voxels are the features: blobs, one zero, zeros in two opposite corners, a plane and a line of zeros, a checkerboard, no zero"""
    out = []
    for name, a, b in mask_pairs(shape):
        if name in ("single", "both_corners", "plane_line", "checker", "blobs"):
            out.append(~a)
        if name == "plane_line":
            out.append(~b)
    out.append(np.ones(shape, bool))                       # no background at all: +inf
    return np.stack(out)


def brute_sq(img, spacing=None):
    """min over all zero voxels of the squared offset: int64 exactly at unit spacing, float64 with a spacing; +inf (-1 for integers) without a zero voxel"""
    pts = np.argwhere(np.ones(img.shape, bool))
    bg = np.argwhere(~img)
    if len(bg) == 0:
        return np.full(img.shape, -1 if spacing is None else np.inf)
    best = None
    for i in range(0, len(bg), 256):
        d = pts[:, None, :] - bg[None, i:i + 256, :]
        d = (d * d).sum(-1) if spacing is None else ((d * np.asarray(spacing, np.float64)) ** 2).sum(-1)
        m = d.min(1)
        best = m if best is None else np.minimum(best, m)
    return best.reshape(img.shape)


def case_edt_vs_brute_force(device):
    """unit spacing: fp64 output == np.sqrt(brute force) bit for bit and fp32 output == its cast (so the squared distances are the exact integers);
    with a spacing |ours - t| <= 8 * 2^-53 * t for fp64 (3 roundings per scaled square, 2 for the sums, half of that through the root plus its own
    rounding: ~4 units, doubled because an fp64 comparison may choose a feature within rounding of the minimum) and one fp32 ulp for fp32"""
    from monai_amd import ops

    worst64 = worst32 = 0.0
    for shape in SHAPES:
        imgs = edt_images(shape)
        for dtype in (torch.bool, torch.uint8, torch.float32):
            t = torch.from_numpy(imgs).to(dtype).to(device)
            exp = np.stack([brute_sq(im) for im in imgs])
            exp = np.where(exp < 0, np.inf, np.sqrt(exp.astype(np.float64)))
            got64, got32 = ops.edt(t, float64=True).cpu().numpy(), ops.edt(t).cpu().numpy()
            assert got64.dtype == np.float64 and got32.dtype == np.float32
            np.testing.assert_array_equal(got64, exp, err_msg=str(shape))
            np.testing.assert_array_equal(got32, exp.astype(np.float32), err_msg=str(shape))
            if dtype != torch.bool:
                continue
            for sp in (spacing_of(shape), 0.7):
                spv = [sp] * len(shape) if isinstance(sp, float) else sp
                tr = np.sqrt(np.stack([brute_sq(im, spv) for im in imgs]))
                got64, got32 = ops.edt(t, sampling=sp, float64=True).cpu().numpy(), ops.edt(t, sampling=sp).cpu().numpy()
                fin = np.isfinite(tr)
                np.testing.assert_array_equal(np.isinf(got64), ~fin)
                np.testing.assert_array_equal(np.isinf(got32), ~fin)
                e64 = np.abs(got64[fin] - tr[fin])
                assert (e64 <= 8 * 2.0 ** -53 * tr[fin]).all(), (shape, sp)
                ulp32 = np.spacing(np.abs(tr[fin]).astype(np.float32)).astype(np.float64)
                e32 = np.abs(got32[fin].astype(np.float64) - tr[fin])
                assert (e32 <= ulp32).all(), (shape, sp)
                nz = tr[fin] > 0
                if nz.any():
                    worst64 = max(worst64, float((e64[nz] / tr[fin][nz]).max() / 2.0 ** -53))
                    worst32 = max(worst32, float((e32[nz] / ulp32[nz]).max()))
    print("edt with spacing: max |ours - t| / t =", worst64, "x 2^-53 (fp64);", worst32, "fp32 ulp")
    return worst64, worst32


# ---------------------------------------------------------------------------------------------------------------- edges
LABEL_DTYPES = (torch.float32, torch.uint8, torch.int64)
CHANNEL_DTYPES = (torch.float32, torch.uint8, torch.bool)


def edge_inputs(shape):
    """(label map [2, 1, *shape] with 3 classes, its bool one-hot [2, 3, *shape])"""
    lab = torch.cat([labels5(shape, 20) % 3, labels5(shape, 30) % 3])
    if np.prod(shape) > 1:
        lab.view(2, -1)[1, 0] = 2                          # a foreground voxel in the corner: always an edge
    return lab, onehot(lab, 3, torch.bool)


def run_edges(device=None):
    """name -> packed bits of the expected edge maps, from scipy (golden generator only)"""
    from scipy.ndimage import binary_erosion

    out = {}
    for shape in SHAPES:
        _, oh = edge_inputs(shape)
        m = oh.numpy()
        e = np.stack([np.stack([binary_erosion(m[b, c]) ^ m[b, c] for c in range(3)]) for b in range(2)])
        out["edges_" + _tag(shape)] = np.packbits(e.reshape(-1))
    return out


def case_edges_vs_scipy(device):
    """ops.mask_edges == scipy's binary_erosion(m) ^ m (stored in the golden) for every form / dtype pair; a full volume has its edges on its faces"""
    from monai_amd import ops

    g = np.load(os.path.join(GOLDEN, "surface_metrics.npz"))
    n = 0
    for shape in SHAPES:
        lab, oh = edge_inputs(shape)
        exp = np.unpackbits(g["edges_" + _tag(shape)])[: oh.numel()].reshape(oh.shape).astype(bool)
        sides = [(lab.to(dt), "labels") for dt in LABEL_DTYPES] + [(oh.to(dt), "channel") for dt in CHANNEL_DTYPES]
        for i, (a, _) in enumerate(sides):
            b = sides[(i + 1) % len(sides)][0]           # every form / dtype on each side, in mixed pairs
            ep, et = ops.mask_edges(a.to(device), b.to(device), 3)
            assert ep.dtype == torch.bool and tuple(ep.shape) == tuple(exp.shape)
            np.testing.assert_array_equal(ep.cpu().numpy(), exp, err_msg=f"{shape} {a.dtype}")
            np.testing.assert_array_equal(et.cpu().numpy(), exp, err_msg=f"{shape} {b.dtype}")
            n += 2
        # a channel whose values are not 0 / 1: only == 1 is foreground (the reference's seg == label_idx), a bool channel is used as it is
        two = oh.float() * 2.0
        ep, _ = ops.mask_edges(two.to(device), two.to(device), 3)
        assert not bool(ep.any())
        full = torch.ones((1, 1) + shape, dtype=torch.bool)
        ef, _ = ops.mask_edges(full.to(device), full.to(device), 1)
        face = np.zeros(shape, bool)
        for a in range(len(shape)):
            for side in (0, -1):
                face[(slice(None),) * a + (side,)] = True
        np.testing.assert_array_equal(ef[0, 0].cpu().numpy(), face)
    return n


# ---------------------------------------------------------------------------------------------------------------- metrics against the reference
def _np(t):
    return t.detach().cpu().numpy()


def asd_jobs():
    """(name, y_pred, y, keywords) of every average-surface-distance result: `run_all` computes them, `truths` their float64 truths"""
    jobs = []
    for shape in SHAPES:
        p, y = batch(shape)
        tag = _tag(shape)
        jobs += [(f"asd_{tag}_s0", p, y, {}), (f"asd_{tag}_s1", p, y, {"symmetric": True}), (f"asd_{tag}_bg", p, y, {"symmetric": True, "include_background": True})]
    p, y = batch((17, 16, 15))
    jobs.append(("asd_k1", p[:, 1:].contiguous(), y[:, 1:].contiguous(), {"symmetric": True}))
    p5 = torch.cat([onehot(labels5((17, 16, 15), 40), 5), onehot(labels5((17, 16, 15), 50), 5)])
    y5 = torch.cat([onehot(labels5((17, 16, 15), 60), 5), onehot(labels5((17, 16, 15), 50), 5)])
    jobs += [("asd_k5_b0", p5, y5, {"symmetric": True}), ("asd_k5_b1", p5, y5, {"symmetric": True, "include_background": True})]
    p, y = batch((12, 13))
    jobs.append(("cls_asd_calls", p, y, {"symmetric": True}))      # computed through the class in `run_all`
    for shape in SPACED_SHAPES:
        p, y, sp = spaced_inputs(shape)
        jobs.append((f"sp_asd_{_tag(shape)}", p, y, {"symmetric": True, "include_background": True, "spacing": sp}))
    return jobs


PARTS = len(SHAPES) + 1      # one part per shape, one for the rest (K = 1 and 5, the classes, everything with a spacing)


def run_all(mod, device, part=None):
    """name -> result of the reference-shaped API of `mod` (monai.metrics or monai_amd.metrics) on tensors of `device`: bit-comparable results.
    `part`: None for everything, i < len(SHAPES) for the results of SHAPES[i], len(SHAPES) for the rest."""
    out = {}
    rest = part is None or part == len(SHAPES)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for shape in (SHAPES if part is None else SHAPES[part:part + 1]):
            p, y = (t.to(device) for t in batch(shape))
            tag = _tag(shape)
            for pc in (None, 95, 50):
                for directed in (False, True):
                    for bg in (False, True):
                        out[f"hd_{tag}_p{pc}_d{int(directed)}_b{int(bg)}"] = _np(mod.compute_hausdorff_distance(p, y, include_background=bg, percentile=pc, directed=directed))
            for thr in THRESHOLDS:
                out[f"nsd_{tag}_t{thr:.3f}"] = _np(mod.compute_surface_dice(p, y, [thr]))
            out[f"nsd_{tag}_bg"] = _np(mod.compute_surface_dice(p, y, [1.0, SQRT2], include_background=True))
        for name, jp, jy, kw in asd_jobs():
            of_shape = name.startswith("asd_") and not name.startswith("asd_k")
            mine = (part is None or name.startswith(f"asd_{_tag(SHAPES[part])}_")) if (of_shape and part != len(SHAPES)) else (rest and not of_shape)
            if mine and not name.startswith("cls_") and not name.startswith("sp_"):
                out[name] = _np(mod.compute_average_surface_distance(jp.to(device), jy.to(device), **kw))
        if not rest:
            return out
        # K = 1 (a single channel stays whatever include_background says) and K = 5
        p, y = (t[:, 1:].contiguous().to(device) for t in batch((17, 16, 15)))
        out["hd_k1"] = _np(mod.compute_hausdorff_distance(p, y, percentile=95))
        out["nsd_k1"] = _np(mod.compute_surface_dice(p, y, [1.0]))
        p5 = torch.cat([onehot(labels5((17, 16, 15), 40), 5), onehot(labels5((17, 16, 15), 50), 5)]).to(device)
        y5 = torch.cat([onehot(labels5((17, 16, 15), 60), 5), onehot(labels5((17, 16, 15), 50), 5)]).to(device)
        for bg in (False, True):
            out[f"hd_k5_b{int(bg)}"] = _np(mod.compute_hausdorff_distance(p5, y5, include_background=bg))
            out[f"hd95_k5_b{int(bg)}"] = _np(mod.compute_hausdorff_distance(p5, y5, include_background=bg, percentile=95))
            out[f"nsd_k5_b{int(bg)}"] = _np(mod.compute_surface_dice(p5, y5, [0.0, 1.0, SQRT2, 2.0, 3.0][: 5 if bg else 4], include_background=bg))
        # the three classes: a batch tensor, then a list of channel-first tensors; every reduction, get_not_nans, reset
        p, y = (t.to(device) for t in batch((12, 13)))
        makers = {"hd": lambda **kw: mod.HausdorffDistanceMetric(percentile=95, **kw), "asd": lambda **kw: mod.SurfaceDistanceMetric(symmetric=True, **kw),
                  "nsd": lambda **kw: mod.SurfaceDiceMetric(class_thresholds=[1.0], **kw)}
        for name, make in makers.items():
            for red in REDUCTIONS:
                m = make(reduction=red, get_not_nans=True)
                first = m(p[:6], y[:6])
                second = m(list(p[6:]), list(y[6:]))
                f, nn = m.aggregate()
                out[f"cls_{name}_{red}_nn"] = _np(nn)
                if name == "asd":      # a float32 mean per sample (toleranced, `cls_asd_calls`): the reduction is checked against the module's own function
                    assert torch.equal(f.nan_to_num(-1.0), mod.do_metric_reduction(m.get_buffer(), red)[0].nan_to_num(-1.0))
                else:
                    out[f"cls_{name}_{red}"] = _np(f)
                if red == "none":
                    out[f"cls_{name}_calls"] = np.concatenate([_np(first), _np(second)])
                m.reset()
                assert m.get_buffer() is None
                m(p[:2], y[:2])
                if name != "asd":
                    out[f"cls_{name}_{red}_after_reset"] = _np(m.aggregate()[0])
    return out


def spaced_inputs(shape):
    """B = 2 with a different spacing per item, and the blobs / single-voxel pairs of `shape`"""
    pairs = {n: (a, b) for n, a, b in mask_pairs(shape)}
    a0, b0 = pairs["blobs"]
    a1, b1 = pairs["both_corners"]
    p = torch.from_numpy(np.stack([np.stack([~a0, a0]), np.stack([~a1, a1])])).float()
    y = torch.from_numpy(np.stack([np.stack([~b0, b0]), np.stack([~b1, b1])])).float()
    return p, y, [spacing_of(shape), [0.7] * len(shape)]


def run_toleranced(mod, device, percentiles=None):
    """name -> results that are compared against a float64 truth: everything with a spacing.  `percentiles`: None for all of them, False for the
    maxima and means only, True for the percentile results only"""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for shape in SPACED_SHAPES:
            p, y, sp = spaced_inputs(shape)
            p, y = p.to(device), y.to(device)
            tag = _tag(shape)
            for pc in (None, 95, 50):
                if percentiles is None or percentiles == bool(pc):
                    out[f"sp_hd_{tag}_p{pc}"] = _np(mod.compute_hausdorff_distance(p, y, include_background=True, percentile=pc, spacing=sp))
            if percentiles:
                continue
            out[f"sp_hd_{tag}_scalar"] = _np(mod.compute_hausdorff_distance(p, y, include_background=True, spacing=0.7))
            out[f"sp_asd_{tag}"] = _np(mod.compute_average_surface_distance(p, y, include_background=True, symmetric=True, spacing=sp))
    return out


def _ref_distances(p, y, sp, symmetric):
    """float64 distances of the reference's definition for one (b, c): scipy's edges and float64 EDT (golden generator only)"""
    from scipy.ndimage import binary_erosion, distance_transform_edt

    ep, ey = binary_erosion(p) ^ p, binary_erosion(y) ^ y
    if not ep.any() and not ey.any():
        return []
    if not ep.any() or not ey.any():
        return [np.array([np.inf])]
    ds = [distance_transform_edt(~ey, sampling=sp)[ep]]
    if symmetric:
        ds.append(distance_transform_edt(~ep, sampling=sp)[ey])
    return ds


def truths():
    """float64 truths (golden generator only): for every average surface distance the mean, formed in float64, of the float32 distances (unit spacing)
    or of the float64 distances (with a spacing); for the spaced Hausdorff results the float64 maximum / numpy percentile"""
    out = {}
    for name, p, y, kw in asd_jobs():
        p, y = p.numpy().astype(bool), y.numpy().astype(bool)
        chans = list(range(p.shape[1])) if (kw.get("include_background") or p.shape[1] == 1) else list(range(1, p.shape[1]))
        t = np.full((p.shape[0], len(chans)), np.nan)
        for b in range(p.shape[0]):
            sp = kw["spacing"][b] if "spacing" in kw else None
            for i, c in enumerate(chans):
                ds = _ref_distances(p[b, c], y[b, c], sp, kw.get("symmetric", False))
                if ds:
                    d = np.concatenate(ds)
                    t[b, i] = (d if sp is not None else d.astype(np.float32).astype(np.float64)).mean()
        out[name] = t
    for shape in SPACED_SHAPES:
        p, y, sp = spaced_inputs(shape)
        p, y = p.numpy().astype(bool), y.numpy().astype(bool)
        tag = _tag(shape)
        for name, pc, spc in [(f"sp_hd_{tag}_p{pc}", pc, sp) for pc in (None, 95, 50)] + [(f"sp_hd_{tag}_scalar", None, [[0.7] * len(shape)] * 2)]:
            t = np.full((2, 2), np.nan)
            for b in range(2):
                for c in range(2):
                    ds = _ref_distances(p[b, c], y[b, c], spc[b], True)
                    if ds:
                        t[b, c] = max((np.percentile(d, pc) if pc else d.max()) for d in ds)
            out[name] = t
    return out


def _same_specials(a, b, name):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=name)
    np.testing.assert_array_equal(np.isposinf(a), np.isposinf(b), err_msg=name)
    return np.isfinite(b)


def _compare_with_golden(got, g):
    exact, worst = 0, 0.0
    for name, v in got.items():
        assert name in g.files, name
        ref = g[name]
        assert v.shape == ref.shape and v.dtype == ref.dtype, (name, v.shape, ref.shape, v.dtype, ref.dtype)
        if name + "_truth" not in g.files:
            np.testing.assert_array_equal(v, ref, err_msg=name)
            exact += 1
            continue
        t, ref_err = g[name + "_truth"], g[name + "_ref_err"]
        fin = _same_specials(v, ref, name)
        np.testing.assert_array_equal(fin, np.isfinite(t), err_msg=name)
        v64, r64 = v.astype(np.float64)[fin], ref.astype(np.float64)[fin]
        t, ref_err = t[fin], ref_err[fin]
        np.testing.assert_array_equal(ref_err, np.abs(r64 - t), err_msg=name)      # the stored distance is the reference's own
        err, eps = np.abs(v64 - t), EPS32 * np.abs(t)
        rel = float((err[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0
        worst = max(worst, rel)
        print(name, "max |ours - t| / |t| =", rel, " max |ref - t| / |t| =", float((ref_err[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0)
        assert (err <= eps).all(), (name, err, eps)
        assert (np.abs(v64 - r64) <= ref_err + eps).all(), name
    print("bit-equal results", exact, "; toleranced worst |ours - t| / |t| =", worst, "of", EPS32)
    return exact


def case_metrics_vs_reference(device, part):
    """compute_hausdorff_distance (percentile None / 95 / 50, directed or not, with and without background) and compute_surface_dice (thresholds 0, 1,
    float32(sqrt 2)) at unit spacing, the three classes under every reduction: bit-equal to the real reference (tests/golden/make_golden_surface.py),
    inf / nan by position.  compute_average_surface_distance is a float32 mean whose order of summation differs by device: against the float64 truth t
    of the golden, |ours - t| <= 2^-23 |t| and |ours - ref| <= |ref - t| + 2^-23 |t|.  With a spacing the Hausdorff maxima go through the same rule (the
    percentiles: `case_spaced_percentiles_vs_truth`).  The reference's own distance from the truth is part of the golden: no bound comes from the
    code under test.  `part` of PARTS: see `run_all`."""
    import monai_amd.metrics as ours

    g = np.load(os.path.join(GOLDEN, "surface_metrics.npz"))
    got = run_all(ours, device, part)
    if part == len(SHAPES):
        got.update(run_toleranced(ours, device, percentiles=False))
    return _compare_with_golden(got, g)


def case_golden_is_covered():
    """the golden holds exactly the results that the parts of `run_all` and `run_toleranced` produce (their names, spelled out here), a truth and the
    reference's distance from it for every toleranced one, the edge maps and the transform outputs"""
    g = np.load(os.path.join(GOLDEN, "surface_metrics.npz"))
    names = set()
    for shape in SHAPES:
        tag = _tag(shape)
        names |= {f"hd_{tag}_p{pc}_d{d}_b{b}" for pc in (None, 95, 50) for d in (0, 1) for b in (0, 1)} | {f"nsd_{tag}_t{t:.3f}" for t in THRESHOLDS}
        names |= {f"nsd_{tag}_bg", f"asd_{tag}_s0", f"asd_{tag}_s1", f"asd_{tag}_bg"}
    names |= {"hd_k1", "nsd_k1", "asd_k1"} | {f"{m}_k5_b{b}" for m in ("hd", "hd95", "nsd", "asd") for b in (0, 1)}
    for m in ("hd", "nsd", "asd"):
        names |= {f"cls_{m}_calls"} | {f"cls_{m}_{red}_nn" for red in REDUCTIONS}
        if m != "asd":
            names |= {f"cls_{m}_{red}{suffix}" for red in REDUCTIONS for suffix in ("", "_after_reset")}
    toleranced = {n for n in names if n.startswith("asd_") or n == "cls_asd_calls"}
    for shape in SPACED_SHAPES:
        tag = _tag(shape)
        sp = {f"sp_hd_{tag}_p{pc}" for pc in (None, 95, 50)} | {f"sp_hd_{tag}_scalar", f"sp_asd_{tag}"}
        names |= sp
        toleranced |= sp
    extra = {"edges_" + _tag(s) for s in SHAPES} | {"edt_12x13", "edt_12x13_sampling", "edt_17x16x15", "edt_17x16x15_sampling"}
    assert set(g.files) == names | extra | {n + "_truth" for n in toleranced} | {n + "_ref_err" for n in toleranced}
    return len(names)


def case_spaced_percentiles_vs_truth(device):
    """Percentile Hausdorff distances WITH a spacing against the float64 truth t (numpy percentile of scipy's float64 distances) under the rule the
    issue sets: |ours - t| <= one float32 ulp (2^-23 |t|) and |ours - ref| <= |ref - t| + 2^-23 |t|.  The reference's own float32 quantile is 2.24 ulp
    from t on sp_hd_12x13_p95 (its distance is part of the golden); the product interpolates in float64 over the float32 distances and rounds once:
    each neighbour is within 2^-24 of its truth, so is their convex combination, and the final rounding adds 2^-24."""
    import monai_amd.metrics as ours

    g = np.load(os.path.join(GOLDEN, "surface_metrics.npz"))
    return _compare_with_golden(run_toleranced(ours, device, percentiles=True), g)


def case_edt_transform_vs_reference(device):
    """the transform and the function on C = 2 images against the reference's (scipy, float64) output: float64_distances=True bit-equal at unit
    spacing, float32 its cast; with a sampling within 8 * 2^-53 (the bound of `case_edt_vs_brute_force`); MetaTensor-free plain tensors in and out"""
    import monai_amd.transforms as T

    g = np.load(os.path.join(GOLDEN, "surface_metrics.npz"))
    for shape in ((12, 13), (17, 16, 15)):
        img = torch.from_numpy(np.stack([blobs(shape, 70), ~blobs(shape, 71)])).float().to(device)
        tag = _tag(shape)
        ref = g[f"edt_{tag}"]
        assert ref.dtype == np.float64
        got = T.distance_transform_edt(img, float64_distances=True)
        assert got.dtype == torch.float64 and got.device == img.device
        np.testing.assert_array_equal(_np(got), ref)
        for out in (T.distance_transform_edt(img), T.DistanceTransformEDT()(img), T.DistanceTransformEDTd(keys="m")({"m": img, "other": 1})["m"]):
            assert out.dtype == torch.float32
            np.testing.assert_array_equal(_np(out), ref.astype(np.float32))
        sp = spacing_of(shape)
        refs = g[f"edt_{tag}_sampling"]
        got = _np(T.distance_transform_edt(img, sampling=sp, float64_distances=True))
        assert (np.abs(got - refs) <= 16 * 2.0 ** -53 * refs).all()      # both sides are within 8 units of the truth
        got = _np(T.DistanceTransformEDT(sampling=sp)(img)).astype(np.float64)
        assert (np.abs(got - refs) <= np.spacing(refs.astype(np.float32)).astype(np.float64) + 16 * 2.0 ** -53 * refs).all()
    full = torch.ones((1, 4, 5), device=device)
    assert bool(torch.isinf(T.distance_transform_edt(full)).all())      # no background voxel: +inf (documented; scipy's output there is an artefact)


# ---------------------------------------------------------------------------------------------------------------- label maps, determinism
def case_label_maps_equal_onehots(device):
    """ops.surface_records on uint8 / int64 / float label maps == the same call on their float one-hots, bit for bit, in every mix of the two sides; three
    device-to-host reads at most, whatever B and K"""
    from monai_amd import ops

    shape, k = (17, 16, 15), 5
    lp = torch.cat([labels5(shape, 40), labels5(shape, 50)]).to(device)
    ly = torch.cat([labels5(shape, 60), labels5(shape, 50)]).to(device)
    op, oy = onehot(lp.cpu(), k).to(device), onehot(ly.cpu(), k).to(device)
    thr = [0.0, 1.0, SQRT2, 2.0, 3.0]
    base = ops.surface_records(op, oy, k, thresholds=thr, want_distances=True)
    assert base.reads == 3 and bool(base.present.all()) and float(base.records[..., 0].min()) > 0
    for a, b in ((lp, ly), (lp.long(), oy), (op.bool(), ly.float()), (op.to(torch.uint8), ly)):
        r = ops.surface_records(a, b, k, thresholds=thr, want_distances=True)
        assert torch.equal(r.records, base.records) and torch.equal(r.present, base.present) and r.reads == 3
        assert set(r.distances) == set(base.distances) and all(torch.equal(r.distances[key], base.distances[key]) for key in base.distances)
    sub = ops.surface_records(lp, ly, k, thresholds=thr[1:], first_class=1, symmetric=False)
    assert sub.reads == 2 and torch.equal(sub.records[:, :, 0], base.records[:, 1:, 0]) and float(sub.records[:, :, 1].abs().max()) == 0.0
    one = ops.surface_records(lp[:1], ly[:1], k, thresholds=thr)
    assert one.reads == 2 and torch.equal(one.records, base.records[:1])


def case_inferer_labels_to_surface(device):
    """a 2-window sliding_window_argmax label map goes straight into ops.surface_records and scores exactly like its float one-hot"""
    from monai_amd import ops
    from monai_amd.inferers.utils import sliding_window_argmax

    k = 3
    gen = torch.Generator().manual_seed(4600)
    vol = torch.randn((1, 1, 8, 8, 12), generator=gen).to(device)
    w = torch.tensor([1.0, -1.0, 0.25], device=device).reshape(1, k, 1, 1, 1)

    def predictor(x):
        return x * w + torch.tensor([0.0, 0.1, 0.3], device=x.device).reshape(1, k, 1, 1, 1)

    labels = sliding_window_argmax(vol, (8, 8, 8), 1, predictor, overlap=0.25, labels_dtype=torch.uint8)
    assert labels.dtype == torch.uint8 and torch.unique(labels).tolist() == [0, 1, 2]
    truth = torch.randint(0, k, (1, 1, 8, 8, 12), generator=gen).to(torch.uint8).to(device)
    got = ops.surface_records(labels, truth, k, thresholds=[1.0] * k)
    exp = ops.surface_records(onehot(labels.cpu(), k).to(device), onehot(truth.cpu(), k).to(device), k, thresholds=[1.0] * k)
    assert torch.equal(got.records, exp.records) and float(got.records[..., 0].min()) > 0


def case_deterministic(device):
    """two calls on (2, 70, 66) blobs: bitwise equal records, compacted distances and distance fields"""
    from monai_amd import ops

    p, y = (t[7:8].contiguous().to(device) for t in batch((2, 70, 66)))
    a = ops.surface_records(p, y, 2, spacing=[[0.8, 1.25, 2.5]], thresholds=[1.0, 2.0], want_distances=True)
    b = ops.surface_records(p, y, 2, spacing=[[0.8, 1.25, 2.5]], thresholds=[1.0, 2.0], want_distances=True)
    assert torch.equal(a.records, b.records) and all(torch.equal(a.distances[key], b.distances[key]) for key in a.distances)
    assert float(a.records[..., 0].min()) > 256      # more than one 256-voxel trip holds edge voxels
    for kw in ({}, {"sampling": [0.8, 1.25, 2.5]}):
        f1, f2 = ops.edt(p[0], **kw), ops.edt(p[0], **kw)
        assert torch.equal(f1, f2)


# ---------------------------------------------------------------------------------------------------------------- API
def case_surface_api(device, device_is_real=True):
    """the reference's errors and warnings, the explicit errors of what is not on the HIP path, the attribute names of the three classes"""
    import pytest

    import monai_amd.metrics as m
    import monai_amd.transforms as T
    from monai_amd._fallback import UnsupportedOnDevice

    x = torch.zeros((2, 3, 4, 4), device=device)
    x[:, 1, 1:3, 1:3] = 1
    x[:, 0] = 1 - x[:, 1]
    with pytest.raises(ValueError, match="y_pred and y should have same shapes"):
        m.compute_hausdorff_distance(x, x[:, :, :2].contiguous())
    with pytest.raises(ValueError, match="y_pred and y should have same shapes"):
        m.compute_average_surface_distance(x, x[:, :2].contiguous())
    with pytest.raises(ValueError, match="should have same shape, but instead, shapes are"):
        m.compute_surface_dice(x, x[:, :, :2].contiguous(), [1.0, 1.0])
    with pytest.raises(ValueError, match="at least three dimensions"):
        m.HausdorffDistanceMetric()(x[:, :, 0, 0], x[:, :, 0, 0])
    with pytest.raises(ValueError, match="at least three dimensions"):
        m.SurfaceDistanceMetric()(x[:, :, 0, 0], x[:, :, 0, 0])
    with pytest.raises(ValueError, match=r"one-hot encoded: \[B,C,H,W\] or \[B,C,H,W,D\]"):
        m.SurfaceDiceMetric([1.0, 1.0])(x[:, :, 0], x[:, :, 0])
    with pytest.raises(ValueError, match="y_pred and y must be PyTorch Tensor"):
        m.compute_surface_dice(x, [1.0], [1.0, 1.0])
    with pytest.raises(ValueError, match=r"number of classes \(2\) does not match number of class thresholds \(1\)"):
        m.compute_surface_dice(x, x, [1.0])
    with pytest.raises(ValueError, match="All class thresholds need to be finite"):
        m.compute_surface_dice(x, x, [1.0, float("inf")])
    with pytest.raises(ValueError, match="All class thresholds need to be >= 0"):
        m.compute_surface_dice(x, x, [1.0, -0.5])
    with pytest.raises(ValueError, match="percentile should be a value between 0 and 100, get 101"):
        m.compute_hausdorff_distance(x, x, percentile=101)
    for cls in (m.HausdorffDistanceMetric, m.SurfaceDistanceMetric, lambda: m.SurfaceDiceMetric([1.0])):
        with pytest.raises(ValueError, match="the data to aggregate must be PyTorch Tensor"):
            cls().aggregate()
    # every prepare_spacing message (host only)
    assert m.prepare_spacing(None, 2, 3) == [None, None] and m.prepare_spacing(0.8, 2, 3) == [0.8, 0.8]
    assert m.prepare_spacing([0.8, 0.5, 0.9], 2, 3) == [[0.8, 0.5, 0.9]] * 2 and m.prepare_spacing([[1, 2], [3, 4]], 2, 2) == [[1, 2], [3, 4]]
    for bad, msg in (
        ([0.8, [0.5, 0.9]], "its elements should be of same type"),
        ([[1.0, 2.0]], r"the outer sequence should have same length as batch size \(2\)"),
        ([[1.0, 2.0], [1.0, 2.0]], r"should either have same length asimage dim \(3\)"),
        ([["a", "b", "c"], ["a", "b", "c"]], "the elements should be integers or floats"),
        ([0.8, 0.5], r"it should have same length as image dim \(3\)"),
        (["a", "b", "c"], "unsupported type"),
        ("abc", "should either be a number, a sequence of numbers or a sequence of sequences"),
    ):
        with pytest.raises(ValueError, match=msg):
            m.prepare_spacing(bad, 2, 3)
    with pytest.raises(ValueError, match="same length as image dim"):
        m.compute_hausdorff_distance(x, x, spacing=[1.0, 2.0, 3.0])
    # the two "all 0" warnings, with the class index the reference names (after the background is dropped)
    empty = torch.zeros_like(x)
    empty[:, 0] = 1
    with pytest.warns(UserWarning, match="the ground truth of class 0 is all 0, this may result in nan/inf distance"):
        m.compute_hausdorff_distance(x[:, :2].contiguous(), empty[:, :2].contiguous())
    with pytest.warns(UserWarning, match="the prediction of class 1 is all 0, this may result in nan/inf distance"):
        r = m.compute_average_surface_distance(empty, x, include_background=True)
    assert tuple(r.shape) == (2, 3) and bool(torch.isinf(r[:, 1]).all()) and bool(torch.isnan(r[:, 2]).all()) and r.device == x.device
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert float(m.compute_hausdorff_distance(x[:, :2].contiguous(), x[:, :2].contiguous()).abs().max()) == 0.0
    # not on the HIP path: the explicit errors (the test environment pins MONAI_AMD_NO_FALLTHROUGH=1)
    for dm in ("chessboard", "taxicab"):
        with pytest.raises(NotImplementedError, match="chamfer"):
            m.compute_hausdorff_distance(x, x, distance_metric=dm)
        with pytest.raises(NotImplementedError, match="chamfer"):
            m.SurfaceDistanceMetric(distance_metric=dm)(x, x)
    with pytest.raises(NotImplementedError, match="use_subvoxels"):
        m.compute_surface_dice(x, x, [1.0, 1.0], use_subvoxels=True)
    with pytest.raises(NotImplementedError, match="device tensors"):
        m.compute_hausdorff_distance(x.cpu().numpy(), x.cpu().numpy())
    with pytest.raises(NotImplementedError, match="return_indices"):
        T.distance_transform_edt(x[0], return_indices=True)
    with pytest.raises(NotImplementedError, match="caller-supplied"):
        T.distance_transform_edt(x[0], distances=torch.zeros_like(x[0]))
    with pytest.raises(RuntimeError, match="Neither return_distances nor return_indices True"):
        T.distance_transform_edt(x[0], return_distances=False)
    with pytest.raises(RuntimeError, match="Wrong input dimensionality"):
        T.distance_transform_edt(x[0, 0])
    with pytest.raises(RuntimeError, match="extent of 2049"):
        from monai_amd import ops

        ops.edt(torch.zeros((1, 1, 2049), dtype=torch.uint8, device=device))      # int32 squared distances: axes up to 2048, refused before a launch
    if device_is_real:
        for call in (lambda: m.compute_hausdorff_distance(x.cpu(), x.cpu()), lambda: m.SurfaceDistanceMetric()(x.cpu(), x.cpu()),
                     lambda: m.compute_surface_dice(x.cpu(), x.cpu(), [1.0, 1.0]), lambda: T.distance_transform_edt(x[0].cpu()),
                     lambda: m.get_mask_edges(x[0, 1].cpu(), x[0, 1].cpu())):
            with pytest.raises(UnsupportedOnDevice):
                call()
    # the utilities
    ep, et = m.get_mask_edges(x[0, 1], x[0, 1] * 2, label_idx=1)
    assert ep.dtype == torch.bool and tuple(ep.shape) == (4, 4) and int(ep.sum()) == 4 and not bool(et.any())      # cropped: the 2 x 2 square plus margin 1
    ep, _ = m.get_mask_edges(x[0, 0], x[0, 0], crop=False)
    assert tuple(ep.shape) == (4, 4) and int(ep.sum()) == 12
    big, _ = m.get_mask_edges(x[0, 0], x[0, 0])
    assert tuple(big.shape) == (6, 6) and int(big.sum()) == 12                                                     # the box leaves the image: padded
    (e1, e2), dist, areas = m.get_edge_surface_distance(x[0, 1], x[0, 0], symmetric=True, class_index=3)
    assert areas == () and len(dist) == 2 and dist[0].dtype == torch.float32 and float(dist[0].max()) == 1.0 and int(dist[0].numel()) == 4
    d = m.get_surface_distance(e1, torch.zeros_like(e1))
    assert d.numel() == 4 and bool(torch.isinf(d).all())
    # API shell: names and attributes of the reference's classes
    h = m.HausdorffDistanceMetric(include_background=True, distance_metric="euclidean", percentile=95, directed=True, reduction="sum", get_not_nans=True)
    assert (h.include_background, h.distance_metric, h.percentile, h.directed, h.reduction, h.get_not_nans) == (True, "euclidean", 95, True, "sum", True)
    s = m.SurfaceDistanceMetric()
    assert (s.include_background, s.symmetric, s.distance_metric, s.reduction, s.get_not_nans) == (False, False, "euclidean", "mean", False)
    n = m.SurfaceDiceMetric(class_thresholds=[1.0, 2.0])
    assert (n.class_thresholds, n.include_background, n.distance_metric, n.reduction, n.get_not_nans, n.use_subvoxels) == ([1.0, 2.0], False, "euclidean", "mean", False, False)
    assert m.HausdorffDistanceMetric().include_background is False and m.HausdorffDistanceMetric().percentile is None
    for obj in (h, s, n):
        assert isinstance(obj, m.CumulativeIterationMetric) and str(obj) == type(obj).__name__
    assert T.DistanceTransformEDT(sampling=2.0).sampling == 2.0 and T.DistanceTransformEDTd(keys=["a"], sampling=[1, 2]).sampling == [1, 2]
    assert T.DistanceTransformEDTD is T.DistanceTransformEDTd and T.DistanceTransformEDTDict is T.DistanceTransformEDTd
    hd = m.HausdorffDistanceMetric(include_background=True, reduction="none")
    out = hd(x, x, spacing=[2.0, 3.0])
    assert tuple(out.shape) == (2, 3) and out.device == x.device and out.dtype == torch.float32 and bool(torch.isnan(out[:, 2]).all())
