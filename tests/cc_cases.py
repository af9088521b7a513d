"""Shared cases of tests/test_cc_post_emu.py (SIMT emulator) and tests/test_cc_post_gpu.py (MI355X): the connected-component kernels
(monai_amd/csrc/kernels/ccl.h) against an independent partition, and KeepLargestConnectedComponent / FillHoles / LabelFilter against the golden file
tests/golden/cc_post.npz (tests/golden/make_golden_cc.py).

The reference partition is `canonical`: every voxel carries 1 + the smallest linear index of its component, from a plain numpy minimum propagation
(the smallest label goes to the voxel a label names and everybody jumps there, so a one-voxel-wide path through the whole volume takes a logarithmic
number of rounds).  Nothing here uses the code under test."""
import functools
import itertools
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cc_post.npz")

EMU_SHAPES = ((17, 16, 15), (5, 7, 70))          # the second: rows longer than a wave
GPU_SHAPE = (37, 41, 150)                        # several workgroups along every axis, rows of more than two waves
EMU_SHAPES_2D = ((16, 15), (7, 70))
GPU_SHAPE_2D = (41, 150)


# ------------------------------------------------------------------------------------------------------------------ the independent partition
def offsets(rank, conn):
    return [o for o in itertools.product((-1, 0, 1), repeat=rank) if 0 < sum(abs(v) for v in o) <= conn]


def canonical(cls, conn):
    """cls: integer class ids (0 background) of rank 2 or 3 -> int32 labels, 0 for background, else 1 + the smallest C-order index of the component"""
    cls = np.asarray(cls)
    n, shape = cls.size, cls.shape
    lab = np.where(cls > 0, np.arange(n, dtype=np.int64).reshape(shape), n)
    pairs = []
    for o in offsets(cls.ndim, conn):
        dst = tuple(slice(max(0, -v), shape[a] - max(0, v)) for a, v in enumerate(o))
        src = tuple(slice(max(0, v), shape[a] - max(0, -v)) for a, v in enumerate(o))
        pairs.append((dst, src, (cls[dst] == cls[src]) & (cls[dst] > 0)))
    flat = lab.reshape(-1)
    fg = np.flatnonzero(flat < n)
    while True:
        cand = lab.copy()
        for dst, src, same in pairs:             # the smallest label among a voxel and its neighbours of the same class
            np.minimum(cand[dst], np.where(same, lab[src], n), out=cand[dst])
        cflat = cand.reshape(-1)
        new = flat.copy()
        np.minimum.at(new, flat[fg], cflat[fg])  # the voxel a label names takes the smallest label any voxel of that label has seen ...
        new[fg] = np.minimum(new[fg], cflat[fg])
        while True:                              # ... and everybody jumps to the label of the voxel its label names, until nothing moves
            nxt = new[new[fg]]
            if np.array_equal(nxt, new[fg]):
                break
            new[fg] = nxt
        if np.array_equal(new, flat):
            break
        flat[:] = new
    return np.where(cls > 0, lab + 1, 0).astype(np.int32)


def records_of(labels, rank):
    """(sizes, border) at root positions from a canonical label array of one item (leading axes of extent 1 beyond `rank` are no border)"""
    flat = labels.reshape(-1)
    sizes = np.zeros(flat.size, dtype=np.int32)
    counts = np.bincount(flat)[1:]
    sizes[: counts.size] = counts
    edge = np.zeros(labels.shape, dtype=bool)
    for a in range(labels.ndim - rank, labels.ndim):
        sl = [slice(None)] * labels.ndim
        for side in (0, labels.shape[a] - 1):
            sl[a] = side
            edge[tuple(sl)] = True
    border = np.zeros(flat.size, dtype=bool)
    border[np.unique(flat[edge.reshape(-1) & (flat > 0)]) - 1] = True
    return sizes, border


# ------------------------------------------------------------------------------------------------------------------ masks
def serpentine(shape):
    """one voxel wide, through the whole volume: full rows on every other row of every other plane, joined at alternating ends"""
    m = np.zeros(shape, dtype=bool)
    v = m.reshape((1,) * (3 - m.ndim) + shape)
    d, h, w = v.shape
    x_end, y_up = w - 1, True
    for z in range(0, d, 2):
        ys = list(range(0, h, 2))
        ys = ys if y_up else ys[::-1]
        for k, y in enumerate(ys):
            v[z, y, :] = True
            if k + 1 < len(ys):
                v[z, (y + ys[k + 1]) // 2, x_end] = True
                x_end = 0 if x_end else w - 1
        if z + 1 < d:
            v[z + 1, ys[-1], x_end] = True                       # on to the next plane from the end the last row ran to
            x_end = 0 if x_end else w - 1
        y_up = not y_up
    return m


def masks(shape, seed=0):
    """name -> bool mask of `shape` (rank 2 or 3)"""
    rng = np.random.default_rng(1000 + seed + sum(shape))
    rank = len(shape)
    out = {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool)}
    one = np.zeros(shape, bool)
    one[tuple(s // 2 for s in shape)] = True
    out["single"] = one
    out["checkerboard"] = (np.indices(shape).sum(0) % 2).astype(bool)
    touch = np.zeros(shape, bool)
    if rank == 3:
        touch[0:2, 0:2, 0:2] = True       # A
        touch[2:4, 2:4, 0:2] = True       # B meets A only across an edge (two hops)
        touch[4:5, 4:6, 2:4] = True       # C meets B only across a corner (three hops)
    else:
        touch[0:2, 0:2] = True
        touch[2:4, 2:4] = True            # across a corner of the plane (two hops)
        touch[0:2, 5:7] = True            # apart
    out["touch"] = touch
    out["serpentine"] = serpentine(shape)
    u = np.zeros(shape, bool)
    u[..., 0, :] = True
    u[..., -1, :] = True
    if rank == 3:
        u[-1] = True                      # the two arms meet in the last plane only
    else:
        u[:, -1] = True
    out["u"] = u
    for dens in (0.1, 0.35, 0.6):
        out[f"random{dens}"] = rng.random(shape) < dens
    tail, head = np.zeros(shape, bool), np.zeros(shape, bool)
    tail[(-1,) * rank] = tail[(-1,) * (rank - 1) + (-2,)] = True
    head[(0,) * rank] = head[(0,) * (rank - 1) + (1,)] = True
    out["tail"], out["head"] = tail, head      # adjacent items: the last voxels of one and the first of the next are foreground and must not join
    return out


def thin_shapes(shape):
    return [shape[:a] + (1,) + shape[a + 1:] for a in range(len(shape))]


def blobs_labels(shape, k, seed, speckle=True):
    """a label map with classes 1 .. k: smooth blobs plus speckle -- single voxels, or (speckle=False) a few rods of lengths that are all different,
    so that the largest components of every class and of their union have different sizes"""
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    f = np.stack([ndimage.uniform_filter(rng.random(shape), 5, mode="constant") for _ in range(k)])
    lab = np.where(f.max(0) > np.quantile(f.max(0), 0.55), f.argmax(0) + 1, 0)
    if speckle:
        sp = rng.random(shape) < 0.06
        lab[sp] = rng.integers(0, k + 1, size=int(sp.sum()))
    else:
        for c in range(1, k + 1):
            for length in (c, c + k, c + 2 * k):
                at = [int(rng.integers(0, s)) for s in shape]
                at[-1] = int(rng.integers(0, shape[-1] - length + 1))
                lab[tuple(at[:-1]) + (slice(at[-1], at[-1] + length),)] = c
    return lab.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ kernel cases
def _label_batch(mask_list, conn, device, dtype=torch.uint8, rule=None, **row):
    from monai_amd import ops

    shape = mask_list[0].shape
    src = torch.from_numpy(np.stack(mask_list)).to(dtype).to(device)
    n = int(np.prod(shape))
    items = ops.CcItems(shape, [dict(src=k * n, rule=ops.CC_GT if rule is None else rule, **row) for k in range(len(mask_list))], device)
    labels = ops.cc_label(src, items, conn)
    return src, items, labels


@functools.lru_cache(maxsize=None)
def _reference(shape, conn):
    ms = masks(shape)
    return tuple(ms), tuple(canonical(m.astype(np.int8), conn) for m in ms.values())


def case_labels_vs_partition(device, shape, conn, twice=False):
    """every mask of `masks(shape)` as one item of ONE call: int32 labels equal to the canonical partition, records equal to bincount / a direct border test"""
    from monai_amd import ops

    names, refs = _reference(shape, conn)
    ms = masks(shape)
    src, items, labels = _label_batch([ms[k] for k in names], conn, device)
    assert labels.dtype == torch.int32
    got = labels.cpu().numpy().reshape((len(names),) + shape)
    for k, name in enumerate(names):
        assert np.array_equal(got[k], refs[k]), (name, shape, conn, int((got[k] != refs[k]).sum()))
    sizes, border = ops.cc_records(labels, items)
    sizes, border = sizes.cpu().numpy().reshape(len(names), -1), border.cpu().numpy().reshape(len(names), -1)
    for k, name in enumerate(names):
        s, b = records_of(refs[k], len(shape))
        assert np.array_equal(sizes[k], s) and np.array_equal(border[k], b), (name, shape, conn)
    if twice:
        labels2 = ops.cc_label(src, items, conn)
        sizes2, border2 = ops.cc_records(labels2, items)
        assert torch.equal(labels, labels2) and np.array_equal(sizes2.cpu().numpy().reshape(sizes.shape), sizes) and np.array_equal(border2.cpu().numpy().reshape(border.shape), border)
    ncomp = [int((np.unique(r) > 0).sum()) for r in refs]
    cb = names.index("checkerboard")
    if conn == 1:
        assert ncomp[cb] == ms["checkerboard"].sum()      # every voxel its own component
    if conn == len(shape):
        assert ncomp[cb] == 1
    t = names.index("touch")
    assert ncomp[t] == {1: 3, 2: 2, 3: 1}[conn], (ncomp[t], conn)      # only across an edge: two hops; only across a corner: three
    assert ncomp[names.index("serpentine")] == 1 and ncomp[names.index("u")] == 1
    return len(names)


def case_thin_volumes(device, shape):
    """extents of 1 along each axis, every connectivity"""
    rng = np.random.default_rng(77)
    n = 0
    for sh in thin_shapes(shape):
        m = [rng.random(sh) < 0.45 for _ in range(2)]
        for conn in range(1, len(sh) + 1):
            _, _, labels = _label_batch(m, conn, device)
            got = labels.cpu().numpy().reshape((2,) + sh)
            for k in range(2):
                assert np.array_equal(got[k], canonical(m[k].astype(np.int8), conn)), (sh, conn)
                n += 1
    return n


def case_rules_and_dtypes(device, shape):
    """the five rules on float32 / uint8 / int64 / bool sources; CC_LIST_VALUE labels every listed class in one pass"""
    from monai_amd import ops

    rng = np.random.default_rng(5)
    vals = rng.choice(np.array([0, 1, 2, 3, 7]), size=shape, p=[0.3, 0.25, 0.2, 0.15, 0.1])
    conn = len(shape)
    n = 0
    for dtype in (torch.float32, torch.uint8, torch.int64):
        for rule, row, cls in ((ops.CC_GT, {}, vals > 0), (ops.CC_EQ, {"v": 2.0}, vals == 2), (ops.CC_NE, {"v": 2.0}, vals != 2),
                               (ops.CC_LIST_ANY, {"labels": [7, 1]}, np.isin(vals, [7, 1])),
                               (ops.CC_LIST_VALUE, {"labels": [7, 1, 2]}, np.select([vals == 7, vals == 1, vals == 2], [1, 2, 3], 0))):
            _, _, labels = _label_batch([vals], conn, device, dtype=dtype, rule=rule, **row)
            assert np.array_equal(labels.cpu().numpy().reshape(shape), canonical(cls.astype(np.int8), conn)), (dtype, rule)
            n += 1
        _, _, labels = _label_batch([vals], conn, device, dtype=dtype, rule=ops.CC_VALUE)      # every non-zero value its own class
        assert np.array_equal(labels.cpu().numpy().reshape(shape), canonical(vals.astype(np.int8), conn)), dtype
        # one table, a rule per row, on the same non-binary volume: rows that tell classes apart by value next to rows that do not
        rows = [dict(src=0, rule=ops.CC_LIST_VALUE, labels=[7, 1, 2]), dict(src=0, rule=ops.CC_GT), dict(src=0, rule=ops.CC_VALUE),
                dict(src=0, rule=ops.CC_LIST_ANY, labels=[3, 2]), dict(src=0, rule=ops.CC_NE, v=1.0)]
        exp = [np.select([vals == 7, vals == 1, vals == 2], [1, 2, 3], 0), vals > 0, vals, np.isin(vals, [3, 2]), vals != 1]
        src = torch.from_numpy(vals).to(dtype).to(device)
        got = ops.cc_label(src, ops.CcItems(shape, rows, device), conn).cpu().numpy().reshape((len(rows),) + shape)
        for k, cls in enumerate(exp):
            assert np.array_equal(got[k], canonical(np.asarray(cls).astype(np.int8), conn)), (dtype, "mixed table, row", k)
        n += 2
    _, _, labels = _label_batch([vals > 1], 1, device, dtype=torch.bool)
    assert np.array_equal(labels.cpu().numpy().reshape(shape), canonical((vals > 1).astype(np.int8), 1))
    return n + 1


def case_canonical_vs_scipy():
    """the independent partition itself against scipy.ndimage.label (same components, relabelled to the smallest index)"""
    from scipy import ndimage

    n = 0
    for shape in EMU_SHAPES + EMU_SHAPES_2D:
        for conn in range(1, len(shape) + 1):
            for name, m in masks(shape).items():
                lab, k = ndimage.label(m, ndimage.generate_binary_structure(len(shape), conn))
                exp = np.zeros(shape, np.int32)
                if k:
                    first = ndimage.minimum(np.arange(m.size).reshape(shape), lab, np.arange(1, k + 1)).astype(np.int64)
                    exp = np.where(lab > 0, np.concatenate([[0], first + 1])[lab], 0).astype(np.int32)
                assert np.array_equal(canonical(m.astype(np.int8), conn), exp), (name, shape, conn)
                n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------ golden cases of the transforms
DTYPES = {"float32": torch.float32, "uint8": torch.uint8, "int64": torch.int64}
SEEDS = (31, 30)      # of the two label maps: chosen so that no case has two components of equal size at the cut (make_golden_cc.py asserts it)


def inputs():
    """name -> int64 array [C, spatial...]: label maps (C = 1) and their one-hot forms"""
    out = {}
    lab3 = blobs_labels((10, 11, 13), 3, SEEDS[0], speckle=False)
    lab3[4:9, 3:9, 3:10][(lab3[4:9, 3:9, 3:10] == 0)] = 2
    lab3[5:8, 4:8, 5:8] = 1                           # label 1 fully enclosed by label 2
    lab3[6, 6, 6] = 0                                 # and a hole inside it
    lab2 = blobs_labels((23, 27), 3, SEEDS[1], speckle=False)
    ring = np.array([[0, 1, 1, 1, 0, 0, 0], [1, 1, 0, 1, 0, 3, 3], [1, 0, 1, 1, 0, 3, 0], [1, 1, 1, 0, 0, 3, 3]])      # holes open only through a diagonal
    lab2[0:4, 0:7] = 0
    lab2[2:6, 10:17] = ring
    out["lab3"], out["lab2"] = lab3[None], lab2[None]
    for k in ("lab3", "lab2"):
        out["oh" + k[3]] = np.stack([(out[k][0] == c) for c in range(4)]).astype(np.int64)
    # the four worked examples of the reference's class docstring, as data
    out["doc3"] = np.array([[[1, 0, 0], [0, 1, 1], [0, 1, 1]]])
    out["doc5"] = np.array([[[0, 0, 1, 0, 0], [0, 2, 1, 1, 1], [1, 2, 1, 0, 0], [1, 2, 0, 1, 0], [2, 2, 0, 0, 2]]])
    hole3 = np.zeros((1, 7, 7, 7), np.int64)
    hole3[0, 1:6, 1:6, 1:6] = 2
    hole3[0, 2:5, 2:5, 2:5] = 0                       # a cavity in a shell ...
    hole3[0, 1, 1, 1] = 0                             # ... whose corner voxel is missing: the cavity is open only through a diagonal of three hops
    out["hole3"] = hole3
    return out


def golden_cases():
    """the manifest: dicts with an `id`; what make_golden_cc.py runs on the reference and the tests run on the product"""
    cases = []
    for name in ("lab3", "lab2", "oh3", "oh2"):
        rank = 3 if name.endswith("3") else 2
        explicit = name.startswith("oh")
        for conn in [None] + list(range(1, rank + 1)):
            for applied in (None, (1, 2)):
                cases.append(dict(kind="fill", inp=name, dtype="float32", applied=applied, conn=conn))
                for nc in (1, 2):
                    for independent in (True, False):
                        cases.append(dict(kind="keep", inp=name, dtype="float32", applied=applied, onehot=None, independent=independent, conn=conn, nc=nc))
                        if conn is None:
                            cases.append(dict(kind="keep", inp=name, dtype="float32", applied=applied, onehot=explicit, independent=independent, conn=conn, nc=nc))
                            for dtype in ("uint8", "int64"):
                                cases.append(dict(kind="keep", inp=name, dtype=dtype, applied=applied, onehot=None, independent=independent, conn=conn, nc=nc))
        cases.append(dict(kind="fill", inp=name, dtype="uint8", applied=(2,), conn=1))
        cases.append(dict(kind="fill", inp=name, dtype="int64", applied=None, conn=None))
        cases.append(dict(kind="filter", inp=name, dtype="float32", applied=(1, 3)))
        cases.append(dict(kind="filter", inp=name, dtype="int64", applied=(2,)))
    for conn in (None, 1, 2, 3):
        cases.append(dict(kind="fill", inp="hole3", dtype="uint8", applied=None, conn=conn))
    cases.append(dict(kind="keep", inp="doc3", dtype="float32", applied=(1,), onehot=False, independent=True, conn=1, nc=1))
    cases.append(dict(kind="keep", inp="doc5", dtype="float32", applied=(1, 2), onehot=False, independent=False, conn=1, nc=1))
    cases.append(dict(kind="keep", inp="doc5", dtype="float32", applied=(1, 2), onehot=False, independent=True, conn=1, nc=1))
    cases.append(dict(kind="keep", inp="doc5", dtype="float32", applied=(1, 2), onehot=False, independent=False, conn=2, nc=1))
    for c in cases:
        c["id"] = "|".join(f"{k}={c[k]}" for k in sorted(c))
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


DOC_EXPECTED = {      # the right-hand sides of the four docstring examples
    0: [[0, 0, 0], [0, 1, 1], [0, 1, 1]],
    1: [[0, 0, 1, 0, 0], [0, 2, 1, 1, 1], [1, 2, 1, 0, 0], [1, 2, 0, 0, 0], [2, 2, 0, 0, 0]],
    2: [[0, 0, 1, 0, 0], [0, 2, 1, 1, 1], [0, 2, 1, 0, 0], [0, 2, 0, 0, 0], [2, 2, 0, 0, 0]],
    3: [[0, 0, 1, 0, 0], [0, 2, 1, 1, 1], [1, 2, 1, 0, 0], [1, 2, 0, 1, 0], [2, 2, 0, 0, 2]],
}


def build(mod, case):
    """the transform of `case` from `mod` (the reference's monai.transforms or monai_amd.transforms)"""
    if case["kind"] == "fill":
        return mod.FillHoles(applied_labels=case["applied"], connectivity=case["conn"])
    if case["kind"] == "filter":
        return mod.LabelFilter(case["applied"])
    return mod.KeepLargestConnectedComponent(applied_labels=case["applied"], is_onehot=case["onehot"], independent=case["independent"], connectivity=case["conn"],
                                             num_components=case["nc"])


def run_case(mod, case, device, ins=None):
    x = torch.from_numpy((ins or inputs())[case["inp"]]).clone().to(DTYPES[case["dtype"]]).to(device)
    before = x.clone()
    out = build(mod, case)(x)
    return x, before, out


@functools.lru_cache(maxsize=None)
def golden():
    """id -> the reference's output (the file holds them stacked per input, in the order of the manifest)"""
    z = np.load(GOLDEN)
    out, at = {"manifest": json.loads(str(z["manifest"]))}, {}
    cases = {c["id"]: c for c in golden_cases()}
    for cid in out["manifest"]:
        inp = cases[cid]["inp"]
        out[cid] = z["out|" + inp][at.get(inp, 0)]
        at[inp] = at.get(inp, 0) + 1
    return out


def case_transforms_vs_golden(device, kind, part=0, parts=1):
    """bit-equal to what the reference's own classes gave (tests/golden/make_golden_cc.py); the dtype and the in-place / new-tensor behaviour included"""
    import monai_amd.transforms as T

    g, ins = golden(), inputs()
    manifest = g["manifest"]
    mine = [c for c in golden_cases() if c["kind"] == kind]
    assert [c["id"] for c in golden_cases()] == manifest, "tests/golden/cc_post.npz is not the file make_golden_cc.py writes for these cases"
    n = 0
    for c in mine[part::parts]:
        x, before, out = run_case(T, c, device, ins)
        exp = g[c["id"]]
        assert out.dtype == DTYPES[c["dtype"]] and out.device == x.device and tuple(out.shape) == exp.shape, c["id"]
        assert np.array_equal(out.cpu().numpy().astype(np.int64), exp.astype(np.int64)), (c["id"], int((out.cpu().numpy() != exp).sum()))
        if kind == "keep":
            assert out is x                                   # written into the input, as the reference does
        else:
            assert torch.equal(x, before) and out.data_ptr() != x.data_ptr()      # a new tensor, the device input untouched
        n += 1
    return n


def case_doc_examples(device):
    import monai_amd.transforms as T

    docs = [c for c in golden_cases() if c["inp"].startswith("doc")]
    assert len(docs) == 4
    for k, c in enumerate(docs):
        _, _, out = run_case(T, c, device)
        assert out[0].cpu().tolist() == DOC_EXPECTED[k], (k, out[0].cpu().tolist())


def case_tie_rule(device):
    """product only: of two components of equal size the one whose first voxel comes LATER is kept"""
    import monai_amd.transforms as T
    from monai_amd.transforms.utils import get_largest_connected_component_mask

    x = torch.zeros((1, 6, 9), device=device)
    x[0, 0, 0:3] = 1
    x[0, 2, 4:7] = 1
    x[0, 5, 1:4] = 1
    x[0, 4, 8] = 1
    out = T.KeepLargestConnectedComponent(applied_labels=[1])(x.clone())
    assert out[0].nonzero().tolist() == [[5, 1], [5, 2], [5, 3]]
    out = T.KeepLargestConnectedComponent(applied_labels=[1], num_components=2)(x.clone())
    assert out[0].nonzero().tolist() == [[2, 4], [2, 5], [2, 6], [5, 1], [5, 2], [5, 3]]
    m = get_largest_connected_component_mask(x[0], num_components=3)
    assert m.dtype == torch.bool and m.nonzero().tolist() == [v for v in x[0].nonzero().tolist() if v != [4, 8]]
    m = get_largest_connected_component_mask(x[0] > 0, num_components=9)      # fewer components than asked for: all of them
    assert torch.equal(m, x[0] > 0)
    # touching regions of different values are different components, as skimage.measure.label reads an integer image
    y = torch.zeros((5, 8), dtype=torch.int64, device=device)
    y[1, 0:5] = 1
    y[2, 0:4] = 2
    y[4, 6:8] = 2
    assert get_largest_connected_component_mask(y).nonzero().tolist() == [[1, 0], [1, 1], [1, 2], [1, 3], [1, 4]]
    assert get_largest_connected_component_mask(y > 0).nonzero().tolist() == (y > 0).nonzero().tolist()[:9]
    # num_components: 0 removes everything (the reference's empty cut); more than 32 per class is not on the HIP path and leaves the input as it was
    assert int(T.KeepLargestConnectedComponent(applied_labels=[1], num_components=0)(x.clone()).count_nonzero()) == 0
    assert int(get_largest_connected_component_mask(x[0], num_components=0).count_nonzero()) == 0
    os.environ["MONAI_AMD_NO_FALLTHROUGH"] = "1"
    try:
        z = x.clone()
        with __import__("pytest").raises(NotImplementedError):
            T.KeepLargestConnectedComponent(applied_labels=[1], num_components=33)(z)
        assert torch.equal(z, x)
    finally:
        os.environ.pop("MONAI_AMD_NO_FALLTHROUGH", None)


def case_dictionary_and_meta(device):
    """the dictionary forms, MetaTensor in -> MetaTensor out, more than 32 classes in a label map, a non-contiguous input"""
    import monai_amd.transforms as T
    from monai_amd.data.meta_tensor import MetaTensor

    ins = inputs()
    lab = torch.from_numpy(ins["lab3"]).float().to(device)
    exp_keep = T.KeepLargestConnectedComponent(applied_labels=[1, 2, 3])(lab.clone())
    exp_fill = T.FillHoles()(exp_keep)
    d = {"pred": MetaTensor(lab.clone()), "other": 1}
    out = T.FillHolesd("pred")(T.KeepLargestConnectedComponentd("pred", applied_labels=[1, 2, 3])(d))
    assert isinstance(out["pred"], MetaTensor) and torch.equal(out["pred"].as_tensor(), exp_fill) and out["other"] == 1
    assert torch.equal(T.LabelFilterd("pred", applied_labels=[2])(d)["pred"].as_tensor(), torch.where(d["pred"].as_tensor() == 2, 2.0, 0.0))
    with __import__("pytest").raises(KeyError):
        T.FillHolesd("missing")(d)
    # 40 classes: two chunks of the 32-label list
    rng = np.random.default_rng(3)
    many = torch.from_numpy(rng.integers(0, 41, size=(1, 12, 13))).to(device)
    got = T.KeepLargestConnectedComponent(connectivity=1)(many.clone())
    exp = many.clone()
    for v in range(1, 41):
        fg = (many[0] == v).cpu().numpy()
        lab_v = canonical(fg.astype(np.int8), 1)
        s, _ = records_of(lab_v, 2)
        key = s.astype(np.int64) * (1 << 32) + np.arange(s.size)
        root = int(np.argmax(np.where(s > 0, key, -1)))
        exp[0][torch.from_numpy(fg & (lab_v != root + 1)).to(device)] = 0
    assert torch.equal(got, exp)
    # a non-contiguous view is still written into
    base = torch.from_numpy(ins["lab2"]).float().to(device)
    wide = torch.zeros((1, 23, 54), device=device)
    view = wide[:, :, ::2]
    view.copy_(base)
    T.KeepLargestConnectedComponent(applied_labels=[1, 2, 3])(view)
    assert torch.equal(view, T.KeepLargestConnectedComponent(applied_labels=[1, 2, 3])(base.clone()))


def case_inferer_labels(device):
    """the inferer's fused-argmax uint8 label map goes straight into KeepLargestConnectedComponent -> FillHoles and gives what its float form gives"""
    import monai_amd.transforms as T
    from monai_amd.inferers.utils import sliding_window_argmax

    k = 3
    gen = torch.Generator().manual_seed(4600)
    vol = torch.randn((1, 1, 8, 8, 12), generator=gen).to(device)
    w = torch.tensor([1.0, -1.0, 0.25], device=device).reshape(1, k, 1, 1, 1)

    def predictor(x):
        return x * w + torch.tensor([0.0, 0.1, 0.3], device=x.device).reshape(1, k, 1, 1, 1)

    labels = sliding_window_argmax(vol, (8, 8, 8), 1, predictor, overlap=0.25, labels_dtype=torch.uint8)[0]
    assert labels.dtype == torch.uint8 and torch.unique(labels).tolist() == [0, 1, 2]
    as_float = labels.float()
    post = lambda t: T.FillHoles(connectivity=1)(T.KeepLargestConnectedComponent(connectivity=1)(t))      # noqa: E731
    a, b = post(labels.clone()), post(as_float)
    assert a.dtype == torch.uint8 and torch.equal(a.float(), b)
    cls = labels[0].cpu().numpy()
    exp = cls.copy()
    for v in (1, 2):
        lab_v = canonical((cls == v).astype(np.int8), 1)
        s, _ = records_of(lab_v, 3)
        key = s.astype(np.int64) * (1 << 32) + np.arange(s.size)
        exp[(cls == v) & (lab_v != int(np.argmax(np.where(s > 0, key, -1))) + 1)] = 0
    kept = T.KeepLargestConnectedComponent(connectivity=1)(labels.clone())
    assert np.array_equal(kept[0].cpu().numpy(), exp) and int((exp != cls).sum()) > 0


def case_transforms_deterministic(device, shape):
    """two calls on a blobs-plus-speckle label map: identical bits"""
    import monai_amd.transforms as T

    lab = torch.from_numpy(blobs_labels(shape, 4, 9)[None]).to(torch.uint8).to(device)
    outs = []
    for _ in range(2):
        k = T.KeepLargestConnectedComponent(num_components=2)(lab.clone())
        outs.append((k, T.FillHoles(connectivity=1)(k)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], lab) and not torch.equal(outs[0][1], outs[0][0])


def case_api(device):
    """errors with the reference's texts; what is not on the HIP path is refused (no reference to fall through to under MONAI_AMD_NO_FALLTHROUGH=1)"""
    import pytest

    import monai_amd.transforms as T
    from monai_amd import ops
    from monai_amd._fallback import UnsupportedOnDevice
    from monai_amd.transforms.utils import get_unique_labels

    x = torch.zeros((1, 5, 6), device=device)
    x[0, 1:3, 1:3] = 2
    with pytest.raises(ValueError, match="Connectivity for 2D images"):
        T.KeepLargestConnectedComponent(applied_labels=[2], connectivity=3)(x)
    with pytest.raises(ValueError, match="should only be 1 channel"):
        get_unique_labels(torch.zeros((2, 4, 4), device=device), False)
    assert get_unique_labels(x, False, discard=0) == {2.0} and get_unique_labels(torch.stack([x[0], x[0] * 0]), True) == {0}
    with pytest.raises(IndexError):
        T.FillHoles(applied_labels=[5])(torch.zeros((2, 4, 4), device=device))
    assert T.FillHoles(applied_labels=[1], connectivity=7)(x).equal(x)      # scipy clamps the connectivity of its structuring element
    os.environ["MONAI_AMD_NO_FALLTHROUGH"] = "1"
    try:
        for bad in (torch.zeros((1, 7), device=device), torch.zeros((1, 2, 2, 2, 2), device=device)):      # rank 1 and rank 4
            for t in (T.KeepLargestConnectedComponent(applied_labels=[1]), T.FillHoles(applied_labels=[1])):
                with pytest.raises((NotImplementedError, UnsupportedOnDevice)):
                    t(bad)
        with pytest.raises((NotImplementedError, UnsupportedOnDevice)):
            T.LabelFilter([1])(torch.zeros(7, device=device))
        with pytest.raises(NotImplementedError):
            T.LabelFilter([1])("text")
    finally:
        os.environ.pop("MONAI_AMD_NO_FALLTHROUGH", None)
    with pytest.raises(RuntimeError, match="cc_label: connectivity 4"):
        items = ops.CcItems((4, 4, 4), [{"src": 0}], device)
        ops.cc_label(torch.zeros((4, 4, 4), dtype=torch.uint8, device=device), items, 4)
    with pytest.raises(RuntimeError, match="leaves the tensor"):
        items = ops.CcItems((4, 4, 4), [{"src": 1}], device)
        ops.cc_label(torch.zeros((4, 4, 4), dtype=torch.uint8, device=device), items, 1)
