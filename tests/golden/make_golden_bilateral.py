"""Golden outputs of the reference's OWN exact bilateral filter (monai/csrc/filtering/bilateral/bilateralfilter_cpu.cpp:20-124, compiled by
oracle/build_ref.py into oracle/_ref/) on the cases of tests/bilateral_cases.py -> tests/golden/bilateral.npz and bilateral_2.npz (two files, each well under the size limit) and, for the
two 40 x 41 x 42 volumes that only the MI355X runs, tests/golden/bilateral_gpu_s2.npz / bilateral_gpu_s3.npz.  Per case id: ``<id>/ref32``, the bits of the float32 output
as uint32, and ``<id>/ref64``, the float64 output for the same float32 values.  A float64 case stores the float32 output of its values as ``ref32``
as well (the NaN positions are read from it).

The script also evaluates the definition in plain numpy float64 --
    out_c = sum_t w_t x_c[nb_t] / sum_t w_t,  w_t = prod_axes exp(-d^2 / (2 sigma_s^2)) exp(-sum_c (x_c[home] - x_c[nb_t])^2 / (2 sigma_c^2)),
K = ceil(5.0f * sigma_s) | 1 taps per axis with the product in float32, clamped indices, the two constants -1 / (2 sigma^2) rounded to float32 as
the reference computes them -- and requires ``ref64`` to match it to 1e-12 max|x|, NaN for NaN: the golden pins the formula and not an accident
of the build.  For the colour sigma of 1e4 the output is also required to be the plain Gaussian average within the size of the neglected colour term.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bilateral.py"""
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import bilateral_cases as bc  # noqa: E402
from oracle import build_ref  # noqa: E402

build_ref.build()
ref = build_ref.load()
assert ref is not None, "oracle/_ref is not built (the reference checkout is needed)"
torch.set_num_threads(1)


def definition(x: np.ndarray, ss: float, cs: float, color: bool = True) -> np.ndarray:
    """(B, C, spatial...) float64 from the definition; color=False: the spatial Gaussian alone"""
    k = int(np.ceil(np.float32(5.0) * np.float32(ss))) | 1
    h = k // 2
    ks = float(np.float32(-1.0) / (np.float32(2) * np.float32(ss) * np.float32(ss)))
    kc = float(np.float32(-1.0) / (np.float32(2) * np.float32(cs) * np.float32(cs)))
    x = x.astype(np.float64)
    sd = x.ndim - 2
    pad = np.pad(x, [(0, 0), (0, 0)] + [(h, h)] * sd, mode="edge")
    num, den = np.zeros_like(x), np.zeros((x.shape[0], 1) + x.shape[2:])
    g = np.exp(np.arange(-h, h + 1, dtype=np.float64) ** 2 * ks)
    with np.errstate(invalid="ignore", over="ignore"):
        for tap in itertools.product(range(k), repeat=sd):
            nb = pad[(slice(None), slice(None)) + tuple(slice(t, t + n) for t, n in zip(tap, x.shape[2:]))]
            w = np.prod([g[t] for t in tap])
            if color:
                w = w * np.exp(((x - nb) ** 2).sum(axis=1, keepdims=True) * kc)
            num += nb * w
            den += w
        return num / den


def main():
    files: dict = {}
    for case in bc.all_cases():
        if case["id"] != bc.golden_key(case):       # the float64 twin of a stored case
            continue
        x = bc.inputs(case)
        t = torch.from_numpy(x.copy())
        ref32 = ref.bilateral_filter(t, case["ss"], case["cs"], False).numpy()
        ref64 = ref.bilateral_filter(t.double(), case["ss"], case["cs"], False).numpy()
        assert ref32.dtype == np.float32 and ref64.dtype == np.float64 and ref32.shape == ref64.shape == case["shape"], case["id"]
        assert np.array_equal(np.isnan(ref32), np.isnan(ref64)), case["id"]
        xmax = float(np.abs(x[np.isfinite(x)]).max())
        want = definition(x, case["ss"], case["cs"])
        nan = np.isnan(ref64)
        assert np.array_equal(np.isnan(want), nan), (case["id"], "NaN positions differ from the definition's")
        dev = float(np.abs(want[~nan] - ref64[~nan]).max())
        assert dev <= 1e-12 * xmax, (case["id"], dev, xmax)
        if case["poke"] is not None:        # NaN exactly in the windows that hold the poked value (its channel; every channel for a NaN)
            hit = np.zeros(case["shape"], bool)
            h = bc.window(case["ss"]) // 2
            at = case["poke"][0]
            box = tuple(slice(max(0, a - h), a + h + 1) for a in at[2:])
            hit[(at[0], slice(None) if np.isnan(case["poke"][1]) else at[1]) + box] = True
            hit[(at[0], slice(None)) + tuple(at[2:])] = True      # at the poked voxel itself the home tap's weight is NaN (inf - inf)
            assert np.array_equal(nan, hit), (case["id"], "NaN is not exactly the windows that hold the non-finite value")
        if case["cs"] >= 1e4:
            gauss = definition(x, case["ss"], case["cs"], color=False)
            spread = float(x.max() - x.min())
            slack = (x.shape[1] * spread ** 2 / (2 * case["cs"] ** 2)) * 2 * xmax       # every weight is within this factor of 1
            assert float(np.abs(gauss - ref64).max()) <= slack, (case["id"], float(np.abs(gauss - ref64).max()), slack)
        if bc.window(case["ss"]) == 1:
            assert ref32.tobytes() == x.tobytes(), (case["id"], "a window of one tap is the identity")
        e_ref = float(np.abs(ref32[~nan].astype(np.float64) - ref64[~nan]).max())
        print("%-34s K=%-3d e_ref %.3e = %.2f x 2^-24 max|x|   definition %.1e" % (case["id"], bc.window(case["ss"]), e_ref, e_ref / (2.0 ** -24 * xmax), dev / xmax))
        f = files.setdefault(case["file"], {"manifest": []})
        f[case["id"] + "/ref32"] = ref32.view(np.uint32).copy()
        f[case["id"] + "/ref64"] = ref64
        f["manifest"].append(case["id"])
    for name, arrays in files.items():
        n = len(arrays["manifest"])
        arrays["manifest"] = np.array(json.dumps(arrays["manifest"]))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name + ".npz:", n, "cases,", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20, path


if __name__ == "__main__":
    main()
