"""Golden outputs of the reference's OWN MedianFilter / median_filter (monai/networks/layers/simplelayers.py:441-539) and MedianSmooth(d)
(monai/transforms/intensity/array.py:1561-1587, dictionary.py:1157-1181) on the cases of tests/median_cases.py, CPU -> tests/golden/median.npz:
per case id the bits of the whole fp32 output as uint32.

Every finite single-pass case is also required to agree bit for bit with scipy.ndimage.median_filter(mode="nearest") -- an independent
implementation -- except that the reference writes +0.0 where the selected value is -0.0 (its one-hot convolution starts the sum at +0.0);
repeated passes are checked against scipy applied as often.  For the non-finite cases the script checks the rule the kernel reproduces: NaN exactly
in the windows that hold the non-finite value.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_median.py"""
import json
import os
import sys
import warnings

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
import monai.networks.layers as ref_layers  # noqa: E402
import monai.transforms as ref_transforms  # noqa: E402
import median_cases as mc  # noqa: E402

warnings.filterwarnings("ignore")
torch.set_num_threads(8)


def scipy_median(case, a):
    sd = case["sd"]
    r = case["radius"] if isinstance(case["radius"], list) else [case["radius"]] * sd
    size = [1] * (a.ndim - sd) + [2 * v + 1 for v in r]
    for _ in range(case["passes"]):
        a = ndimage.median_filter(a, size=size, mode="nearest")
    return a


arrays, manifest = {}, []
n_zero_fixed = 0
for case in mc.golden_cases():
    cid = case["id"]
    out = mc.run_case(ref_layers, ref_transforms, case, "cpu")
    o = torch.as_tensor(out).numpy()
    assert o.dtype == np.float32 and o.shape == case["shape"], (cid, o.dtype, o.shape)
    a = mc.inputs(case)
    if case["poke"] is None:
        want = scipy_median(case, a)
        neg_zero = (want == 0) & np.signbit(want)
        n_zero_fixed += int(neg_zero.sum())
        want = np.where(neg_zero, np.float32(0.0), want)
        assert np.array_equal(o.view(np.uint32), want.view(np.uint32)), (cid, "scipy.ndimage.median_filter disagrees")
    else:
        sd = case["sd"]
        r = case["radius"] if isinstance(case["radius"], list) else [case["radius"]] * sd
        size = [1] * (a.ndim - sd) + [2 * v + 1 for v in r]
        hit = ndimage.maximum_filter((~np.isfinite(a)).astype(np.uint8), size=size, mode="nearest").astype(bool)
        assert np.array_equal(np.isnan(o), hit), (cid, "NaN is not exactly the windows that hold the non-finite value")
        fin = ndimage.median_filter(np.where(np.isfinite(a), a, np.float32(0)), size=size, mode="nearest")
        assert np.array_equal(o[~hit].view(np.uint32), fin[~hit].view(np.uint32)), cid
    arrays[cid] = o.view(np.uint32).copy()
    manifest.append(cid)
assert n_zero_fixed > 0, "no case selects -0.0"
arrays["manifest"] = np.array(json.dumps(manifest))
path = os.path.join(HERE, "median.npz")
np.savez_compressed(path, **arrays)
print("median golden:", len(manifest), "cases,", n_zero_fixed, "selected -0.0 written as +0.0 by the reference,", os.path.getsize(path), "bytes")
