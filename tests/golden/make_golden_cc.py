"""Golden outputs of the reference's OWN FillHoles, LabelFilter and KeepLargestConnectedComponent (monai/transforms/post/array.py) on the cases of
tests/cc_cases.py, CPU -> tests/golden/cc_post.npz: per input the outputs stacked in the order of the manifest (a JSON list of case ids).

FillHoles and LabelFilter run on the reference as it is (scipy alone).  KeepLargestConnectedComponent labels through skimage.measure.label, and
scikit-image is not installed where this file is made, so ONE primitive is supplied: a stand-in for `skimage.measure.label` -- the few lines below over
scipy.ndimage.label with generate_binary_structure(ndim, connectivity or ndim) -- goes into sys.modules before the reference is imported.  The
partition into connected components is unique by definition, so any correct labelling gives the reference the same components (only their numbering
is free, and the class never looks at it beyond bincount / isin).  Everything else is the reference's own code: bincount, the cut, isin,
`independent`, `is_onehot`.  The one thing a different numbering could change is the unstable argsort among components of EQUAL size, so this script
asserts that no case has two components of equal size at the cut; the product's own tie rule is pinned by a product-only test.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cc.py"""
import json
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CALLS = []      # per labelling call: the component sizes, largest first


def label(label_image, background=None, return_num=False, connectivity=None):
    arr = np.asarray(label_image)
    lab, num = ndimage.label(arr != 0, ndimage.generate_binary_structure(arr.ndim, connectivity or arr.ndim))
    CALLS.append(sorted(np.bincount(lab.reshape(-1))[1:].tolist(), reverse=True))
    return (lab, num) if return_num else lab


assert "skimage" not in sys.modules
try:
    import skimage  # noqa: F401

    raise SystemExit("scikit-image is installed: record the golden with the real skimage.measure.label instead of the stand-in")
except ImportError:
    pass
pkg, measure = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
pkg.__version__, pkg.measure, measure.label = "0.22.0", measure, label
pkg.__path__ = []
sys.modules["skimage"], sys.modules["skimage.measure"] = pkg, measure

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
import monai.transforms as ref  # noqa: E402
import cc_cases as cc  # noqa: E402

ins = cc.inputs()
stacks, manifest = {}, []
for case in cc.golden_cases():
    del CALLS[:]
    x, before, out = cc.run_case(ref, case, "cpu", ins)
    if case["kind"] == "keep":
        assert CALLS, case["id"]
        for sizes in CALLS:
            nc = case["nc"]
            assert len(sizes) <= nc or sizes[nc - 1] != sizes[nc], ("two components of equal size at the cut", case["id"], sizes[: nc + 2])
    o = np.asarray(out)
    assert o.shape == ins[case["inp"]].shape and np.array_equal(o, o.astype(np.uint8)), case["id"]
    stacks.setdefault(case["inp"], []).append(o.astype(np.uint8))
    manifest.append(case["id"])
arrays = {"out|" + k: np.stack(v) for k, v in stacks.items()}
arrays["manifest"] = np.array(json.dumps(manifest))
path = os.path.join(HERE, "cc_post.npz")
np.savez_compressed(path, **arrays)
print("cc golden:", len(manifest), "cases,", os.path.getsize(path), "bytes")
