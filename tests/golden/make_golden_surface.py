"""Golden outputs of the reference's compute_hausdorff_distance / compute_surface_dice / compute_average_surface_distance, its three metric classes
(monai/metrics/hausdorff_distance.py, surface_dice.py, surface_distance.py) and DistanceTransformEDT on the cases of tests/surface_cases.py, CPU; the
edge maps scipy's binary_erosion gives (packed bits).  For every toleranced result the file also holds a float64 truth (`*_truth`) and the
reference's own distance from it (`*_ref_err`): the tests' bounds come from there, never from the code under test.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_surface.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
import monai.metrics as ref  # noqa: E402
import monai.transforms as ref_t  # noqa: E402
import surface_cases as sc  # noqa: E402

out = sc.run_all(ref, "cpu")
out.update(sc.run_toleranced(ref, "cpu"))
for name, t in sc.truths().items():
    assert name in out and out[name].shape == t.shape, name
    out[name + "_truth"] = t
    with np.errstate(invalid="ignore"):
        out[name + "_ref_err"] = np.abs(out[name].astype(np.float64) - t)
out.update(sc.run_edges())
for shape in ((12, 13), (17, 16, 15)):
    img = torch.from_numpy(np.stack([sc.blobs(shape, 70), ~sc.blobs(shape, 71)])).float()
    out["edt_" + sc._tag(shape)] = ref_t.DistanceTransformEDT()(img).numpy().astype(np.float64)
    out["edt_" + sc._tag(shape) + "_sampling"] = ref_t.distance_transform_edt(img, sampling=sc.spacing_of(shape)).numpy().astype(np.float64)
np.savez_compressed(os.path.join(HERE, "surface_metrics.npz"), **out)
print("surface golden:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "surface_metrics.npz")), "bytes")
