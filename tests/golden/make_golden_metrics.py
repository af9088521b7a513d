"""Golden outputs of the reference's DiceMetric / DiceHelper / compute_dice, MeanIoU / compute_iou and ConfusionMatrixMetric with its functions
(monai/metrics/meandice.py, meaniou.py, confusion_matrix.py) on the cases of tests/metrics_cases.py, CPU.  For the soft-truth cases the file also
holds the reference's own distance from the float64 numpy truth (`*_ref_err`): the tests' bound comes from there, never from the code under test.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
import monai.metrics as ref  # noqa: E402
from metrics_cases import run_all, run_soft, soft_truth  # noqa: E402

out = run_all(ref, "cpu")
assert all(name.startswith("exact_") for name in out)
truth = soft_truth()
for name, v in run_soft(ref, "cpu").items():
    out[name] = v
    out[name + "_ref_err"] = np.abs(v.astype(np.float64) - truth[name])
np.savez_compressed(os.path.join(HERE, "metrics.npz"), **out)
print("metrics golden:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "metrics.npz")), "bytes")
