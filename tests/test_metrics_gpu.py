"""-m gpu: DiceMetric / MeanIoU / ConfusionMatrixMetric and the one-pass overlap kernel (csrc/kernels/metrics.h) on the MI355X: the record against its
definition in numpy (exact), the metrics against the real reference's outputs (tests/golden/metrics.npz)."""
import pytest

import metrics_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_overlap_sums_exact():
    print("records checked", mc.case_overlap_sums_exact(DEV))


def test_overlap_sums_beyond_fp32():
    mc.case_overlap_sums_beyond_fp32(DEV)


def test_overlap_sums_deterministic():
    mc.case_overlap_sums_deterministic(DEV)


def test_dice_iou_confusion_vs_reference():
    print("golden results compared", mc.case_dice_iou_confusion_vs_reference(DEV))


def test_metrics_api():
    mc.case_metrics_api(DEV)


def test_inferer_labels_to_dice():
    mc.case_inferer_labels_to_dice(DEV)
