"""``ConfusionMatrixMetric`` and its functions on the one-pass overlap kernel (csrc/kernels/metrics.h).  Drop-ins for
monai/metrics/confusion_matrix.py:25-322.

``get_confusion_matrix`` takes true positives (p + y == 2), true negatives (p + y == 0) and the ground-truth sum from slots 5, 6 and 2 of the
record; false positives / negatives follow from them and the voxel count.  The derived metrics work on [B, C, 4]-sized tensors: plain
torch in the reference's operation order, so float32 results agree bit for bit.  The class warns about inputs that are not binarized
(``is_binary_tensor``'s message, from slot 7 of the same record: no extra pass)."""

from __future__ import annotations

import warnings
from collections.abc import Sequence

import torch

from .._fallback import function_fallback, reference_fallback
from ..utils.misc import ensure_tuple
from .meaniou import _same_shape_record
from .metric import CumulativeIterationMetric
from .utils import do_metric_reduction

__all__ = ["ConfusionMatrixMetric", "get_confusion_matrix", "compute_confusion_matrix_metric", "check_confusion_matrix_metric_name"]

# short name -> every spelling the reference accepts (confusion_matrix.py:286-321), blanks as underscores, lower case
_NAMES = {
    "tpr": ("sensitivity", "recall", "hit_rate", "true_positive_rate", "tpr"),
    "tnr": ("specificity", "selectivity", "true_negative_rate", "tnr"),
    "ppv": ("precision", "positive_predictive_value", "ppv"),
    "npv": ("negative_predictive_value", "npv"),
    "fnr": ("miss_rate", "false_negative_rate", "fnr"),
    "fpr": ("fall_out", "false_positive_rate", "fpr"),
    "fdr": ("false_discovery_rate", "fdr"),
    "for": ("false_omission_rate", "for"),
    "pt": ("prevalence_threshold", "pt"),
    "ts": ("threat_score", "critical_success_index", "ts", "csi"),
    "acc": ("accuracy", "acc"),
    "ba": ("balanced_accuracy", "ba"),
    "f1": ("f1_score", "f1"),
    "mcc": ("matthews_correlation_coefficient", "mcc"),
    "fm": ("fowlkes_mallows_index", "fm"),
    "bm": ("informedness", "bookmaker_informedness", "bm", "youden_index", "youden"),
    "mk": ("markedness", "deltap", "mk"),
}
_SHORT = {alias: short for short, aliases in _NAMES.items() for alias in aliases}


# no call-time fall-through of the class: get_confusion_matrix falls through on its own and the matrices land in THIS object's buffers either way
@reference_fallback("monai.metrics.confusion_matrix", "ConfusionMatrixMetric", methods=())
class ConfusionMatrixMetric(CumulativeIterationMetric):
    """Confusion-matrix metrics per (batch item, class): every call adds the [B, C, 4] matrices (tp, fp, tn, fn) to the buffer, ``aggregate``
    returns one result per name in ``metric_name``."""

    def __init__(self, include_background: bool = True, metric_name: Sequence[str] | str = "hit_rate", compute_sample: bool = False,
                 reduction="mean", get_not_nans: bool = False) -> None:
        super().__init__()
        self.include_background = include_background
        self.metric_name = ensure_tuple(metric_name)
        self.compute_sample = compute_sample
        self.reduction = reduction
        self.get_not_nans = get_not_nans

    def _compute_tensor(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        dims = y_pred.ndimension()
        if dims < 2:
            raise ValueError("y_pred should have at least two dimensions.")
        if dims == 2 or (dims == 3 and y_pred.shape[-1] == 1):
            if self.compute_sample:
                warnings.warn("As for classification task, compute_sample should be False.")
                self.compute_sample = False
        return get_confusion_matrix(y_pred=y_pred, y=y, include_background=self.include_background, _monai_amd_binary_warning=True)

    def aggregate(self, compute_sample: bool = False, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the data to aggregate must be PyTorch Tensor.")
        results = []
        for metric_name in self.metric_name:
            if compute_sample or self.compute_sample:      # the metric of every sample first, then the reduction
                f, not_nans = do_metric_reduction(compute_confusion_matrix_metric(metric_name, data), reduction or self.reduction)
            else:                                          # the reduced matrices first
                f, not_nans = do_metric_reduction(data, reduction or self.reduction)
                f = compute_confusion_matrix_metric(metric_name, f)
            results.append((f, not_nans) if self.get_not_nans else f)
        return results


@function_fallback("monai.metrics.confusion_matrix", "get_confusion_matrix")
def get_confusion_matrix(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool = True, _monai_amd_binary_warning: bool = False) -> torch.Tensor:
    """[B, C, 4] float32: true positives, false positives, true negatives, false negatives of every (batch item, class); ``y_pred`` and ``y``
    binarized one-hot tensors of one shape ([B, C] for classification: one value per class)."""
    record = _same_shape_record(y_pred, y, include_background, _monai_amd_binary_warning)
    voxels = 1
    for v in y.shape[2:]:
        voxels *= int(v)
    tp, tn, p = record[..., 5], record[..., 6], record[..., 2]
    n = voxels - p
    return torch.stack([tp, n - tn, tn, p - tp], dim=-1).to(torch.float32)


def compute_confusion_matrix_metric(metric_name: str, confusion_matrix: torch.Tensor) -> torch.Tensor:
    """The metric `metric_name` (any spelling of ``check_confusion_matrix_metric_name``) of [..., 4] confusion matrices; NaN where it is undefined."""
    metric = check_confusion_matrix_metric_name(metric_name)
    if confusion_matrix.ndimension() == 1:
        confusion_matrix = confusion_matrix.unsqueeze(dim=0)
    if confusion_matrix.shape[-1] != 4:
        raise ValueError("the size of the last dimension of confusion_matrix should be 4.")
    tp, fp, tn, fn = (confusion_matrix[..., i] for i in range(4))
    p, n = tp + fn, fp + tn
    nan = torch.tensor(float("nan"), device=confusion_matrix.device)

    def rate(num, den):
        return torch.where(den > 0, num / den, nan)

    if metric in ("pt", "ba", "fm", "bm", "mk"):      # built from rates that are NaN where their own denominator is empty
        tpr, tnr = rate(tp, p), rate(tn, n)
        if metric == "pt":
            numerator, denominator = torch.sqrt(tpr * (1.0 - tnr)) + tnr - 1.0, tpr + tnr - 1.0
        elif metric == "ba":
            numerator, denominator = tpr + tnr, 2.0
        elif metric == "fm":
            numerator, denominator = torch.sqrt(rate(tp, tp + fp) * tpr), 1.0
        elif metric == "bm":
            numerator, denominator = tpr + tnr - 1.0, 1.0
        else:
            numerator, denominator = rate(tp, tp + fp) + rate(tn, tn + fn) - 1.0, 1.0
    elif metric == "mcc":
        numerator, denominator = tp * tn - fp * fn, torch.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn))
    else:
        numerator, denominator = {
            "tpr": (tp, p), "tnr": (tn, n), "ppv": (tp, tp + fp), "npv": (tn, tn + fn), "fnr": (fn, p), "fpr": (fp, n),
            "fdr": (fp, fp + tp), "for": (fn, fn + tn), "ts": (tp, tp + fn + fp), "acc": (tp + tn, p + n),
            "f1": (tp * 2.0, tp * 2.0 + fn + fp),
        }[metric]
    if isinstance(denominator, torch.Tensor):
        return torch.where(denominator != 0, numerator / denominator, nan)
    return numerator / denominator


def check_confusion_matrix_metric_name(metric_name: str) -> str:
    """The short name (``"tpr"``, ``"f1"``, ...) of any accepted spelling; ``NotImplementedError`` for an unknown one."""
    key = metric_name.replace(" ", "_").lower()
    if key not in _SHORT:
        raise NotImplementedError("the metric is not implemented.")
    return _SHORT[key]
