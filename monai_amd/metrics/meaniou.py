"""``MeanIoU`` / ``compute_iou`` on the one-pass overlap kernel (csrc/kernels/metrics.h).  Drop-ins for monai/metrics/meaniou.py:22-147.

Intersection (sum of y * y_pred), ground-truth and prediction sums are slots 3, 2 and 4 of the record; the quotient is formed in float64 and
rounded once to float32 -- for binarized inputs with fewer than 2^24 voxels per class the reference's float32 result bit for bit.
``include_background=False`` drops column 0 of the record instead of slicing (and copying) the volumes.  The class warns about inputs
that are not binarized (``is_binary_tensor``'s message, from slot 7 of the same record: no extra pass)."""

from __future__ import annotations

import torch

from .._fallback import function_fallback, reference_fallback
from .metric import CumulativeIterationMetric
from .utils import do_metric_reduction, overlap_record, warn_if_not_binary

__all__ = ["MeanIoU", "compute_iou"]


def _shape_without_background(t: torch.Tensor, include_background: bool) -> tuple:
    """the shape `ignore_background` would leave (monai/metrics/utils.py:54-68)"""
    s = tuple(t.shape)
    return s if include_background or s[1] <= 1 else (s[0], s[1] - 1) + s[2:]


def _same_shape_record(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool, binary_warning: bool) -> torch.Tensor:
    """the record of two channel-form tensors of one shape, background column dropped on request -- shared with the confusion matrix"""
    sp, sy = _shape_without_background(y_pred, include_background), _shape_without_background(y, include_background)
    if sy != sp:
        raise ValueError(f"y_pred and y should have same shapes, got {torch.Size(sp)} and {torch.Size(sy)}.")
    if y_pred.shape[1] != y.shape[1]:      # [B, 2, ...] against [B, 1, ...] without background: the reference compares channel 1 with channel 0
        raise NotImplementedError("monai_amd.metrics: a single-channel tensor against a two-channel one is not on the HIP path")
    record = overlap_record(y_pred, y, int(y_pred.shape[1]))
    if not include_background and record.shape[1] > 1:
        record = record[:, 1:]
    if binary_warning:
        warn_if_not_binary(record, "y_pred / y")
    return record


# no call-time fall-through of the class: compute_iou falls through on its own and the values land in THIS object's buffers either way
@reference_fallback("monai.metrics.meaniou", "MeanIoU", methods=())
class MeanIoU(CumulativeIterationMetric):
    """Intersection over union per (batch item, class), accumulated over calls and reduced by ``aggregate``."""

    def __init__(self, include_background: bool = True, reduction="mean", get_not_nans: bool = False, ignore_empty: bool = True) -> None:
        super().__init__()
        self.include_background = include_background
        self.reduction = reduction
        self.get_not_nans = get_not_nans
        self.ignore_empty = ignore_empty

    def _compute_tensor(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        dims = y_pred.ndimension()
        if dims < 3:
            raise ValueError(f"y_pred should have at least 3 dimensions (batch, channel, spatial), got {dims}.")
        return compute_iou(y_pred=y_pred, y=y, include_background=self.include_background, ignore_empty=self.ignore_empty, _monai_amd_binary_warning=True)

    def aggregate(self, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the data to aggregate must be PyTorch Tensor.")
        f, not_nans = do_metric_reduction(data, reduction or self.reduction)
        return (f, not_nans) if self.get_not_nans else f


@function_fallback("monai.metrics.meaniou", "compute_iou")
def compute_iou(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool = True, ignore_empty: bool = True,
                _monai_amd_binary_warning: bool = False) -> torch.Tensor:
    """IoU per batch item and class, [B, C] float32; ``y_pred`` and ``y`` one-hot / multi-channel tensors of one shape."""
    record = _same_shape_record(y_pred, y, include_background, _monai_amd_binary_warning)
    inter, y_o, pred_o = record[..., 3], record[..., 2], record[..., 4]
    union = y_o + pred_o - inter
    if ignore_empty:
        out = torch.where(y_o > 0, inter / union, torch.full((), float("nan"), dtype=torch.float64, device=record.device))
    else:
        out = torch.where(union > 0, inter / union, torch.ones((), dtype=torch.float64, device=record.device))
    return out.to(torch.float32)
