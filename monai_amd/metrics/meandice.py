"""``DiceMetric`` / ``compute_dice`` / ``DiceHelper`` on the one-pass overlap kernel (csrc/kernels/metrics.h).  Drop-ins for
monai/metrics/meandice.py:24-337: same arguments, attributes, defaults, errors and result shapes.

The reference walks every (batch item, class) in Python -- a compare, a ``masked_select``, three full-volume sums and an ``if y_o > 0``
host synchronisation each.  Here the two tensors are read once, in whichever mix of one-hot / multi-channel and label-map forms they come
(the fused-argmax uint8 label map of ``SlidingWindowInferer`` included, without a dtype conversion), and the per-class rules of
``compute_channel`` are one ``torch.where`` chain over the [B, C] record: ``2 s0 / (s2 + s1)`` formed in float64 and rounded once to float32,
which for binary inputs with fewer than 2^24 voxels per class is the reference's float32 quotient bit for bit.  A float label map is
truncated to class indices (``one_hot``'s ``.long()``); the reference's ``==`` agrees for every integral label."""

from __future__ import annotations

import warnings

import numpy as np
import torch

from .. import ops
from .._fallback import reference_fallback
from ..utils.misc import look_up_option
from .metric import CumulativeIterationMetric
from .utils import REDUCTIONS, _plain, do_metric_reduction, overlap_record

__all__ = ["DiceMetric", "compute_dice", "DiceHelper"]

_ABOVE_HALF = float(np.nextafter(np.float32(0.5), np.float32(1.0)))      # x > 0.5  <=>  x >= the next float32 after 0.5


# the volume passes of DiceMetric happen inside its DiceHelper, which falls through on its own: results land in THIS object's buffers either way
@reference_fallback("monai.metrics.meandice", "DiceMetric", methods=())
class DiceMetric(CumulativeIterationMetric):
    """Dice per (batch item, class), accumulated over calls and reduced by ``aggregate``.  ``y_pred`` / ``y``: BCHW[D] one-hot / multi-channel
    tensors, or B1HW[D] label maps together with ``num_classes``."""

    def __init__(self, include_background: bool = True, reduction="mean", get_not_nans: bool = False, ignore_empty: bool = True,
                 num_classes: int | None = None, return_with_label: bool | list[str] = False) -> None:
        super().__init__()
        self.include_background = include_background
        self.reduction = reduction
        self.get_not_nans = get_not_nans
        self.ignore_empty = ignore_empty
        self.num_classes = num_classes
        self.return_with_label = return_with_label
        self.dice_helper = DiceHelper(include_background=self.include_background, reduction="none", get_not_nans=False, apply_argmax=False,
                                      ignore_empty=self.ignore_empty, num_classes=self.num_classes)

    def _compute_tensor(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        dims = y_pred.ndimension()
        if dims < 3:
            raise ValueError(f"y_pred should have at least 3 dimensions (batch, channel, spatial), got {dims}.")
        return self.dice_helper(y_pred=y_pred, y=y)

    def aggregate(self, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError(f"the data to aggregate must be PyTorch Tensor, got {type(data)}.")
        f, not_nans = do_metric_reduction(data, reduction or self.reduction)
        if look_up_option(self.reduction, REDUCTIONS, "reduction") == "mean_batch" and self.return_with_label:
            if isinstance(self.return_with_label, bool):
                first = 0 if self.include_background else 1
                f = {f"label_{i + first}": round(v.item(), 4) for i, v in enumerate(f)}
            else:
                f = {key: round(v.item(), 4) for key, v in zip(self.return_with_label, f)}
        return (f, not_nans) if self.get_not_nans else f


def compute_dice(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool = True, ignore_empty: bool = True,
                 num_classes: int | None = None) -> torch.Tensor:
    """Dice per batch item and class, [B, C]; the computation of ``DiceMetric`` without its buffers."""
    return DiceHelper(include_background=include_background, reduction="none", get_not_nans=False, apply_argmax=False, ignore_empty=ignore_empty,
                      num_classes=num_classes)(y_pred=y_pred, y=y)


@reference_fallback("monai.metrics.meandice", "DiceHelper", methods=("__call__",))
class DiceHelper:
    """Dice between ``y_pred`` and ``y`` with the optional discretisation of the prediction (``apply_argmax`` over the channel axis, or
    ``threshold`` at 0.5) in front.  ``activate=True`` (a sigmoid before the threshold) is not on the HIP path."""

    def __init__(self, include_background: bool | None = None, threshold: bool = False, apply_argmax: bool | None = None, activate: bool = False,
                 get_not_nans: bool = True, reduction="mean_batch", ignore_empty: bool = True, num_classes: int | None = None,
                 sigmoid: bool | None = None, softmax: bool | None = None) -> None:
        if sigmoid is not None:      # the reference's deprecated spellings (meandice.py:251-270)
            warnings.warn("Argument `sigmoid` has been deprecated since version 1.5. Use `threshold` instead.", FutureWarning)
            threshold = sigmoid
        if softmax is not None:
            warnings.warn("Argument `softmax` has been deprecated since version 1.5. Use `apply_argmax` instead.", FutureWarning)
            apply_argmax = softmax
        if activate:
            raise NotImplementedError("monai_amd.DiceHelper: activate=True (sigmoid before the threshold) is not on the HIP path")
        self.threshold = threshold
        self.reduction = reduction
        self.get_not_nans = get_not_nans
        self.include_background = threshold if include_background is None else include_background
        self.apply_argmax = not threshold if apply_argmax is None else apply_argmax
        self.activate = activate
        self.ignore_empty = ignore_empty
        self.num_classes = num_classes

    def _scores(self, record: torch.Tensor) -> torch.Tensor:
        """the rules of ``compute_channel`` (meandice.py:281-298) on the record's slots 0-2, [B, C] float32, without a host synchronisation"""
        inter, pred_o, y_o = record[..., 0], record[..., 1], record[..., 2]
        denom = y_o + pred_o
        nan, one, zero = (torch.full((), v, dtype=torch.float64, device=record.device) for v in (float("nan"), 1.0, 0.0))
        empty = nan if self.ignore_empty else torch.where(denom <= 0, one, zero)
        return torch.where(y_o > 0, 2.0 * inter / denom, empty).to(torch.float32)

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor):
        y_pred, y = _plain(y_pred), _plain(y)
        if y_pred.dim() < 2 or y.dim() < 2:
            raise NotImplementedError("monai_amd.DiceHelper: [B, C, spatial...] tensors are what the HIP path takes")
        apply_argmax, threshold = self.apply_argmax, self.threshold
        if self.num_classes is None:
            n_pred_ch = int(y_pred.shape[1])
        else:
            n_pred_ch = int(self.num_classes)
            if y_pred.shape[1] == 1 and self.num_classes > 1:      # class indices already
                apply_argmax = threshold = False
        if apply_argmax and n_pred_ch > 1:
            if y_pred.dtype != torch.float32:
                raise NotImplementedError(f"monai_amd.DiceHelper: argmax of {y_pred.dtype} predictions is not on the HIP path")
            y_pred = torch.stack([ops.channel_reduce("argmax", item) for item in y_pred], dim=0)
        elif threshold:
            if y_pred.dtype != torch.float32:
                raise NotImplementedError(f"monai_amd.DiceHelper: the threshold of {y_pred.dtype} predictions is not on the HIP path")
            y_pred = ops.pointwise("threshold", y_pred, _ABOVE_HALF)

        # one channel means a label map (`== c`), several mean one stored value per class; a single-class problem scores class 1 of the binary map
        k = n_pred_ch if n_pred_ch > 1 else 2
        for t, who in ((y_pred, "y_pred"), (y, "y")):
            if t.shape[1] != 1 and t.shape[1] != k:
                raise NotImplementedError(f"monai_amd.DiceHelper: {who} has {t.shape[1]} channels for {n_pred_ch} classes; one or one per class is what the HIP path takes")
        if n_pred_ch == 1 and y_pred.shape[1] != 1:
            raise NotImplementedError("monai_amd.DiceHelper: a multi-channel prediction with num_classes = 1 is not on the HIP path")
        first_ch = 1 if n_pred_ch == 1 else (0 if self.include_background else 1)
        data = self._scores(overlap_record(y_pred, y, k)[:, first_ch:]).contiguous()
        f, not_nans = do_metric_reduction(data, self.reduction)
        return (f, not_nans) if self.get_not_nans else f
