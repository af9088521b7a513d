"""``SurfaceDiceMetric`` / ``compute_surface_dice`` on the edge, exact-EDT and surface-record kernels (csrc/kernels/edt.h).  Drop-ins for
monai/metrics/surface_dice.py:27-279: same arguments, attributes, defaults, errors, warnings and result shapes.

The record holds, per direction, the number of edge voxels and the number of them whose float32 distance is <= the float32 threshold (the
reference compares a float32 tensor with a Python scalar: in float32); the score is the float32 quotient of the two integer sums."""

from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .._fallback import function_fallback, reference_fallback
from .metric import CumulativeIterationMetric
from .utils import do_metric_reduction, prepare_spacing, surface_path_check, surface_scores_input, warn_empty

__all__ = ["SurfaceDiceMetric", "compute_surface_dice"]


@reference_fallback("monai.metrics.surface_dice", "SurfaceDiceMetric", methods=())
class SurfaceDiceMetric(CumulativeIterationMetric):
    """Normalised surface Dice per (batch item, class) under class-specific thresholds, accumulated over calls and reduced by ``aggregate``."""

    def __init__(self, class_thresholds: list[float], include_background: bool = False, distance_metric: str = "euclidean", reduction="mean",
                 get_not_nans: bool = False, use_subvoxels: bool = False) -> None:
        super().__init__()
        self.class_thresholds = class_thresholds
        self.include_background = include_background
        self.distance_metric = distance_metric
        self.reduction = reduction
        self.get_not_nans = get_not_nans
        self.use_subvoxels = use_subvoxels

    def _compute_tensor(self, y_pred: torch.Tensor, y: torch.Tensor, **kwargs) -> torch.Tensor:
        return compute_surface_dice(y_pred=y_pred, y=y, class_thresholds=self.class_thresholds, include_background=self.include_background,
                                    distance_metric=self.distance_metric, spacing=kwargs.get("spacing"), use_subvoxels=self.use_subvoxels)

    def aggregate(self, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the data to aggregate must be PyTorch Tensor.")
        f, not_nans = do_metric_reduction(data, reduction or self.reduction)
        return (f, not_nans) if self.get_not_nans else f


@function_fallback("monai.metrics.surface_dice", "compute_surface_dice")
def compute_surface_dice(y_pred, y, class_thresholds: list[float], include_background: bool = False, distance_metric: str = "euclidean", spacing=None,
                         use_subvoxels: bool = False) -> torch.Tensor:
    """Normalised surface Dice, float32 [B, C]: NaN where a class is in neither tensor, 0 where it is in one only."""
    if not isinstance(y_pred, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise ValueError("y_pred and y must be PyTorch Tensor.")
    if y_pred.ndimension() not in (4, 5) or y.ndimension() not in (4, 5):
        raise ValueError("y_pred and y should be one-hot encoded: [B,C,H,W] or [B,C,H,W,D].")
    p, t, k, first = surface_scores_input(y_pred, y, include_background, "y_pred and y should have same shape, but instead, shapes are {0} (y_pred) and {1} (y).")
    n_class = k - first
    if n_class != len(class_thresholds):
        raise ValueError(f"number of classes ({n_class}) does not match number of class thresholds ({len(class_thresholds)}).")
    if any(~np.isfinite(class_thresholds)):
        raise ValueError("All class thresholds need to be finite.")
    if any(np.array(class_thresholds) < 0):
        raise ValueError("All class thresholds need to be >= 0.")
    spacing_list = prepare_spacing(spacing=spacing, batch_size=int(p.shape[0]), img_dim=p.dim() - 2)
    surface_path_check(distance_metric, use_subvoxels)
    sr = ops.surface_records(p, t, k, spacing=spacing_list, thresholds=list(class_thresholds), symmetric=True, first_class=first)
    warn_empty(sr.present)
    both = sr.present[..., 0] & sr.present[..., 1]
    either = sr.present[..., 0] | sr.present[..., 1]
    rec = sr.records.sum(dim=2).to(torch.int64)
    score = rec[..., 3] / rec[..., 0]      # int64 / int64 -> float32: the correctly rounded quotient of two counts below 2^24
    empty = torch.where(either, torch.tensor(0.0), torch.tensor(float("nan")))
    return torch.where(both, score.to(torch.float32), empty).to(p.device)
