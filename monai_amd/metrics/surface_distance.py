"""``SurfaceDistanceMetric`` / ``compute_average_surface_distance`` on the edge, exact-EDT and surface-record kernels (csrc/kernels/edt.h).  Drop-ins
for monai/metrics/surface_distance.py:27-186: same arguments, attributes, defaults, errors, warnings and result shapes.

The mean is the fp64 sum of the float32 distances over their count, rounded once to float32 (the reference's float32 ``mean`` differs from it by its
own summation error only)."""

from __future__ import annotations

import torch

from .. import ops
from .._fallback import function_fallback, reference_fallback
from .metric import CumulativeIterationMetric
from .utils import do_metric_reduction, prepare_spacing, surface_path_check, surface_scores_input, warn_empty

__all__ = ["SurfaceDistanceMetric", "compute_average_surface_distance"]


@reference_fallback("monai.metrics.surface_distance", "SurfaceDistanceMetric", methods=())
class SurfaceDistanceMetric(CumulativeIterationMetric):
    """Average (symmetric) surface distance per (batch item, class), accumulated over calls and reduced by ``aggregate``."""

    def __init__(self, include_background: bool = False, symmetric: bool = False, distance_metric: str = "euclidean", reduction="mean",
                 get_not_nans: bool = False) -> None:
        super().__init__()
        self.include_background = include_background
        self.distance_metric = distance_metric
        self.symmetric = symmetric
        self.reduction = reduction
        self.get_not_nans = get_not_nans

    def _compute_tensor(self, y_pred: torch.Tensor, y: torch.Tensor, **kwargs) -> torch.Tensor:
        if y_pred.dim() < 3:
            raise ValueError("y_pred should have at least three dimensions.")
        return compute_average_surface_distance(y_pred=y_pred, y=y, include_background=self.include_background, symmetric=self.symmetric,
                                                distance_metric=self.distance_metric, spacing=kwargs.get("spacing"))

    def aggregate(self, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the data to aggregate must be PyTorch Tensor.")
        f, not_nans = do_metric_reduction(data, reduction or self.reduction)
        return (f, not_nans) if self.get_not_nans else f


@function_fallback("monai.metrics.surface_distance", "compute_average_surface_distance")
def compute_average_surface_distance(y_pred, y, include_background: bool = False, symmetric: bool = False, distance_metric: str = "euclidean",
                                     spacing=None) -> torch.Tensor:
    """Average surface distance from ``y_pred`` to ``y`` (of both directions with ``symmetric``), float32 [B, C]: NaN where both sides are empty,
    +inf where one is."""
    p, t, k, first = surface_scores_input(y_pred, y, include_background, "y_pred and y should have same shapes, got {0} and {1}.")
    spacing_list = prepare_spacing(spacing=spacing, batch_size=int(p.shape[0]), img_dim=p.dim() - 2)
    surface_path_check(distance_metric)
    sr = ops.surface_records(p, t, k, spacing=spacing_list, symmetric=symmetric, first_class=first)
    warn_empty(sr.present)
    both = sr.present[..., 0] & sr.present[..., 1]
    either = sr.present[..., 0] | sr.present[..., 1]
    rec = sr.records.sum(dim=2)      # a direction that was not asked for holds zeros
    mean = (rec[..., 2] / rec[..., 0]).to(torch.float32)
    empty = torch.where(either, torch.tensor(float("inf")), torch.tensor(float("nan")))
    return torch.where(both, mean, empty).to(p.device)
