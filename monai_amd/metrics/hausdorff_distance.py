"""``HausdorffDistanceMetric`` / ``compute_hausdorff_distance`` on the edge, exact-EDT and surface-record kernels (csrc/kernels/edt.h).  Drop-ins for
monai/metrics/hausdorff_distance.py:28-212: same arguments, attributes, defaults, errors, warnings and result shapes.

The reference walks every (batch item, class) in Python: a CropForegroundd, two scipy binary erosions and one or two scipy distance transforms on
one CPU thread, with the masks copied to the host and the distances copied back.  Here the boxes, the edge maps, the distance fields and the
records of all (b, c, direction) come from batched launches; the host reads the boxes, the [B, C, 2, 4] record and -- for a percentile -- the
compacted float32 distances, whatever the volume size.  The maximum is ``float32(sqrt(max squared distance))`` with the squared distance an exact
integer at unit spacing: the reference's bits.  A percentile is ``torch.quantile`` over the host copy of the float32 distances: in float32 at unit
spacing, which is the reference's interpolation bit for bit; with a spacing -- where the distances are not the reference's bits anyway -- rank and
interpolation are formed in float64 and rounded once, because a float32 rank (``q * (n - 1)``) and a float32 lerp err relative to the larger
neighbour, not to the result: the reference itself is more than two float32 ulp from the float64 truth on small percentiles there."""

from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .._fallback import function_fallback, reference_fallback
from .metric import CumulativeIterationMetric
from .utils import do_metric_reduction, prepare_spacing, surface_path_check, surface_scores_input, warn_empty

__all__ = ["HausdorffDistanceMetric", "compute_hausdorff_distance"]


# the volume passes happen inside compute_hausdorff_distance, which falls through on its own: results land in THIS object's buffers either way
@reference_fallback("monai.metrics.hausdorff_distance", "HausdorffDistanceMetric", methods=())
class HausdorffDistanceMetric(CumulativeIterationMetric):
    """(Percentile, directed) Hausdorff distance per (batch item, class), accumulated over calls and reduced by ``aggregate``.  ``y_pred`` / ``y``:
    BCHW[D] binarised one-hot tensors; ``spacing`` is a keyword of the call."""

    def __init__(self, include_background: bool = False, distance_metric: str = "euclidean", percentile: float | None = None, directed: bool = False,
                 reduction="mean", get_not_nans: bool = False) -> None:
        super().__init__()
        self.include_background = include_background
        self.distance_metric = distance_metric
        self.percentile = percentile
        self.directed = directed
        self.reduction = reduction
        self.get_not_nans = get_not_nans

    def _compute_tensor(self, y_pred: torch.Tensor, y: torch.Tensor, **kwargs) -> torch.Tensor:
        if y_pred.ndimension() < 3:
            raise ValueError("y_pred should have at least three dimensions.")
        return compute_hausdorff_distance(y_pred=y_pred, y=y, include_background=self.include_background, distance_metric=self.distance_metric,
                                          percentile=self.percentile, directed=self.directed, spacing=kwargs.get("spacing"))

    def aggregate(self, reduction=None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the data to aggregate must be PyTorch Tensor.")
        f, not_nans = do_metric_reduction(data, reduction or self.reduction)
        return (f, not_nans) if self.get_not_nans else f


@function_fallback("monai.metrics.hausdorff_distance", "compute_hausdorff_distance")
def compute_hausdorff_distance(y_pred, y, include_background: bool = False, distance_metric: str = "euclidean", percentile: float | None = None,
                               directed: bool = False, spacing=None) -> torch.Tensor:
    """Hausdorff distance per batch item and class, float32 [B, C] on ``y_pred``'s device: NaN where both sides are empty, +inf where one is (NaN under a
    percentile, like the reference, whose quantile interpolates between infinities)."""
    p, t, k, first = surface_scores_input(y_pred, y, include_background, "y_pred and y should have same shapes, got {0} and {1}.")
    spacing_list = prepare_spacing(spacing=spacing, batch_size=int(p.shape[0]), img_dim=p.dim() - 2)
    surface_path_check(distance_metric)
    spaced = any(sp is not None for sp in spacing_list)
    sr = ops.surface_records(p, t, k, spacing=spacing_list, symmetric=not directed, first_class=first, want_distances=bool(percentile))
    warn_empty(sr.present)
    hd = torch.empty(sr.present.shape[:2], dtype=torch.float32)
    for b in range(hd.shape[0]):
        for c in range(hd.shape[1]):
            has_p, has_t = bool(sr.present[b, c, 0]), bool(sr.present[b, c, 1])
            if not (has_p or has_t):
                hd[b, c] = float("nan")
                continue
            if percentile and not 0 <= percentile <= 100:
                raise ValueError(f"percentile should be a value between 0 and 100, get {percentile}.")
            if not (has_p and has_t):
                # every distance is +inf; the reference's torch.quantile interpolates between infinities (inf - inf): NaN
                hd[b, c] = float("nan") if percentile else float("inf")
                continue
            vals = []
            for d in ((0,) if directed else (0, 1)):
                if percentile and spaced:
                    vals.append(torch.quantile(sr.distances[(b, c, d)].double(), percentile / 100).to(torch.float32))
                elif percentile:
                    vals.append(torch.quantile(sr.distances[(b, c, d)], percentile / 100))
                else:
                    vals.append(torch.tensor(np.float32(np.sqrt(np.float64(sr.records[b, c, d, 1].item())))))
            hd[b, c] = torch.max(torch.stack(vals))
    return hd.to(p.device)
