"""``do_metric_reduction`` / ``ignore_background`` / ``is_binary_tensor`` (monai/metrics/utils.py:54-130, 347-363) and the one door of the
metrics to the overlap kernel.  The reductions work on [B, C]-sized tensors: plain torch."""

from __future__ import annotations

import warnings

import torch

from .. import ops
from .._fallback import function_fallback
from ..utils.misc import look_up_option

__all__ = ["do_metric_reduction", "ignore_background", "is_binary_tensor"]

REDUCTIONS = ("none", "mean", "sum", "mean_batch", "sum_batch", "mean_channel", "sum_channel")      # monai.utils.MetricReduction


def _plain(t) -> torch.Tensor:
    """the tensor under a MetaTensor, contiguous"""
    if not isinstance(t, torch.Tensor):
        raise NotImplementedError(f"monai_amd.metrics: device tensors are what the HIP path takes, got {type(t).__name__}")
    if type(t) is not torch.Tensor and hasattr(t, "as_tensor"):
        t = t.as_tensor()
    return t.contiguous()


def overlap_record(y_pred, y, num_classes: int) -> torch.Tensor:
    """[B, num_classes, 8] float64 overlap record of `ops.overlap_sums`: the only pass over the two volumes that any metric of this package makes"""
    return ops.overlap_sums(_plain(y_pred), _plain(y), num_classes)


def warn_if_not_binary(record: torch.Tensor, name: str) -> None:
    """the reference's is_binary_tensor warning from slot 7 of a record that is there anyway (one small device-to-host copy, no pass over the volume)"""
    if bool((record[..., 7] != 0).any()):      # a NaN count cannot occur: slot 7 is a count
        warnings.warn(f"{name} should be a binarized tensor.")


def ignore_background(y_pred, y):
    """drop channel 0 of both (a single-channel tensor is left alone): views, no copy"""
    y = y[:, 1:] if y.shape[1] > 1 else y
    y_pred = y_pred[:, 1:] if y_pred.shape[1] > 1 else y_pred
    return y_pred, y


def do_metric_reduction(f: torch.Tensor, reduction="mean"):
    """Reduce the [B, C, ...] values `f` over the batch and / or channel axis, counting only what is not NaN; returns (reduced values,
    not_nans) with not_nans the number of values that entered each result.  ``"none"`` returns `f` itself (no synchronisation).

    The sums of a real reduction are formed on the host and the results returned on `f`'s device: the tensor is [B, C]-sized, and torch adds in a
    different order on each device, so this is what makes an aggregated value the same float32 as the reference's wherever the samples were scored."""
    device = f.device
    if look_up_option(reduction, REDUCTIONS, "reduction") != "none" and device.type != "cpu":
        reduced, not_nans = do_metric_reduction(f.cpu(), reduction)
        return reduced.to(device), not_nans.to(device)
    nans = torch.isnan(f)
    not_nans = ~nans
    zero = torch.zeros(1, device=f.device, dtype=torch.float)
    reduction = look_up_option(reduction, REDUCTIONS, "reduction")
    if reduction == "none":
        return f, not_nans.float()
    f = torch.where(nans, torch.zeros((), device=f.device, dtype=f.dtype), f)
    if reduction == "mean":
        # channel average of every sample first, then the average over the samples that had a value
        not_nans = not_nans.sum(dim=1).float()
        f = torch.where(not_nans > 0, f.sum(dim=1).float() / not_nans, zero)
        not_nans = (not_nans > 0).sum(dim=0).float()
        f = torch.where(not_nans > 0, f.sum(dim=0).float() / not_nans, zero)
    elif reduction == "sum":
        not_nans = not_nans.sum(dim=[0, 1]).float()
        f = torch.sum(f, dim=[0, 1])
    elif reduction == "mean_batch":
        not_nans = not_nans.sum(dim=0).float()
        f = torch.where(not_nans > 0, f.sum(dim=0).float() / not_nans, zero)
    elif reduction == "sum_batch":
        not_nans = not_nans.sum(dim=0).float()
        f = f.sum(dim=0).float()
    elif reduction == "mean_channel":
        not_nans = not_nans.sum(dim=1).float()
        f = torch.where(not_nans > 0, f.sum(dim=1).float() / not_nans, zero)
    else:      # sum_channel
        not_nans = not_nans.sum(dim=1).float()
        f = f.sum(dim=1).float()
    return f, not_nans


@function_fallback("monai.metrics.utils", "is_binary_tensor")
def is_binary_tensor(input: torch.Tensor, name: str) -> None:
    """Warn when `input` holds a value that is neither 0 nor 1 (slot 7 of the overlap record of the tensor with itself: one kernel pass in
    place of the reference's byte round trip, max and min)."""
    if not isinstance(input, torch.Tensor):
        raise ValueError(f"{name} must be of type PyTorch Tensor.")
    flat = _plain(input).reshape(1, 1, -1)
    warn_if_not_binary(ops.overlap_sums(flat, flat, 1), name)
