"""``do_metric_reduction`` / ``ignore_background`` / ``is_binary_tensor`` (monai/metrics/utils.py:54-130, 347-363) and the one door of the
metrics to the overlap kernel.  The reductions work on [B, C]-sized tensors: plain torch.

``get_mask_edges`` / ``get_surface_distance`` / ``get_edge_surface_distance`` / ``prepare_spacing`` (monai/metrics/utils.py:139-344, 400-462) and
``surface_scores_input``, the one door of the surface metrics to the edge / exact-EDT / record kernels (csrc/kernels/edt.h)."""

from __future__ import annotations

import warnings

import torch

from .. import ops
from .._fallback import function_fallback
from ..utils.misc import look_up_option

__all__ = ["do_metric_reduction", "ignore_background", "is_binary_tensor", "get_mask_edges", "get_surface_distance", "get_edge_surface_distance",
           "prepare_spacing"]

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


# ------------------------------------------------------------------------------------------------------------------ surface metrics
def _number(v) -> bool:
    return isinstance(v, (int, float))


def _sequence(v) -> bool:
    import numpy as np
    from collections.abc import Sequence

    return isinstance(v, (Sequence, np.ndarray)) and not isinstance(v, str)


@function_fallback("monai.metrics.utils", "prepare_spacing")
def prepare_spacing(spacing, batch_size: int, img_dim: int):
    """`spacing` with a batch axis: one entry (None, a number, or `img_dim` numbers) per batch item.  Host only; the accepted forms and the
    messages are those of monai/metrics/utils.py:400-462."""
    if spacing is None or _number(spacing):
        return [spacing] * batch_size
    if not _sequence(spacing):
        raise ValueError(f"`spacing` should either be a number, a sequence of numbers or a sequence of sequences, got {spacing}.")
    items = list(spacing)
    first = spacing[0]
    if not all(isinstance(s, type(first)) for s in items):
        raise ValueError(f"if `spacing` is a sequence, its elements should be of same type, got {spacing}.")
    if _sequence(first):
        if len(spacing) != batch_size:
            raise ValueError(f"if `spacing` is a sequence of sequences, the outer sequence should have same length as batch size ({batch_size}), got {spacing}.")
        if not all(len(s) == img_dim for s in items):
            raise ValueError(f"each element of `spacing` list should either have same length asimage dim ({img_dim}), got {spacing}.")
        if not all(_number(i) for s in items for i in list(s)):
            raise ValueError(f"if `spacing` is a sequence of sequences or 2D np.ndarray, the elements should be integers or floats, got {spacing}.")
        return items
    if _number(first):
        if len(spacing) != img_dim:
            raise ValueError(f"if `spacing` is a sequence of numbers, it should have same length as image dim ({img_dim}), got {spacing}.")
        return [spacing for _ in range(batch_size)]
    raise ValueError(f"`spacing` is a sequence of elements with unsupported type: {type(first)}")


def _channels(t: torch.Tensor) -> torch.Tensor:
    """a channel-form tensor the kernels read as it is (float32 / uint8: value == 1, bool), any other dtype compared with 1 first"""
    t = _plain(t)
    return t if t.dtype in (torch.float32, torch.uint8, torch.bool) else (t == 1)


def surface_scores_input(y_pred, y, include_background: bool, same_shape_message: str):
    """(y_pred, y, number of channels, first scored channel) for `ops.surface_records`; the shape error speaks of the shapes the reference sees
    (background channel dropped)"""
    for t in (y_pred, y):
        if not isinstance(t, torch.Tensor):
            raise NotImplementedError(f"monai_amd.metrics: device tensors are what the HIP path takes, got {type(t).__name__}")
    first = 1 if (not include_background and y_pred.shape[1] > 1) else 0
    shp = [torch.Size([t.shape[0], t.shape[1] - (1 if (not include_background and t.shape[1] > 1) else 0)] + list(t.shape[2:])) for t in (y_pred, y)]
    if shp[0] != shp[1]:
        raise ValueError(same_shape_message.format(shp[0], shp[1]))
    if y_pred.dim() < 3:
        raise NotImplementedError("monai_amd.metrics: [B, C, spatial...] tensors are what the HIP path takes")
    return _channels(y_pred), _channels(y), int(y_pred.shape[1]), first


def surface_path_check(distance_metric: str, use_subvoxels: bool = False) -> None:
    if distance_metric != "euclidean":
        raise NotImplementedError(f"monai_amd.metrics: distance_metric={distance_metric!r} (scipy's chamfer transform) is not on the HIP path; 'euclidean' is")
    if use_subvoxels:
        raise NotImplementedError("monai_amd.metrics: use_subvoxels=True is not on the HIP path")


def warn_empty(present: torch.Tensor) -> None:
    """the reference's two warnings of get_edge_surface_distance, per (b, c) in its order; present: host bool [B, C, 2] = (prediction, truth)"""
    for b in range(present.shape[0]):
        for c in range(present.shape[1]):
            if not bool(present[b, c, 1]):
                warnings.warn(f"the ground truth of class {c} is all 0, this may result in nan/inf distance.")
            if not bool(present[b, c, 0]):
                warnings.warn(f"the prediction of class {c} is all 0, this may result in nan/inf distance.")


@function_fallback("monai.metrics.utils", "get_mask_edges")
def get_mask_edges(seg_pred, seg_gt, label_idx: int = 1, crop: bool = True, spacing=None, always_return_as_numpy: bool = False):
    """(edges of seg_pred, edges of seg_gt) of two (H, W[, D]) masks or label fields: bool, `mask & ~binary_erosion(mask)` (face-connected element,
    outside the image background).  With `crop` both are cut to the bounding box of the union with a margin of one voxel, padded where the box leaves
    the image, as the reference's CropForegroundd call does; two empty masks come back as zeros of the input shape."""
    if not isinstance(seg_pred, torch.Tensor) or not isinstance(seg_gt, torch.Tensor):
        raise NotImplementedError("monai_amd.get_mask_edges: device tensors are what the HIP path takes")
    if seg_pred.shape != seg_gt.shape:
        raise ValueError(f"seg_pred and seg_gt should have same shapes, got {seg_pred.shape} and {seg_gt.shape}.")
    if spacing is not None:
        raise NotImplementedError("monai_amd.get_mask_edges: sub-voxel edges (spacing) are not on the HIP path")
    sides = []
    for t in (_plain(seg_pred), _plain(seg_gt)):
        if t.dtype != torch.bool and (label_idx != 1 or t.dtype not in (torch.float32, torch.uint8)):
            t = t == label_idx
        sides.append(t[None, None])
    ep, et = ops.mask_edges(sides[0], sides[1], 1)
    ep, et = ep[0, 0], et[0, 0]
    if crop:
        union = ep | et      # the extreme voxels of a mask are edge voxels: the box of the edges is the box of the masks
        dims = list(range(union.dim()))
        spans = torch.stack([torch.nn.functional.pad(union.any(dim=[d for d in dims if d != a]), (0, max(union.shape) - union.shape[a])) for a in dims]).cpu()
        if not bool(spans.any()):
            ep, et = torch.zeros_like(ep), torch.zeros_like(et)
        else:
            pad, cut = [], []
            for a in dims:
                on = torch.nonzero(spans[a]).flatten()
                lo, hi = int(on[0]) - 1, int(on[-1]) + 2
                cut.append(slice(max(lo, 0), min(hi, union.shape[a])))
                pad = [max(-lo, 0), max(hi - union.shape[a], 0)] + pad
            ep, et = (torch.nn.functional.pad(e[tuple(cut)], pad) for e in (ep, et))
    if always_return_as_numpy:
        return ep.cpu().numpy(), et.cpu().numpy()
    return ep, et


@function_fallback("monai.metrics.utils", "get_surface_distance")
def get_surface_distance(seg_pred, seg_gt, distance_metric: str = "euclidean", spacing=None):
    """float32 distances from every voxel of the edge map `seg_pred` to the nearest voxel of the edge map `seg_gt` (both bool, (H, W[, D])), in voxel
    order; all +inf where a side has no voxel, with the reference's lengths (monai/metrics/utils.py:271-277)."""
    if not isinstance(seg_pred, torch.Tensor) or not isinstance(seg_gt, torch.Tensor):
        raise NotImplementedError("monai_amd.get_surface_distance: device tensors are what the HIP path takes")
    if distance_metric not in ("euclidean", "chessboard", "taxicab"):
        raise ValueError(f"distance_metric {distance_metric} is not implemented.")
    surface_path_check(distance_metric)
    if seg_pred.dtype != torch.bool or seg_gt.dtype != torch.bool:
        raise NotImplementedError("monai_amd.get_surface_distance: bool edge maps are what the HIP path takes")
    seg_pred, seg_gt = _plain(seg_pred), _plain(seg_gt)
    has_p, has_t = (bool(v) for v in torch.stack([seg_pred.any(), seg_gt.any()]).cpu())
    if not has_t or not has_p:
        n = int((seg_pred if not has_t else seg_gt).sum())
        return torch.full((n,), float("inf"), dtype=torch.float32, device=seg_pred.device)
    dis = ops.edt((~seg_gt)[None], sampling=spacing, float64=True)[0].to(torch.float32)
    return dis[seg_pred]


@function_fallback("monai.metrics.utils", "get_edge_surface_distance")
def get_edge_surface_distance(y_pred, y, distance_metric: str = "euclidean", spacing=None, use_subvoxels: bool = False, symmetric: bool = False,
                              class_index: int = -1):
    """((edges_pred, edges_gt), (distances pred -> gt[, distances gt -> pred]), ()) of two (H, W[, D]) masks, with the reference's warnings."""
    surface_path_check(distance_metric, use_subvoxels)
    edges_pred, edges_gt = get_mask_edges(y_pred, y, crop=True)
    name = class_index if class_index != -1 else "Unknown"
    if not bool(edges_gt.any()):
        warnings.warn(f"the ground truth of class {name} is all 0, this may result in nan/inf distance.")
    if not bool(edges_pred.any()):
        warnings.warn(f"the prediction of class {name} is all 0, this may result in nan/inf distance.")
    distances = (get_surface_distance(edges_pred, edges_gt, distance_metric, spacing),)
    if symmetric:
        distances += (get_surface_distance(edges_gt, edges_pred, distance_metric, spacing),)
    return (edges_pred, edges_gt), distances, ()
