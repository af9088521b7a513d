"""``distance_transform_edt`` on the exact Euclidean distance transform kernels (csrc/kernels/edt.h).  Drop-in for
monai/transforms/utils.py:2426-2560 under the contract of the reference's GPU form (cuCIM, which does not exist for ROCm): float32 distances, or
float64 with ``float64_distances=True``.

Every channel is transformed on its own: the distance of each non-zero voxel to the nearest zero voxel of its channel.  Without ``sampling`` the
squared distances are exact integers and the result is ``sqrt`` formed in fp64 (rounded once for float32): scipy's float64 output bit for bit.
A channel WITHOUT any zero voxel comes out ``+inf`` everywhere: there is no background to measure to (scipy returns an artefact of its algorithm
there, which is not reproduced).

``get_largest_connected_component_mask``, ``fill_holes`` and ``get_unique_labels`` (monai/transforms/utils.py:1134-1180, 1504-1560, 1478-1501) on the
connected-component kernels (csrc/kernels/ccl.h): device tensors with two or three spatial axes; everything else goes to the reference."""

from __future__ import annotations

import torch

from .. import ops
from .._fallback import function_fallback

__all__ = ["distance_transform_edt", "get_largest_connected_component_mask", "fill_holes", "get_unique_labels"]


@function_fallback("monai.transforms.utils", "distance_transform_edt")
def distance_transform_edt(img, sampling=None, return_distances: bool = True, return_indices: bool = False, distances=None, indices=None, *,
                           block_params=None, float64_distances: bool = False):
    """Euclidean distance transform of a channel-first ``(num_channels, H, W[, D])`` device tensor; any dtype, non-zero is foreground.  The feature
    transform (``return_indices``) and caller-supplied output arrays are not on the HIP path; ``block_params`` (a cuCIM tuning knob) is ignored."""
    if not return_distances and not return_indices:
        raise RuntimeError("Neither return_distances nor return_indices True")
    if not (img.ndim >= 3 and img.ndim <= 4):
        raise RuntimeError("Wrong input dimensionality. Use (num_channels, H, W [,D])")
    if return_indices or indices is not None:
        raise NotImplementedError("monai_amd.distance_transform_edt: the feature transform (return_indices) is not on the HIP path")
    if distances is not None:
        raise NotImplementedError("monai_amd.distance_transform_edt: a caller-supplied `distances` array is not on the HIP path")
    if not isinstance(img, torch.Tensor):
        raise NotImplementedError(f"monai_amd.distance_transform_edt: device tensors are what the HIP path takes, got {type(img).__name__}")
    is_meta = type(img) is not torch.Tensor and hasattr(img, "as_tensor")
    t = (img.as_tensor() if is_meta else img).contiguous()
    if t.dtype not in (torch.float32, torch.uint8, torch.bool):
        t = t != 0
    out = ops.edt(t, sampling=sampling, float64=float64_distances)
    return type(img)(out).copy_meta_from(img) if is_meta else out


# ------------------------------------------------------------------------------------------ connected components
_CC_DTYPES = (torch.float32, torch.uint8, torch.int64, torch.bool)


def _is_meta(x) -> bool:
    return type(x) is not torch.Tensor and hasattr(x, "as_tensor")


def _cc_device_tensor(img, who: str) -> torch.Tensor:
    if not isinstance(img, torch.Tensor):
        raise NotImplementedError(f"monai_amd.{who}: device tensors are what the HIP path takes, got {type(img).__name__}")
    return img.as_tensor() if _is_meta(img) else img


def _cc_work(t: torch.Tensor) -> torch.Tensor:
    """a contiguous tensor of a dtype the kernels read: `t` itself where it is one"""
    if t.dtype not in _CC_DTYPES:
        t = t.to(torch.float32 if t.is_floating_point() else torch.int64)
    return t.contiguous()


def _cc_connectivity(connectivity, rank: int) -> int:
    if connectivity is None:
        return rank
    if not 1 <= int(connectivity) <= rank:      # skimage.measure.label's own refusal
        raise ValueError(f"Connectivity for {rank}D images should be in [1, ..., {rank}]. Got {connectivity}.")
    return int(connectivity)


def _cc_largest_roots(items, labels: torch.Tensor, num_components: int, classes=None) -> torch.Tensor:
    """int32 [nitems, width]: per item -- and per listed class of a CC_LIST_VALUE item -- the root labels of the `num_components` (0 .. 32) largest
    components, 0 where there are fewer.  The key is (size << 32) | root as int64, unique per component, so the choice is deterministic: of two
    components of equal size the one whose first voxel comes LATER wins.  All on the device; `items` in the default layout (item k at k * n).
    Sizes are non-zero at root positions only, so a key below 2^32 is no component: one int64 copy of the sizes becomes the keys in place."""
    import numpy as np

    k, n = int(num_components), items.n
    if not 0 <= k <= ops.CC_MAX_LABELS:
        raise NotImplementedError(f"monai_amd: num_components = {k} is not on the HIP path (0 .. {ops.CC_MAX_LABELS} roots per item and class)")
    if not np.array_equal(items.host[:, 0], np.arange(items.nitems, dtype=np.int64) * n):
        raise RuntimeError("monai_amd: component selection needs the default item layout (item k at voxel offset k * n)")
    if k == 0:      # the reference's `features_to_keep[:0]`: nothing is kept
        return torch.zeros((items.nitems, 1), dtype=torch.int32, device=labels.device)
    k = min(k, n)
    sizes, _ = ops.cc_records(labels, items)
    keys = sizes.view(items.nitems, n).to(torch.int64)
    del sizes
    keys.bitwise_left_shift_(32)
    keys += torch.arange(n, device=keys.device, dtype=torch.int64)
    largest = (lambda x: x.amax(dim=-1, keepdim=True)) if k == 1 else (lambda x: x.topk(k, dim=-1).values)
    if classes is None:
        top = largest(keys)
    else:      # classes[item]: (the item's volume of the source [n], its listed values): a root belongs to the class whose value its voxel holds
        tops = []
        width = max(len(c[1]) for c in classes)
        zero = torch.zeros((), dtype=torch.int64, device=keys.device)
        for i, (vol, values) in enumerate(classes):
            row = [largest(torch.where(vol == v, keys[i], zero)) for v in values]
            row += [torch.zeros((k,), dtype=torch.int64, device=keys.device)] * (width - len(values))
            tops.append(torch.cat(row))
        top = torch.stack(tops)
    return torch.where(top >= (1 << 32), (top & 0xFFFFFFFF) + 1, torch.zeros((), dtype=torch.int64, device=top.device)).to(torch.int32).contiguous()


@function_fallback("monai.transforms.utils", "get_largest_connected_component_mask")
def get_largest_connected_component_mask(img, connectivity: int | None = None, num_components: int = 1):
    """Mask (bool, the shape and device of `img`, a MetaTensor where it got one) of the `num_components` (0 .. 32) largest connected components of
    `img` ``(spatial_dim1, spatial_dim2[, spatial_dim3])``; fewer components than that keeps all of them.  As skimage.measure.label reads it, 0 is
    background and touching regions of DIFFERENT non-zero values are different components (a bool mask has one value).  `connectivity`: orthogonal
    hops to a neighbour, 1 .. img.ndim, None = img.ndim.

    Tie rule: the reference ranks components by an unstable ``argsort(bincount)[::-1]`` and so defines nothing for equal sizes; here, of two components
    of equal size, the one whose first voxel (C order) comes LATER wins.  Labelling, ranking and masking run on the device without a host read."""
    t = _cc_device_tensor(img, "get_largest_connected_component_mask")
    if t.dim() not in (2, 3) or t.numel() == 0:
        raise NotImplementedError(f"monai_amd.get_largest_connected_component_mask: two or three non-empty spatial axes on the HIP path, got {tuple(t.shape)}")
    conn = _cc_connectivity(connectivity, t.dim())
    work = _cc_work(t)
    items = ops.CcItems(t.shape, [{"src": 0, "rule": ops.CC_VALUE}], t.device)
    labels = ops.cc_label(work, items, conn)
    keep = _cc_largest_roots(items, labels, num_components)
    out = torch.ones(t.shape, dtype=torch.uint8, device=t.device)
    ops.cc_keep(out, labels, keep, items)
    out = (out.view(torch.bool) & (labels.view(t.shape) > 0))
    return type(img)(out).copy_meta_from(img) if _is_meta(img) else out


def get_unique_labels(img, is_onehot: bool, discard=None) -> set:
    """Set of the non-discarded labels of a ``[C, spatial...]`` image: the channels with a positive sum of a one-hot image, the unique values of a
    label map (monai/transforms/utils.py:1478-1501).  One small device-to-host read."""
    from ..utils.misc import ensure_tuple

    n_channels = img.shape[0]
    if is_onehot:
        if isinstance(img, torch.Tensor):
            t = img.as_tensor() if _is_meta(img) else img
            sums = t.reshape(n_channels, -1).sum(dim=1, dtype=torch.float64 if t.is_floating_point() else torch.int64).cpu().tolist()
            applied_labels = {i for i, s in enumerate(sums) if s > 0}
        else:
            applied_labels = {i for i, s in enumerate(img) if s.sum() > 0}
    else:
        if n_channels != 1:
            raise ValueError(f"If input not one-hotted, should only be 1 channel, got {n_channels}.")
        if isinstance(img, torch.Tensor):
            applied_labels = set(torch.unique(img.as_tensor() if _is_meta(img) else img).cpu().tolist())
        else:
            import numpy as np

            applied_labels = set(np.unique(img).tolist())
    if discard is not None:
        for i in ensure_tuple(discard):
            applied_labels.discard(i)
    return applied_labels


@function_fallback("monai.transforms.utils", "fill_holes")
def fill_holes(img, applied_labels=None, connectivity: int | None = None):
    """Fill the enclosed holes of a ``[C, spatial...]`` device tensor (two or three spatial axes): a hole of label v is a component of the voxels
    that are not v -- connected under `connectivity` -- that does not touch the border of the volume.  C == 1: a label map, one labelling pass per label
    in the iteration order of the reference's Python ``set``, since a later label sees the earlier fills; C > 1: one-hot, the applied channels batched
    into one set of launches, each rewritten as 0 / 1.  Returns a NEW tensor of the input's dtype; the input is untouched.  Without
    `applied_labels` one small device-to-host read (the unique values) precedes the launches; nothing else reads back."""
    t = _cc_device_tensor(img, "fill_holes")
    rank = t.dim() - 1
    if rank not in (2, 3) or t.numel() == 0:
        raise NotImplementedError(f"monai_amd.fill_holes: two or three non-empty spatial axes on the HIP path, got {tuple(t.shape)}")
    conn = min(max(int(connectivity or rank), 1), rank)      # scipy's generate_binary_structure clamps the same way
    is_one_hot = t.shape[0] > 1
    out = _cc_work(t)
    if out.data_ptr() == t.data_ptr():
        out = out.clone()
    labels_set = set(applied_labels) if applied_labels is not None else get_unique_labels(out, is_one_hot)
    labels_set.discard(0)
    spatial, n = tuple(t.shape[1:]), out[0].numel()
    if is_one_hot:
        chans = []
        for label in labels_set:
            if int(label) != label or not -t.shape[0] <= int(label) < t.shape[0]:
                raise IndexError(f"index {label} is out of bounds for axis 0 with size {t.shape[0]}")
            chans.append(int(label) % t.shape[0])
        if chans:
            items = ops.CcItems(spatial, [{"src": c * n, "rule": ops.CC_EQ, "v": 0.0, "fill_mode": ops.CC_FILL_BINARY} for c in chans], t.device)
            lab = ops.cc_label(out, items, conn)
            _, border = ops.cc_records(lab, items)
            ops.cc_fill(out, lab, border, items)
    else:
        for label in labels_set:
            items = ops.CcItems(spatial, [{"src": 0, "rule": ops.CC_NE, "v": float(label), "fill": float(label)}], t.device)
            lab = ops.cc_label(out, items, conn)
            _, border = ops.cc_records(lab, items)
            ops.cc_fill(out, lab, border, items)
    out = out.to(t.dtype)
    return type(img)(out).copy_meta_from(img) if _is_meta(img) else out
