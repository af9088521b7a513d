"""``Activations`` / ``AsDiscrete`` -- the step after the sliding-window inferer in every segmentation bundle -- on HIP
kernels (csrc/kernels/post.h).  Drop-ins for monai/transforms/post/array.py:61-237: same arguments, defaults and errors.
Channel-first tensors (no batch axis), reductions over ``dim=0`` (the reference's default; other axes are not on the HIP
path).  Outputs are float32 like the reference's (``convert_to_dst_type(..., dtype=torch.float)``)."""

from __future__ import annotations

from collections.abc import Callable

import torch

from ... import ops
from ...utils.misc import ensure_tuple, look_up_option

__all__ = ["Activations", "AsDiscrete", "DistanceTransformEDT", "KeepLargestConnectedComponent", "FillHoles", "LabelFilter"]


def _is_meta(x) -> bool:
    return type(x) is not torch.Tensor and hasattr(x, "as_tensor")


def _like(out: torch.Tensor, img):
    if _is_meta(img):
        return type(img)(out).copy_meta_from(img)
    return out


def _plain(img) -> torch.Tensor:
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"monai_amd: a device tensor is required, got {type(img).__name__} (no CPU / numpy path in the product)")
    return img.as_tensor() if _is_meta(img) else img


class Activations:
    def __init__(self, sigmoid: bool = False, softmax: bool = False, other: Callable | None = None, **kwargs) -> None:
        self.sigmoid = sigmoid
        self.softmax = softmax
        self.kwargs = kwargs
        if other is not None and not callable(other):
            raise TypeError(f"other must be None or callable but is {type(other).__name__}.")
        self.other = other

    def __call__(self, img, sigmoid: bool | None = None, softmax: bool | None = None, other: Callable | None = None):
        if sigmoid and softmax:
            raise ValueError("Incompatible values: sigmoid=True and softmax=True.")
        if other is not None and not callable(other):
            raise TypeError(f"other must be None or callable but is {type(other).__name__}.")
        t = _plain(img).to(torch.float32).contiguous()
        if sigmoid or self.sigmoid:
            t = ops.pointwise("sigmoid", t)
        if softmax or self.softmax:
            if self.kwargs.get("dim", 0) != 0:
                raise NotImplementedError("monai_amd.Activations: softmax over dim=0 (the channel axis) is what the HIP path implements")
            t = ops.channel_reduce("softmax", t)
        act_func = self.other if other is None else other
        if act_func is not None:
            t = act_func(t)
        return _like(t, img)


class AsDiscrete:
    def __init__(self, argmax: bool = False, to_onehot: int | None = None, threshold: float | None = None, rounding: str | None = None, **kwargs) -> None:
        self.argmax = argmax
        if isinstance(to_onehot, bool):
            raise ValueError("`to_onehot=True/False` is deprecated, please use `to_onehot=num_classes` instead.")
        self.to_onehot = to_onehot
        self.threshold = threshold
        self.rounding = rounding
        self.kwargs = kwargs

    def __call__(self, img, argmax: bool | None = None, to_onehot: int | None = None, threshold: float | None = None, rounding: str | None = None):
        if isinstance(to_onehot, bool):
            raise ValueError("`to_onehot=True/False` is deprecated, please use `to_onehot=num_classes` instead.")
        if self.kwargs.get("dim", 0) != 0 or not self.kwargs.get("keepdim", True) or self.kwargs.get("dtype", torch.float) not in (torch.float, torch.float32):
            raise NotImplementedError("monai_amd.AsDiscrete: dim=0, keepdim=True, dtype=float32 (the reference's defaults) are what the HIP path implements")
        t = _plain(img).to(torch.float32).contiguous()
        argmax = self.argmax if argmax is None else argmax
        if argmax:
            t = ops.channel_reduce("argmax", t)
        to_onehot = self.to_onehot if to_onehot is None else to_onehot
        if to_onehot is not None:
            if not isinstance(to_onehot, int):
                raise ValueError(f"the number of classes for One-Hot must be an integer, got {type(to_onehot)}.")
            if t.dim() < 2:      # a scalar / 1-D label: the reference's one_hot reshapes it (networks/utils.py:170-220); not a volume for the kernel
                raise NotImplementedError("monai_amd.AsDiscrete: one-hot of a label without spatial axes is not on the HIP path")
            if t.shape[0] != 1:
                raise AssertionError("labels should have a channel with length equal to one.")
            t = ops.onehot(t, to_onehot)
        threshold = self.threshold if threshold is None else threshold
        if threshold is not None:
            t = ops.pointwise("threshold", t, float(threshold))
        rounding = self.rounding if rounding is None else rounding
        if rounding is not None:
            look_up_option(rounding, ["torchrounding"])
            t = ops.pointwise("round", t)
        return _like(t, img)


class DistanceTransformEDT:
    """Exact Euclidean distance transform of a channel-first image, channel by channel (monai/transforms/post/array.py:996-1029): float32 distances to
    the nearest zero voxel, ``+inf`` in a channel without one (see `monai_amd.transforms.utils.distance_transform_edt`)."""

    def __init__(self, sampling=None) -> None:
        self.sampling = sampling

    def __call__(self, img):
        from ..utils import distance_transform_edt

        return distance_transform_edt(img=img, sampling=self.sampling)


class KeepLargestConnectedComponent:
    """Keep the `num_components` largest connected components (monai/transforms/post/array.py:239-354: same arguments, defaults and results) on the
    connected-component kernels (csrc/kernels/ccl.h).  The one-hot channels, or the applied classes of a label map, are labelled, ranked and cleaned in
    ONE set of launches; ``independent=False`` labels the union of the applied labels.  Like the reference it writes into its input and returns it in
    the input's dtype, as a MetaTensor where it got one.  Equal sizes: the component whose first voxel comes later wins (see
    `monai_amd.transforms.utils.get_largest_connected_component_mask`).  `num_components` 0 .. 32 (0 removes every component, as the reference's
    empty cut does); more is not on the HIP path.  ``applied_labels=None`` costs one small device-to-host read (the unique
    values); nothing else in a call reads back."""

    def __init__(self, applied_labels=None, is_onehot: bool | None = None, independent: bool = True, connectivity: int | None = None,
                 num_components: int = 1) -> None:
        self.applied_labels = ensure_tuple(applied_labels) if applied_labels is not None else None
        self.is_onehot = is_onehot
        self.independent = independent
        self.connectivity = connectivity
        self.num_components = num_components

    def __call__(self, img):
        from .. import utils as U

        t = U._cc_device_tensor(img, "KeepLargestConnectedComponent")
        rank = t.dim() - 1
        if rank not in (2, 3) or t.numel() == 0:
            raise NotImplementedError(f"monai_amd.KeepLargestConnectedComponent: two or three non-empty spatial axes on the HIP path, got {tuple(t.shape)}")
        ops._lib.require_device(t, dtypes=(t.dtype,))
        is_onehot = t.shape[0] > 1 if self.is_onehot is None else self.is_onehot
        applied = self.applied_labels if self.applied_labels is not None else tuple(U.get_unique_labels(t, is_onehot, discard=0))
        applied = tuple(dict.fromkeys(applied))
        if not applied:
            return img
        conn = U._cc_connectivity(self.connectivity, rank)
        work = U._cc_work(t)
        spatial, n, nch, dev = tuple(t.shape[1:]), t[0].numel(), int(t.shape[0]), t.device
        classes = None

        def channel(i):
            if int(i) != i or not -nch <= int(i) < nch:
                raise IndexError(f"index {i} is out of bounds for dimension 0 with size {nch}")
            return int(i) % nch

        if is_onehot and self.independent:
            source = work
            items = apply_items = ops.CcItems(spatial, [{"src": channel(i) * n, "rule": ops.CC_GT} for i in applied], dev)
        elif is_onehot:
            source = (work[[channel(i) for i in applied]] == 1).any(0).to(torch.uint8).contiguous()
            items = ops.CcItems(spatial, [{"src": 0, "rule": ops.CC_GT}], dev)
            apply_items = ops.CcItems(spatial, [{"src": channel(i) * n, "off": 0} for i in applied], dev)
        else:
            values = torch.as_tensor(applied, dtype=work.dtype).tolist() if not self.independent else list(applied)      # the reference casts the union's labels to the image's dtype
            values = list(dict.fromkeys(float(v) for v in values))
            source = work
            if self.independent:
                chunks = [values[k:k + ops.CC_MAX_LABELS] for k in range(0, len(values), ops.CC_MAX_LABELS)]
                items = apply_items = ops.CcItems(spatial, [{"src": 0, "rule": ops.CC_LIST_VALUE, "labels": c} for c in chunks], dev)
                classes = [(work[0].reshape(-1), c) for c in chunks]
            else:
                if len(values) > ops.CC_MAX_LABELS:
                    raise NotImplementedError(f"monai_amd.KeepLargestConnectedComponent: a union of at most {ops.CC_MAX_LABELS} labels on the HIP path")
                items = apply_items = ops.CcItems(spatial, [{"src": 0, "rule": ops.CC_LIST_ANY, "labels": values}], dev)
        labels = ops.cc_label(source, items, conn)
        keep = U._cc_largest_roots(items, labels, self.num_components, classes)
        if apply_items is not items:
            keep = keep.expand(apply_items.nitems, keep.shape[1]).contiguous()
        ops.cc_keep(work, labels, keep, apply_items)
        if work.data_ptr() != t.data_ptr():
            t.copy_(work)
        return img


class FillHoles:
    """Fill the enclosed holes of every applied label (monai/transforms/post/array.py:503-578) on the connected-component kernels: see
    `monai_amd.transforms.utils.fill_holes`.  Returns a new tensor; the device input stays untouched."""

    def __init__(self, applied_labels=None, connectivity: int | None = None) -> None:
        self.applied_labels = ensure_tuple(applied_labels) if applied_labels else None
        self.connectivity = connectivity

    def __call__(self, img):
        from ..utils import fill_holes

        return fill_holes(img, self.applied_labels, self.connectivity)


class LabelFilter:
    """Keep the values that are in `applied_labels`, everything else becomes 0 (monai/transforms/post/array.py:445-500): one kernel, any shape."""

    _mh_numpy_to_reference = True      # the reference answers a numpy array with a numpy array

    def __init__(self, applied_labels) -> None:
        self.applied_labels = ensure_tuple(applied_labels)

    def __call__(self, img):
        import numpy as np

        if not isinstance(img, (np.ndarray, torch.Tensor)):
            raise NotImplementedError(f"{self.__class__} can not handle data of type {type(img)}.")
        if not isinstance(img, torch.Tensor) or img.dim() < 2:
            raise ops._lib.UnsupportedOnDevice("monai_amd.LabelFilter: device tensors with at least two axes are what the HIP path takes")
        t = _plain(img)
        if t.dtype not in (torch.float32, torch.uint8, torch.int64, torch.bool):
            raise NotImplementedError(f"monai_amd.LabelFilter: dtype {t.dtype} is not on the HIP path")
        return _like(ops.cc_filter(t.contiguous(), self.applied_labels), img)
