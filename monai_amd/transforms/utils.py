"""``distance_transform_edt`` on the exact Euclidean distance transform kernels (csrc/kernels/edt.h).  Drop-in for
monai/transforms/utils.py:2426-2560 under the contract of the reference's GPU form (cuCIM, which does not exist for ROCm): float32 distances, or
float64 with ``float64_distances=True``.

Every channel is transformed on its own: the distance of each non-zero voxel to the nearest zero voxel of its channel.  Without ``sampling`` the
squared distances are exact integers and the result is ``sqrt`` formed in fp64 (rounded once for float32): scipy's float64 output bit for bit.
A channel WITHOUT any zero voxel comes out ``+inf`` everywhere: there is no background to measure to (scipy returns an artefact of its algorithm
there, which is not reproduced)."""

from __future__ import annotations

import torch

from .. import ops
from .._fallback import function_fallback

__all__ = ["distance_transform_edt"]


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
