"""``GaussianSmooth`` (monai/transforms/intensity/array.py:1590-1622, the fused smoothing kernel), ``MedianSmooth`` (array.py:1561-1587,
the exact median-filter kernel), ``ScaleIntensityRange``
(array.py:958-1012, one element-wise pass), ``NormalizeIntensity``, ``ScaleIntensity`` and the percentile transforms
``ScaleIntensityRangePercentiles`` (array.py:1299-1418) and ``ClipIntensityPercentiles`` (array.py:1015-1157) on the exact
order-statistic kernel."""

from __future__ import annotations

from collections.abc import Sequence

import numpy as np
import torch

from ...data.meta_tensor import is_meta
from ...networks.layers.simplelayers import GaussianFilter, MedianFilter
from ...utils.misc import ensure_tuple_rep

__all__ = ["GaussianSmooth", "MedianSmooth", "ScaleIntensityRange", "NormalizeIntensity", "ScaleIntensity", "ScaleIntensityRangePercentiles", "ClipIntensityPercentiles"]


class GaussianSmooth:
    """Gaussian smoothing of a channel-first image; ``sigma`` is a scalar or one value per spatial axis."""

    def __init__(self, sigma: Sequence[float] | float = 1.0, approx: str = "erf") -> None:
        self.sigma, self.approx = sigma, approx

    def __call__(self, img):
        data = img.as_tensor() if is_meta(img) else torch.as_tensor(img)
        x = data.to(torch.float)
        sigma = list(self.sigma) if isinstance(self.sigma, Sequence) else self.sigma
        out = GaussianFilter(x.ndim - 1, sigma, approx=self.approx)(x.unsqueeze(0)).squeeze(0)
        if is_meta(img):
            return type(img)(out, meta=dict(img.meta), applied_operations=list(getattr(img, "applied_operations", [])))
        return out


class MedianSmooth:
    """``monai.transforms.MedianSmooth`` (monai/transforms/intensity/array.py:1561-1587): median filter of a channel-first image over a box of
    ``radius`` (a scalar or one value per spatial axis), replicate padding, on the exact selection kernel (csrc/kernels/median.h) -- one pass
    over the image, where the reference writes every voxel's whole window out before ``torch.median``.  The image is converted to float32,
    as there; finite inputs give the reference's bits."""

    def __init__(self, radius: Sequence[int] | int = 1) -> None:
        self.radius = radius

    def __call__(self, img):
        data = img.as_tensor() if is_meta(img) else torch.as_tensor(img)
        x = data.to(torch.float)
        spatial_dims = x.ndim - 1
        out = MedianFilter(ensure_tuple_rep(self.radius, spatial_dims), spatial_dims=spatial_dims)(x)
        if is_meta(img):
            return type(img)(out, meta=dict(img.meta), applied_operations=list(getattr(img, "applied_operations", [])))
        return out


_NP2T = {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16, "int16": torch.int16, "int32": torch.int32,
         "int64": torch.int64, "uint8": torch.uint8, "int8": torch.int8, "bool": torch.bool}


def _to_torch_dtype(dtype):
    if dtype is None or isinstance(dtype, torch.dtype):
        return dtype
    import numpy as np

    return _NP2T[np.dtype(dtype).name]


class ScaleIntensityRange:
    """``monai.transforms.ScaleIntensityRange`` (monai/transforms/intensity/array.py:958-1012) as one HIP pass over the device
    tensor: ``(img - a_min) / (a_max - a_min)``, optionally ``* (b_max - b_min) + b_min``, optionally clamped -- the reference's
    operator sequence with each of its fp32 roundings kept, so the results are bit-identical to the reference's.  Integer images
    are promoted to float32 first (what the reference's first subtraction does); float64 / half images are not on this path."""

    def __init__(self, a_min: float, a_max: float, b_min: float | None = None, b_max: float | None = None, clip: bool = False,
                 dtype=torch.float32) -> None:
        self.a_min, self.a_max, self.b_min, self.b_max, self.clip, self.dtype = a_min, a_max, b_min, b_max, clip, dtype

    def __call__(self, img):
        from ... import ops
        import warnings

        data = img.as_tensor() if is_meta(img) else torch.as_tensor(img)
        if data.dtype in (torch.float64, torch.float16, torch.bfloat16) or data.is_complex():
            raise NotImplementedError(f"monai_amd.ScaleIntensityRange: {data.dtype} images are not on the HIP path (float32 / integer images are)")
        x = data.to(torch.float32).contiguous()
        dtype = _to_torch_dtype(self.dtype) or x.dtype
        if self.a_max - self.a_min == 0.0:                       # array.py:999-1003: no division, no clip, no dtype conversion
            warnings.warn("Divide by zero (a_min == a_max)", Warning)
            out = ops.scale_intensity_range(x, self.a_min, 1.0, None if self.b_min is None else 1.0, self.b_min or 0.0, None, None)
        else:
            rescale = self.b_min is not None and self.b_max is not None
            if self.clip and self.b_min is None and self.b_max is None:       # array.py:1009 -> torch.clamp(img, None, None)
                raise RuntimeError("torch.clamp: At least one of 'min' or 'max' must not be None")
            out = ops.scale_intensity_range(
                x, self.a_min, self.a_max - self.a_min, (self.b_max - self.b_min) if rescale else None, self.b_min if rescale else 0.0,
                self.b_min if self.clip else None, self.b_max if self.clip else None)
            if out.dtype != dtype:
                out = out.to(dtype)
        if is_meta(img):
            return type(img)(out, meta=dict(img.meta), applied_operations=list(getattr(img, "applied_operations", [])))
        return out


class NormalizeIntensity:
    """``monai.transforms.NormalizeIntensity`` (monai/transforms/intensity/array.py:816-907): ``(img - mean) / std`` over the whole
    image or per channel, optionally over the non-zero voxels only (which are then the only ones rewritten), or with given
    ``subtrahend`` / ``divisor``.  Two HBM passes on the device tensor: fp64 {count, sum, sum of squares} per workgroup folded into
    the fp32 {mean, std} pair per channel ON THE DEVICE, then the apply pass reads that pair -- the reference's ``.item()`` round
    trips between the two do not exist here.  The reference's sums are fp32 tree sums, these are fp64: results agree to fp32
    rounding (<= 1e-6 relative, stated in the tests), not bit for bit.  Scalar / per-channel ``subtrahend`` / ``divisor`` only
    (voxel-wise arrays are not on the HIP path).  The input is never modified (the reference normalises float inputs in place)."""

    def __init__(self, subtrahend=None, divisor=None, nonzero: bool = False, channel_wise: bool = False, dtype=torch.float32) -> None:
        self.subtrahend, self.divisor, self.nonzero, self.channel_wise, self.dtype = subtrahend, divisor, nonzero, channel_wise, dtype

    @staticmethod
    def _per_channel(v, c: int, what: str):
        """None | scalar | sequence of c scalars -> list of c floats (or None)"""
        import numpy as np

        if v is None:
            return None
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if a.ndim == 0:
            return [float(a)] * c
        if a.ndim == 1 and a.shape[0] == c:
            return [float(x) for x in a]
        raise NotImplementedError(f"monai_amd.NormalizeIntensity: a {what} of shape {a.shape} is not on the HIP path (scalars / one value per channel are)")

    def __call__(self, img):
        from ... import ops

        data = img.as_tensor() if is_meta(img) else torch.as_tensor(img)
        if data.dtype in (torch.float64, torch.float16, torch.bfloat16) or data.is_complex():
            raise NotImplementedError(f"monai_amd.NormalizeIntensity: {data.dtype} images are not on the HIP path (float32 / integer images are)")
        dtype = _to_torch_dtype(self.dtype) or data.dtype
        if self.channel_wise:
            if self.subtrahend is not None and len(self.subtrahend) != len(data):
                raise ValueError(f"img has {len(data)} channels, but subtrahend has {len(self.subtrahend)} components.")
            if self.divisor is not None and len(self.divisor) != len(data):
                raise ValueError(f"img has {len(data)} channels, but divisor has {len(self.divisor)} components.")
        x = data.to(torch.float32).contiguous()
        c = int(x.shape[0]) if self.channel_wise and x.dim() > 0 else 1
        sub = self._per_channel(self.subtrahend, c, "subtrahend")
        div = self._per_channel(self.divisor, c, "divisor")
        if div is not None:
            div = [1.0 if d == 0.0 else d for d in div]                       # array.py:866-868
        if not x.numel():
            out = x
        else:
            n = x.numel() // c
            if sub is not None and div is not None:
                table = torch.tensor([[s, d] for s, d in zip(sub, div)], dtype=torch.float32).to(x.device)
            else:
                table = ops.normalize_stats(x, c, n, self.nonzero)
                if sub is not None:
                    table[:, 0] = torch.tensor(sub, dtype=torch.float32).to(x.device)
                if div is not None:
                    table[:, 1] = torch.tensor(div, dtype=torch.float32).to(x.device)
            out = ops.normalize_apply(x, c, n, self.nonzero, table)
        if out.dtype != dtype:
            out = out.to(dtype)
        if is_meta(img):
            return type(img)(out, meta=dict(img.meta), applied_operations=list(getattr(img, "applied_operations", [])))
        return out


class ScaleIntensity:
    """``monai.transforms.ScaleIntensity`` (monai/transforms/intensity/array.py:445-491): rescale to ``[minv, maxv]`` from the image's (or
    each channel's) own minimum / maximum, or multiply by ``1 + factor`` when both are None.  Min / max are exact reductions left in device
    memory, the apply pass keeps the reference's fp32 operator sequence: bit-identical results, no host round trip.  The reference
    converts the image to ``dtype`` BEFORE the arithmetic (rescale_array, monai/transforms/utils.py:229-251); float32 is on the HIP path."""

    def __init__(self, minv: float | None = 0.0, maxv: float | None = 1.0, factor: float | None = None, channel_wise: bool = False,
                 dtype=torch.float32) -> None:
        self.minv, self.maxv, self.factor, self.channel_wise, self.dtype = minv, maxv, factor, channel_wise, dtype

    def __call__(self, img):
        from ... import ops

        data = img.as_tensor() if is_meta(img) else torch.as_tensor(img)
        dtype = _to_torch_dtype(self.dtype)
        if data.dtype in (torch.float64, torch.float16, torch.bfloat16) or data.is_complex() or dtype not in (None, torch.float32):
            raise NotImplementedError("monai_amd.ScaleIntensity: float32 arithmetic only (float32 / integer images, dtype float32 or None)")
        if dtype is None and data.dtype != torch.float32:
            raise NotImplementedError("monai_amd.ScaleIntensity: dtype=None on an integer image is integer arithmetic in the reference; not on the HIP path")
        x = data.to(torch.float32).contiguous()
        if self.minv is not None or self.maxv is not None:
            c = int(x.shape[0]) if self.channel_wise and x.dim() > 0 else 1
            if not x.numel():
                out = x
            else:
                both = self.minv is not None and self.maxv is not None
                out = ops.minmax_scale(x, c, x.numel() // c, (self.maxv - self.minv) if both else None, self.minv if both else 0.0, self.minv)
        elif self.factor is not None:
            out = ops.scale_intensity_range(x, 0.0, 1.0, 1 + self.factor, 0.0, None, None)      # (x - 0) / 1 * (1 + factor) + 0: exact steps around one multiply
        else:
            out = x
        if is_meta(img):
            return type(img)(out, meta=dict(img.meta), applied_operations=list(getattr(img, "applied_operations", [])))
        return out


def _percentile_input(img, name: str, channel_wise: bool):
    """the float32 image as a contiguous tensor, the number of runs and their length"""
    data = img.as_tensor() if is_meta(img) else torch.as_tensor(img)
    if data.dtype != torch.float32:
        raise NotImplementedError(f"monai_amd.{name}: {data.dtype} images are not on the HIP path (float32 images are)")
    x = data.contiguous()
    c = int(x.shape[0]) if channel_wise and x.dim() > 0 else 1
    if not x.numel() or c < 1:
        raise NotImplementedError(f"monai_amd.{name}: an empty image has no percentiles")
    return x, c, x.numel() // c


class ScaleIntensityRangePercentiles:
    """``monai.transforms.ScaleIntensityRangePercentiles`` (monai/transforms/intensity/array.py:1299-1418): ScaleIntensityRange from the image's
    (or, ``channel_wise``, each channel's) own ``lower`` / ``upper`` intensity percentiles to ``[b_min, b_max]``; ``relative`` scales to the
    corresponding percentiles of ``[b_min, b_max]`` instead (computed on the host in doubles, as the reference does).  The percentiles come from an
    exact radix select on the device (csrc/kernels/select.h) and stay in device memory for the apply pass: the reference's copy of every image
    above 1,000,000 elements to the host, its ``np.percentile`` there and its full sort below that size do not exist here, and nothing is
    read back.  The percentile values reproduce the reference's two regimes (np.percentile above 1,000,000 elements per call, torch.quantile
    below) and the apply pass keeps ScaleIntensityRange's fp32 operator sequence.

    One deliberate difference: a constant image (``a_min == a_max``) takes the reference's branch without a division -- decided on the
    device -- but the reference's ``"Divide by zero (a_min == a_max)"`` warning is NOT issued: it would need the values on the host.
    float32 images only; other dtypes are not on the HIP path."""

    def __init__(self, lower: float, upper: float, b_min: float | None, b_max: float | None, clip: bool = False, relative: bool = False,
                 channel_wise: bool = False, dtype=np.float32) -> None:
        if lower < 0.0 or lower > 100.0:
            raise ValueError("Percentiles must be in the range [0, 100]")
        if upper < 0.0 or upper > 100.0:
            raise ValueError("Percentiles must be in the range [0, 100]")
        self.lower, self.upper, self.b_min, self.b_max = lower, upper, b_min, b_max
        self.clip, self.relative, self.channel_wise, self.dtype = clip, relative, channel_wise, dtype

    def __call__(self, img):
        from ... import ops

        x, c, n = _percentile_input(img, "ScaleIntensityRangePercentiles", self.channel_wise)
        dtype = _to_torch_dtype(self.dtype) or x.dtype
        b_min, b_max = self.b_min, self.b_max
        if self.relative:
            if (self.b_min is None) or (self.b_max is None):
                raise ValueError("If it is relative, b_min and b_max should not be None.")
            b_min = ((self.b_max - self.b_min) * (self.lower / 100.0)) + self.b_min
            b_max = ((self.b_max - self.b_min) * (self.upper / 100.0)) + self.b_min
        if self.clip and b_min is None and b_max is None:       # array.py:1009 -> torch.clamp(img, None, None)
            raise RuntimeError("torch.clamp: At least one of 'min' or 'max' must not be None")
        table = ops.percentiles(x, c, n, (self.lower, self.upper))
        rescale = b_min is not None and b_max is not None
        out = ops.scale_intensity_table(x, c, n, table, (b_max - b_min) if rescale else None, b_min, b_min if self.clip else None,
                                        b_max if self.clip else None)
        if out.dtype != dtype:
            out = out.to(dtype)
        if is_meta(img):
            return type(img)(out, meta=dict(img.meta), applied_operations=list(getattr(img, "applied_operations", [])))
        return out


class ClipIntensityPercentiles:
    """``monai.transforms.ClipIntensityPercentiles`` (monai/transforms/intensity/array.py:1015-1157), the hard clip: ``torch.clamp`` of the image
    (or, ``channel_wise``, of each channel) to its own ``lower`` / ``upper`` intensity percentiles; a ``None`` bound is percentile 0 / 100.  The
    percentiles come from the exact radix select on the device (csrc/kernels/select.h) and are read by the clamp pass from device memory; only
    ``return_clipping_values=True`` reads them back -- one device-to-host copy of the whole table -- to fill ``meta["clipping_values"]`` the way
    the reference does (the list the instance keeps, one ``(lower, upper)`` tuple appended per image or per channel).  ``dtype`` only reaches the
    reference's soft clip, as there.  The soft clip (``sharpness_factor``) and images other than float32 are not on the HIP path."""

    def __init__(self, lower: float | None, upper: float | None, sharpness_factor: float | None = None, channel_wise: bool = False,
                 return_clipping_values: bool = False, dtype=np.float32) -> None:
        if lower is None and upper is None:
            raise ValueError("lower or upper percentiles must be provided")
        if lower is not None and (lower < 0.0 or lower > 100.0):
            raise ValueError("Percentiles must be in the range [0, 100]")
        if upper is not None and (upper < 0.0 or upper > 100.0):
            raise ValueError("Percentiles must be in the range [0, 100]")
        if upper is not None and lower is not None and upper < lower:
            raise ValueError("upper must be greater than or equal to lower")
        if sharpness_factor is not None and sharpness_factor <= 0:
            raise ValueError("sharpness_factor must be greater than 0")
        if sharpness_factor is not None:
            raise NotImplementedError("monai_amd.ClipIntensityPercentiles: the soft clip (sharpness_factor) is not on the HIP path")
        self.lower, self.upper, self.sharpness_factor, self.channel_wise = lower, upper, sharpness_factor, channel_wise
        if return_clipping_values:
            self.clipping_values: list = []
        self.return_clipping_values, self.dtype = return_clipping_values, dtype

    def __call__(self, img):
        from ... import ops
        from ...data.meta_tensor import MetaTensor

        x, c, n = _percentile_input(img, "ClipIntensityPercentiles", self.channel_wise)
        table = ops.percentiles(x, c, n, (0.0 if self.lower is None else self.lower, 100.0 if self.upper is None else self.upper))
        out = ops.clamp_table(x, c, n, table)
        meta = dict(img.meta) if is_meta(img) else {}
        if self.return_clipping_values:
            self.clipping_values.extend((float(lo), float(hi)) for lo, hi in table.cpu().tolist())      # the one device-to-host read
            meta["clipping_values"] = self.clipping_values
        if is_meta(img):
            return type(img)(out, meta=meta, applied_operations=list(getattr(img, "applied_operations", [])))
        return MetaTensor(out, meta=meta) if self.return_clipping_values else out
