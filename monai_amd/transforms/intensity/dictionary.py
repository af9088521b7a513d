"""``GaussianSmoothd`` (monai/transforms/intensity/dictionary.py:1184-1216), ``MedianSmoothd`` (dictionary.py:1157-1181) and ``ScaleIntensityRanged``
(dictionary.py:855-892)."""

from __future__ import annotations

import numpy as np

from ...utils.misc import ensure_tuple
from .array import ClipIntensityPercentiles, GaussianSmooth, MedianSmooth, NormalizeIntensity, ScaleIntensity, ScaleIntensityRange, ScaleIntensityRangePercentiles

__all__ = ["GaussianSmoothd", "GaussianSmoothD", "GaussianSmoothDict", "ScaleIntensityRanged", "ScaleIntensityRangeD", "ScaleIntensityRangeDict",
           "NormalizeIntensityd", "NormalizeIntensityD", "NormalizeIntensityDict", "ScaleIntensityd", "ScaleIntensityD", "ScaleIntensityDict",
           "ScaleIntensityRangePercentilesd", "ScaleIntensityRangePercentilesD", "ScaleIntensityRangePercentilesDict",
           "ClipIntensityPercentilesd", "ClipIntensityPercentilesD", "ClipIntensityPercentilesDict", "MedianSmoothd", "MedianSmoothD", "MedianSmoothDict"]


class GaussianSmoothd:
    def __init__(self, keys, sigma=1.0, approx: str = "erf", allow_missing_keys: bool = False) -> None:
        self.keys = ensure_tuple(keys)
        self.allow_missing_keys = allow_missing_keys
        self.converter = GaussianSmooth(sigma, approx=approx)

    def __call__(self, data):
        d = dict(data)
        for key in self.keys:
            if key not in d:
                if self.allow_missing_keys:
                    continue
                raise KeyError(f"Key `{key}` of transform `{type(self).__name__}` was missing in the data and allow_missing_keys==False.")
            d[key] = self.converter(d[key])
        return d


GaussianSmoothD = GaussianSmoothDict = GaussianSmoothd


class ScaleIntensityRanged(GaussianSmoothd):
    """Dictionary version of :class:`ScaleIntensityRange` (same key handling as the class above)."""

    def __init__(self, keys, a_min: float, a_max: float, b_min=None, b_max=None, clip: bool = False, dtype="float32", allow_missing_keys: bool = False) -> None:

        self.keys = ensure_tuple(keys)
        self.allow_missing_keys = allow_missing_keys
        self.scaler = self.converter = ScaleIntensityRange(a_min, a_max, b_min, b_max, clip, dtype)


ScaleIntensityRangeD = ScaleIntensityRangeDict = ScaleIntensityRanged


class NormalizeIntensityd(GaussianSmoothd):
    """Dictionary version of :class:`NormalizeIntensity` (monai/transforms/intensity/dictionary.py:782-820)."""

    def __init__(self, keys, subtrahend=None, divisor=None, nonzero: bool = False, channel_wise: bool = False, dtype="float32",
                 allow_missing_keys: bool = False) -> None:
        self.keys = ensure_tuple(keys)
        self.allow_missing_keys = allow_missing_keys
        self.normalizer = self.converter = NormalizeIntensity(subtrahend, divisor, nonzero, channel_wise, dtype)


NormalizeIntensityD = NormalizeIntensityDict = NormalizeIntensityd


class ScaleIntensityd(GaussianSmoothd):
    """Dictionary version of :class:`ScaleIntensity` (monai/transforms/intensity/dictionary.py:547-590)."""

    def __init__(self, keys, minv=0.0, maxv=1.0, factor=None, channel_wise: bool = False, dtype="float32", allow_missing_keys: bool = False) -> None:
        self.keys = ensure_tuple(keys)
        self.allow_missing_keys = allow_missing_keys
        self.scaler = self.converter = ScaleIntensity(minv, maxv, factor, channel_wise, dtype)


ScaleIntensityD = ScaleIntensityDict = ScaleIntensityd


class ScaleIntensityRangePercentilesd(GaussianSmoothd):
    """Dictionary version of :class:`ScaleIntensityRangePercentiles` (monai/transforms/intensity/dictionary.py:895-948)."""

    def __init__(self, keys, lower: float, upper: float, b_min, b_max, clip: bool = False, relative: bool = False, channel_wise: bool = False,
                 dtype=np.float32, allow_missing_keys: bool = False) -> None:
        self.keys = ensure_tuple(keys)
        self.allow_missing_keys = allow_missing_keys
        self.scaler = self.converter = ScaleIntensityRangePercentiles(lower, upper, b_min, b_max, clip, relative, channel_wise, dtype)


ScaleIntensityRangePercentilesD = ScaleIntensityRangePercentilesDict = ScaleIntensityRangePercentilesd


class ClipIntensityPercentilesd(GaussianSmoothd):
    """Dictionary version of :class:`ClipIntensityPercentiles` (monai/transforms/intensity/dictionary.py:951-989)."""

    def __init__(self, keys, lower, upper, sharpness_factor=None, channel_wise: bool = False, dtype=np.float32, allow_missing_keys: bool = False) -> None:
        self.keys = ensure_tuple(keys)
        self.allow_missing_keys = allow_missing_keys
        self.scaler = self.converter = ClipIntensityPercentiles(lower=lower, upper=upper, sharpness_factor=sharpness_factor, channel_wise=channel_wise, dtype=dtype)


ClipIntensityPercentilesD = ClipIntensityPercentilesDict = ClipIntensityPercentilesd


class MedianSmoothd(GaussianSmoothd):
    """Dictionary version of :class:`MedianSmooth` (monai/transforms/intensity/dictionary.py:1157-1181)."""

    def __init__(self, keys, radius, allow_missing_keys: bool = False) -> None:
        self.keys = ensure_tuple(keys)
        self.allow_missing_keys = allow_missing_keys
        self.converter = MedianSmooth(radius)


MedianSmoothD = MedianSmoothDict = MedianSmoothd
