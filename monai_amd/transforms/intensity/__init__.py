from .array import ClipIntensityPercentiles, GaussianSmooth, MedianSmooth, NormalizeIntensity, ScaleIntensity, ScaleIntensityRange, ScaleIntensityRangePercentiles  # noqa: F401
from .dictionary import (  # noqa: F401
    ClipIntensityPercentilesD, ClipIntensityPercentilesDict, ClipIntensityPercentilesd, GaussianSmoothD, GaussianSmoothDict, GaussianSmoothd,
    MedianSmoothD, MedianSmoothDict, MedianSmoothd,
    NormalizeIntensityD, NormalizeIntensityDict, NormalizeIntensityd, ScaleIntensityD, ScaleIntensityDict, ScaleIntensityRangeD,
    ScaleIntensityRangeDict, ScaleIntensityRangePercentilesD, ScaleIntensityRangePercentilesDict, ScaleIntensityRangePercentilesd,
    ScaleIntensityRanged, ScaleIntensityd,
)
