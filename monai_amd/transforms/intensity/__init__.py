from .array import ClipIntensityPercentiles, GaussianSmooth, NormalizeIntensity, ScaleIntensity, ScaleIntensityRange, ScaleIntensityRangePercentiles  # noqa: F401
from .dictionary import (  # noqa: F401
    ClipIntensityPercentilesD, ClipIntensityPercentilesDict, ClipIntensityPercentilesd, GaussianSmoothD, GaussianSmoothDict, GaussianSmoothd,
    NormalizeIntensityD, NormalizeIntensityDict, NormalizeIntensityd, ScaleIntensityD, ScaleIntensityDict, ScaleIntensityRangeD,
    ScaleIntensityRangeDict, ScaleIntensityRangePercentilesD, ScaleIntensityRangePercentilesDict, ScaleIntensityRangePercentilesd,
    ScaleIntensityRanged, ScaleIntensityd,
)
