from .array import Activations, AsDiscrete, DistanceTransformEDT, FillHoles, KeepLargestConnectedComponent, LabelFilter  # noqa: F401
from .dictionary import (  # noqa: F401
    ActivationsD, ActivationsDict, Activationsd, AsDiscreteD, AsDiscreteDict, AsDiscreted, DistanceTransformEDTD, DistanceTransformEDTDict, DistanceTransformEDTd,
    FillHolesD, FillHolesDict, FillHolesd, KeepLargestConnectedComponentD, KeepLargestConnectedComponentDict, KeepLargestConnectedComponentd, LabelFilterD,
    LabelFilterDict, LabelFilterd,
)
