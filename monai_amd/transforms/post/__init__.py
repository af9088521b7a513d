from .array import Activations, AsDiscrete, DistanceTransformEDT  # noqa: F401
from .dictionary import (  # noqa: F401
    ActivationsD, ActivationsDict, Activationsd, AsDiscreteD, AsDiscreteDict, AsDiscreted, DistanceTransformEDTD, DistanceTransformEDTDict, DistanceTransformEDTd,
)
