from .filtering import BilateralFilter  # noqa: F401
from .simplelayers import GaussianFilter, MedianFilter, gaussian_1d, median_filter, separable_filtering  # noqa: F401
from .spatial_transforms import AffineTransform, grid_count, grid_grad, grid_pull, grid_push  # noqa: F401
