"""``gaussian_1d`` / ``separable_filtering`` / ``GaussianFilter`` on the fused MI355X smoothing kernel -- drop-ins for
monai/networks/layers/convutils.py:78-131 and monai/networks/layers/simplelayers.py:207-249, :542-595 -- and ``median_filter`` /
``MedianFilter`` (simplelayers.py:430-539) on the exact median-filter kernel."""

from __future__ import annotations

from collections.abc import Sequence

import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ..._fallback import function_fallback
from ...utils.misc import ensure_tuple_rep

__all__ = ["gaussian_1d", "separable_filtering", "GaussianFilter", "get_binary_kernel", "median_filter", "MedianFilter"]


def gaussian_1d(sigma, truncated: float = 4.0, approx: str = "erf", normalize: bool = False) -> torch.Tensor:
    """1-D discrete Gaussian with ``tail = int(max(sigma * truncated, 0.5) + 0.5)`` taps each side, evaluated on the HOST
    in fp32 with the same torch operators as the reference ("erf": 0.5*(erf(t(x+.5)) - erf(t(x-.5))), t = 0.70710678/|sigma|,
    clamped at 0; "sampled": exp(-x^2 / 2 sigma^2) / (2.5066282 sigma)) so the taps are bit-identical to the reference's CPU
    kernel.  "scalespace" (discrete Gaussian, I_k(sigma^2) e^{-sigma^2}) uses scipy's exponentially scaled Bessel function in
    fp64 instead of the reference's fp32 polynomial recurrences: equal to ~1e-7."""
    sigma = torch.as_tensor(sigma, dtype=torch.float).detach().cpu()
    if truncated <= 0.0:
        raise ValueError(f"truncated must be positive, got {truncated}.")
    tail = int(max(float(sigma) * truncated, 0.5) + 0.5)
    kind = approx.lower()
    if kind == "erf":
        x = torch.arange(-tail, tail + 1, dtype=torch.float)
        t = 0.70710678 / torch.abs(sigma)
        out = 0.5 * ((t * (x + 0.5)).erf() - (t * (x - 0.5)).erf())
        out = out.clamp(min=0)
    elif kind == "sampled":
        x = torch.arange(-tail, tail + 1, dtype=torch.float)
        out = torch.exp(-0.5 / (sigma * sigma) * x**2)
        if not normalize:
            out = out / (2.5066282 * sigma)
    elif kind == "scalespace":
        from scipy.special import ive

        s2 = float(sigma) * float(sigma)
        pos = [float(ive(k, s2)) for k in range(tail + 1)]
        out = torch.tensor(pos[:0:-1] + pos, dtype=torch.float)
    else:
        raise NotImplementedError(f"Unsupported option: approx='{approx}'.")
    return out / out.sum() if normalize else out


def separable_filtering(x: torch.Tensor, kernels, mode: str = "zeros") -> torch.Tensor:
    """1-D convolution along every spatial axis of ``x`` (batch, channels, spatial...), zero padding, one fused pass."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a torch.Tensor but is {type(x).__name__}.")
    if mode != "zeros":
        raise NotImplementedError("monai_amd.separable_filtering: only mode='zeros' is on the HIP path")
    sd = x.dim() - 2
    if sd not in (2, 3):
        raise NotImplementedError("monai_amd.separable_filtering: 2-D and 3-D inputs only")
    if isinstance(kernels, torch.Tensor):
        kernels = [kernels] * sd
    ks = [np.asarray(torch.as_tensor(k).detach().cpu(), dtype=np.float32).reshape(-1) for k in kernels]
    if len(ks) != sd:
        raise ValueError(f"expected {sd} kernels, got {len(ks)}")
    for k in ks:
        if k.size % 2 == 0:
            raise NotImplementedError("monai_amd.separable_filtering: even-length kernels are not on the HIP path")
    ks = [np.ones(1, dtype=np.float32)] * (3 - sd) + ks
    data = x.as_tensor() if hasattr(x, "as_tensor") else x
    src = data.to(torch.float32).contiguous()
    b, c = src.shape[:2]
    sp = (1,) * (3 - sd) + tuple(src.shape[2:])
    out = ops.separable_filter3d(src.reshape((b * c,) + sp), ks)
    return out.reshape(src.shape)


def get_binary_kernel(window_size, dtype=torch.float, device=None) -> torch.Tensor:
    """The reference's one-hot window kernel (monai/networks/layers/simplelayers.py:430-438): ``prod(window) x 1 x window``, output channel i
    picks window position i.  The HIP path never evaluates it; ``MedianFilter.kernel`` keeps it for callers that read the attribute."""
    win = [int(w) for w in window_size]
    prod = int(np.prod(win))
    return torch.diag(torch.ones(prod, dtype=dtype, device=device)).view([prod, 1, *win])


def _box_window(kernel, spatial_dims: int):
    """the window of a custom ``kernel=`` when it is the full box identity (what get_binary_kernel builds), else NotImplementedError"""
    if not isinstance(kernel, torch.Tensor) or kernel.dim() != spatial_dims + 2 or kernel.shape[1] != 1:
        raise NotImplementedError("monai_amd.median_filter: a custom kernel that is not the one-hot box kernel is not on the HIP path")
    window = tuple(int(k) for k in kernel.shape[2:])
    prod = int(np.prod(window))
    k2 = kernel.detach().reshape(kernel.shape[0], -1)
    if kernel.shape[0] != prod or not torch.equal(k2, torch.eye(prod, dtype=k2.dtype, device=k2.device)):
        raise NotImplementedError("monai_amd.median_filter: a custom kernel that is not the one-hot box kernel is not on the HIP path")
    return window


@function_fallback("monai.networks.layers.simplelayers", "median_filter")
def median_filter(in_tensor: torch.Tensor, kernel_size=(3, 3, 3), spatial_dims: int = 3, kernel=None, **kwargs) -> torch.Tensor:
    """Median over a ``kernel_size`` box along the last ``spatial_dims`` axes with replicate padding (monai/networks/layers/simplelayers.py:441-498),
    as one exact selection kernel (``ops.median_filter``): no padded copy, no window-sized feature tensor.  Not on the HIP path: a custom ``kernel``
    other than the box identity, even sizes, extra arguments for the convolution, tensors that are not float32 device tensors, windows above 343."""
    if not isinstance(in_tensor, torch.Tensor):
        raise TypeError(f"Input type is not a torch.Tensor. Got {type(in_tensor)}")
    if kwargs:
        raise NotImplementedError(f"monai_amd.median_filter: convolution arguments {sorted(kwargs)} are not on the HIP path")
    window = ensure_tuple_rep(kernel_size, spatial_dims) if kernel is None else _box_window(kernel, spatial_dims)
    if any(int(k) != k or k < 1 or int(k) % 2 == 0 for k in window):
        raise NotImplementedError(f"monai_amd.median_filter: even (or non-positive) kernel sizes {tuple(window)} are not on the HIP path")
    data = in_tensor.as_tensor() if hasattr(in_tensor, "as_tensor") else in_tensor
    return ops.median_filter(data, [(int(k) - 1) // 2 for k in window], spatial_dims)


class MedianFilter(nn.Module):
    """``monai.networks.layers.MedianFilter`` (monai/networks/layers/simplelayers.py:501-539): the median over a box of ``radius`` (one value, or
    one per spatial axis) with replicate padding, ``number_of_passes`` times, on the exact selection kernel.  ``kernel`` -- the reference's one-hot
    tensor of ``prod(window)^2`` elements -- is built when it is first read; the forward pass does not use it."""

    def __init__(self, radius, spatial_dims: int = 3, device="cpu") -> None:
        super().__init__()
        self.spatial_dims = spatial_dims
        self.radius = ensure_tuple_rep(radius, spatial_dims)
        self.window = [1 + 2 * int(r) for r in self.radius]
        self._kernel_device, self._kernel = device, None

    @property
    def kernel(self) -> torch.Tensor:
        if self._kernel is None:
            self._kernel = get_binary_kernel(self.window, device=self._kernel_device)
        return self._kernel

    def forward(self, in_tensor: torch.Tensor, number_of_passes=1) -> torch.Tensor:
        if not isinstance(in_tensor, torch.Tensor):
            raise TypeError(f"Input type is not a torch.Tensor. Got {type(in_tensor)}")
        if number_of_passes < 1:
            return in_tensor
        data = in_tensor.as_tensor() if hasattr(in_tensor, "as_tensor") else in_tensor
        return ops.median_filter(data, [int(r) for r in self.radius], self.spatial_dims, passes=int(number_of_passes))


class GaussianFilter(nn.Module):
    def __init__(self, spatial_dims: int, sigma, truncated: float = 4.0, approx: str = "erf", requires_grad: bool = False) -> None:
        if isinstance(sigma, (Sequence, np.ndarray)) and not isinstance(sigma, str):
            if len(sigma) != spatial_dims:
                raise ValueError
            sig = list(sigma)
        elif isinstance(sigma, torch.Tensor) and sigma.ndim > 0:
            if len(sigma) != spatial_dims:
                raise ValueError
            sig = list(sigma)
        else:
            sig = [sigma for _ in range(spatial_dims)]
        super().__init__()
        if requires_grad:
            raise NotImplementedError("monai_amd.GaussianFilter: trainable sigma is not on the (inference) HIP path")
        self.sigma = [torch.nn.Parameter(torch.as_tensor(s, dtype=torch.float).detach().cpu(), requires_grad=False) for s in sig]
        self.truncated, self.approx = truncated, approx
        for idx, param in enumerate(self.sigma):
            self.register_parameter(f"kernel_sigma_{idx}", param)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        kernels = [gaussian_1d(s, truncated=self.truncated, approx=self.approx) for s in self.sigma]
        return separable_filtering(x=x, kernels=kernels)
