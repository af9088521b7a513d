"""``BilateralFilter`` of monai/networks/layers/filtering.py:23-63 over the exact bilateral-filter kernels (csrc/kernels/bilateral.h).

The reference's ``PHLFilter`` and the permutohedral approximation of ``BilateralFilter`` (``fast_approx=True``, its default) are not built: its two
implementations of the lattice do not agree with each other and the splat is built on float atomics.  The trainable bilateral layers are training code and
are not here either."""

from __future__ import annotations

import torch

from ... import _C

__all__ = ["BilateralFilter"]


class BilateralFilter(torch.autograd.Function):
    """Blurs the input tensor spatially whilst preserving edges: (B, C, 1 to 3 spatial axes), the colour distance joint over the channels.

    ``BilateralFilter.apply(input, spatial_sigma=5, color_sigma=0.5, fast_approx=True)`` -- the reference's signature and defaults.  Only the exact filter
    is built, so ``fast_approx=False`` has to be passed; the default raises ``RuntimeError`` and says so.  ``backward`` is the reference's: the same
    filter applied to ``grad_output`` with the gradient's own values as colours (its definition, not the derivative).  Unlike the reference, ``forward``
    does not synchronise the device."""

    @staticmethod
    def forward(ctx, input, spatial_sigma=5, color_sigma=0.5, fast_approx=True):
        ctx.ss = spatial_sigma
        ctx.cs = color_sigma
        ctx.fa = fast_approx
        return _C.bilateral_filter(input, spatial_sigma, color_sigma, fast_approx)

    @staticmethod
    def backward(ctx, grad_output):
        spatial_sigma, color_sigma, fast_approx = ctx.ss, ctx.cs, ctx.fa
        grad_input = _C.bilateral_filter(grad_output, spatial_sigma, color_sigma, fast_approx)
        return grad_input, None, None, None
