"""The conv + norm engine the network modules share (BasicUNet, UNet, DynUNet, SegResNet, UNETR / SwinUNETR): how a 3x3x3 convolution and the
normalisation behind it are dispatched.  A new kernel form is wired in HERE, once.

One `ConvEngine` per network holds what is derived from its parameters (packed weights, folded BatchNorm tables, ... -- rebuilt when a source
parameter changed, moved or got new storage) and the grow-only scratch (statistics records, the stride-2 kernel's workspace), and offers

  * `conv3`        one convolution step: configuration, statistics tiles and buffer, profiling span, launch -- stride 1 on the selected configuration,
                   stride 2 on the split-precision stride-2 kernel where `ops.conv3d_k3s2_selected`, the strided direct kernel otherwise;
  * `conv3_split`  the same convolution evaluated in two ranges of its input channels (it is linear in them);
  * `launch3`      the single stride-1 launch both are made of, for the structures that stay in the networks (UpCat's composite term, an
                   output-channel split, a residual join inside the convolution);
  * `norm_record`  the normalisation + activation that follows a raw tensor as the [N, C, 4] records {alpha, beta, slope, bound} its consumer applies on load.

What a network decides itself -- and hands over as an argument, never by who it is -- is whether its input's records carry magnitude bounds
(`bounded`), whether it wants the epilogue's statistics, and whether tiny channel counts go to the direct kernel."""

from __future__ import annotations

from typing import Optional

import torch

from .. import _prof, ops

__all__ = ["ConvEngine", "split_configs", "accumulates", "identity_records"]


def split_configs() -> tuple:
    """ids of the split-precision configurations (direct, 16-cout groups, in-plane Winograd): fp16 matrix cores, fp32-equivalent, inputs with magnitude bounds only"""
    return ops.conv3d_k3_h2_config(), ops.conv3d_k3_h2c_config(), ops.conv3d_k3_h2w_config()


def accumulates(cfg: int) -> bool:
    """does configuration `cfg` have an accumulating form (out += conv, statistics of the sum)?  The split-precision kernels do."""
    return cfg in split_configs()


def identity_records(t: torch.Tensor) -> torch.Tensor:
    """fresh identity records for a plain tensor that is about to be written (its producer -- add_act, a transposed convolution -- leaves the magnitude bounds in them)"""
    return ops.nrm_identity(torch.empty((t.shape[0], t.shape[1], 4), dtype=torch.float32, device=t.device))


def _kernel3(w: torch.Tensor) -> torch.Tensor:
    """a layer's weight as the 3x3x3 kernel the engine runs.  A 2-D layer's [O, I, kh, kw] is the one-plane kernel [O, I, 1, kh, kw]; a kernel extent of 1 along
    an axis is a 3-tap kernel whose outer taps are zero: with padding 1 the centre tap sits on the same sample (s * o) as the reference's padding-0 extent-1
    kernel.  Exact (the zero taps multiply the padding or nothing that counts); they cost matrix time, not accuracy."""
    if w.dim() == 4:
        w = w.unsqueeze(2)
    if tuple(w.shape[2:]) == (3, 3, 3):
        return w
    w3 = torch.zeros(w.shape[:2] + (3, 3, 3), dtype=w.dtype, device=w.device)
    w3[(slice(None), slice(None)) + tuple(slice(0, 3) if k == 3 else slice(1, 2) for k in w.shape[2:])] = w
    return w3


class ConvEngine:
    def __init__(self):
        self._derived: dict = {}    # slot -> (version key of the source parameters, what was built from them)
        self._scratch: dict = {}    # (what, device) -> grow-only fp32 buffer

    # ---- parameter-derived tensors -------------------------------------------------------------------
    def derived(self, slot, sources, build, *extra):
        """`build()` cached under `slot`; rebuilt when (data_ptr, _version, device) of a source parameter -- or `extra` -- changed"""
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in sources) + extra
        hit = self._derived.get(slot)
        if hit is None or hit[0] != key:
            hit = self._derived[slot] = (key, build())
        return hit[1]

    def conv3_pack(self, conv, cfg: int, cin: Optional[tuple] = None, cout: Optional[tuple] = None) -> torch.Tensor:
        """the layer's weights packed for configuration `cfg` (one slot per configuration and slice); cin / cout = (lo, hi): those input / output channels only"""
        def build():
            w = _kernel3(conv.weight)
            if cout is not None:
                w = w[cout[0]:cout[1]]
            if cin is not None:
                w = w[:, cin[0]:cin[1]].contiguous()
            return ops.conv3d_k3_pack(cfg, w)

        return self.derived((id(conv), "k3", cfg, cin, cout), [conv.weight], build)

    def conv3s2_pack(self, conv) -> torch.Tensor:
        """the stride-2 split-precision kernel's tap matrices of a [Cout, Cin, 3, 3, 3] weight"""
        return self.derived((id(conv), "s2"), [conv.weight], lambda: ops.conv3d_k3s2_pack(conv.weight))

    def conv1x1_h2_pack(self, conv) -> torch.Tensor:
        return self.derived((id(conv), "1x1"), [conv.weight], lambda: ops.conv1x1_h2_pack(conv.weight.view(conv.weight.shape[0], -1)))

    def upconv_pack(self, conv, dec, at: int):
        """UpCat without its up-sampled intermediate (csrc/kernels/upconv_h2.h): the composite of the transposed convolution `dec` and `conv`'s weights for the up
        channels (input channels `at` on) -> (the composite kernel's tap matrices, its bias table)"""
        def build():
            w4, table = ops.upconv_k4s2_weights(dec.weight, dec.bias, conv.weight[:, at:])
            return ops.upconv_k4s2_pack(w4), table

        return self.derived((id(conv), "upconv"), [conv.weight, dec.weight] + ([dec.bias] if dec.bias is not None else []), build)

    def linear_pack(self, weight: torch.Tensor) -> torch.Tensor:
        return self.derived((id(weight), "lin"), [weight], lambda: ops.linear_pack(weight.reshape(weight.shape[0], -1)))

    def scalar(self, param: torch.Tensor) -> float:
        """a one-element parameter (PReLU's slope) on the host: one device -> host read per parameter version, not per launch"""
        return self.derived((id(param), "scalar"), [param], lambda: float(param.detach().float().cpu()))

    def bn_fold(self, bn, slope: float) -> torch.Tensor:
        """Eval-mode BatchNorm + activation as the consumer-side table [C, 4] = {alpha = weight / sqrt(running_var + eps), beta = bias - running_mean * alpha, slope, 0}
        -- the x * alpha + beta form of ATen's CPU batch norm.  A parameter fold over C values, no pass over activations, no statistics -- and no magnitude bound
        (0: none given)."""
        if bn.running_mean is None or bn.running_var is None:
            raise NotImplementedError("monai_amd: BatchNorm without running statistics is not on the (inference) HIP path")

        def build():
            invstd = 1.0 / torch.sqrt(bn.running_var.float() + bn.eps)
            alpha = invstd * bn.weight.float() if bn.affine else invstd
            beta = (bn.bias.float() if bn.affine else 0.0) - bn.running_mean.float() * alpha
            return torch.stack([alpha, beta, torch.full_like(alpha, slope), torch.zeros_like(alpha)], dim=1).contiguous()

        return self.derived((id(bn), "bn"), [bn.running_mean, bn.running_var] + ([bn.weight, bn.bias] if bn.affine else []), build, slope)

    def act_records(self, slope: float, n: int, c: int, device) -> torch.Tensor:
        """[n, c, 4] records {1, 0, slope, 0}: the bare activation (no normalisation in front of it; no magnitude bound)"""
        return self.derived(("act", slope, n, c, str(device)), [],
                            lambda: torch.tensor([1.0, 0.0, slope, 0.0], dtype=torch.float32, device=device).repeat(n, c, 1).contiguous())

    # ---- scratch -------------------------------------------------------------------------------------
    def _buf(self, what: str, floats: int, device) -> torch.Tensor:
        """one buffer per purpose and device, grown to the largest request (the stride-2 kernel's workspace: the phase-split fp16 pieces of its input)"""
        buf = self._scratch.get((what, device))
        if buf is None or buf.numel() < floats:
            buf = self._scratch[(what, device)] = torch.empty(floats, dtype=torch.float32, device=device)
        return buf

    def stats_buf(self, floats: int, device) -> torch.Tensor:
        """the statistics records of the convolution in flight (two live sets at most: the one a convolution writes while its input's has already been finalised)"""
        return self._buf("stats", floats, device)

    # ---- convolutions --------------------------------------------------------------------------------
    def epilogue_stats(self, cfg: int, out):
        """(the engine's statistics buffer sized for the raw tensor `out`, tile count) of configuration `cfg`'s epilogue; (None, 0) where it has none"""
        n, cout, d, h, w = out.shape
        tiles = ops.conv3d_k3_stat_tiles(cfg, d, h, w)
        return (self.stats_buf(n * cout * tiles * 3, out.device), tiles) if tiles else (None, 0)

    def launch3(self, cfg: int, x, x_nrm, packed, bias, out, want_stats: bool = True, accumulate: bool = False, pool=None, stats=None):
        """one stride-1 launch of configuration `cfg` under its profiling span -> (statistics records or None, their tile count or 0).  `stats`: where the
        records go (default: the engine's buffer); accumulate: out += (the statistics are those of the sum); pool = (maxima, minima): the pooling epilogue."""
        n, cout, d, h, w = out.shape
        own, tiles = self.epilogue_stats(cfg, out) if want_stats else (None, 0)
        stats = (own if stats is None else stats) if tiles else None
        with _prof.span(f"conv3d_k3/cfg{cfg}", 2.0 * 27 * x.shape[1] * cout * d * h * w * n):
            if pool is not None:
                ops.conv3d_k3_pool(cfg, x, x_nrm, packed, bias, out, stats, *pool)
            else:
                ops.conv3d_k3(cfg, x, x_nrm, packed, bias, out, stats, accumulate=accumulate)
        return stats, tiles

    def conv3(self, conv, x, x_nrm, stride=1, out=None, *, bounded: bool, want_stats: bool = True, tiny_direct: bool = False, accumulate: bool = False, pool=None):
        """3x3x3 convolution (+ bias) of the (deferred) input `x` under its records `x_nrm` -> (raw output, statistics records or None, tiles).
        stride: an int (isotropic) or (sz, sy, sx); out: where the raw output goes (default: a new tensor).
        bounded: every record of `x_nrm` carries a magnitude bound (written by the finalize kernels, or folded into identity records by a raw producer) -- what
        the split-precision kernels scale their input by; folded BatchNorm records and interpolated tensors have none.
        want_stats: take the statistics of the output from the epilogue where the kernel has one (tiles 0 otherwise: `norm_record` then makes its own pass).
        tiny_direct: at most 8 channels on both sides (a 5-class top level) go to the direct kernel -- the matrix tiles would pad them to 32, it runs at the
        channels' true width.  accumulate / pool: see `launch3` (stride 1 only)."""
        n, cin, d, h, w = x.shape
        cout = conv.weight.shape[0]
        st = (int(stride),) * 3 if isinstance(stride, int) else tuple(stride)
        sp = tuple((v - 1) // s + 1 for v, s in zip((d, h, w), st))
        if out is None:
            out = torch.empty((n, cout) + sp, dtype=torch.float32, device=x.device)
        if st == (1, 1, 1) and not (tiny_direct and cin <= 8 and cout <= 8):
            cfg = ops.conv3d_k3_select(cin, cout, d, h, w, bounded=bounded)
            return (out,) + self.launch3(cfg, x, x_nrm, self.conv3_pack(conv, cfg), conv.bias, out, want_stats, accumulate, pool)
        if tuple(conv.weight.shape[2:]) == (3, 3, 3) and ops.conv3d_k3s2_selected(cin, cout, d, h, w, st, bounded=bounded):
            # the down-sampling convolution on the fp16 matrix cores (csrc/kernels/conv3d_s2_h2.h); it always leaves the statistics of its output
            tiles = ops.conv3d_k3s2_stat_tiles(d, h, w)
            stats = self.stats_buf(n * cout * tiles * 3, x.device)
            with _prof.span("conv3d_k3s2", 2.0 * 27 * cin * cout * sp[0] * sp[1] * sp[2] * n):
                fused = ops.conv3d_k3s2_fused(cin, cout, d * h * w)          # conversion inside the GEMM's staging, or a phase-split pass into the workspace first
                ws = None if fused else self._buf("s2 workspace", ops.conv3d_k3s2_workspace_floats(n, cin, d, h, w), x.device)
                ops.conv3d_k3s2(x, x_nrm, self.conv3s2_pack(conv), conv.bias, out, stats, ws, fused)
            return out, stats, (tiles if want_stats else 0)
        # other strides, an unbounded input, or so few channels that the matrix tiles would mostly pad: the direct kernel at the true width, no statistics
        if isinstance(stride, int):
            ops.conv3d_k3_strided(x, x_nrm, self.conv3_pack(conv, 0), conv.bias, out, stride)
        else:
            ops.conv3d_k3_strided3(x, x_nrm, self.conv3_pack(conv, 0), conv.bias, out, st)
        return out, None, 0

    def conv3_split(self, conv, cfg: int, x, x_nrm, at: int, out, bias_on: Optional[str]):
        """conv(x) = conv[:, :at](x[:, :at]) + conv[:, at:](x[:, at:]) on a configuration with an accumulating form: the first range written by the plain form, the
        second added onto it by the accumulating form, which leaves the statistics of the sum -> (statistics records, tiles).  What it buys: more input channels
        than the split-precision kernel keeps records for (a 512-channel concat), or halves that a faster kernel takes where the whole is not its shape.
        bias_on: "first" | "second" | None -- which launch adds the bias; it decides the rounding of the sum, so callers keep their placement."""
        cin, b = x.shape[1], conv.bias
        self.launch3(cfg, x[:, :at], x_nrm[:, :at], self.conv3_pack(conv, cfg, cin=(0, at)), b if bias_on == "first" else None, out, want_stats=False)
        return self.launch3(cfg, x[:, at:], x_nrm[:, at:], self.conv3_pack(conv, cfg, cin=(at, cin)), b if bias_on == "second" else None, out, accumulate=True)

    # ---- normalisation records -----------------------------------------------------------------------
    def norm_record(self, raw, stats, tiles: int, norm, slope: float, groups: Optional[int] = None, out=None):
        """{alpha, beta, slope, bound} of `norm` (+ the activation of `slope`) for the raw tensor `raw` -> [N, C, 4] records (written into `out` when given).
        stats / tiles: the producing kernel's statistics records, or tiles 0: one reduction pass over `raw` here.  norm: the InstanceNorm / GroupNorm module (its
        weight, bias, eps), or None = no affine map, eps 1e-5.  groups: None = per channel (`instnorm_finalize`), else `groupnorm_finalize` merging C / groups channels."""
        n, c = raw.shape[:2]
        if not tiles:
            tiles = ops.instnorm_stat_tiles(*raw.shape[2:])
            stats = self.stats_buf(n * c * tiles * 3, raw.device)
            ops.instnorm_stats(raw, stats)
        if out is None:
            out = torch.empty((n, c, 4), dtype=torch.float32, device=raw.device)
        gamma, beta, eps = (None, None, 1e-5) if norm is None else (norm.weight, norm.bias, norm.eps)
        if groups is None:
            return ops.instnorm_finalize(stats, tiles, n, c, gamma, beta, eps, slope, out)
        return ops.groupnorm_finalize(stats, tiles, n, c, groups, gamma, beta, eps, slope, out)

