"""``sliding_window_inference`` on the MI355X kernels -- drop-in for monai/inferers/utils.py:42-321.

Same signature and results as the reference (bit-identical blend for the same window logits), different
schedule.  The reference runs a Python loop that, per window batch, multiplies the predictor output by the
importance map and read-modify-writes it into the output volume and a count map (5x the algorithmic HBM
traffic).  Here:

  1. windows are gathered by ``mh_window_extract_f32`` straight from the volume into a batch buffer;
  2. the predictor writes its logits into ONE buffer holding every window of the image
     (``[num_win, K, roi]`` -- 17.7 GB for 512^3 / 96^3 / overlap 0.5 / 5 classes; HBM is 288 GB);
  3. ``mh_sw_blend_f32`` produces every output voxel in a single gather pass that walks the covering windows
     in ascending window index: ``acc += logit*w; cnt += w; out = acc/cnt`` -- exactly the floating-point
     operations, in exactly the order, of the reference's ``*=``, ``+=``, ``/=``; the count map is never stored.

With window sharding enabled (monai_amd.parallel) each rank runs the predictor on a contiguous range of
windows and one RCCL all-gather of the logits precedes the (replicated, deterministic) blend.
"""

from __future__ import annotations

import itertools
import math
import os
import threading
import warnings
from collections.abc import Callable, Mapping, Sequence
from typing import Any, NamedTuple

import torch
import torch.nn.functional as F

from .. import _lib, _prof, ops, parallel
from .._fallback import function_fallback
from ..data.utils import compute_importance_map, get_valid_patch_size, importance_map_factors, window_starts
from ..utils.misc import ensure_tuple, ensure_tuple_rep, fall_back_tuple, look_up_option

__all__ = ["sliding_window_inference", "sliding_window_argmax"]

_PAD_MODES = ("constant", "reflect", "replicate", "circular")
_NEAREST = "nearest-exact"


def _get_scan_interval(image_size, roi_size, num_spatial_dims: int, overlap) -> tuple:
    """monai/inferers/utils.py:363-384: ``int(roi * (1 - overlap))``, at least 1; the roi itself when it spans the image."""
    if len(image_size) != num_spatial_dims:
        raise ValueError(f"len(image_size) {len(image_size)} different from spatial dims {num_spatial_dims}.")
    if len(roi_size) != num_spatial_dims:
        raise ValueError(f"len(roi_size) {len(roi_size)} different from spatial dims {num_spatial_dims}.")
    steps = []
    for size, roi, o in zip(image_size, roi_size, overlap):
        if roi == size:
            steps.append(int(roi))
        else:
            step = int(roi * (1 - o))
            steps.append(step if step > 0 else 1)
    return tuple(steps)


def _flatten_struct(seg_out):
    """tensor | tuple | dict -> (sorted keys or None, tuple of tensors)  (utils.py:387-398)"""
    if isinstance(seg_out, torch.Tensor):
        return None, (seg_out,)
    if isinstance(seg_out, Mapping):
        keys = sorted(seg_out.keys())
        return keys, tuple(seg_out[k] for k in keys)
    return None, ensure_tuple(seg_out)


def _pack_struct(seg_out, dict_keys=None):
    if dict_keys is not None:
        return dict(zip(dict_keys, seg_out))
    if isinstance(seg_out, (list, tuple)) and len(seg_out) == 1:
        return seg_out[0]
    return ensure_tuple(seg_out)


def _to3(values, fill):
    """left-pad a 1/2/3-element spatial tuple to 3 entries"""
    values = tuple(values)
    return (fill,) * (3 - len(values)) + values


def _auto_batch(predictor, roi3, num_win: int, sw_batch_size: int, device, world: int = 1, sharded: bool = False) -> int:
    """Windows per predictor call.  A generic predictor gets exactly the user's ``sw_batch_size``.  The fused engines
    size the batch for 288 GB of HBM instead (results do not depend on the batch: InstanceNorm is per sample): more
    windows per launch fill the 256 CUs at the deep U-Net levels, and a power-of-two count keeps the workgroup grids of
    the large layers whole multiples of the CU count -- measured on the BASELINE workload (profiles/): 25 windows per
    launch 1.85 s, 32: 1.75 s, 64: 1.73 s, 128: 1.72 s.  Default 64 on one GPU.  When the windows are sharded over `world`
    GPUs the rounds follow parallel.WindowShard.schedule (main rounds of world x nb windows, shorter tail rounds): nb is the value in [32, 64] that
    gives the busiest rank the fewest windows, ties to the larger.
    `num_win` is the TOTAL number of windows.  Override with MONAI_AMD_SW_BATCH; MONAI_AMD_STRICT_SW_BATCH=1 keeps the user's value."""
    if not hasattr(predictor, "forward_into") or os.environ.get("MONAI_AMD_STRICT_SW_BATCH") == "1":
        return max(1, int(sw_batch_size))
    per_rank = max(-(-num_win // world), 1)
    env = os.environ.get("MONAI_AMD_SW_BATCH")
    if env:
        return max(1, min(int(env), per_rank))
    cap = 64
    if device.type == "cuda":
        free, _ = torch.cuda.mem_get_info(device)
        per_win = 6.0 * 4 * max(getattr(predictor, "features", (32,))[0], 1) * roi3[0] * roi3[1] * roi3[2]
        fit = int(max(1, (0.35 * free) // max(per_win, 1)))
        while cap > 1 and cap > fit:
            cap //= 2
    cap = max(cap, int(sw_batch_size)) if cap >= sw_batch_size else cap
    cap = max(1, min(cap, per_rank))
    if (world > 1 or sharded) and cap > 1:
        # the busiest rank (rank 0: a full slot in every round of parallel.WindowShard.schedule) sets the step time: the nb in [cap / 2, cap] that gives it the fewest
        # windows, a launch counted as at least 7 windows (below that the large layers no longer fill 256 CUs), ties to the larger nb
        probe = parallel.partition(num_win, world, 0, force=sharded)
        best, best_cost = cap, None
        for nb in range(cap, max(cap // 2, 1) - 1, -1):
            cost = sum(max(n, min(7, nb)) for _, n in probe.schedule(nb))
            if best_cost is None or cost < best_cost:
                best, best_cost = nb, cost
        cap = best
    return cap


class _Geometry(NamedTuple):
    """The window geometry of one (sub-)volume, computed once per volume: the whole volume, or each slab's sub-volume (`_slabwise`)."""

    spatial: tuple       # the volume's own spatial size
    roi_size: tuple
    image_size: tuple    # after the padding up to the roi
    pad_size: tuple      # in F.pad's order (last dim first); all zero when the volume is at least the roi
    starts: list         # per axis, the window starts
    num_win: int
    roi3: tuple          # roi_size / image_size / starts as the kernels' 3-D view
    img3: tuple
    grid3: list


def _geometry(spatial, roi_size, overlap) -> _Geometry:
    nsd = len(spatial)
    # pad when the image is smaller than the roi (utils.py:163-170), centred, last dim first
    image_size = tuple(max(spatial[i], roi_size[i]) for i in range(nsd))
    pad_size = []
    for k in range(nsd - 1, -1, -1):
        diff = max(roi_size[k] - spatial[k], 0)
        pad_size.extend([diff // 2, diff - diff // 2])
    starts = window_starts(image_size, roi_size, _get_scan_interval(image_size, roi_size, nsd, overlap))
    return _Geometry(tuple(spatial), tuple(roi_size), image_size, tuple(pad_size), starts, math.prod(len(s) for s in starts), _to3(roi_size, 1),
                     _to3(image_size, 1), [[0]] * (3 - nsd) + [list(s) for s in starts])


class _Call(NamedTuple):
    """What one public call asks of every (sub-)volume it runs: its arguments after the checks, with the private keyword taken out of `kwargs`."""

    predictor: Callable[..., Any]
    args: tuple
    kwargs: dict
    process_fn: Callable | None
    with_coord: bool
    sw_batch_size: int
    progress: bool
    argmax_dtype: Any    # fused AsDiscrete(argmax=True) epilogue (sliding_window_argmax below): the labels' dtype, else None
    fused: bool          # the predictor writes its logits itself (`forward_into` / `forward_into_windows`) and takes nothing but the windows
    imp: torch.Tensor    # importance map of the roi on the host, and the cache key of a map this module evaluated itself (a caller's roi_weight_map is uploaded per call)
    imp_key: tuple | None
    mode: str
    sigma_scale: Any
    out_device: torch.device


@function_fallback("monai.inferers.utils", "sliding_window_inference")
def sliding_window_inference(
    inputs: torch.Tensor,
    roi_size: Sequence[int] | int,
    sw_batch_size: int,
    predictor: Callable[..., Any],
    overlap: Sequence[float] | float = 0.25,
    mode: str = "constant",
    sigma_scale: Sequence[float] | float = 0.125,
    padding_mode: str = "constant",
    cval: float = 0.0,
    sw_device=None,
    device=None,
    progress: bool = False,
    roi_weight_map: torch.Tensor | None = None,
    process_fn: Callable | None = None,
    buffer_steps: int | None = None,
    buffer_dim: int = -1,
    with_coord: bool = False,
    *args: Any,
    **kwargs: Any,
):
    """See the reference docstring (monai/inferers/utils.py:63-141) for the argument semantics; they are kept.

    ``buffer_steps`` / ``buffer_dim`` (utils.py:239-253, 276-284, 324-348): the reference's buffered schedule sums in ANOTHER ORDER than its plain path
    (windows sorted by their start along ``buffer_dim``, slabs of ``buffer_steps`` distinct starts accumulated from zero and then added to the output), so
    its result differs from the plain one by roundings (tests/golden/buffered.npz: up to 26 000 voxels of a small volume, <= 6e-7).  The schedule itself --
    a memory-saving device -- is not reproduced (the logits of all windows sit in HBM), its ARITHMETIC is: with ``buffer_steps`` the blend runs in the
    buffered order (``mh_sw_blend_buffered_f32``) and returns the bits of the reference's buffered run.  With ``process_fn`` / ``with_coord`` / tuple or dict
    outputs the predictor is also CALLED as the reference calls it there (windows in the sorted order, batches that end at the slab boundaries, the sorted
    slices as coordinates; only the FIRST output is blended, as utils.py:244 does; the count map is the weight map of the batch at the first flush):
    ``_buffered_batches``.  Multi-resolution outputs with ``buffer_steps`` fail in the reference too and are refused.
    Other differences, all result-neutral: when the logits of all windows do not fit in HBM the volume is processed slab by slab along its first spatial
    axis with bit-identical results, see ``_slabwise``; ``sw_device`` must be a ROCm device (a CPU volume is moved to it once; half / bfloat16 volumes are widened to fp32 and the result
    returned in the caller's dtype).  A predictor with ``forward_into`` (the conv engines) is given up to 64 windows per launch
    instead of ``sw_batch_size`` -- result-neutral, but it changes peak memory; MONAI_AMD_STRICT_SW_BATCH=1 keeps the caller's value
    and MONAI_AMD_SW_BATCH=n sets it.  ``process_fn`` (utils.py:232-234) is honoured with
    the reference's semantics: each batch is multiplied by the weight map it returns, the count map uses the first batch's.

    One call makes one pass: check and normalise the arguments, plan the windows (``_geometry``), run (``_run_volume``; when the logits do not fit: the buffered
    order falls back to the plain one, the whole volume to ``_slabwise``), give the result the caller's dtype and tensor type.
    """
    num_spatial_dims = inputs.dim() - 2
    argmax_dtype = kwargs.pop("_monai_amd_argmax", None)      # the one private keyword (sliding_window_argmax, inferers/inferer.py); what is left is the predictor's own
    buffer = None                                             # (axis, steps) of the reference's buffered schedule
    if buffer_steps is not None and buffer_steps > 0:
        if buffer_dim < -num_spatial_dims or buffer_dim > num_spatial_dims:
            raise ValueError(f"buffer_dim must be in [{-num_spatial_dims}, {num_spatial_dims}], got {buffer_dim}.")
        if buffer_dim < 0:
            buffer_dim += num_spatial_dims
        if buffer_dim >= num_spatial_dims:
            raise NotImplementedError("monai_amd: buffer_steps with buffer_dim == the number of spatial dims is not on the HIP path")
        if argmax_dtype is not None:       # rejected BEFORE any window is predicted (a fall-through would otherwise predict them all twice)
            raise NotImplementedError("monai_amd: the fused argmax epilogue with buffer_steps is not on the HIP path (blend in the buffered order, then AsDiscrete)")
        buffer = (buffer_dim, int(buffer_steps))
    overlap = ensure_tuple_rep(overlap, num_spatial_dims)
    for o in overlap:
        if o < 0 or o >= 1:
            raise ValueError(f"overlap must be >= 0 and < 1, got {overlap}.")
    if num_spatial_dims < 1 or num_spatial_dims > 3:
        raise NotImplementedError(f"monai_amd: sliding windows over {num_spatial_dims} spatial dims are not supported (1-3 are)")
    meta_src = inputs if (type(inputs) is not torch.Tensor and hasattr(inputs, "as_tensor")) else None
    if meta_src is not None:
        inputs = inputs.as_tensor()
    if torch.is_grad_enabled() and inputs.requires_grad:
        # the reference's result carries the autograd graph of the windows (tests/inferers/test_sliding_window_inference.py:124-139);
        # the kernels do not record one: such a call belongs to the reference path
        raise NotImplementedError("monai_amd: sliding_window_inference of an input that requires grad (autograd through the blend) is not on the HIP path")
    # drop-in input handling (utils.py:146-153 take any float dtype and any inputs/sw_device pair): half / bfloat16 volumes are
    # widened to fp32 for the kernels and the result is returned in the caller's dtype; a CPU volume with a ROCm `sw_device` is
    # moved to HBM once (the reference moves it window by window) and the result goes back to `device` or the inputs' device
    out_device = torch.device(device) if device is not None else inputs.device
    narrow = inputs.dtype if inputs.dtype in (torch.float16, torch.bfloat16) else None
    host_in = (not inputs.is_cuda) and sw_device is not None and torch.device(sw_device).type == "cuda"
    if narrow is not None or host_in:
        inputs = inputs.to(device=torch.device(sw_device) if host_in else inputs.device, dtype=torch.float32)
    _lib.require_device(inputs)
    if sw_device is not None and torch.device(sw_device).type != inputs.device.type:
        raise RuntimeError("monai_amd: sw_device must be the ROCm device of the inputs (windows are gathered in HBM)")

    roi_size = fall_back_tuple(roi_size, inputs.shape[2:])
    geo = _geometry(tuple(inputs.shape[2:]), roi_size, overlap)
    if any(geo.pad_size):
        inputs = F.pad(inputs, pad=list(geo.pad_size), mode=look_up_option(padding_mode, _PAD_MODES, "padding_mode"), value=cval)
    inputs = inputs.contiguous()

    # importance map, always evaluated on the host in fp32 (bit-identical to the reference's CPU map)
    valid_patch_size = get_valid_patch_size(geo.image_size, roi_size)
    imp, imp_key = roi_weight_map, None
    if valid_patch_size != tuple(roi_size) or roi_weight_map is None:
        try:
            imp, imp_key = _host_importance_map(valid_patch_size, mode, sigma_scale, inputs.dtype)
        except Exception as e:  # same wrapping as the reference (utils.py:205-209)
            raise RuntimeError(
                f"patch size {valid_patch_size}, mode={mode}, sigma_scale={sigma_scale}, device={device}\n"
                "Seems to be OOM. Please try smaller patch size or mode='constant' instead of mode='gaussian'."
            ) from e
    imp = imp.to(dtype=inputs.dtype)
    while imp.dim() > num_spatial_dims:
        imp = imp[0]

    fused = (hasattr(predictor, "forward_into") and hasattr(predictor, "out_channels") and getattr(predictor, "window_sized_output", True)
             and not with_coord and not args and not kwargs and process_fn is None)
    call = _Call(predictor, args, kwargs, process_fn, with_coord, sw_batch_size, progress, argmax_dtype, fused, imp, imp_key, mode, sigma_scale, out_device)

    def finish(out):      # the caller's dtype and tensor type
        keys, parts = _flatten_struct(out)
        if narrow is not None:
            parts = [t.to(narrow) if t.is_floating_point() else t for t in parts]
        if meta_src is not None:
            parts = [_restore_meta(t, meta_src) for t in parts]
        return _pack_struct(parts, keys)

    if buffer is not None:
        # `buffer_steps` is the reference's MEMORY-SAVING option: the callers who pass it are the ones with large volumes.  The buffered summation order
        # needs the logits of all windows resident; when they do not fit, the volume goes through the plain order slab by slab (bit-identical to the
        # reference's plain run, which differs from its buffered run by roundings <= 1e-6 -- tests/golden/buffered.npz) instead of failing.
        try:
            return finish(_run_volume(inputs, geo, call, buffer))
        except _LogitsDoNotFit as e:
            if process_fn is not None or with_coord:      # no slab-wise form exists for these (their semantics are tied to the whole volume)
                raise
            reason = str(e).split(" (")[0]
        warnings.warn(f"{reason}: buffer_steps={buffer_steps} is served in the plain summation order, slab by slab "
                      "(equal to the reference's unbuffered result; its buffered result differs from that by roundings)")
    try:
        return finish(_run_volume(inputs, geo, call, None))
    except _LogitsDoNotFit as e:      # leave the handler before retrying: the traceback keeps the failed call's buffers alive
        # all-window logits that do not fit in HBM: slab by slab along the first spatial axis (see _slabwise)
        if with_coord or process_fn is not None or any(geo.pad_size) or len(geo.starts[0]) < 2:
            raise
        need, budget = e.need, (0.9 * e.budget if _logits_budget(inputs.device) is None else e.budget)

    def sub_volume(x):
        return _run_volume(x.contiguous(), _geometry(tuple(x.shape[2:]), roi_size, overlap), call, None)

    return finish(_slabwise(inputs, roi_size, geo.starts[0], need, budget, sub_volume))


def _channels(store) -> int:
    return store.k if isinstance(store, ops.LogitsMosaic) else int(store.shape[1])


class _WindowLogits:
    """The logits of every window of an image and what is known of the predictor's outputs.  `open` allocates them, once: from `out_channels` before the first
    predictor call where the predictor has it (the fit decision is then taken before a predictor or `process_fn` has seen a batch: neither may see one twice),
    else from the first prediction.  `predict` fills the rows of one batch of windows."""

    def __init__(self, call: _Call, geo: _Geometry, shard, nb: int, buffer, first_only: bool, dtype, dev):
        self.call, self.geo, self.shard, self.nb, self.buffer, self.first_only, self.dtype, self.dev = call, geo, shard, nb, buffer, first_only, dtype, dev
        self.stores = None        # per output: window-major rows [num_win_padded, K, *seg3] (`_alloc_logits`), or the mosaic layout (`_alloc_mosaic`)
        self.seg_shapes = None    # per output: spatial shape of one window's prediction (native dims)
        self.zscales = None       # per output: None at the windows' resolution, else prediction size / roi per axis
        self.dict_keys = None
        self.proc_weights = None  # process_fn: per output, the weight map behind the count map (the caller takes it from the first batch / the first flush)
        self.imp_dev = call.imp.to(dev) if call.process_fn is not None else None

    def open(self, channels, seg_shapes) -> None:
        c, geo = self.call, self.geo
        self.stores = []
        for k, sh in zip(channels, seg_shapes):
            # fused on one GPU in the plain order: the mosaic layout when the path allows it (the network's last kernel writes it directly)
            mosaic = _alloc_mosaic(c.predictor, self.shard, c.argmax_dtype, k, geo.grid3, geo.roi3, self.dtype, self.dev) if c.fused and self.buffer is None else None
            self.stores.append(mosaic if mosaic is not None else _alloc_logits(self.shard, self.nb, k, _to3(sh, 1), self.dtype, self.dev))
        self.seg_shapes = [tuple(sh) for sh in seg_shapes]
        self.zscales = [None if sh == geo.roi_size else [o / float(i) for o, i in zip(sh, geo.roi_size)] for sh in self.seg_shapes]

    def predict(self, win_data: torch.Tensor, coords, runs) -> list:
        """Call the predictor on `win_data` (with `coords` under with_coord), then `process_fn`; write the (weighted) predictions to the rows `runs` = [(first row,
        count)] of every output, consecutive batch elements to consecutive runs.  -> per output the weight map `process_fn` returned, [] without one."""
        c = self.call
        seg_out = c.predictor(win_data, *(() if coords is None else (coords,)), *c.args, **c.kwargs)
        self.dict_keys, segs = _flatten_struct(seg_out)
        w = None
        if c.process_fn is not None:     # utils.py:232-238: the callback may edit the predictions and the weight map
            segs, w = c.process_fn(segs, win_data, self.imp_dev)
            segs = tuple(segs) if isinstance(segs, (list, tuple)) else (segs,)
            if w.dim() == len(self.geo.roi_size):
                w = w[None, None]
            w = w.to(dtype=self.dtype, device=self.dev)
        if self.first_only:              # the reference's buffered schedule keeps the first output only (utils.py:244)
            self.dict_keys, segs = self.dict_keys and self.dict_keys[:1], segs[:1]
        if self.buffer is not None and (len(segs) != 1 or tuple(segs[0].shape[2:]) != self.geo.roi_size):
            raise NotImplementedError("monai_amd: buffer_steps with several / multi-resolution predictor outputs is not on the HIP path (the reference fails there too)")
        if self.stores is None:
            self.open([int(s.shape[1]) for s in segs], [s.shape[2:] for s in segs])
        weights = []
        for s, store, sh, z in zip(segs, self.stores, self.seg_shapes, self.zscales):
            if int(s.shape[1]) != _channels(store):
                raise RuntimeError(f"monai_amd: the predictor returned {int(s.shape[1])} channels, the logits were sized for {_channels(store)} (its `out_channels`, or its first batch)")
            if s.dtype != self.dtype and s.is_floating_point():
                # a predictor under torch.autocast returns half precision; the reference weights it in that precision and
                # accumulates in compute_dtype (utils.py:286-288) -- here it is widened first (never less precise)
                s = s.to(self.dtype)
            _lib.require_device(s)
            if w is not None:
                if z is not None:        # cumulative nearest resampling, as utils.py:260-263
                    w = F.interpolate(w, sh, mode=_NEAREST)
                if not self.first_only and (w.shape[0] != 1 or w.shape[1] != 1):
                    raise RuntimeError("monai_amd: process_fn must return a weight map broadcastable over batch and channels "
                                       f"(got {tuple(w.shape)}; the reference's count map needs [1, 1, *spatial])")
                weights.append(w)
            k = 0
            for r0, n in runs:
                dst = store[r0 : r0 + n]
                src = s[k : k + n].reshape(dst.shape)
                if w is None:
                    dst.copy_(src)
                else:                    # `seg *= w_t`
                    torch.mul(src, (w if w.shape[0] == 1 else w[k : k + n]).reshape((-1, w.shape[1]) + tuple(dst.shape[2:])), out=dst)
                k += n
        return weights

    def count_from(self, weights) -> None:
        """the reference builds its count map once, from the weight map current then (utils.py:264-275)"""
        self.proc_weights = [w[0, 0].reshape(_to3(sh, 1)).contiguous().clone() for w, sh in zip(weights, self.seg_shapes)]


def _run_volume(inputs: torch.Tensor, geo: _Geometry, c: _Call, buffer):
    """Every window of the (padded, contiguous) volume `inputs` through the predictor into the all-window logits, one blend per image and output, the padding
    cropped (utils.py:300-313), the result on `c.out_device`: the packed outputs.  `buffer`: (axis, steps) for the reference's buffered summation order, else None.
    Raises `_LogitsDoNotFit` -- before the predictor is called wherever its `out_channels` is known."""
    num_spatial_dims, roi_size, roi3, grid3, num_win = len(geo.roi_size), geo.roi_size, geo.roi3, geo.grid3, geo.num_win
    batch_size, in_ch = inputs.shape[:2]
    dtype, dev = inputs.dtype, inputs.device

    # windows owned by this rank: all of them, or (window sharding on) its slot of every round -- monai_amd/parallel.py
    shard = parallel.window_shard(num_win)
    nb = _auto_batch(c.predictor, roi3, num_win, c.sw_batch_size, dev, world=shard.world, sharded=shard.sharded)
    nb = shard.agree_batch(nb, dev)
    my_rounds = shard.rounds(nb)
    # buffer_steps with a callback in the loop: the predictor sees the reference's buffered batch schedule (sorted windows, batches cut at the slab ends)
    buffered_calls = buffer is not None and not c.fused and (c.process_fn is not None or c.with_coord or not shard.sharded)
    if buffered_calls and shard.sharded:
        raise NotImplementedError("monai_amd: buffer_steps with process_fn / with_coord under window sharding is not on the HIP path")
    win_buf = torch.empty((int(c.sw_batch_size) if buffered_calls else nb, in_ch) + roi3, dtype=dtype, device=dev)
    windows_nd = [tuple(slice(s, s + r) for s, r in zip(w, roi_size)) for w in itertools.product(*geo.starts)] if c.with_coord else None

    def predict(b, n, runs):      # the first `n` windows of win_buf, which hold the rows `runs` of image `b`
        coords = [[slice(b, b + 1), slice(None), *windows_nd[r]] for r0, cnt in runs for r in range(r0, r0 + cnt)] if c.with_coord else None
        return logits.predict(win_buf[:n].reshape((n, in_ch) + roi_size), coords, runs)

    logits = _WindowLogits(c, geo, shard, nb, buffer, buffered_calls, dtype, dev)
    if hasattr(c.predictor, "out_channels") and (c.fused or buffered_calls):
        # sized from the engine's out_channels, not from a first prediction: a rank whose slot of the first round is empty allocates too
        logits.open([int(c.predictor.out_channels)], [roi_size])
    outputs = None     # per output: [B, K, *out_img3]
    weights = None     # per output: importance map resampled to the prediction size (device)
    for b in range(batch_size):
        vol3 = inputs[b].reshape((in_ch,) + geo.img3)
        steps = list(enumerate(my_rounds))
        if c.progress:
            try:
                from tqdm import tqdm

                steps = tqdm(steps)
            except ImportError:
                pass
        pending = []
        if buffered_calls:
            steps = []            # the windows of this image are predicted here, in the reference's buffered order; the blend below reads their rows
            first_flush = _buffered_batches(vol3, geo, int(c.sw_batch_size), buffer, win_buf, lambda n, runs: predict(b, n, runs))
            if b == 0 and first_flush:
                logits.count_from(first_flush)
        for q, (w0, n) in steps:
            if n > 0:
                ops.window_extract(vol3, grid3, w0, n, roi3, win_buf[:n])
            if n > 0 and c.fused:
                with _prof.span("sw_predictor"):
                    if isinstance(logits.stores[0], ops.LogitsMosaic):     # the network's last kernel writes the windows straight into the mosaic layout
                        c.predictor.forward_into_windows(win_buf[:n], logits.stores[0], w0)
                    else:
                        c.predictor.forward_into(win_buf[:n], logits.stores[0][w0 : w0 + n])
            elif n > 0:
                first_batch = predict(b, n, [(w0, n)])
                if first_batch and logits.proc_weights is None:
                    logits.count_from(first_batch)
            if shard.sharded:
                if logits.stores is None:
                    raise RuntimeError("monai_amd: a rank without windows in the first round cannot size the logits buffer "
                                       "(fewer windows than ranks x windows per launch: lower sw_batch_size)")
                # this round's rows travel while the next round computes
                pending += [shard.gather_round(lg, q, nb) for lg in logits.stores]

        if logits.stores is None:
            raise RuntimeError("monai_amd: no windows were processed")
        with _prof.span("sw_gather_wait"):         # what the compute stream still has to wait for after its last round
            for work in pending:
                work.wait()

        if weights is None:  # importance map per output resolution (the reference resamples cumulatively, utils.py:260-263)
            weights, w_t = [], c.imp[None, None]
            for sh, z in zip(logits.seg_shapes, logits.zscales):
                if z is not None:
                    w_t = F.interpolate(w_t, sh, mode=_NEAREST)
                weights.append(_on_device(w_t[0, 0].reshape(_to3(sh, 1)).contiguous(), dev, cache_key=None if c.imp_key is None else c.imp_key + (tuple(sh),)))
            outputs = []
            for lg, z in zip(logits.stores, logits.zscales):
                osz = [int(i * zz) for i, zz in zip(geo.image_size, z)] if z else list(geo.image_size)
                # with the fused argmax only the label map is ever written: [B, 1, ...]
                k_out, dtype_out = (1, c.argmax_dtype) if c.argmax_dtype is not None else (_channels(lg), dtype)
                outputs.append(torch.empty((batch_size, k_out) + _to3(osz, 1), dtype=dtype_out, device=dev))
        for ss, (lg, z) in enumerate(zip(logits.stores, logits.zscales)):
            g = grid3 if z is None else [[0]] * (3 - num_spatial_dims) + [[int(s * zz) for s in ax] for ax, zz in zip(geo.starts, z)]
            out = outputs[ss][b]
            nlog = num_win * _channels(lg) * math.prod(_to3(logits.seg_shapes[ss], 1))
            with _prof.span("sw_blend", 4.0 * nlog + out.numel() * out.element_size()):      # logits read once + output written once
                if logits.proc_weights is not None:
                    w = logits.proc_weights[ss]
                elif isinstance(lg, ops.LogitsMosaic) and c.imp_key is not None:
                    w = _factored_map(c.imp_key, c.imp, roi3, c.mode, c.sigma_scale, dev)
                else:
                    w = weights[ss]
                _blend(lg, w, out, geo, g, _to3(logits.seg_shapes[ss], 1), buffer, c.argmax_dtype is not None, logits.proc_weights is not None)

    # back to the caller's rank / crop the padding (utils.py:300-313) / output device
    finals = []
    for o, z in zip(outputs, logits.zscales):
        osz = [int(i * zz) for i, zz in zip(geo.image_size, z)] if z else list(geo.image_size)
        o = o.reshape((batch_size, o.shape[1]) + tuple(osz))
        if any(geo.pad_size):
            zoom = [sd / float(rd) for sd, rd in zip(o.shape[2:], roi_size)]
            cut = []
            for sp in range(num_spatial_dims):
                si = num_spatial_dims - sp - 1
                cut.insert(0, slice(int(round(geo.pad_size[sp * 2] * zoom[si])), int(round((geo.pad_size[sp * 2] + geo.spatial[si]) * zoom[si]))))
            o = o[(slice(None), slice(None), *cut)]
        finals.append(o if o.device == c.out_device else o.to(c.out_device))
    return _pack_struct(finals, logits.dict_keys)


def _blend(store, weight, out, geo: _Geometry, grid, seg3, buffer, argmax: bool, premultiplied: bool) -> None:
    """The one blend launch of an output of an image (`out` [K or 1, *img3]): the reference's buffered summation order (single output at window resolution), the
    mosaic layout, the fused argmax epilogue, or the plain blend.  premultiplied: a process_fn's weights are already in the rows; `weight` feeds the count only."""
    if buffer is not None:
        ops.sw_blend_buffered(store[: geo.num_win], weight, out, grid, seg3, buffer[0] + 3 - len(geo.roi_size), buffer[1], premultiplied=premultiplied)
    elif isinstance(store, ops.LogitsMosaic):
        ops.sw_blend_mosaic(store, weight, out)
    elif argmax:
        _blend_argmax(store[: geo.num_win], weight, out[0], grid, seg3, premultiplied=premultiplied)
    else:
        ops.sw_blend(store[: geo.num_win], weight, out, grid, seg3, premultiplied=premultiplied)


def _buffered_batches(vol3, geo: _Geometry, sw_batch_size: int, buffer, win_buf, predict) -> list:
    """The predictor calls of the reference's buffered schedule for one image (monai/inferers/utils.py:215-253 with `_create_buffered_slices`, :324-348): windows
    stably sorted by their start along the buffer axis; flush boundaries after every min(#distinct starts, buffer_steps) distinct starts; batches of `sw_batch_size`
    sorted windows that END at a boundary, gathered into `win_buf` and handed to `predict(count, runs)`.  Every window's prediction goes to row = its row-major index
    of ONE all-window buffer: `mh_sw_blend_buffered_f32` then sums in the buffered order.  -> what `predict` returned for the last batch of the FIRST flush: the
    reference builds its count map then."""
    import numpy as np

    buffer_dim, buffer_steps = buffer
    wins = np.asarray(list(itertools.product(*[range(len(s)) for s in geo.starts])), dtype=np.int64)             # [num_win, nsp] per-axis window numbers, row-major
    start_along = np.asarray(geo.starts[buffer_dim], dtype=np.int64)[wins[:, buffer_dim]]
    order = np.argsort(start_along, kind="mergesort")
    _, counts = np.unique(start_along[order], return_counts=True)
    b_ends = np.cumsum(counts).tolist()
    x = [0, *b_ends][:: min(len(b_ends), buffer_steps)]
    if x[-1] < b_ends[-1]:
        x.append(b_ends[-1])
    first_flush = []
    for gi in range(len(x) - 1):
        for g0 in range(x[gi], x[gi + 1], sw_batch_size):
            idx = [int(order[i]) for i in range(g0, min(g0 + sw_batch_size, x[gi + 1]))]
            k = 0
            while k < len(idx):                 # one gather launch per run of consecutive window indices (the whole batch when buffer_dim is the first axis)
                run = 1
                while k + run < len(idx) and idx[k + run] == idx[k] + run:
                    run += 1
                ops.window_extract(vol3, geo.grid3, idx[k], run, geo.roi3, win_buf[k : k + run])
                k += run
            last = predict(len(idx), [(w, 1) for w in idx])
        if gi == 0:
            first_flush = last
    return first_flush


# ---- importance maps: host evaluation and upload happen once per (patch size, mode, sigma, dtype), not once per call -------------------------
# The map is evaluated on the host (bit-identical to the reference's CPU map) and uploaded from pageable memory -- a synchronous copy that is
# stream-ordered behind everything already enqueued.  Issued per call, right in front of the blend, that copy made the host wait for the whole
# predictor queue and left the GPU idle while the blend's arguments were being built (0.4 ms per 512^3 volume, visible as the gap between the HIP-event
# span and the kernel's own duration in profiles/r03_bench_kernel_trace_stats_v2.txt).  Result-neutral: the same values, kept.
_HOST_MAPS: dict = {}
_DEVICE_MAPS: dict = {}
_MAPS_LOCK = threading.RLock()      # inferers may run concurrently in threads (a server, DataLoader workers): lookups and the clear-all eviction are atomic


def _host_importance_map(patch_size, mode, sigma_scale, dtype):
    key = (tuple(int(v) for v in patch_size), str(mode), tuple(float(v) for v in ensure_tuple(sigma_scale)), dtype)
    with _MAPS_LOCK:
        hit = _HOST_MAPS.get(key)
        if hit is None:
            if len(_HOST_MAPS) >= 8:
                _HOST_MAPS.clear()
                _DEVICE_MAPS.clear()
            hit = _HOST_MAPS[key] = compute_importance_map(patch_size, mode=mode, sigma_scale=sigma_scale, device="cpu", dtype=dtype)
    return hit, key


def _factored_map(imp_key, host_map, roi3, mode, sigma_scale, dev) -> torch.Tensor:
    """[gz | gy | gx | floor] on the device for the mosaic blend (it re-forms the importance map from its factors in registers: same fp32 values, no
    roi^3 map competing with the logits stream for L2), or the full map when the factorisation is not available (non-3-D roi, alignment)."""
    key = ("factored",) + imp_key + (str(dev),)
    with _MAPS_LOCK:
        hit = _DEVICE_MAPS.get(key)
        if hit is None:
            fac = importance_map_factors(imp_key[0], mode, sigma_scale) if len(imp_key[0]) == 3 and (roi3[0] + roi3[1]) % 4 == 0 else None
            if fac is None:     # the caller's own host map (never re-read from the cache: another thread may have evicted it)
                hit = _on_device(host_map.reshape(roi3).contiguous(), dev, cache_key=imp_key + (tuple(roi3),))
            else:
                hit = torch.cat([fac[0], fac[1], fac[2], torch.tensor([fac[3]], dtype=torch.float32)]).to(dev)
            _DEVICE_MAPS[key] = hit
    return hit


def _on_device(host_map: torch.Tensor, dev, cache_key=None) -> torch.Tensor:
    if cache_key is None:
        return host_map.to(dev)
    key = cache_key + (str(dev),)
    with _MAPS_LOCK:
        hit = _DEVICE_MAPS.get(key)
        if hit is None:
            if len(_DEVICE_MAPS) >= 16:
                _DEVICE_MAPS.clear()
            hit = _DEVICE_MAPS[key] = host_map.to(dev)
    return hit


def _finish_reference_result(result, private: dict):
    """a call that fell through to the reference's sliding_window_inference (CPU input, float64, autograd ...) with the fused-argmax switch set:
    AsDiscrete(argmax=True) of the reference's blended result, per output"""
    dtype = private.get("_monai_amd_argmax")
    if dtype is None:
        return result
    keys, parts = _flatten_struct(result)
    return _pack_struct([t.argmax(dim=1, keepdim=True).to(dtype) for t in parts], keys)


sliding_window_inference.__wrapped__._mh_after_reference = _finish_reference_result


def _window_stride(dense: int) -> int:
    """Floats between consecutive windows' logits.  The blend reads the K class blocks of up to 8 (27) covering windows of a
    voxel concurrently; with the dense stride (K * roi * 4 B, a multiple of 128 KiB at 96^3) those streams fall on the same HBM
    channels.  Large windows get a stride of 17 x 256 B modulo 128 KiB (measured with tools/ubench/hbm_stream.hip and
    tools/blend_bench.py, profiles/r02_*); MONAI_AMD_LOGITS_PAD (floats, multiple of 4) overrides, 0 = dense."""
    env = os.environ.get("MONAI_AMD_LOGITS_PAD")
    if env is not None and env != "":
        pad = max(0, int(env))
        return dense + pad - pad % 4
    if dense % 4 or dense * 4 < (1 << 20):
        return dense
    pad_bytes = (17 * 256 - dense * 4) % (1 << 17)
    return dense + pad_bytes // 4


def _check_fit(need, shard, dev) -> None:
    """The fit rule of the all-window logits, either layout: at most 90 % of the free HBM and at most the explicit cap (`_logits_budget`).  The decision must be
    the same on every rank (a rank that went slab-wise alone would dead-lock the others' collectives): under window sharding the free memory is the MINIMUM over
    the ranks (`agree_batch`; the identity, and no collective, when the call is not sharded)."""
    if dev.type == "cuda":
        free, _ = torch.cuda.mem_get_info(dev)
        free = float(shard.agree_batch(int(free), dev))
        if need > 0.9 * free:
            raise _LogitsDoNotFit(need, free)
    limit = _logits_budget(dev)
    if limit is not None and need > limit:
        raise _LogitsDoNotFit(need, limit)


def _alloc_logits(shard, nb: int, k: int, seg3, dtype, dev) -> torch.Tensor:
    """Logits of every window of the image, [num_win (padded to whole rounds when sharded), K, *seg3] as a view of one flat
    buffer with a padded window stride (`_window_stride`): the predictor writes its windows' rows, window sharding completes
    the others (`flat_rows`), the blend reads it once."""
    rows = shard.padded_windows(nb)
    dense = k * seg3[0] * seg3[1] * seg3[2]
    ws = _window_stride(dense)
    _check_fit(rows * ws * 4, shard, dev)
    flat = torch.empty(rows * ws, dtype=dtype, device=dev)
    return flat.as_strided((rows, k) + tuple(seg3), (ws, seg3[0] * seg3[1] * seg3[2], seg3[1] * seg3[2], seg3[2], 1))


def _alloc_mosaic(predictor, shard, argmax_dtype, k: int, grid3, roi3, dtype, dev):
    """The mosaic logits layout (ops.LogitsMosaic: the windows of one residue class per axis as dense arrays, so the blend reads long runs instead of
    384-byte pieces of 8 ... 27 x K window blocks) when the path allows it: a predictor whose last kernel can write it (`forward_into_windows`), one GPU
    (window sharding gathers window-major rows), the plain blend (the fused-argmax epilogue reads window-major), a regular grid with <= 4 residue
    classes, K <= 8.  Same result bits either way; MONAI_AMD_LOGITS_LAYOUT=windows keeps the window-major buffer."""
    if (not hasattr(predictor, "forward_into_windows") or shard.sharded or argmax_dtype is not None or dtype != torch.float32
            or os.environ.get("MONAI_AMD_LOGITS_LAYOUT") == "windows" or not ops.LogitsMosaic.supported(grid3, roi3, k)):
        return None
    layout = ops.LogitsMosaic(grid3, roi3, k, dev, dtype, allocate=False)
    _check_fit(4.0 * layout.total, shard, dev)
    return layout.allocate()


def _blend_argmax(logits, imp, labels, grid, seg3, premultiplied: bool) -> None:
    """labels [D, H, W] = argmax over the classes of the blended logits, in ONE pass when the window grid has
    dense_patch_slices' regular form (mh_sw_blend_argmax_f32); otherwise blend, then the channel argmax kernel."""
    try:
        ops.sw_blend_argmax(logits, imp, labels, grid, seg3, int(logits.shape[1]), premultiplied=premultiplied)
    except RuntimeError as e:
        if "irregular window starts" not in str(e):
            raise
        tmp = torch.empty((int(logits.shape[1]),) + tuple(labels.shape), dtype=logits.dtype, device=logits.device)
        ops.sw_blend(logits, imp, tmp, grid, seg3, premultiplied=premultiplied)
        labels.copy_(ops.channel_reduce("argmax", tmp)[0].to(labels.dtype))


def sliding_window_argmax(inputs, roi_size, sw_batch_size, predictor, *args, labels_dtype=torch.float32, **kwargs):
    """``sliding_window_inference`` followed by ``AsDiscrete(argmax=True)`` -- the post-processing step segmentation bundles put
    behind the inferer (monai/transforms/post/array.py:132-237: ``torch.argmax(img, dim=0, keepdim=True)`` converted to float32)
    -- with the argmax fused into the blend's epilogue: every voxel's K blended values are formed in registers exactly as the
    blend forms them and only the label is written (K x 4 B of output traffic per voxel -> 4 B, or 1 B with
    ``labels_dtype=torch.uint8``).  Same positional / keyword arguments as ``sliding_window_inference``; returns
    ``[B, 1, *spatial]`` labels (tuple / dict outputs: one label map per output), bit-identical to
    ``AsDiscrete(argmax=True)`` applied to each batch element of the unfused result (ties -> first index, NaN maximal)."""
    if labels_dtype not in (torch.float32, torch.uint8):
        raise ValueError("sliding_window_argmax: labels_dtype must be torch.float32 (AsDiscrete's output dtype) or torch.uint8")
    return sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, *args, _monai_amd_argmax=labels_dtype, **kwargs)


def flat_rows(logits: torch.Tensor, r0: int, r1: int) -> torch.Tensor:
    """Rows [r0, r1) of an `_alloc_logits` buffer as ONE contiguous 1-D tensor (padding included): what a collective sends."""
    ws = logits.stride(0)
    base = logits._base if logits._base is not None else logits
    return base.reshape(-1)[r0 * ws : r1 * ws]


class _LogitsDoNotFit(RuntimeError):
    """The all-window logits buffer exceeds the memory budget: the caller retries slab by slab (`_slabwise`)."""

    def __init__(self, need: int, budget: float):
        super().__init__(
            f"monai_amd: the all-window logits buffer needs {need / 2**30:.2f} GiB, the budget is {budget / 2**30:.2f} GiB of HBM "
            "(and the volume cannot be cut into slabs along its first spatial axis: a single row of windows does not fit, the image is padded "
            "up to the roi, or the call uses with_coord / process_fn, whose semantics are tied to the whole volume)"
        )
        self.need, self.budget = need, budget


def _logits_budget(dev):
    """Explicit cap on the logits buffer (bytes) from MONAI_AMD_MAX_LOGITS_BYTES -- tests use it to force the slab-wise
    path on small volumes; without it the cap is 90 % of the free HBM (checked in _alloc_logits)."""
    env = os.environ.get("MONAI_AMD_MAX_LOGITS_BYTES")
    return float(env) if env else None


def _slabwise(inputs, roi_size, starts0, need: int, budget: float, call):
    """Volumes whose all-window logits do not fit in HBM: cut the FIRST spatial axis into slabs of whole window rows and run
    the same inference on each slab's sub-volume -- the span of every window row that intersects the slab, so each owned
    output plane sees exactly the windows it sees in the whole volume, at the same positions and in the same order
    (results are bit-identical; the rows shared by two neighbouring sub-volumes are computed twice: one extra row per slab at
    overlap 0.5).  `call(sub_inputs)` runs the normal path; returns the packed outputs of the whole volume."""
    rows = len(starts0)
    roi0 = int(roi_size[0])
    size0 = int(inputs.shape[2])
    per_row = need / rows
    first_of = lambda a: min(r for r in range(rows) if starts0[r] + roi0 > starts0[a])  # noqa: E731
    # greedy grouping of owned rows [a, b): owned + re-computed rows must fit in the budget
    groups, a = [], 0
    while a < rows:
        b = a + 1
        while b < rows and (b + 1 - first_of(a)) * per_row <= budget:
            b += 1
        if (b - first_of(a)) * per_row > budget:
            raise _LogitsDoNotFit(int((b - first_of(a)) * per_row), budget)
        groups.append((a, b))
        a = b
    if len(groups) < 2:
        raise _LogitsDoNotFit(need, budget)
    finals, keys = None, None
    for a, b in groups:
        r0 = first_of(a)
        lo, hi = int(starts0[r0]), int(starts0[b - 1]) + roi0
        own_lo, own_hi = int(starts0[a]), (int(starts0[b]) if b < rows else size0)
        res = call(inputs[:, :, lo:hi])
        keys, parts = _flatten_struct(res)
        if finals is None:
            finals = []
            for t in parts:
                scale = t.shape[2] / float(hi - lo)
                finals.append(torch.empty(tuple(t.shape[:2]) + (int(round(size0 * scale)),) + tuple(t.shape[3:]), dtype=t.dtype, device=t.device))
        for t, f in zip(parts, finals):
            scale = t.shape[2] / float(hi - lo)
            p0, p1, q0 = own_lo * scale, own_hi * scale, lo * scale
            if abs(p0 - round(p0)) > 1e-6 or abs(p1 - round(p1)) > 1e-6 or abs(q0 - round(q0)) > 1e-6:
                raise RuntimeError("monai_amd: slab-wise blending needs output planes aligned with the window rows "
                                   f"(output/input scale {scale} along the first spatial axis)")
            p0, p1, q0 = int(round(p0)), int(round(p1)), int(round(q0))
            f[:, :, p0:p1] = t[:, :, p0 - q0 : p1 - q0]
        del res, parts
    return _pack_struct(finals, keys)


def _restore_meta(out: torch.Tensor, src):
    """Give the result the input's MetaTensor type and metadata (the reference's ``convert_to_dst_type(final_output,
    temp_meta)``, utils.py:316-319) when the input was a MetaTensor-like tensor subclass."""
    try:
        res = type(src)(out)
        if hasattr(res, "copy_meta_from"):
            res.copy_meta_from(src, copy_attr=False)
        return res
    except Exception:
        return out
