"""``spatial_resample`` on the MI355X resampling kernel -- the eager path of
monai/transforms/spatial/functional.py:68-184."""

from __future__ import annotations

import numpy as np
import torch

from ... import _lib, ops
from ...data.meta_tensor import is_meta
from ...data.utils import AFFINE_TOL, compute_shape_offset, to_affine_nd
from ...networks.utils import index_matrix
from ...utils.misc import ensure_tuple, fall_back_tuple

__all__ = ["spatial_resample"]


def spline_order(mode):
    """The spline order 0..5 when `mode` selects the reference's scipy branch -- an integer, an integer-valued enum or a digit string, what
    ``resolves_modes(backend=None)`` looks up in ``SplineMode`` (monai/transforms/utils.py:2319-2328) -- else None."""
    m = getattr(mode, "value", mode)
    if isinstance(m, bool):
        return None
    if isinstance(m, (int, np.integer)):
        return int(m) if 0 <= int(m) <= 5 else None
    if isinstance(m, str) and len(m) == 1 and m in "012345":
        return int(m)
    return None


def _mode_name(mode) -> str:
    m = str(getattr(mode, "value", mode)).lower()
    if m in ("bilinear", "trilinear", "linear"):
        return "bilinear"
    if m == "nearest":
        return "nearest"
    raise ValueError(f"Unsupported mode: {mode}, available options are ['bilinear', 'nearest'].")


# scipy.ndimage boundary names -> grid_sample padding modes, the table of the reference's `_to_torch_resample_padding_mode`
# (monai/transforms/utils.py:2281-2297, reached through `resolves_modes` from spatial_resample / Resample)
_NDIMAGE_PAD = {"constant": "zeros", "grid-constant": "zeros", "nearest": "border", "reflect": "reflection", "wrap": "reflection",
                "grid-wrap": "reflection", "grid-mirror": "reflection"}


def _pad_name(padding_mode) -> str:
    p = str(getattr(padding_mode, "value", padding_mode)).lower()
    p = _NDIMAGE_PAD.get(p, p)
    if p not in ("zeros", "border", "reflection"):
        raise ValueError(f"Unsupported padding_mode: {padding_mode}, available options are {sorted(_NDIMAGE_PAD) + ['zeros', 'border', 'reflection']}.")
    return p


# grid_sample padding names -> scipy.ndimage boundary modes, the table of the reference's `_to_numpy_resample_padding_mode` (monai/transforms/utils.py:2266-2278)
_NDIMAGE_MODES = ("reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap")
_TORCH_TO_NDIMAGE = {"zeros": "constant", "border": "nearest", "reflection": "reflect"}


def _spline_pad_name(padding_mode) -> str:
    p = str(getattr(padding_mode, "value", padding_mode)).lower()
    p = _TORCH_TO_NDIMAGE.get(p, p)
    if p not in _NDIMAGE_MODES:
        raise ValueError(f"Unsupported padding_mode: {padding_mode}, available options are {sorted(_TORCH_TO_NDIMAGE) + list(_NDIMAGE_MODES)}.")
    return p


def spline_index_matrix(xform, in_size, out_size, align_corners: bool) -> np.ndarray:
    """3 x 4 fp64 matrix M with  input index = M @ (output index, 1)  of the reference's integer-mode branch (functional.py:161-173): ``xform @
    translate((d_out - 1) / 2)`` handed to ``Affine(normalized=True)``, whose ``AffineGrid`` applies it to the centred grid ``o - (d_out - 1) / 2``
    (scaled by ``d / (d - 1)`` per output axis under align_corners, array.py:1775-1780) and whose ``Resample(norm_coords=False)`` leaves the result
    alone, or maps it with ``(d_in - 1) / d_in * (g + 0.5)`` under align_corners (array.py:2076-2082).  2-D transforms get a leading zero row."""
    xform = np.asarray(xform, dtype=np.float64)
    r = len(xform) - 1
    m = xform.copy()
    if align_corners:
        def translate(v):
            t = np.eye(r + 1)
            t[:r, -1] = v
            return t

        c_out = [(float(d) - 1.0) / 2.0 for d in out_size]
        # the reference builds this scale with torch.as_tensor of Python floats (create_scale, transforms/utils.py:1016-1021): float32 values
        s_out = np.diag([float(np.float32(max(int(d), 2) / (max(int(d), 2) - 1.0))) for d in out_size] + [1.0])
        s_in = np.diag([(max(int(d), 2) - 1.0) / max(int(d), 2) for d in in_size] + [1.0])
        m = s_in @ translate([0.5] * r) @ xform @ translate(c_out) @ s_out @ translate([-v for v in c_out])
    full = np.zeros((3, 4))
    full[3 - r:, 3 - r:3] = m[:r, :r]
    full[3 - r:, 3] = m[:r, -1]
    return full


def spatial_resample(img, dst_affine, spatial_size, mode, padding_mode, align_corners, dtype_pt, transform_info=None):
    """Resample channel-first `img` from its own affine to `dst_affine` / `spatial_size`.

    Same decisions as the reference: ``xform = solve(src_affine, dst_affine)`` in fp64 (:126-132); unchanged affine and
    size -> the input comes back as float32 without resampling (:133-151); otherwise the default (non-compiled)
    branch, ``AffineTransform(normalized=False, reverse_indexing=True)`` (:174-179).  The interpolation arithmetic
    runs in `dtype_pt` (fp64 by default); input is read and output written as fp32 (:183).
    Returns (tensor, xform or None, output spatial size)."""
    src_affine = img.meta["affine"] if is_meta(img) and "affine" in img.meta else torch.eye(4, dtype=torch.float64)
    data = img.as_tensor() if is_meta(img) else img
    original_shape = tuple(data.shape[1:])
    out_size, xform, src_a, unchanged = resample_plan(original_shape, src_affine, dst_affine, spatial_size)
    spatial_rank = len(xform) - 1
    if unchanged:
        return data.to(torch.float32), None, tuple(int(v) for v in out_size), src_a
    return _execute_resample(data, xform, out_size, spatial_rank, mode, padding_mode, align_corners, dtype_pt) + (src_a,)


_PLANS: dict = {}      # host algebra of recent (shape, affines, size) combinations: a data set resampled to one spacing repeats a handful of them for every volume


def memo(key, make):
    """`make()` once per key (a bounded process-wide table): the fp64 host algebra in front of a resampling launch takes longer than the launch itself at 512^3
    (0.3 ms against 0.28 ms per volume on the benchmark hosts); the values are treated as read-only by every caller (arrays are handed out as copies)"""
    hit = _PLANS.get(key)
    if hit is None:
        if len(_PLANS) >= 256:
            _PLANS.clear()
        hit = _PLANS[key] = make()
    return hit


def _bytes(a) -> bytes:
    if a is None:
        return b""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.astype(np.float64, copy=False).tobytes() + bytes(str(a.shape), "ascii")


def resample_plan(original_shape, src_affine, dst_affine, spatial_size):
    """Host algebra of ``spatial_resample`` (functional.py:100-151): (output size, xform = solve(src, dst), src affine at the
    spatial rank, unchanged?) -- shared by the eager path and the lazy path (which only records xform and the size)."""
    size_key = spatial_size if (spatial_size is None or isinstance(spatial_size, int)) else tuple(int(v) for v in ensure_tuple(spatial_size))
    out_size, xform, src_a, unchanged = memo(("plan", tuple(int(v) for v in original_shape), _bytes(src_affine), _bytes(dst_affine), size_key),
                                            lambda: _resample_plan(original_shape, src_affine, dst_affine, spatial_size))
    return out_size.copy(), xform.copy(), src_a.copy(), unchanged


def _resample_plan(original_shape, src_affine, dst_affine, spatial_size):
    src_affine = np.asarray(src_affine.detach().cpu() if isinstance(src_affine, torch.Tensor) else src_affine, dtype=np.float64)
    spatial_rank = min(len(original_shape), src_affine.shape[0] - 1, 3)
    if (not isinstance(spatial_size, int) or spatial_size != -1) and spatial_size is not None:
        spatial_rank = min(len(ensure_tuple(spatial_size)), 3)
    src_a = to_affine_nd(spatial_rank, src_affine)
    dst_a = to_affine_nd(spatial_rank, dst_affine) if dst_affine is not None else src_a
    in_size = np.asarray(original_shape[:spatial_rank])
    if isinstance(spatial_size, int) and spatial_size == -1:
        out_size = in_size
    elif spatial_size is None and spatial_rank > 1:
        out_size, _ = compute_shape_offset(in_size, src_a, dst_a)
    else:
        out_size = spatial_size
    out_size = np.asarray(fall_back_tuple(ensure_tuple(out_size)[:spatial_rank], in_size, lambda x: x >= 0), dtype=int)
    try:
        xform = np.eye(spatial_rank + 1) if spatial_rank < 2 else np.linalg.solve(src_a, dst_a)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"src affine is not invertible {src_a}, {dst_a}.") from e
    same_size = np.allclose(out_size, in_size)
    unchanged = (np.allclose(src_a, dst_a, atol=AFFINE_TOL) and same_size) or (np.allclose(xform, np.eye(len(xform)), atol=AFFINE_TOL) and same_size)
    return out_size, xform, src_a, bool(unchanged)


def _execute_resample(data, xform, out_size, spatial_rank, mode, padding_mode, align_corners, dtype_pt):
    sizes = list(data.shape)
    chns, in_sp, extra = sizes[0], sizes[1:spatial_rank + 1], sizes[spatial_rank + 1:]
    x = data.reshape([-1] + in_sp) if extra else data
    x = x.to(torch.float32).contiguous()
    _lib.require_device(x)
    if spatial_rank == 1:
        raise NotImplementedError("monai_amd: 1-D spatial_resample is not on the HIP path")
    order = spline_order(mode)
    if order is not None:
        # the reference's scipy branch (functional.py:161-173): one prefilter and one sampling launch on float64 coefficients; `dtype_pt` only
        # chooses the precision of the reference's coordinate grid, here the coordinates are fp64 either way
        if data.dtype != torch.float32:
            raise _lib.UnsupportedOnDevice(f"monai_amd: spline-order resampling of a {data.dtype} image is not on the HIP path (float32 is)")
        ac = bool(align_corners) if align_corners not in (None, "none") else False
        m = memo(("spline-index", _bytes(xform), tuple(int(v) for v in in_sp), tuple(int(v) for v in out_size), ac),
                 lambda: spline_index_matrix(xform, in_sp, [int(v) for v in out_size], ac))
        pad = 3 - spatial_rank
        vol = x.reshape((x.shape[0],) + (1,) * pad + tuple(in_sp))
        out = ops.spline_resample(vol, order, _spline_pad_name(padding_mode), out_size=(1,) * pad + tuple(int(v) for v in out_size), m=m.reshape(-1),
                                  rank=spatial_rank)
        out = out.reshape((x.shape[0],) + tuple(int(v) for v in out_size))
        if extra:
            out = out.reshape((chns, *[int(v) for v in out_size], *extra))
        return out, xform, tuple(int(v) for v in out_size)
    m = memo(("index", _bytes(xform), tuple(int(v) for v in in_sp), tuple(int(v) for v in out_size), bool(align_corners)),
             lambda: index_matrix(xform, in_sp, [int(v) for v in out_size], normalized=False, align_corners=bool(align_corners), reverse_indexing=True))
    pad = 3 - spatial_rank
    vol = x.reshape((x.shape[0],) + (1,) * pad + tuple(in_sp))
    out = ops.affine_resample(vol, m.reshape(-1), (1,) * pad + tuple(int(v) for v in out_size), _mode_name(mode), _pad_name(padding_mode),
                              bool(align_corners), dtype_pt == torch.float64)
    out = out.reshape((x.shape[0],) + tuple(int(v) for v in out_size))
    if extra:
        out = out.reshape((chns, *[int(v) for v in out_size], *extra))
    return out, xform, tuple(int(v) for v in out_size)
