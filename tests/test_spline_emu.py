"""Spline-order resampling (integer `mode` of Spacing(d) / SpatialResample / Resample / lazy resampling, ops.spline_prefilter / ops.spline_resample) and the
kernels under it on the SIMT emulator (CPU): the cases of tests/spline_cases.py against the reference's and scipy's own outputs, the argument checks
of the C entries that need no device, and the launch / host-read contract."""
import ctypes

import pytest
import torch

import spline_cases as sc

PRE_GROUPS = ("pre-o2", "pre-o3", "pre-o4", "pre-o5")
OPS_GROUPS = ("ops-o0", "ops-o1", "ops-o2", "ops-o3", "ops-o4", "ops-o5")
T_GROUPS = ("spacing-", "sresample-", "exact-o0", "exact-o1", "exact-o2", "exact-o3", "exact-o4", "exact-o5", "exact-shift", "resample-", "lazy-", "inverse-", "spacingd-")


@pytest.mark.parametrize("group", PRE_GROUPS)
def test_prefilter_against_scipy(emu, group):
    assert sc.case_prefilter("cpu", lambda cid: cid.startswith(group)) > 0


@pytest.mark.parametrize("group", OPS_GROUPS)
def test_sampler_against_scipy(emu, group):
    assert sc.case_samples("cpu", lambda cid: cid.startswith(group)) > 0


@pytest.mark.parametrize("group", T_GROUPS)
def test_transforms_against_the_reference(emu, group):
    assert sc.case_transforms("cpu", lambda cid: cid.startswith(group)) > 0


def test_every_case_is_in_one_group_and_every_order_meets_every_mode():
    for cases, groups in ((sc.prefilter_cases(), PRE_GROUPS), (sc.sample_cases(), OPS_GROUPS), (sc.transform_cases(), T_GROUPS)):
        assert all(sum(c["id"].startswith(g) for g in groups) == 1 for c in cases)
    assert {(c["order"], c["mode"]) for c in sc.sample_cases()} >= {(o, m) for o in range(6) for m in sc.MODES}
    assert {(c["order"], c["pad"]) for c in sc.transform_cases() if c["exact"]} >= {(o, m) for o in range(6) for m in sc.MODES}
    assert {(c["order"], c["mode"]) for c in sc.prefilter_cases()} >= {(o, m) for o in range(2, 6) for m in sc.MODES}


def test_spline_api(emu):
    sc.case_api("cpu")


def _dll():
    from monai_amd import _lib, build

    build.build()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    dll.mh_last_error.restype = ctypes.c_char_p
    dll.mh_spline_workspace_bytes.restype = ctypes.c_int64
    return dll


def test_exports_and_symbols():
    """the names this feature adds (absent before it)"""
    from monai_amd import ops
    from monai_amd.transforms.spatial.functional import spline_index_matrix, spline_order  # noqa: F401

    assert callable(ops.spline_prefilter) and callable(ops.spline_resample)
    dll = _dll()
    for name in ("mh_spline_workspace_bytes", "mh_spline_prefilter_f64", "mh_spline_resample_affine_f32", "mh_spline_resample_grid_f32"):
        assert hasattr(dll, name), name


def test_workspace_size_is_host_arithmetic():
    ws = _dll().mh_spline_workspace_bytes          # (order, mode, rank, NC, D, H, W); modes: tests/spline_cases.py MODES order
    assert ws(3, 5, 3, 1, 512, 512, 512) == 8 * 512 ** 3 and ws(3, 4, 3, 1, 512, 512, 512) == 8 * 536 ** 3 and ws(5, 3, 3, 2, 4, 5, 6) == 2 * 8 * 28 * 29 * 30
    assert ws(3, 4, 2, 3, 1, 9, 6) == 3 * 8 * 33 * 30 and ws(2, 0, 2, 1, 1, 9, 6) == 8 * 54
    assert ws(1, 4, 3, 1, 8, 8, 8) == 0 and ws(0, 3, 3, 1, 8, 8, 8) == 0
    dll = _dll()
    assert ws(6, 0, 3, 1, 8, 8, 8) == -1 and dll.mh_last_error() == b"spline order not supported"
    assert ws(-1, 0, 3, 1, 8, 8, 8) == -1 and dll.mh_last_error() == b"spline order not supported"
    assert ws(3, 8, 3, 1, 8, 8, 8) == -1 and b"boundary mode" in dll.mh_last_error()
    assert ws(3, 0, 1, 1, 1, 1, 8) == -1 and b"2 or 3 spatial axes" in dll.mh_last_error()
    assert ws(3, 0, 2, 1, 2, 8, 8) == -1 and b"2-D image" in dll.mh_last_error()


def test_argument_errors_need_no_gpu():
    dll = _dll()
    a, b, c = 0x10000, 0x20000, 0x30000
    m = (ctypes.c_double * 12)()
    pre = dll.mh_spline_prefilter_f64
    pre.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    assert pre(a, b, 1, 3, 8, 8, 8, 6, 0, None) == -1 and dll.mh_last_error() == b"spline order not supported"
    assert pre(a, b, 1, 3, 8, 8, 8, 1, 0, None) == -1 and b"no prefilter" in dll.mh_last_error()
    assert pre(None, b, 1, 3, 8, 8, 8, 3, 0, None) == -1 and pre(a, b, 0, 3, 8, 8, 8, 3, 0, None) == -1 and pre(a, b, 1, 3, 8, 0, 8, 3, 0, None) == -1
    aff = dll.mh_spline_resample_affine_f32
    aff.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert aff(a, 1, 3, 8, 8, 8, b, 4, 4, 4, m, 6, 0, None) == -1 and dll.mh_last_error() == b"spline order not supported"
    assert aff(a, 1, 3, 8, 8, 8, b, 4, 4, 4, None, 3, 0, None) == -1 and b"null matrix" in dll.mh_last_error()
    assert aff(a, 1, 3, 8, 8, 8, b, 4, 0, 4, m, 3, 0, None) == -1 and b"output shape" in dll.mh_last_error()
    assert aff(a, 1, 3, 8, 8, 8, b, 4, 4, 4, m, 3, 9, None) == -1 and aff(None, 1, 3, 8, 8, 8, b, 4, 4, 4, m, 3, 0, None) == -1
    grd = dll.mh_spline_resample_grid_f32
    grd.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assert grd(a, 1, 3, 8, 8, 8, None, 1, None, None, b, 4, 4, 4, 3, 0, None) == -1 and b"null grid" in dll.mh_last_error()
    assert grd(a, 1, 3, 8, 8, 8, c, 1, None, None, b, 4, 4, 4, -2, 0, None) == -1 and dll.mh_last_error() == b"spline order not supported"


class _HostReads:
    """counts device-to-host reads of image data: .cpu() / .item() / .tolist() / .numpy() / conversions to Python scalars of anything larger than a 4 x 4
    affine (the affines of a MetaTensor live on the host and are read there)"""

    NAMES = ("cpu", "item", "tolist", "numpy", "__bool__", "__float__", "__int__", "__index__")

    def __init__(self):
        self.count, self.saved = 0, {}

    def __enter__(self):
        for name in self.NAMES:
            orig = self.saved[name] = getattr(torch.Tensor, name)

            def wrapper(t, *a, _orig=orig, **k):
                self.count += int(t.numel() > 16)
                return _orig(t, *a, **k)

            setattr(torch.Tensor, name, wrapper)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


def test_spacing_with_a_spline_order_is_two_entries_and_reads_nothing_back():
    """Spacing(pixdim, mode=3) on a float32 image returns a float32 MetaTensor with the reference's affine and record, through one prefilter and one
    sampling entry (orders 0 and 1: the sampling entry alone), with no device-to-host read; so does a lazy Spacing + SpatialPad executed once"""
    from launch_trace import launch_trace
    import monai_amd.transforms as ours
    from monai_amd.data.meta_tensor import MetaTensor
    from monai_amd.transforms.lazy import apply_pending

    aff = torch.diag(torch.tensor([1.3, 0.7, 1.1, 1.0], dtype=torch.float64))
    img = MetaTensor(torch.randn(2, 6, 20, 9), affine=aff)

    def spacing(order, pad="border"):
        return ours.Spacing(pixdim=(1.0, 1.0, 1.0), mode=order, padding_mode=pad)(img)

    def lazy():
        y = ours.SpatialPad(spatial_size=(10, 16, 12), lazy=True)(ours.Spacing(pixdim=(1.0, 1.0, 1.0), lazy=True)(img))
        return apply_pending(y, overrides={"mode": 3, "padding_mode": "border"})[0]

    def resample():
        return ours.Resample(mode=3, padding_mode="reflect")(img, grid=torch.zeros(4, 3, 4, 5, dtype=torch.float64))

    spacingd = ours.Spacingd(keys=["image", "label"], pixdim=(1.0, 1.0, 1.0), mode=(3, "nearest"))
    for call, names, shape in ((lambda: spacing(3), ["spline_prefilter_f64", "spline_resample_affine_f32"], (2, 8, 14, 10)),
                               (lambda: spacing(5, "reflect"), ["spline_prefilter_f64", "spline_resample_affine_f32"], (2, 8, 14, 10)),
                               (lambda: spacing(1), ["spline_resample_affine_f32"], (2, 8, 14, 10)),
                               (lambda: spacing(0, "zeros"), ["spline_resample_affine_f32"], (2, 8, 14, 10)),
                               (lazy, ["spline_prefilter_f64", "spline_resample_affine_f32"], (2, 10, 16, 12)),
                               (resample, ["spline_prefilter_f64", "spline_resample_grid_f32"], (2, 3, 4, 5)),
                               (lambda: spacingd({"image": img, "label": img})["image"], ["spline_prefilter_f64", "spline_resample_affine_f32", "affine_resample_f32"], (2, 8, 14, 10))):
        with launch_trace() as lines, _HostReads() as host:
            out = call()
        assert [ln.split()[0] for ln in lines] == names, lines
        assert host.count == 0, host.count
        assert isinstance(out, MetaTensor) and out.dtype == torch.float32 and tuple(out.shape) == shape, (type(out), out.dtype, out.shape)
    with launch_trace() as lines:
        out = spacing(3)
    # prefilter: src coef NC rank D H W order mode stream; `border` is scipy's `nearest` (4)
    assert lines[0].split()[3:10] == ["2", "3", "6", "20", "9", "3", "4"], lines[0]
    assert lines[1].split()[2:7] == ["2", "3", "6", "20", "9"] and lines[1].split()[8:11] == ["8", "14", "10"] and lines[1].split()[-3:-1] == ["3", "4"], lines[1]
    assert torch.allclose(torch.as_tensor(out.meta["affine"]), torch.eye(4, dtype=torch.float64), atol=1e-12)
    rec = out.applied_operations[-1]
    assert rec["class"] == "SpatialResample" and tuple(rec["orig_size"]) == (6, 20, 9) and rec["extra_info"]["mode"] == 3 and rec["extra_info"]["padding_mode"] == "border"
