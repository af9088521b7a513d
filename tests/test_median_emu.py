"""The median filter (MedianSmooth(d), MedianFilter, median_filter, ops.median_filter) and the kernels under it on the SIMT emulator (CPU): the cases
of tests/median_cases.py against the reference's own outputs, the argument checks of the C entry that need no device, and the launch / host-read
contract."""
import ctypes

import pytest
import torch

import median_cases as mc

GROUPS = ("small", "unit", "fast3d", "fast2d", "fast-r011", "func", "smooth", "2d", "1d", "radii", "general", "passes", "nonfinite")


@pytest.mark.parametrize("group", GROUPS)
def test_golden_cases_bit_identical_to_the_reference(emu, group):
    paths = mc.case_golden("cpu", lambda cid: cid.startswith(group))
    assert paths, group
    print(group, "paths taken", sorted(paths))


def test_every_case_is_in_a_group_and_both_kernels_are_reached():
    cases = mc.golden_cases()
    assert all(sum(c["id"].startswith(g) for g in GROUPS) == 1 for c in cases)
    assert {mc.expected_path(c) for c in cases} == {mc.FAST, mc.GENERAL}
    for group, path in (("fast3d", mc.FAST), ("fast2d", mc.FAST), ("fast-r011", mc.FAST), ("general", mc.GENERAL), ("small", mc.GENERAL)):
        assert {mc.expected_path(c) for c in cases if c["id"].startswith(group)} == {path}, group
    assert {mc.expected_path(c) for c in cases if c["id"].startswith("nonfinite")} == {mc.FAST, mc.GENERAL}


def test_median_api(emu):
    mc.case_api("cpu")


def _dll():
    from monai_amd import _lib, build

    build.build()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    dll.mh_last_error.restype = ctypes.c_char_p
    return dll


def test_exports_and_symbols():
    """the names this feature adds (absent before it)"""
    from monai_amd.transforms import MedianSmooth, MedianSmoothD, MedianSmoothDict, MedianSmoothd  # noqa: F401
    from monai_amd.networks.layers import MedianFilter, median_filter  # noqa: F401
    from monai_amd import ops

    assert callable(ops.median_filter)
    dll = _dll()
    assert hasattr(dll, "mh_median_filter_f32") and hasattr(dll, "mh_median_filter_accepts")


def test_path_choice_is_host_arithmetic():
    dll = _dll()
    acc = dll.mh_median_filter_accepts
    assert acc(64, 64, 64, 1, 1, 1) == 1 and acc(1, 64, 64, 0, 1, 1) == 1 and acc(7, 64, 64, 0, 1, 1) == 1
    assert acc(64, 64, 64, 2, 2, 2) == 2 and acc(64, 64, 64, 3, 3, 3) == 2 and acc(2, 3, 5, 1, 2, 4) == 2 and acc(4, 3, 2, 3, 2, 1) == 2
    assert acc(1, 1, 64, 0, 0, 1) == 2 and acc(64, 64, 64, 1, 0, 1) == 2 and acc(64, 64, 64, 0, 0, 0) == 2 and acc(1, 1, 4096, 0, 0, 171) == 2
    assert acc(64, 64, 64, 4, 3, 3) == 0 and acc(64, 64, 64, 3, 3, 4) == 0 and acc(1, 1, 4096, 0, 0, 172) == 0      # 9 x 7 x 7, 7 x 7 x 9, 345
    assert acc(64, 64, 64, 1, 1, -1) == 0 and acc(0, 64, 64, 1, 1, 1) == 0 and acc(64, 64, 64, 1 << 30, 1 << 30, 1 << 30) == 0
    assert acc(2047, 2047, 2047, 1, 1, 1) == 1 and acc(1 << 30, 1 << 30, 1 << 30, 1, 1, 1) == 0                       # more than 2^31 - 1 workgroups


def test_argument_errors_need_no_gpu():
    dll = _dll()
    f = dll.mh_median_filter_f32
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    a, b = 0x10000, 0x20000
    assert f(a, b, 1, 16, 16, 16, 4, 3, 3, None) == -3 and b"more than 343 values" in dll.mh_last_error() and b"9 x 7 x 7" in dll.mh_last_error()
    assert f(a, a, 1, 16, 16, 16, 1, 1, 1, None) == -1 and b"same buffer" in dll.mh_last_error()
    assert f(a, b, 1, 16, 16, 16, 1, -1, 1, None) == -1 and b"negative radius" in dll.mh_last_error()
    assert f(None, b, 1, 16, 16, 16, 1, 1, 1, None) == -1 and f(a, b, 0, 16, 16, 16, 1, 1, 1, None) == -1 and f(a, b, 1, 16, 0, 16, 1, 1, 1, None) == -1
    assert f(a, b, 70000, 16, 16, 16, 1, 1, 1, None) == -3 and b"65535" in dll.mh_last_error()


class _HostReads:
    """counts device-to-host reads: .cpu() / .item() / .tolist() / .numpy() / conversions to Python scalars"""

    NAMES = ("cpu", "item", "tolist", "numpy", "__bool__", "__float__", "__int__", "__index__")

    def __init__(self):
        self.count, self.saved = 0, {}

    def __enter__(self):
        for name in self.NAMES:
            orig = self.saved[name] = getattr(torch.Tensor, name)

            def wrapper(t, *a, _orig=orig, **k):
                self.count += 1
                return _orig(t, *a, **k)

            setattr(torch.Tensor, name, wrapper)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


def test_one_launch_per_pass_and_nothing_is_read_back():
    from launch_trace import launch_trace
    import monai_amd.transforms as ours
    from monai_amd import ops
    from monai_amd.networks.layers import MedianFilter, median_filter

    x = torch.randn(3, 6, 10, 11)
    for call, launches, args in (
            (lambda: ours.MedianSmooth(1)(x), 1, "3 6 10 11 1 1 1"),
            (lambda: ours.MedianSmoothd("img", [1, 2, 3])({"img": x}), 1, "3 6 10 11 1 2 3"),
            (lambda: MedianFilter(2)(x, number_of_passes=3), 3, "3 6 10 11 2 2 2"),
            (lambda: MedianFilter([2, 1], spatial_dims=2)(x), 1, "18 1 10 11 0 2 1"),
            (lambda: MedianFilter(3, spatial_dims=1)(x), 1, "180 1 1 11 0 0 3"),
            (lambda: median_filter(x, kernel_size=(3, 5, 3)), 1, "3 6 10 11 1 2 1"),
            (lambda: ops.median_filter(x, 1, passes=2), 2, "3 6 10 11 1 1 1")):
        with launch_trace() as lines, _HostReads() as host:
            call()
        assert len(lines) == launches and all(ln.split()[0] == "median_filter_f32" for ln in lines), lines
        assert all(" ".join(ln.split()[3:10]) == args for ln in lines), (lines, args)
        assert host.count == 0, host.count
