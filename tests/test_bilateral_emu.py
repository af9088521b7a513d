"""The exact bilateral filter (monai_amd._C.bilateral_filter, ops.bilateral_filter, networks.layers.BilateralFilter) and the kernels under it on the
SIMT emulator (CPU): the cases of tests/bilateral_cases.py against the reference's own outputs, the host arithmetic and the argument checks of the C
entries that need no device, the launch / host-read contract and the autograd function.

The emulator takes libm's exp2f where the MI355X has v_exp_f32, so the float32 ratios printed here and by tests/test_bilateral_gpu.py differ a little."""
import ctypes

import numpy as np
import pytest
import torch

import bilateral_cases as bc


@pytest.mark.parametrize("group", bc.GROUPS)
def test_golden_cases_within_the_reference_error(emu, group):
    cases = [c for c in bc.golden_cases() if c["id"].split("-")[0] == group]
    assert cases, group
    worst = bc.check_cases("cpu", cases)
    print(group, "worst |ours - ref64| / e_ref per kernel (1 tile, 2 generic):", {k: round(v, 2) for k, v in sorted(worst.items())})


def test_every_case_is_in_a_group_and_both_kernels_are_reached():
    cases = bc.golden_cases()
    assert all(c["id"].split("-")[0] in bc.GROUPS for c in cases) and len({c["id"] for c in cases}) == len(cases)
    for group, paths in (("tile3d", {bc.TILE}), ("tile2d", {bc.TILE}), ("tile1d", {bc.TILE}), ("win3d", {bc.TILE}), ("win2d", {bc.TILE}), ("win1d", {bc.TILE}),
                         ("f64", {bc.GENERIC}), ("chan", {bc.TILE, bc.GENERIC}), ("generic", {bc.TILE, bc.GENERIC}), ("nonfinite", {bc.TILE, bc.GENERIC})):
        assert {c["path"] for c in cases if c["id"].split("-")[0] == group} == paths, group
    assert {c["shape"][1] for c in cases if c["id"].startswith("chan-c")} == {1, 2, 3, 4, 5, 16}
    assert all(c["shape"][0] == 2 for c in cases if c["id"].startswith("chan-"))
    assert {bc.window(c["ss"]) for c in cases if c["id"].startswith("win3d")} | {5} == {3, 5, 7, 9, 11, 15}


def _dll():
    from monai_amd import _lib, build

    build.build()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    dll.mh_last_error.restype = ctypes.c_char_p
    dll.mh_bilateral_window.argtypes = [ctypes.c_float]
    return dll


def test_exports_and_symbols():
    """the names this feature adds (absent before it)"""
    import monai_amd.networks.layers as layers
    from monai_amd import _C, ops, patch
    from monai_amd.networks.layers import BilateralFilter
    from monai_amd.networks.layers.filtering import BilateralFilter as direct

    assert BilateralFilter is direct is layers.BilateralFilter and issubclass(BilateralFilter, torch.autograd.Function)
    assert "bilateral_filter" in _C.__all__ and callable(_C.bilateral_filter) and callable(ops.bilateral_filter) and callable(ops.bilateral_filter_path)
    assert patch._TARGETS["monai.networks.layers.filtering"]["BilateralFilter"] == ("monai_amd.networks.layers.filtering", "BilateralFilter")
    dll = _dll()
    for name in ("mh_bilateral_window", "mh_bilateral_filter_accepts", "mh_bilateral_filter_f32", "mh_bilateral_filter_f64"):
        assert hasattr(dll, name), name


def test_window_rule_is_the_float32_product():
    dll = _dll()
    w = dll.mh_bilateral_window
    assert [w(s) for s, _ in bc.WINDOW_RULE] == [1, 3, 3, 5, 5, 7, 11] == [k for _, k in bc.WINDOW_RULE]
    assert w(51.0) == 255 and w(50.8) == 255 and w(51.2) == 257
    assert [w(s) for s in (1.0, 1.4, 2.0, 2.6, 3.0, 5.0)] == [5, 7, 11, 13, 15, 25]
    # the three a double-precision product of the float value gets wrong
    assert [int(np.ceil(5.0 * float(np.float32(s)))) | 1 for s in (0.2, 0.6, 2.2)] == [3, 5, 13]
    assert w(0.0) == -1 and w(-1.0) == -1 and w(float("nan")) == -1 and w(float("inf")) == -1 and w(1e30) == 0x7fffffff
    from monai_amd import ops

    assert [ops.bilateral_window(s) for s, _ in bc.WINDOW_RULE] == [k for _, k in bc.WINDOW_RULE]


def test_path_choice_is_host_arithmetic():
    acc = _dll().mh_bilateral_filter_accepts      # (C, D, H, W, K, is_f64)
    T, G = bc.TILE, bc.GENERIC
    # 3-D at C = 1: every window up to 15 taps is staged, 17 taps are not
    assert [acc(1, 64, 64, 64, k, 0) for k in (3, 5, 7, 9, 11, 13, 15, 17, 255)] == [T] * 7 + [G, G]
    # 2-D at C <= 4: every window up to 25 taps (and 31); 35 taps at 4 channels are not
    assert all(acc(c, 1, 300, 300, k, 0) == T for c in (1, 2, 3, 4) for k in range(3, 27, 2))
    assert acc(4, 1, 300, 300, 31, 0) == T and acc(4, 1, 300, 300, 35, 0) == G and acc(1, 1, 300, 300, 35, 0) == T
    # 1-D: every window
    assert all(acc(c, 1, 1, 5000, k, 0) == T for c in (1, 4) for k in (3, 63, 255))
    # more than 4 channels, float64 and a window of one tap are the generic kernel's
    assert acc(5, 64, 64, 64, 5, 0) == G and acc(16, 1, 64, 64, 5, 0) == G and acc(1, 64, 64, 64, 5, 1) == G and acc(1, 64, 64, 64, 1, 0) == G
    # the choice does not depend on the image size (only on which axes have extent 1)
    assert acc(1, 2, 3, 5, 5, 0) == T and acc(1, 1, 1, 7, 5, 0) == T and acc(1, 9, 1, 1, 5, 0) == T and acc(1, 1, 1, 1, 5, 0) == G
    assert acc(17, 8, 8, 8, 5, 0) == 0 and acc(1, 8, 8, 8, 257, 0) == 0 and acc(1, 8, 8, 8, 4, 0) == 0 and acc(1, 0, 8, 8, 5, 0) == 0 and acc(0, 8, 8, 8, 5, 0) == 0
    assert acc(1, 2047, 2047, 2047, 5, 0) == T and acc(1, 1 << 30, 1 << 30, 1 << 30, 5, 0) == 0        # more than 2^31 - 1 workgroups


def test_argument_errors_need_no_gpu():
    dll = _dll()
    for f in (dll.mh_bilateral_filter_f32, dll.mh_bilateral_filter_f64):
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
        a, b = 0x10000, 0x20000
        assert f(a, a, 1, 1, 16, 16, 16, 1.0, 0.5, None) == -1 and b"same buffer" in dll.mh_last_error()
        assert f(a, b, 1, 17, 16, 16, 16, 1.0, 0.5, None) == -1 and b"Bilateral filtering not implemented for channel count > 16" in dll.mh_last_error()
        assert f(a, b, 1, 1, 16, 16, 16, 51.2, 0.5, None) == -1 and b"K = 257" in dll.mh_last_error()
        for ss, cs in ((0.0, 0.5), (-1.0, 0.5), (float("nan"), 0.5), (float("inf"), 0.5), (1.0, 0.0), (1.0, -2.0), (1.0, float("nan")), (1.0, float("inf"))):
            assert f(a, b, 1, 1, 16, 16, 16, ss, cs, None) == -1 and b"finite and positive" in dll.mh_last_error(), (ss, cs)
        assert f(None, b, 1, 1, 16, 16, 16, 1.0, 0.5, None) == -1 and f(a, None, 1, 1, 16, 16, 16, 1.0, 0.5, None) == -1 and b"null" in dll.mh_last_error()
        assert f(a, b, 0, 1, 16, 16, 16, 1.0, 0.5, None) == -1 and f(a, b, 1, 0, 16, 16, 16, 1.0, 0.5, None) == -1 and f(a, b, 1, 1, 16, 0, 16, 1.0, 0.5, None) == -1
        assert f(a, b, 70000, 1, 16, 16, 16, 1.0, 0.5, None) == -3 and b"65535" in dll.mh_last_error()
        assert f(a, b, 1, 1, 1 << 30, 1 << 30, 1 << 30, 1.0, 0.5, None) == -3 and b"workgroups" in dll.mh_last_error()


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


def test_one_launch_per_call_and_nothing_is_read_back(monkeypatch):
    from launch_trace import launch_trace
    from monai_amd import _C, ops
    from monai_amd.networks.layers import BilateralFilter

    synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: synced.append(1))
    x3, x2, x1 = torch.randn(2, 3, 6, 10, 11), torch.randn(2, 5, 10, 11), torch.randn(3, 1, 40)
    for call, entry, args in (
            (lambda: ops.bilateral_filter(x3, 1.0, 0.5), "bilateral_filter_f32", "2 3 6 10 11 1.0 0.5"),
            (lambda: _C.bilateral_filter(x2, 2.0, 0.25, False), "bilateral_filter_f32", "2 5 1 10 11 2.0 0.25"),
            (lambda: BilateralFilter.apply(x1, 3.0, 1.5, False), "bilateral_filter_f32", "3 1 1 1 40 3.0 1.5"),
            (lambda: ops.bilateral_filter(x3.double(), 1.0, 0.5), "bilateral_filter_f64", "2 3 6 10 11 1.0 0.5"),
            (lambda: ops.bilateral_filter(x3.transpose(3, 4), 1.0, 0.5), "bilateral_filter_f32", "2 3 6 11 10 1.0 0.5")):
        with launch_trace() as lines, _HostReads() as host:
            call()
        assert len(lines) == 1 and lines[0].split()[0] == entry, lines
        assert " ".join(lines[0].split()[3:10]) == args, (lines, args)
        assert host.count == 0, host.count
    assert not synced, "BilateralFilter must not synchronise the device"


def test_backward_is_the_filter_of_the_gradient(emu):
    from monai_amd import ops
    from monai_amd.networks.layers import BilateralFilter

    x = torch.from_numpy(bc.inputs(next(c for c in bc.golden_cases() if c["id"] == "chan-c2")).copy()).requires_grad_()
    y = BilateralFilter.apply(x, 1.0, 1.5, False)
    assert torch.equal(y, ops.bilateral_filter(x.detach(), 1.0, 1.5))
    y.sum().backward()
    want = ops.bilateral_filter(torch.ones_like(x), 1.0, 1.5)
    assert x.grad.numpy().tobytes() == want.numpy().tobytes()


def test_half_is_float32_rounded_once(emu):
    from monai_amd import _C, ops

    x = torch.from_numpy(bc.inputs(next(c for c in bc.golden_cases() if c["id"] == "chan-2d-c3")).copy()).half()
    got = ops.bilateral_filter(x, 1.0, 1.5)
    assert got.dtype == torch.float16 and torch.equal(got, ops.bilateral_filter(x.float(), 1.0, 1.5).half())
    assert torch.equal(_C.bilateral_filter(x, 1.0, 1.5, False), got)


def test_python_errors(emu):
    from monai_amd import _C, ops
    from monai_amd._fallback import UnsupportedOnDevice
    from monai_amd.networks.layers import BilateralFilter

    x = torch.randn(1, 2, 5, 6)
    with pytest.raises(RuntimeError, match="fast_approx=False"):
        _C.bilateral_filter(x, 1.0, 0.5, True)
    with pytest.raises(RuntimeError, match="fast_approx=False"):
        BilateralFilter.apply(x)                          # the reference's default is the approximation
    with pytest.raises(RuntimeError, match="Bilateral filtering not implemented for channel count > 16"):
        _C.bilateral_filter(torch.randn(1, 17, 5, 6), 1.0, 0.5, False)
    with pytest.raises(RuntimeError, match="Bilateral filtering not implemented for spatial dimension > 3"):
        _C.bilateral_filter(torch.randn(1, 1, 3, 3, 3, 3), 1.0, 0.5, False)
    with pytest.raises(RuntimeError, match="K = 257"):
        ops.bilateral_filter(x, 51.2, 0.5)
    with pytest.raises(RuntimeError, match="finite and positive"):
        ops.bilateral_filter(x, 1.0, 0.0)
    with pytest.raises(UnsupportedOnDevice):
        ops.bilateral_filter(x.to(torch.int32), 1.0, 0.5)
    with pytest.raises(UnsupportedOnDevice, match="65535"):
        ops.bilateral_filter(torch.zeros(70000, 1, 2), 1.0, 0.5)
    # a non-contiguous input is made contiguous; an empty one comes back empty
    xt = torch.randn(1, 2, 6, 5).transpose(2, 3)
    assert torch.equal(ops.bilateral_filter(xt, 1.0, 0.5), ops.bilateral_filter(xt.contiguous(), 1.0, 0.5))
    assert ops.bilateral_filter(torch.zeros(0, 2, 5, 6), 1.0, 0.5).shape == (0, 2, 5, 6)
    assert ops.bilateral_filter_path((5, 6), 2, 1.0) == bc.TILE and ops.bilateral_filter_path((5, 6), 2, 1.0, torch.float64) == bc.GENERIC
