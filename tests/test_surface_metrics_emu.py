"""-m "not gpu": HausdorffDistanceMetric / SurfaceDistanceMetric / SurfaceDiceMetric, the mask-edge kernel and the exact Euclidean distance transform
(csrc/kernels/edt.h) on the x86 SIMT emulator -- the twins of tests/test_surface_metrics_gpu.py -- and the argument checks of the new C-ABI entries
on a GPU-less host."""
import ctypes

import pytest

import surface_cases as sc
from monai_amd import _lib


def test_edt_vs_brute_force(emu):
    sc.case_edt_vs_brute_force("cpu")


def test_edges_vs_scipy(emu):
    print("edge maps compared", sc.case_edges_vs_scipy("cpu"))


@pytest.mark.parametrize("part", range(sc.PARTS), ids=[sc._tag(s) for s in sc.SHAPES] + ["rest"])
def test_metrics_vs_reference(emu, part):
    print("bit-equal golden results", sc.case_metrics_vs_reference("cpu", part))


def test_spaced_percentiles_vs_truth(emu):
    sc.case_spaced_percentiles_vs_truth("cpu")


def test_golden_is_covered():
    """the golden holds the results the parts of test_metrics_vs_reference and test_spaced_percentiles_vs_truth compare, their truths, the edge maps and the
    transform outputs, and nothing else"""
    assert sc.case_golden_is_covered() == 230


def test_edt_transform_vs_reference(emu):
    sc.case_edt_transform_vs_reference("cpu")


def test_label_maps_equal_onehots(emu):
    sc.case_label_maps_equal_onehots("cpu")


def test_inferer_labels_to_surface(emu):
    sc.case_inferer_labels_to_surface("cpu")


def test_deterministic(emu):
    sc.case_deterministic("cpu")


def test_surface_api(emu):
    sc.case_surface_api("cpu", device_is_real=False)      # inside the emulator context a CPU tensor stands for a device tensor


def test_cpu_tensors_are_refused_outside_the_emulator():
    """the product's own device check (no GPU needed to see it refuse)"""
    import torch

    import monai_amd.metrics as m
    import monai_amd.transforms as T
    from monai_amd._fallback import UnsupportedOnDevice

    x = torch.zeros((1, 2, 3, 3))
    for call in (lambda: m.compute_hausdorff_distance(x, x), lambda: m.SurfaceDistanceMetric()(x, x), lambda: m.SurfaceDiceMetric([1.0])(x, x),
                 lambda: T.DistanceTransformEDT()(x[0]), lambda: m.get_mask_edges(x[0, 0], x[0, 0])):
        with pytest.raises(UnsupportedOnDevice):
            call()


def test_surface_entries_need_no_gpu_for_their_argument_checks():
    """the three workspace queries are host arithmetic; mh_surface_bbox / mh_mask_edges / mh_edt / mh_surface_records refuse null pointers, unknown forms and
    dtypes, axes longer than 2048 and item rows that leave the buffers with MH_ERR_ARG and a message naming the entry BEFORE anything is launched"""
    import numpy as np

    if not __import__("os").path.isfile(_lib.LIB_PATH):
        from monai_amd import build

        build.build()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    dll.mh_last_error.restype = ctypes.c_char_p
    fn = {}
    for name in ("mh_surface_bbox_workspace_bytes", "mh_surface_bbox", "mh_mask_edges", "mh_edt_workspace_bytes", "mh_edt", "mh_surface_records_workspace_bytes",
                 "mh_surface_records"):
        fn[name] = getattr(dll, name)
        fn[name].restype, fn[name].argtypes = _lib.SIGNATURES[name]
    assert fn["mh_surface_bbox_workspace_bytes"](2, 5) == 2 * 5 * 2 * 64 * 8 * 4 and fn["mh_surface_bbox_workspace_bytes"](0, 5) == -1
    assert b"surface_bbox_workspace_bytes" in dll.mh_last_error()
    assert fn["mh_edt_workspace_bytes"](1000, 0) == 1000 * 12 and fn["mh_edt_workspace_bytes"](1000, 1) == 1000 * 20 and fn["mh_edt_workspace_bytes"](0, 0) == -1
    assert fn["mh_surface_records_workspace_bytes"](3) == 3 * 256 * 4 * 8 and fn["mh_surface_records_workspace_bytes"](0) == -1
    p = 0x10000      # never dereferenced: every call below is refused before a launch
    CH, LB, F32, U8, I64, BOOL = 0, 1, 0, 1, 2, 3
    bbox = fn["mh_surface_bbox"]
    assert bbox(None, CH, F32, p, CH, F32, 1, 2, 0, 2, 4, 4, 4, p, p, None) == -1 and b"surface_bbox: null pointer" in dll.mh_last_error()
    assert bbox(p, CH, F32, p, CH, F32, 1, 2, 1, 2, 4, 4, 4, p, p, None) == -1 and b"surface_bbox: bad argument" in dll.mh_last_error()      # classes 1 .. 2 of 2
    assert bbox(p, CH, F32, p, CH, F32, 1, 2, 0, 2, 4, 4, 2049, p, p, None) == -1 and b"longer than 2048" in dll.mh_last_error()
    assert bbox(p, CH, I64, p, CH, F32, 1, 2, 0, 2, 4, 4, 4, p, p, None) == -1 and b"channel-form prediction" in dll.mh_last_error()
    assert bbox(p, CH, F32, p, LB, BOOL, 1, 2, 0, 2, 4, 4, 4, p, p, None) == -1 and b"label-map truth" in dll.mh_last_error()
    assert bbox(p, 2, F32, p, CH, F32, 1, 2, 0, 2, 4, 4, 4, p, p, None) == -1 and b"unknown form 2" in dll.mh_last_error()
    assert bbox(p, CH, 4, p, CH, F32, 1, 2, 0, 2, 4, 4, 4, p, p, None) == -1 and b"unknown dtype 4" in dll.mh_last_error()

    def table(*rows):
        t = np.zeros((len(rows), 16), dtype=np.int64)
        for i, r in enumerate(rows):
            t[i, : len(r)] = r
        t.view(np.float64)[:, 4:7] = 1.0
        return t

    ok = table((0, 2, 3, 4))
    hp = lambda t: t.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    edges = fn["mh_mask_edges"]
    assert edges(None, CH, F32, 1, 1, 3, 2, 3, 4, hp(ok), p, 1, 24, p, None) == -1 and b"mask_edges: null pointer" in dll.mh_last_error()
    assert edges(p, CH, F32, 1, 1, 2, 2, 3, 4, hp(ok), p, 1, 24, p, None) == -1 and b"mask_edges: bad argument" in dll.mh_last_error()        # rank 2 with D = 2
    assert edges(p, CH, F32, 1, 1, 3, 2, 3, 4, None, p, 1, 24, p, None) == -1 and b"null item table" in dll.mh_last_error()
    assert edges(p, CH, F32, 1, 1, 3, 2, 3, 4, hp(ok), p, 1, 23, p, None) == -1 and b"leaves the buffers" in dll.mh_last_error()
    assert edges(p, CH, F32, 1, 1, 3, 2, 3, 4, hp(table((0, 2, 3, 4, 0, 0, 0, 1))), p, 1, 24, p, None) == -1 and b"names batch item 1" in dll.mh_last_error()
    assert edges(p, CH, F32, 1, 1, 3, 2, 3, 4, hp(table((0, 2, 3, 4, 0, 0, 0, 0, 0, 0, 0, 1))), p, 1, 24, p, None) == -1 and b"leaves the volume" in dll.mh_last_error()
    edt = fn["mh_edt"]
    assert edt(None, U8, 1, hp(ok), p, 1, 24, 0, p, p, 0, None) == -1 and b"edt: null pointer" in dll.mh_last_error()
    assert edt(p, I64, 1, hp(ok), p, 1, 24, 0, p, p, 0, None) == -1 and b"uint8 or float32" in dll.mh_last_error()
    assert edt(p, U8, 1, hp(ok), p, 1, 24, 0, p, p, 1, None) == -1 and b"float32 (0) or float64 (3)" in dll.mh_last_error()
    assert edt(p, U8, 1, hp(table((0, 1, 1, 2049))), p, 1, 4096, 0, p, p, 0, None) == -1 and b"edt: item 0 has an extent of 2049" in dll.mh_last_error()
    assert edt(p, U8, 1, hp(table((0, 0, 3, 4))), p, 1, 24, 0, p, p, 0, None) == -1 and b"extent of 0" in dll.mh_last_error()
    assert edt(p, U8, 1, hp(ok), p, 0, 24, 0, p, p, 0, None) == -1 and b"0 items" in dll.mh_last_error()
    bad_sp = table((0, 2, 3, 4))
    bad_sp.view(np.float64)[0, 5] = 0.0
    assert edt(p, U8, 1, hp(bad_sp), p, 1, 24, 1, p, p, 0, None) == -1 and b"spacing" in dll.mh_last_error()
    rec = fn["mh_surface_records"]
    assert rec(None, p, 0, hp(ok), p, 1, 24, 0, p, p, None, 0, None) == -1 and b"surface_records: null pointer" in dll.mh_last_error()
    assert rec(p, p, 0, hp(ok), p, 1, 24, 0, p, None, None, 0, None) == -1 and b"no output" in dll.mh_last_error()
    assert rec(p, p, 0, hp(ok), p, 1, 24, 1, p, None, None, 0, None) == -1 and b"no output" in dll.mh_last_error()
    assert rec(p, p, 0, hp(table((0, 2, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1))), p, 1, 24, 0, p, p, None, 0, None) == -1 and b"surface_records: item 0 leaves the buffers" in dll.mh_last_error()
    assert rec(p, p, 0, hp(table((0, 2, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9))), p, 1, 24, 1, p, None, p, 8, None) == -1 and b"past the distances" in dll.mh_last_error()
