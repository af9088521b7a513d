"""-m "not gpu": DiceMetric / MeanIoU / ConfusionMatrixMetric and the one-pass overlap kernel (csrc/kernels/metrics.h) on the x86 SIMT emulator -- the twins
of tests/test_metrics_gpu.py -- and the argument checks of the two C-ABI entries on a GPU-less host."""
import ctypes

import pytest

import metrics_cases as mc
from monai_amd import _lib


def test_overlap_sums_exact(emu):
    print("records checked", mc.case_overlap_sums_exact("cpu"))


@pytest.mark.heavy_emu
def test_overlap_sums_beyond_fp32(emu):
    mc.case_overlap_sums_beyond_fp32("cpu")


def test_overlap_sums_deterministic(emu):
    mc.case_overlap_sums_deterministic("cpu")


def test_dice_iou_confusion_vs_reference(emu):
    print("golden results compared", mc.case_dice_iou_confusion_vs_reference("cpu"))


def test_metrics_api(emu):
    mc.case_metrics_api("cpu", device_is_real=False)      # inside the emulator context a CPU tensor stands for a device tensor


def test_cpu_tensors_are_refused_outside_the_emulator():
    """the product's own device check (no GPU needed to see it refuse)"""
    import torch

    import monai_amd.metrics as m
    from monai_amd._fallback import UnsupportedOnDevice

    x = torch.zeros((1, 2, 3, 3))
    for call in (lambda: m.compute_dice(x, x), lambda: m.MeanIoU()(x, x), lambda: m.ConfusionMatrixMetric()(x, x), lambda: m.is_binary_tensor(x, "x")):
        with pytest.raises(UnsupportedOnDevice):
            call()


def test_inferer_labels_to_dice(emu):
    mc.case_inferer_labels_to_dice("cpu")


def test_overlap_sums_entries_need_no_gpu_for_their_argument_checks():
    """mh_overlap_sums_workspace_bytes is host arithmetic; mh_overlap_sums refuses null pointers, K < 1, n < 0 and unknown / unsupported form and dtype codes with
    MH_ERR_ARG and a message naming the entry BEFORE anything is launched"""
    if not __import__("os").path.isfile(_lib.LIB_PATH):
        from monai_amd import build

        build.build()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    dll.mh_last_error.restype = ctypes.c_char_p
    ws_bytes, launch = dll.mh_overlap_sums_workspace_bytes, dll.mh_overlap_sums
    ws_bytes.restype, ws_bytes.argtypes = _lib.SIGNATURES["mh_overlap_sums_workspace_bytes"]
    launch.restype, launch.argtypes = _lib.SIGNATURES["mh_overlap_sums"]
    record = 8 * 8      # eight fp64 slots
    assert ws_bytes(1, 5, 0) == 5 * record and ws_bytes(1, 5, 1) == 5 * record and ws_bytes(2, 3, 1024) == 2 * 2 * 3 * record
    assert ws_bytes(1, 5, 512 ** 3) == 2048 * 5 * record      # the grid is sized from the CU count, not from n: at most 2048 block records
    assert ws_bytes(0, 5, 10) == -1 and b"overlap_sums_workspace_bytes" in dll.mh_last_error()
    assert ws_bytes(1, 0, 10) == -1 and ws_bytes(1, 5, -1) == -1
    p = 0x10000      # never dereferenced: every call below is refused before a launch
    CH, LB, F32, U8, I64 = 0, 1, 0, 1, 2
    assert launch(None, LB, U8, p, LB, U8, 1, 5, 100, p, p, None) == -1 and b"overlap_sums: null pointer" in dll.mh_last_error()
    for args in ((p, LB, U8, None, LB, U8, 1, 5, 100, p, p), (p, LB, U8, p, LB, U8, 1, 5, 100, None, p), (p, LB, U8, p, LB, U8, 1, 5, 100, p, None)):
        assert launch(*args, None) == -1 and b"null pointer" in dll.mh_last_error()
    assert launch(p, LB, U8, p, LB, U8, 1, 0, 100, p, p, None) == -1 and b"overlap_sums: bad argument" in dll.mh_last_error()
    assert launch(p, LB, U8, p, LB, U8, 0, 5, 100, p, p, None) == -1 and launch(p, LB, U8, p, LB, U8, 1, 5, -1, p, p, None) == -1
    assert launch(p, LB, 3, p, LB, U8, 1, 5, 100, p, p, None) == -1 and b"overlap_sums: unknown dtype 3 of the prediction" in dll.mh_last_error()
    assert launch(p, LB, U8, p, LB, -1, 1, 5, 100, p, p, None) == -1 and b"of the truth" in dll.mh_last_error()
    assert launch(p, 2, U8, p, LB, U8, 1, 5, 100, p, p, None) == -1 and b"overlap_sums: unknown form 2" in dll.mh_last_error()
    assert launch(p, CH, I64, p, LB, U8, 1, 5, 100, p, p, None) == -1 and b"channel-form prediction" in dll.mh_last_error()
    assert launch(p, CH, F32, p, CH, I64, 1, 5, 100, p, p, None) == -1 and b"channel-form truth" in dll.mh_last_error()
