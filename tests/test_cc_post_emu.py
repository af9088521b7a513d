"""-m "not gpu": the connected-component kernels (csrc/kernels/ccl.h) and KeepLargestConnectedComponent / FillHoles / LabelFilter on the x86 SIMT
emulator -- the twins of tests/test_cc_post_gpu.py -- the independent partition of tests/cc_cases.py against scipy.ndimage.label, and the argument
checks of the new C-ABI entries on a GPU-less host."""
import ctypes

import pytest

import cc_cases as cc
from monai_amd import _lib

KEEP_PARTS = 4


def test_independent_partition_vs_scipy():
    pytest.importorskip("scipy")
    print("partitions compared", cc.case_canonical_vs_scipy())


@pytest.mark.parametrize("shape", cc.EMU_SHAPES, ids=str)
@pytest.mark.parametrize("conn", (1, 2, 3))
def test_labels_and_records_vs_partition_3d(emu, shape, conn):
    print("masks compared", cc.case_labels_vs_partition("cpu", shape, conn, twice=True))


@pytest.mark.parametrize("shape", cc.EMU_SHAPES_2D, ids=str)
@pytest.mark.parametrize("conn", (1, 2))
def test_labels_and_records_vs_partition_2d(emu, shape, conn):
    print("masks compared", cc.case_labels_vs_partition("cpu", shape, conn, twice=True))


def test_thin_volumes(emu):
    print("volumes compared", cc.case_thin_volumes("cpu", cc.EMU_SHAPES[0]) + cc.case_thin_volumes("cpu", cc.EMU_SHAPES_2D[1]))


def test_rules_and_dtypes(emu):
    print("labellings compared", cc.case_rules_and_dtypes("cpu", cc.EMU_SHAPES[1]))


@pytest.mark.parametrize("kind,part", [("fill", 0), ("filter", 0)] + [("keep", p) for p in range(KEEP_PARTS)])
def test_transforms_vs_reference(emu, kind, part):
    print("bit-equal golden results", cc.case_transforms_vs_golden("cpu", kind, part, KEEP_PARTS if kind == "keep" else 1))


def test_golden_is_covered():
    """the golden holds one output per case of cc_cases.golden_cases(), stacked per input, and the manifest: nothing else"""
    import numpy as np

    z = np.load(cc.GOLDEN)
    cases = cc.golden_cases()
    assert sorted(z.files) == sorted(["manifest"] + ["out|" + k for k in {c["inp"] for c in cases}])
    assert sum(z[k].shape[0] for k in z.files if k != "manifest") == len(cases) == 260
    assert {c["kind"] for c in cases} == {"fill", "filter", "keep"}


def test_reference_docstring_examples(emu):
    cc.case_doc_examples("cpu")


def test_tie_rule(emu):
    cc.case_tie_rule("cpu")


def test_dictionary_forms_and_meta_tensors(emu):
    cc.case_dictionary_and_meta("cpu")


def test_inferer_labels_to_post_transforms(emu):
    cc.case_inferer_labels("cpu")


def test_transforms_deterministic(emu):
    cc.case_transforms_deterministic("cpu", (9, 10, 11))


def test_cc_api(emu):
    cc.case_api("cpu")


def test_cpu_tensors_are_refused_outside_the_emulator(monkeypatch):
    """the product's own device check (no GPU needed to see it refuse)"""
    import torch

    import monai_amd.transforms as T
    from monai_amd._fallback import UnsupportedOnDevice
    from monai_amd.transforms.utils import fill_holes, get_largest_connected_component_mask

    monkeypatch.setenv("MONAI_AMD_NO_FALLTHROUGH", "1")
    x = torch.ones((1, 4, 5))
    for call in (lambda: T.KeepLargestConnectedComponent(applied_labels=[1])(x), lambda: T.FillHoles(applied_labels=[1])(x), lambda: T.LabelFilter([1])(x),
                 lambda: T.KeepLargestConnectedComponentd("a", applied_labels=[1])({"a": x}), lambda: T.FillHolesd("a", applied_labels=[1])({"a": x}),
                 lambda: T.LabelFilterd("a", [1])({"a": x}), lambda: fill_holes(x, [1]), lambda: get_largest_connected_component_mask(x[0])):
        with pytest.raises(UnsupportedOnDevice):
            call()


def test_cc_entries_need_no_gpu_for_their_argument_checks():
    """mh_cc_label / mh_cc_records / mh_cc_keep / mh_cc_fill / mh_cc_filter refuse null pointers, unknown dtypes and rules, a connectivity outside 1 .. rank,
    item rows that leave the buffers or the tensor and items over the voxel limit with MH_ERR_ARG and a message naming the entry BEFORE anything is launched"""
    import numpy as np

    if not __import__("os").path.isfile(_lib.LIB_PATH):
        from monai_amd import build

        build.build()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    dll.mh_last_error.restype = ctypes.c_char_p
    fn = {}
    for name in ("mh_cc_label", "mh_cc_records", "mh_cc_keep", "mh_cc_fill", "mh_cc_filter"):
        fn[name] = getattr(dll, name)
        fn[name].restype, fn[name].argtypes = _lib.SIGNATURES[name]
    p = 0x10000      # never dereferenced: every call below is refused before a launch
    F32, U8, I64, BOOL = 0, 1, 2, 3

    def table(*rows):
        t = np.zeros((len(rows), 48), dtype=np.int64)
        for i, r in enumerate(rows):
            t[i, : len(r)] = r
        return t

    hp = lambda t: t.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    err = dll.mh_last_error
    ok = table((0, 0, 2, 3, 4))
    label = fn["mh_cc_label"]
    assert label(None, U8, 24, 3, 1, hp(ok), p, 1, 24, p, None) == -1 and b"cc_label: null pointer" in err()
    assert label(p, U8, 24, 3, 1, hp(ok), p, 1, 24, None, None) == -1 and b"cc_label: null pointer" in err()
    assert label(p, 4, 24, 3, 1, hp(ok), p, 1, 24, p, None) == -1 and b"cc_label: unknown dtype 4" in err()
    assert label(p, U8, 24, 3, 1, None, p, 1, 24, p, None) == -1 and b"cc_label: null item table" in err()
    assert label(p, U8, 24, 3, 1, hp(ok), None, 1, 24, p, None) == -1 and b"cc_label: null item table" in err()
    assert label(p, U8, 24, 3, 0, hp(ok), p, 1, 24, p, None) == -1 and b"cc_label: connectivity 0 at rank 3" in err()
    assert label(p, U8, 24, 3, 4, hp(ok), p, 1, 24, p, None) == -1 and b"cc_label: connectivity 4" in err()
    assert label(p, U8, 12, 2, 3, hp(table((0, 0, 1, 3, 4))), p, 1, 12, p, None) == -1 and b"connectivity 3 at rank 2" in err()
    assert label(p, U8, 24, 2, 1, hp(ok), p, 1, 24, p, None) == -1 and b"leading extent of 2 at rank 2" in err()
    assert label(p, U8, 24, 1, 1, hp(ok), p, 1, 24, p, None) == -1 and b"cc_label: rank 1" in err()
    assert label(p, U8, 24, 3, 1, hp(ok), p, 1, 23, p, None) == -1 and b"cc_label: item 0 leaves the buffers" in err()
    assert label(p, U8, 23, 3, 1, hp(ok), p, 1, 24, p, None) == -1 and b"cc_label: item 0 leaves the tensor" in err()
    assert label(p, U8, 24, 3, 1, hp(table((1, 0, 2, 3, 4))), p, 1, 24, p, None) == -1 and b"leaves the buffers" in err()
    assert label(p, U8, 24, 3, 1, hp(table((0, -1, 2, 3, 4))), p, 1, 24, p, None) == -1 and b"leaves the tensor" in err()
    assert label(p, U8, 24, 3, 1, hp(table((0, 0, 2, 0, 4))), p, 1, 24, p, None) == -1 and b"extent of 0" in err()
    assert label(p, U8, 24, 3, 1, hp(table((0, 0, 2, 3, 4, 6))), p, 1, 24, p, None) == -1 and b"unknown rule 6" in err()
    assert label(p, U8, 24, 3, 1, hp(table((0, 0, 2, 3, 4, 3, 33))), p, 1, 24, p, None) == -1 and b"lists 33 labels" in err()
    assert label(p, U8, 24, 3, 1, hp(ok), p, 0, 24, p, None) == -1 and b"0 items" in err()
    big = 1 << 40
    assert label(p, U8, big, 3, 1, hp(table((0, 0, 1290, 1291, 1290))), p, 1, big, p, None) == -1 and b"more than 2147483646 voxels" in err()      # 2^31 - 1 < voxels
    assert label(p, U8, big, 3, 1, hp(table((0, 0, 1, 1, 2147483647))), p, 1, big, p, None) == -1 and b"extent of 2147483647" in err()
    rec = fn["mh_cc_records"]
    assert rec(None, 3, hp(ok), p, 1, 24, p, p, None) == -1 and b"cc_records: null pointer" in err()
    assert rec(p, 3, hp(ok), p, 1, 24, p, None, None) == -1 and b"cc_records: null pointer" in err()
    assert rec(p, 3, hp(ok), p, 1, 23, p, p, None) == -1 and b"cc_records: item 0 leaves the buffers" in err()
    assert rec(p, 4, hp(ok), p, 1, 24, p, p, None) == -1 and b"cc_records: rank 4" in err()
    keep = fn["mh_cc_keep"]
    assert keep(None, U8, 24, p, p, 1, 3, hp(ok), p, 1, 24, None) == -1 and b"cc_keep: null pointer" in err()
    assert keep(p, U8, 24, p, None, 1, 3, hp(ok), p, 1, 24, None) == -1 and b"cc_keep: null pointer" in err()
    assert keep(p, 7, 24, p, p, 1, 3, hp(ok), p, 1, 24, None) == -1 and b"cc_keep: unknown dtype 7" in err()
    assert keep(p, U8, 24, p, p, 0, 3, hp(ok), p, 1, 24, None) == -1 and b"cc_keep: 0 roots per item" in err()
    assert keep(p, U8, 24, p, p, 1025, 3, hp(ok), p, 1, 24, None) == -1 and b"1025 roots" in err()
    assert keep(p, I64, 24, p, p, 1, 3, hp(table((0, 1, 2, 3, 4))), p, 1, 24, None) == -1 and b"cc_keep: item 0 leaves the tensor" in err()
    fill = fn["mh_cc_fill"]
    assert fill(None, F32, 24, p, p, 3, hp(ok), p, 1, 24, None) == -1 and b"cc_fill: null pointer" in err()
    assert fill(p, F32, 24, p, None, 3, hp(ok), p, 1, 24, None) == -1 and b"cc_fill: null pointer" in err()
    assert fill(p, -1, 24, p, p, 3, hp(ok), p, 1, 24, None) == -1 and b"cc_fill: unknown dtype -1" in err()
    assert fill(p, BOOL, 24, p, p, 3, hp(table((0, 0, 2, 3, 4, 0, 0, 0, 0, 2))), p, 1, 24, None) == -1 and b"unknown fill mode 2" in err()
    assert fill(p, F32, 24, p, p, 3, hp(table((0, 0, 2, 3, 5))), p, 1, 24, None) == -1 and b"cc_fill: item 0 leaves the buffers" in err()
    filt = fn["mh_cc_filter"]
    labs = (ctypes.c_double * 33)()
    assert filt(None, p, F32, 8, labs, 1, None) == -1 and b"cc_filter: null pointer" in err()
    assert filt(p, p, F32, 8, None, 1, None) == -1 and b"cc_filter: null pointer" in err()
    assert filt(p, p, 9, 8, labs, 1, None) == -1 and b"cc_filter: unknown dtype 9" in err()
    assert filt(p, p, F32, 0, labs, 1, None) == -1 and b"bad element count" in err()
    assert filt(p, p, F32, 8, labs, 33, None) == -1 and b"33 labels" in err()
