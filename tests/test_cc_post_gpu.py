"""-m gpu: the connected-component kernels (csrc/kernels/ccl.h) on the MI355X against the independent numpy partition of tests/cc_cases.py, and
KeepLargestConnectedComponent / FillHoles / LabelFilter against the reference's own outputs (tests/golden/cc_post.npz).  Every labelling shape runs
twice and has to give identical bits."""
import pytest

import cc_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("conn", (1, 2, 3))
def test_labels_and_records_vs_partition_3d(conn):
    print("masks compared", cc.case_labels_vs_partition(DEV, cc.GPU_SHAPE, conn, twice=True))


@pytest.mark.parametrize("conn", (1, 2))
def test_labels_and_records_vs_partition_2d(conn):
    print("masks compared", cc.case_labels_vs_partition(DEV, cc.GPU_SHAPE_2D, conn, twice=True))


def test_thin_volumes():
    print("volumes compared", cc.case_thin_volumes(DEV, cc.GPU_SHAPE) + cc.case_thin_volumes(DEV, cc.GPU_SHAPE_2D))


def test_rules_and_dtypes():
    print("labellings compared", cc.case_rules_and_dtypes(DEV, (13, 41, 150)))


@pytest.mark.parametrize("kind", ("fill", "filter", "keep"))
def test_transforms_vs_reference(kind):
    print("bit-equal golden results", cc.case_transforms_vs_golden(DEV, kind))


def test_reference_docstring_examples():
    cc.case_doc_examples(DEV)


def test_tie_rule():
    cc.case_tie_rule(DEV)


def test_dictionary_forms_and_meta_tensors():
    cc.case_dictionary_and_meta(DEV)


def test_inferer_labels_to_post_transforms():
    cc.case_inferer_labels(DEV)


def test_transforms_deterministic():
    cc.case_transforms_deterministic(DEV, cc.GPU_SHAPE)


def test_cc_api():
    cc.case_api(DEV)
