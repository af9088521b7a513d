"""-m gpu: HausdorffDistanceMetric / SurfaceDistanceMetric / SurfaceDiceMetric, the mask-edge kernel and the exact Euclidean distance transform
(csrc/kernels/edt.h) on the MI355X: the EDT against brute force, the edges against scipy's (stored in the golden), the metrics against the real
reference's outputs (tests/golden/surface_metrics.npz)."""
import pytest

import surface_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_edt_vs_brute_force():
    sc.case_edt_vs_brute_force(DEV)


def test_edges_vs_scipy():
    print("edge maps compared", sc.case_edges_vs_scipy(DEV))


@pytest.mark.parametrize("part", range(sc.PARTS), ids=[sc._tag(s) for s in sc.SHAPES] + ["rest"])
def test_metrics_vs_reference(part):
    print("bit-equal golden results", sc.case_metrics_vs_reference(DEV, part))


def test_spaced_percentiles_vs_truth():
    sc.case_spaced_percentiles_vs_truth(DEV)


def test_edt_transform_vs_reference():
    sc.case_edt_transform_vs_reference(DEV)


def test_label_maps_equal_onehots():
    sc.case_label_maps_equal_onehots(DEV)


def test_inferer_labels_to_surface():
    sc.case_inferer_labels_to_surface(DEV)


def test_deterministic():
    sc.case_deterministic(DEV)


def test_surface_api():
    sc.case_surface_api(DEV)
