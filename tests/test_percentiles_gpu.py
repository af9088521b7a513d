"""-m gpu: the order-statistic kernel (csrc/kernels/select.h) on the MI355X against np.sort, and ScaleIntensityRangePercentiles /
ClipIntensityPercentiles against the reference's own outputs (tests/golden/percentiles.npz), bit for bit (tests/percentile_cases.py says why bit
identity is the rule in both regimes).  Every order-statistic case runs twice and has to give identical bits."""
import pytest

import percentile_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("n", pc.LENGTHS)
def test_order_statistics_vs_sort(n):
    checked = sum(pc.case_order_statistics(DEV, n, 1, k) for k in range(len(pc.KINDS)))
    checked += sum(pc.case_order_statistics(DEV, n, 3, k) for k in range(len(pc.KINDS)))
    print("order statistics compared", checked)


@pytest.mark.parametrize("n", (1, 65, pc.SHARE + 1, 70001))
def test_one_nan_makes_its_run_nan(n):
    pc.case_order_statistics(DEV, n, 1, 0, nan_run=0)
    pc.case_order_statistics(DEV, n, 3, 0, nan_run=1)


def test_order_statistics_argument_errors():
    pc.case_order_statistics_errors(DEV)


@pytest.mark.parametrize("which", (("doc", "const"), ("small",), ("n999983", "n1000000"), ("n1000001", "n1010000"), ("cw3",)), ids=lambda w: "+".join(w))
def test_transforms_vs_reference(which):
    print("bit-equal golden cases", pc.case_transforms_vs_golden(DEV, which))


def test_reference_docstring_examples():
    pc.case_doc_examples(DEV)


def test_nan_channel_and_determinism():
    pc.case_nan_and_determinism(DEV)


def test_percentiles_api():
    pc.case_api(DEV)
