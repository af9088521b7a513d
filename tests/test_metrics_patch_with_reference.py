"""Drop-in check of the metrics against the real MONAI (only where /root/reference exists): after ``monai_amd.patch.install()`` a bundle's
``"_target_": "DiceMetric"`` / ``"MeanIoU"`` / ``"ConfusionMatrixMetric"`` resolve to the MI355X classes, the emulator-backed classes reproduce the displaced
reference objects, a CPU tensor falls through to the reference function while the values still land in the product object's buffers, and uninstall
restores everything."""
import os
import sys

import pytest
import torch

REF = "/root/reference"
pytestmark = [pytest.mark.fallthrough, pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "monai")), reason="reference MONAI not available here")]


@pytest.fixture()
def monai_ref():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import monai

    yield monai
    import monai_amd.patch as patch

    patch.uninstall()
    sys.path.remove(REF)


def _inputs():
    gen = torch.Generator().manual_seed(4700)
    lp, ly = torch.randint(0, 3, (2, 1, 5, 6, 7), generator=gen), torch.randint(0, 3, (2, 1, 5, 6, 7), generator=gen)
    oh = lambda t: torch.zeros((2, 3, 5, 6, 7)).scatter_(1, t, 1.0)      # noqa: E731
    return oh(lp), oh(ly)


def test_bundle_targets_resolve_and_cpu_tensors_fall_through(monai_ref, monkeypatch):
    import monai.metrics as ref_metrics
    import monai_amd.metrics as ours
    import monai_amd.patch as patch
    from monai.bundle import ConfigParser
    from monai_amd import _fallback

    monkeypatch.delenv("MONAI_AMD_NO_FALLTHROUGH", raising=False)
    ref_classes = {n: getattr(ref_metrics, n) for n in ("DiceMetric", "MeanIoU", "ConfusionMatrixMetric", "DiceHelper")}
    ref_functions = {n: getattr(ref_metrics, n) for n in ("compute_dice", "compute_iou", "get_confusion_matrix", "do_metric_reduction", "is_binary_tensor")}
    p, y = _inputs()
    expected = {"DiceMetric": ref_classes["DiceMetric"](reduction="mean_batch"), "MeanIoU": ref_classes["MeanIoU"](reduction="mean_batch"),
                "ConfusionMatrixMetric": ref_classes["ConfusionMatrixMetric"](metric_name="f1 score", reduction="mean_batch")}
    for m in expected.values():
        m(p, y)
    done = patch.install()
    for name in list(ref_classes) + list(ref_functions):
        assert getattr(ref_metrics, name) is getattr(ours, name), name
    assert "monai.metrics.meandice.DiceMetric" in done and "monai.metrics.utils.is_binary_tensor" in done
    cfg = {"DiceMetric": {"_target_": "DiceMetric", "reduction": "mean_batch"}, "MeanIoU": {"_target_": "MeanIoU", "reduction": "mean_batch"},
           "ConfusionMatrixMetric": {"_target_": "ConfusionMatrixMetric", "metric_name": "f1 score", "reduction": "mean_batch"}}
    parser = ConfigParser(cfg)
    before = len(_fallback.fell_through())
    for name, ref_obj in expected.items():
        obj = parser.get_parsed_content(name)
        assert isinstance(obj, getattr(ours, name)) and type(obj).__module__.startswith("monai.metrics."), name
        obj(p, y)                                  # CPU tensors: the volume pass goes to the reference function, the values into THIS object's buffer
        got, exp = obj.aggregate(), ref_obj.aggregate()
        got, exp = (got[0], exp[0]) if isinstance(got, list) else (got, exp)
        assert torch.equal(got, exp), name
    fell = [c for c, _ in _fallback.fell_through()[before:]]
    assert any("DiceHelper" in c for c in fell) and "compute_iou" in fell and "get_confusion_matrix" in fell, fell
    assert isinstance(ours.DiceHelper(activate=True, threshold=True), ref_classes["DiceHelper"])      # a named unsupported configuration becomes the reference object
    patch.uninstall()
    for name, obj in {**ref_classes, **ref_functions}.items():
        assert getattr(ref_metrics, name) is obj, name


def test_patched_classes_on_the_emulator_match_the_displaced_reference(monai_ref, emu):
    import monai.metrics as ref_metrics
    import monai_amd.patch as patch
    from monai_amd import _fallback

    p, y = _inputs()
    ref = ref_metrics.DiceMetric(include_background=False, reduction="mean_channel", get_not_nans=True)
    ref(p, y)
    patch.install()
    before = len(_fallback.fell_through())
    got = ref_metrics.DiceMetric(include_background=False, reduction="mean_channel", get_not_nans=True)      # the product class under the reference's name
    got(p, y)
    assert len(_fallback.fell_through()) == before      # served by the kernel (the emulator stands in for the device), nothing fell through
    for a, b in zip(got.aggregate(), ref.aggregate()):
        assert torch.equal(a, b)
