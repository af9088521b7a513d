"""DiceMetric / MeanIoU / ConfusionMatrixMetric and the overlap kernel under them: cases shared by the golden generator (real reference, CPU),
the emulator tests and the MI355X tests."""
import os
import warnings

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the smallest shapes at which the kernel can go wrong: one voxel; odd n (misaligned rows for C = 3); 1-D and 2-D; a workgroup's first stride with head
# and tail; many workgroups and, on the emulator's smaller grid, more than one grid-stride trip
SPATIAL = [(1, 1, 1), (3, 5, 7), (2,), (4, 4), (17, 16, 15), (64, 64, 65)]
REDUCTIONS = ("none", "mean", "sum", "mean_batch", "sum_batch", "mean_channel", "sum_channel")
CM_NAMES = ("sensitivity", "recall", "hit_rate", "true_positive_rate", "tpr", "specificity", "selectivity", "true_negative_rate", "tnr", "precision",
            "positive_predictive_value", "ppv", "negative_predictive_value", "npv", "miss_rate", "false_negative_rate", "fnr", "fall_out", "false_positive_rate",
            "fpr", "false_discovery_rate", "fdr", "false_omission_rate", "for", "prevalence_threshold", "pt", "threat_score", "critical_success_index", "ts",
            "csi", "accuracy", "acc", "balanced_accuracy", "ba", "f1_score", "f1", "matthews_correlation_coefficient", "mcc", "fowlkes_mallows_index", "fm",
            "informedness", "bookmaker_informedness", "bm", "youden_index", "youden", "markedness", "deltap", "mk", "false omission rate", "F1 Score")


# ------------------------------------------------------------------------------------------------- the overlap record, exact
def expected_record(pred: np.ndarray, truth: np.ndarray, k: int) -> np.ndarray:
    """the [B, K, 8] record in numpy float64 / int64, straight from the definition of the slots (include/monai_amd.h)"""
    b = pred.shape[0]

    def side(t, c):
        if t.shape[1] == k:      # channel form: the stored value
            return t[:, c].reshape(b, -1).astype(np.float32)
        with np.errstate(invalid="ignore"):
            lab = t[:, 0].reshape(b, -1)
            idx = np.where(np.isfinite(lab), np.trunc(np.nan_to_num(lab.astype(np.float64))), -1.0) if lab.dtype.kind == "f" else lab.astype(np.float64)
        return (idx == c).astype(np.float32)

    out = np.zeros((b, k, 8), np.float64)
    for c in range(k):
        p, y = side(pred, c), side(truth, c)
        nz = p != 0                                       # NaN != 0
        with np.errstate(invalid="ignore"):
            out[:, c, 0] = np.where(nz, y.astype(np.float64), 0.0).sum(1)
            out[:, c, 1] = nz.sum(1)
            out[:, c, 2] = y.astype(np.float64).sum(1)
            out[:, c, 3] = (y * p).astype(np.float64).sum(1)      # fp32 product, fp64 sum
            out[:, c, 4] = p.astype(np.float64).sum(1)
            s = p + y
            out[:, c, 5] = (s == 2).sum(1)
            out[:, c, 6] = (s == 0).sum(1)
            out[:, c, 7] = ((p != 0) & (p != 1)).sum(1) + ((y != 0) & (y != 1)).sum(1)
    return out


def _labels(gen, b, k, spatial, dtype):
    lab = torch.randint(0, k, (b, 1) + tuple(spatial), generator=gen)
    return lab.to(dtype)


def _onehot(lab, k, dtype):
    oh = torch.zeros((lab.shape[0], k) + tuple(lab.shape[2:]), dtype=torch.float32)
    oh.scatter_(1, lab.long().clamp(0, k - 1), 1.0)
    return oh.to(dtype)


def _check_record(device, pred, truth, k, what):
    from monai_amd import ops

    got = ops.overlap_sums(pred.to(device), truth.to(device), k)
    assert got.dtype == torch.float64 and tuple(got.shape) == (pred.shape[0], k, 8), (what, got.dtype, got.shape)
    np.testing.assert_array_equal(got.cpu().numpy(), expected_record(pred.numpy(), truth.numpy(), k), err_msg=what)


LABEL_DTYPES = (torch.float32, torch.uint8, torch.int64)
CHANNEL_DTYPES = (torch.float32, torch.uint8, torch.bool)


def case_overlap_sums_exact(device):
    """every form combination x every accepted dtype x the shape list, B in {1, 2}, K in {1, 2, 5, 11}; then the planted cases"""
    gen = torch.Generator().manual_seed(4100)
    n_checked = 0
    for si, spatial in enumerate(SPATIAL):
        big = int(np.prod(spatial)) > 5000
        for k in (1, 2, 5, 11):
            b = 1 + (si + k) % 2
            lp, ly = _labels(gen, b, k, spatial, torch.int64), _labels(gen, b, k, spatial, torch.int64)
            # the large shape walks the dtype pairs diagonally (every dtype of every form still occurs), the small ones take the full product
            pairs_ll = [(dp, dy) for dp in LABEL_DTYPES for dy in LABEL_DTYPES]
            pairs_cc = [(dp, dy) for dp in CHANNEL_DTYPES for dy in CHANNEL_DTYPES]
            pairs_cl = [(dp, dy) for dp in CHANNEL_DTYPES for dy in LABEL_DTYPES]
            if big:
                pairs_ll, pairs_cc, pairs_cl = pairs_ll[::4], pairs_cc[::4], pairs_cl[::4]
            if k > 1:      # with one class a single channel IS the channel form
                for dp, dy in pairs_ll:
                    _check_record(device, lp.to(dp), ly.to(dy), k, f"labels {dp} x labels {dy} {spatial} K={k}")
                for dp, dy in pairs_cl:
                    _check_record(device, _onehot(lp, k, dp), ly.to(dy), k, f"channels {dp} x labels {dy} {spatial} K={k}")
                    _check_record(device, lp.to(dy), _onehot(ly, k, dp), k, f"labels {dy} x channels {dp} {spatial} K={k}")
                    n_checked += 2
            for dp, dy in pairs_cc:
                _check_record(device, _onehot(lp, k, dp), _onehot(ly, k, dy), k, f"channels {dp} x channels {dy} {spatial} K={k}")
            n_checked += len(pairs_ll) + len(pairs_cc)
    # soft float values on both sides, odd n and C = 3: misaligned rows.  Multiples of 1 / 256: products and sums are exact in fp64, so the expected
    # record does not depend on the order of summation
    soft_p, soft_y = (torch.floor(torch.rand((2, 3, 3, 5, 7), generator=gen) * 256) / 256 for _ in range(2))
    _check_record(device, soft_p, soft_y, 3, "soft x soft")
    # planted: class 3 absent from both sides, class 4 only in the prediction, labels >= K (no class), negative and NaN labels
    lp = torch.tensor([0, 1, 2, 4, 4, 1, 7, 0, 2, 9, 1, 1, 0, 2, 2, 4, 0, 1], dtype=torch.float32).reshape(1, 1, 2, 3, 3)
    ly = torch.tensor([0, 1, 1, 2, 0, 1, 2, 5, 2, 0, 1, 2, 0, 2, 1, 0, 6, 1], dtype=torch.float32).reshape(1, 1, 2, 3, 3)
    for dt in LABEL_DTYPES:
        _check_record(device, lp.to(dt), ly.to(dt), 5, f"planted labels {dt}")
    lf = lp.clone()
    lf[0, 0, 0, 0, 0], lf[0, 0, 0, 0, 1], lf[0, 0, 0, 0, 2], lf[0, 0, 1, 0, 0] = float("nan"), -0.5, 1.75, -3.0      # no class / class 0 (.long() truncates) / class 1 / no class
    _check_record(device, lf, ly, 5, "planted float labels: NaN, -0.5, 1.75, -3")
    # planted: a NaN in a channel-form prediction (non-zero for slots 0 / 1, NaN in slots 3 / 4) and non-binary values (slot 7)
    cp = _onehot(lp.clamp(0, 4), 5, torch.float32)
    cp[0, 1, 0, 1, 1] = float("nan")
    cp[0, 2, 1, 2, 2], cp[0, 0, 0, 0, 0] = 0.25, 2.0
    cy = _onehot(ly.clamp(0, 4), 5, torch.float32)
    cy[0, 4, 1, 1, 1] = 0.5
    _check_record(device, cp, cy, 5, "planted NaN / non-binary channels")
    _check_record(device, cp, ly, 5, "planted NaN / non-binary channels x labels")
    cu = _onehot(lp.clamp(0, 4), 5, torch.uint8)
    cu[0, 3, 0, 0, 0] = 7                                 # a uint8 channel value that is not binary
    _check_record(device, cu, cy, 5, "planted non-binary uint8 channels")
    return n_checked


def case_overlap_sums_beyond_fp32(device):
    """n = 2^24 + 3 voxels of class 1 on both sides: every count of class 1 is 16777219, which float32 accumulation cannot hold (the next float32 is 16777220)"""
    from monai_amd import ops

    n = (1 << 24) + 3
    lab = torch.ones((1, 1, n), dtype=torch.uint8, device=device)
    rec = ops.overlap_sums(lab, lab, 2).cpu().numpy()
    assert int(np.float32(n)) == n + 1      # float32 cannot hold the count
    np.testing.assert_array_equal(rec[0, 1], np.array([n, n, n, n, n, n, 0, 0], np.float64))
    np.testing.assert_array_equal(rec[0, 0], np.array([0, 0, 0, 0, 0, 0, n, 0], np.float64))


def case_overlap_sums_deterministic(device):
    """two launches over the same soft float truth: bitwise equal records (no atomics, a fixed summation tree)"""
    from monai_amd import ops

    gen = torch.Generator().manual_seed(4200)
    pred = torch.randint(0, 5, (2, 1, 64, 64, 65), generator=gen).to(torch.uint8).to(device)
    truth = torch.rand((2, 5, 64, 64, 65), generator=gen).to(device)
    a, b = ops.overlap_sums(pred, truth, 5), ops.overlap_sums(pred, truth, 5)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    soft = torch.rand((2, 5, 64, 64, 65), generator=gen).to(device)
    a, b = ops.overlap_sums(soft, truth, 5), ops.overlap_sums(soft, truth, 5)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert float(a[..., 3].min()) > 0


# ------------------------------------------------------------------------------------------------- the metrics against the reference
def _inputs():
    """name -> (y_pred, y) CPU tensors; binary / label inputs ("exact") and soft float truths ("soft")"""
    gen = torch.Generator().manual_seed(4300)
    d = {}
    for tag, b, k, spatial in (("a", 2, 5, (3, 5, 7)), ("b", 1, 2, (17, 16, 15)), ("c", 2, 3, (4, 4)), ("d", 2, 11, (9, 6))):
        lp, ly = _labels(gen, b, k, spatial, torch.int64), _labels(gen, b, k, spatial, torch.int64)
        if tag == "a":
            ly[0][ly[0] == 3] = 2             # class 3 absent from the truth of item 0 (present in the prediction): NaN / 0 under the empty rules
            lp[1][lp[1] == 4] = 0
            ly[1][ly[1] == 4] = 0             # class 4 absent from both sides of item 1: NaN / 1
        d[tag] = (lp, ly, k)
    return d


def run_all(mod, device):
    """every golden result: `mod` is monai.metrics (generator) or monai_amd.metrics (tests).  Keys starting with "exact_" must agree bit for bit."""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tag, (lp, ly, k) in _inputs().items():
            ohp, ohy = _onehot(lp, k, torch.float32).to(device), _onehot(ly, k, torch.float32).to(device)
            lpd, lyd = lp.to(device), ly.to(device)
            for bg in (True, False):
                for ie in (True, False):
                    s = f"{tag}_bg{int(bg)}_ie{int(ie)}"
                    out[f"exact_dice_{s}"] = mod.compute_dice(ohp, ohy, include_background=bg, ignore_empty=ie)
                    out[f"exact_dice_ll_{s}"] = mod.compute_dice(lpd, lyd, include_background=bg, ignore_empty=ie, num_classes=k)
                    out[f"exact_dice_lc_{s}"] = mod.compute_dice(lpd.float(), ohy, include_background=bg, ignore_empty=ie, num_classes=k)
                    out[f"exact_dice_cl_{s}"] = mod.compute_dice(ohp, lyd.to(torch.uint8), include_background=bg, ignore_empty=ie, num_classes=k)
                    out[f"exact_iou_{s}"] = mod.compute_iou(ohp, ohy, include_background=bg, ignore_empty=ie)
                out[f"exact_cm_{tag}_bg{int(bg)}"] = mod.get_confusion_matrix(ohp, ohy, include_background=bg)
            # DiceHelper: threshold on scores (0.5 itself is NOT above the threshold) and argmax over scores with ties
            g2 = torch.Generator().manual_seed(4400 + k)
            scores = torch.rand(ohp.shape, generator=g2)
            scores.view(-1)[::7] = 0.5
            flat = scores.view(scores.shape[0], k, -1)
            flat[:, 0, ::5] = flat[:, k - 1, ::5]      # ties: the first index wins
            scores = scores.to(device)
            for red in ("none", "mean_batch", "mean"):
                f, nn = mod.DiceHelper(threshold=True, reduction=red, get_not_nans=True)(scores, ohy)
                out[f"exact_helper_thr_{tag}_{red}"], out[f"exact_helper_thr_nn_{tag}_{red}"] = f, nn
                f, nn = mod.DiceHelper(apply_argmax=True, include_background=True, reduction=red, get_not_nans=True, ignore_empty=False)(scores, lyd)
                out[f"exact_helper_argmax_{tag}_{red}"], out[f"exact_helper_argmax_nn_{tag}_{red}"] = f, nn
            out[f"exact_helper_bin_{tag}"] = mod.DiceHelper(threshold=True, get_not_nans=False, reduction="none")(scores[:, :1].contiguous(), (lyd == 1).float())
            cm = out[f"exact_cm_{tag}_bg1"]
            for name in CM_NAMES:
                out[f"exact_cmm_{tag}_{name.replace(' ', '-')}"] = mod.compute_confusion_matrix_metric(name, cm)
            # the three classes: two calls (a batch tensor, then a list of channel-first tensors), aggregate under every reduction, reset
            for red in REDUCTIONS:
                dm = mod.DiceMetric(include_background=(red != "sum"), reduction=red, get_not_nans=True, num_classes=k)
                r1 = dm(lpd, lyd)
                r2 = dm([t for t in ohp], [t for t in ohy])
                f, nn = dm.aggregate()
                out[f"exact_DiceMetric_{tag}_{red}"], out[f"exact_DiceMetric_nn_{tag}_{red}"] = f, nn
                out[f"exact_DiceMetric_calls_{tag}_{red}"] = torch.cat([r1, r2], 0)
                out[f"exact_DiceMetric_other_{tag}_{red}"] = dm.aggregate(reduction="mean_channel")[0]
                dm.reset()
                assert dm.get_buffer() is None and len(dm) == 0
                im = mod.MeanIoU(include_background=(red != "mean"), reduction=red, get_not_nans=True, ignore_empty=(red != "sum_batch"))
                im(ohp, ohy)
                im(ohy, ohy)
                f, nn = im.aggregate()
                out[f"exact_MeanIoU_{tag}_{red}"], out[f"exact_MeanIoU_nn_{tag}_{red}"] = f, nn
                for sample in (False, True):
                    cmm = mod.ConfusionMatrixMetric(include_background=True, metric_name=["f1 score", "tpr", "mcc"], compute_sample=sample, reduction=red, get_not_nans=True)
                    cmm(ohp, ohy)
                    cmm(ohy, ohp)
                    for i, (f, nn) in enumerate(cmm.aggregate()):
                        out[f"exact_CMM_{tag}_{red}_s{int(sample)}_{i}"], out[f"exact_CMM_nn_{tag}_{red}_s{int(sample)}_{i}"] = f, nn
            lab = mod.DiceMetric(reduction="mean_batch", return_with_label=True, num_classes=k)
            lab(lpd, lyd)
            out[f"exact_labels_bool_{tag}"] = _label_dict(lab.aggregate(), [f"label_{i}" for i in range(k)])
            lab = mod.DiceMetric(include_background=False, reduction="mean_batch", return_with_label=True, num_classes=k)
            lab(lpd, lyd)
            out[f"exact_labels_nobg_{tag}"] = _label_dict(lab.aggregate(), [f"label_{i}" for i in range(1, k)])
            names = [f"organ{i}" for i in range(k)]
            lab = mod.DiceMetric(reduction="mean_batch", return_with_label=names, num_classes=k)
            lab(lpd, lyd)
            out[f"exact_labels_list_{tag}"] = _label_dict(lab.aggregate(), names)
            # classification: [B, C] one value per class
            cls_p, cls_y = ohp.reshape(ohp.shape[0], k, -1)[:, :, 0].contiguous(), ohy.reshape(ohy.shape[0], k, -1)[:, :, 0].contiguous()
            out[f"exact_cm_classification_{tag}"] = mod.get_confusion_matrix(cls_p, cls_y)
    return {name: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for name, v in out.items()}


def _label_dict(d, keys):
    assert isinstance(d, dict) and list(d) == list(keys), (list(d), keys)
    return np.array([d[key] for key in keys], np.float64)


def soft_inputs():
    gen = torch.Generator().manual_seed(4500)
    pred = _onehot(_labels(gen, 2, 4, (17, 16, 15), torch.int64), 4, torch.float32)
    truth = torch.rand((2, 4, 17, 16, 15), generator=gen)      # soft labels: every sum is a genuine floating-point sum
    return pred, truth


def run_soft(mod, device):
    pred, truth = soft_inputs()
    pred, truth = pred.to(device), truth.to(device)
    out = {"soft_dice": mod.compute_dice(pred, truth), "soft_iou": mod.compute_iou(pred, truth), "soft_cm_p": mod.get_confusion_matrix(pred, truth)[..., 0:4:3].sum(-1)}
    return {name: v.detach().cpu().numpy() for name, v in out.items()}


def soft_truth():
    """the same three results in numpy float64: what both implementations approximate"""
    pred, truth = (t.numpy().astype(np.float64).reshape(2, 4, -1) for t in soft_inputs())
    inter, y_o, p_o = (pred * truth).sum(-1), truth.sum(-1), pred.sum(-1)
    return {"soft_dice": 2.0 * inter / (y_o + p_o), "soft_iou": inter / (y_o + p_o - inter), "soft_cm_p": y_o}      # tp + fn = the truth's sum


def case_dice_iou_confusion_vs_reference(device):
    """compute_dice / DiceHelper / compute_iou / get_confusion_matrix / every confusion-matrix metric name / the three classes against the real reference
    (tests/golden/make_golden_metrics.py).  Binary and label inputs: bit-equal (every count is below 2^24, so the reference's float32 quotients are the
    correctly rounded ones).  Soft float truth: against a float64 numpy truth t, |ours - t| <= 2^-23 |t| and |ours - ref| <= |ref - t| + 2^-23 |t| -- the
    reference's own distance from the truth is part of the golden, the bound never comes from the code under test."""
    import monai_amd.metrics as ours

    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    got = run_all(ours, device)
    assert set(got) == {n for n in g.files if n.startswith("exact_")}
    for name, v in got.items():
        exp = g[name]
        assert v.shape == exp.shape and v.dtype == exp.dtype, (name, v.shape, exp.shape, v.dtype, exp.dtype)
        np.testing.assert_array_equal(v, exp, err_msg=name)
    truth = soft_truth()
    for name, v in run_soft(ours, device).items():
        t, ref, ref_err = truth[name], g[name], g[name + "_ref_err"]
        assert v.dtype == np.float32 and v.shape == t.shape, (name, v.dtype, v.shape)
        np.testing.assert_array_equal(ref_err, np.abs(ref.astype(np.float64) - t), err_msg=name)      # the stored distance is the reference's own
        err, eps = np.abs(v.astype(np.float64) - t), 2.0 ** -23 * np.abs(t)
        print(name, "max |ours - t| / |t| =", float((err / np.abs(t)).max()), " max |ref - t| / |t| =", float((ref_err / np.abs(t)).max()))
        assert (err <= eps).all(), (name, err, eps)
        assert (np.abs(v.astype(np.float64) - ref.astype(np.float64)) <= ref_err + eps).all(), name
    return len(got)


def case_metrics_api(device, device_is_real=True):
    """the reference's errors and warnings; the explicit errors of what is not on the HIP path"""
    import pytest

    import monai_amd.metrics as m
    from monai_amd._fallback import UnsupportedOnDevice

    x = torch.zeros((2, 3, 4, 4), device=device)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        m.DiceMetric()(x[:, :, 0, 0], x[:, :, 0, 0])
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        m.MeanIoU()(x[:, :, 0, 0], x[:, :, 0, 0])
    with pytest.raises(ValueError, match="at least two dimensions"):
        m.ConfusionMatrixMetric()(x[:, 0, 0, 0], x[:, 0, 0, 0])
    with pytest.raises(ValueError, match="should have same shapes"):
        m.compute_iou(x, x[:, :, :2].contiguous())
    with pytest.raises(ValueError, match="should have same shapes"):
        m.get_confusion_matrix(x, x[:, :2].contiguous())
    with pytest.raises(NotImplementedError, match="the metric is not implemented"):
        m.compute_confusion_matrix_metric("dice", torch.zeros(2, 3, 4))
    with pytest.raises(NotImplementedError):
        m.check_confusion_matrix_metric_name("true positive")
    assert m.check_confusion_matrix_metric_name("False Omission Rate") == "for"
    with pytest.raises(ValueError, match="last dimension of confusion_matrix should be 4"):
        m.compute_confusion_matrix_metric("f1", torch.zeros(2, 3, 5))
    for cls in (m.DiceMetric, m.MeanIoU, m.ConfusionMatrixMetric):
        with pytest.raises(ValueError, match="the data to aggregate must be PyTorch Tensor"):
            cls().aggregate()
    with pytest.raises(ValueError, match="Unsupported reduction"):
        m.do_metric_reduction(torch.zeros(2, 3), "median")
    with pytest.raises(ValueError, match="must be a list/tuple"):
        m.DiceMetric()(3.0, 4.0)
    with pytest.raises(ValueError, match="must be of type PyTorch Tensor"):
        m.is_binary_tensor([0, 1], "y")
    # the binarized-tensor warning: the helper and the two classes that promise binarized inputs
    soft = torch.full((1, 2, 3, 3), 0.5, device=device)
    binary = (torch.arange(18, device=device).reshape(1, 2, 3, 3) % 2).float()
    with pytest.warns(UserWarning, match="y_pred should be a binarized tensor"):
        m.is_binary_tensor(soft, "y_pred")
    with pytest.warns(UserWarning, match="should be a binarized tensor"):
        m.MeanIoU()(soft, binary)
    with pytest.warns(UserWarning, match="should be a binarized tensor"):
        m.ConfusionMatrixMetric()(binary, soft)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.is_binary_tensor(binary, "y")
        m.is_binary_tensor(binary.bool(), "y")
        m.MeanIoU()(binary, binary)
        m.ConfusionMatrixMetric()(binary, binary)
        m.compute_iou(soft, binary)                      # the functions stay silent, as the reference's
    with pytest.warns(UserWarning, match="compute_sample should be False"):
        cm = m.ConfusionMatrixMetric(compute_sample=True)
        cm(binary[:, :, 0, 0], binary[:, :, 0, 0])
    assert cm.compute_sample is False
    # named unsupported configurations: the explicit error (the test environment pins MONAI_AMD_NO_FALLTHROUGH=1)
    with pytest.raises(NotImplementedError, match="activate=True"):
        m.DiceHelper(activate=True)
    with pytest.raises(NotImplementedError):
        m.compute_dice(x[:, :2].contiguous(), x, num_classes=3)      # two channels for three classes
    with pytest.raises(UnsupportedOnDevice):
        m.compute_dice(x.double(), x.double())
    with pytest.raises(UnsupportedOnDevice):
        m.compute_iou(x.to(torch.int32), x.to(torch.int32))
    if device_is_real:
        with pytest.raises(UnsupportedOnDevice):
            m.compute_dice(x.cpu(), x.cpu())
        with pytest.raises(UnsupportedOnDevice):
            m.MeanIoU()(x.cpu(), x.cpu())
    # API shell: names and attributes of the reference's classes
    dm = m.DiceMetric(include_background=False, reduction="sum", get_not_nans=True, ignore_empty=False, num_classes=4, return_with_label=["a"])
    assert (dm.include_background, dm.reduction, dm.get_not_nans, dm.ignore_empty, dm.num_classes, dm.return_with_label) == (False, "sum", True, False, 4, ["a"])
    assert isinstance(dm.dice_helper, m.DiceHelper) and dm.dice_helper.apply_argmax is False and str(dm) == "DiceMetric"
    assert isinstance(dm, m.CumulativeIterationMetric) and isinstance(dm, m.Cumulative) and isinstance(dm, m.IterationMetric) and isinstance(dm, m.Metric)
    h = m.DiceHelper(threshold=True)
    assert (h.include_background, h.apply_argmax, h.activate, h.get_not_nans, h.reduction) == (True, False, False, True, "mean_batch")
    assert m.ConfusionMatrixMetric(metric_name="f1").metric_name == ("f1",)
    # Cumulative on its own: several buffers, append and extend
    c = m.Cumulative()
    c.append(1, 2)
    c.extend([3, 4], [5, 6])
    a, b = c.get_buffer()
    assert a.tolist() == [1, 3, 4] and b.tolist() == [2, 5, 6] and len(c) == 3
    c.reset()
    assert c.get_buffer() is None and len(c) == 0
    yp, yy = m.ignore_background(x, x[:, :1])
    assert yp.shape[1] == 2 and yy.shape[1] == 1 and yp.data_ptr() == x[:, 1:].data_ptr()      # a view, not a copy


def case_inferer_labels_to_dice(device):
    """a 2-window sliding_window_inference with the argmax epilogue and a fixed tiny predictor: its uint8 label map goes straight into
    DiceMetric(num_classes=K) and scores exactly like compute_dice of the same labels as float32 one-hots"""
    from monai_amd.inferers.utils import sliding_window_argmax
    from monai_amd.metrics import DiceMetric, compute_dice

    k = 3
    gen = torch.Generator().manual_seed(4600)
    vol = torch.randn((1, 1, 8, 8, 12), generator=gen).to(device)
    w = torch.tensor([1.0, -1.0, 0.25], device=device).reshape(1, k, 1, 1, 1)

    def predictor(x):
        return x * w + torch.tensor([0.0, 0.1, 0.3], device=x.device).reshape(1, k, 1, 1, 1)

    labels = sliding_window_argmax(vol, (8, 8, 8), 1, predictor, overlap=0.25, labels_dtype=torch.uint8)
    assert labels.dtype == torch.uint8 and labels.is_contiguous() and torch.unique(labels).tolist() == [0, 1, 2]
    truth = torch.randint(0, k, (1, 1, 8, 8, 12), generator=gen).to(torch.uint8).to(device)
    dm = DiceMetric(num_classes=k, reduction="none")
    got = dm(labels, truth)
    oh_p, oh_y = (torch.zeros((1, k, 8, 8, 12), device=device).scatter_(1, t.long(), 1.0) for t in (labels, truth))
    exp = compute_dice(oh_p, oh_y)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, k)
    assert torch.equal(got, exp) and torch.equal(dm.aggregate(), exp)
    assert bool((got > 0).all()) and bool((got < 1).all())
