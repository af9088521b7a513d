"""Segmentation metrics on the one-pass overlap kernel: the names of monai.metrics that this package implements."""

from .confusion_matrix import ConfusionMatrixMetric, check_confusion_matrix_metric_name, compute_confusion_matrix_metric, get_confusion_matrix
from .meandice import DiceHelper, DiceMetric, compute_dice
from .meaniou import MeanIoU, compute_iou
from .metric import Cumulative, CumulativeIterationMetric, IterationMetric, Metric
from .utils import do_metric_reduction, ignore_background, is_binary_tensor

__all__ = [
    "ConfusionMatrixMetric", "check_confusion_matrix_metric_name", "compute_confusion_matrix_metric", "get_confusion_matrix", "DiceHelper", "DiceMetric",
    "compute_dice", "MeanIoU", "compute_iou", "Cumulative", "CumulativeIterationMetric", "IterationMetric", "Metric", "do_metric_reduction",
    "ignore_background", "is_binary_tensor",
]
