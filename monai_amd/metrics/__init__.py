"""Segmentation metrics on the one-pass overlap kernel and the edge / exact-EDT / surface-record kernels: the names of monai.metrics that this
package implements."""

from .confusion_matrix import ConfusionMatrixMetric, check_confusion_matrix_metric_name, compute_confusion_matrix_metric, get_confusion_matrix
from .hausdorff_distance import HausdorffDistanceMetric, compute_hausdorff_distance
from .meandice import DiceHelper, DiceMetric, compute_dice
from .meaniou import MeanIoU, compute_iou
from .metric import Cumulative, CumulativeIterationMetric, IterationMetric, Metric
from .surface_dice import SurfaceDiceMetric, compute_surface_dice
from .surface_distance import SurfaceDistanceMetric, compute_average_surface_distance
from .utils import (do_metric_reduction, get_edge_surface_distance, get_mask_edges, get_surface_distance, ignore_background, is_binary_tensor,
                    prepare_spacing)

__all__ = [
    "ConfusionMatrixMetric", "check_confusion_matrix_metric_name", "compute_confusion_matrix_metric", "get_confusion_matrix", "DiceHelper", "DiceMetric",
    "compute_dice", "MeanIoU", "compute_iou", "Cumulative", "CumulativeIterationMetric", "IterationMetric", "Metric", "do_metric_reduction",
    "ignore_background", "is_binary_tensor", "HausdorffDistanceMetric", "compute_hausdorff_distance", "SurfaceDistanceMetric",
    "compute_average_surface_distance", "SurfaceDiceMetric", "compute_surface_dice", "get_mask_edges", "get_surface_distance",
    "get_edge_surface_distance", "prepare_spacing",
]
