"""Base classes of the metrics: the API shell of monai/metrics/metric.py (same names, arguments, buffers and errors), no arithmetic.

``IterationMetric`` turns a batch-first tensor or a list of channel-first tensors into ``_compute_tensor`` calls; ``Cumulative`` keeps the
per-sample results of every call in local buffers, gathers them over ``torch.distributed`` when a process group is up and hands the
concatenated tensors to ``aggregate``."""

from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Any

import numpy as np
import torch

__all__ = ["Metric", "IterationMetric", "Cumulative", "CumulativeIterationMetric"]


class Metric(ABC):
    """monai/metrics/metric.py:26-41"""

    @abstractmethod
    def __call__(self, *args: Any, **kwargs: Any) -> Any:
        raise NotImplementedError(f"Subclass {self.__class__.__name__} must implement this method.")

    def __str__(self):
        return self.__class__.__name__


class IterationMetric(Metric):
    """monai/metrics/metric.py:44-122: ``y_pred`` / ``y`` as one batch-first tensor or as lists of channel-first tensors."""

    def __call__(self, y_pred, y=None, **kwargs: Any):
        if isinstance(y_pred, (list, tuple)) or isinstance(y, (list, tuple)):
            return self._compute_list(y_pred, y, **kwargs)
        if isinstance(y_pred, torch.Tensor):
            return self._compute_tensor(y_pred.detach(), y.detach() if isinstance(y, torch.Tensor) else None, **kwargs)
        raise ValueError("y_pred or y must be a list/tuple of `channel-first` Tensors or a `batch-first` Tensor.")

    def _compute_list(self, y_pred, y=None, **kwargs: Any):
        """one ``_compute_tensor`` call per item (a batch of one), the results concatenated along the batch axis"""
        if y is not None:
            ret = [self._compute_tensor(p.detach().unsqueeze(0), t.detach().unsqueeze(0), **kwargs) for p, t in zip(y_pred, y)]
        else:
            ret = [self._compute_tensor(p.detach().unsqueeze(0), None, **kwargs) for p in y_pred]
        if isinstance(ret[0], torch.Tensor):
            return torch.cat(ret, dim=0)
        if isinstance(ret[0], (list, tuple)) and all(isinstance(i, torch.Tensor) for i in ret[0]):
            return [torch.cat(parts, dim=0) for parts in zip(*ret)]
        return ret

    @abstractmethod
    def _compute_tensor(self, y_pred: torch.Tensor, y: torch.Tensor | None = None, **kwargs: Any):
        raise NotImplementedError(f"Subclass {self.__class__.__name__} must implement this method.")


def _as_tensor(d: Any) -> torch.Tensor:
    if isinstance(d, torch.Tensor):
        return d
    if isinstance(d, np.ndarray):
        return torch.as_tensor(np.ascontiguousarray(d))
    if isinstance(d, (list, tuple)) and d and all(isinstance(i, torch.Tensor) for i in d):
        return torch.stack(list(d), dim=0)
    return torch.as_tensor(d)


def _all_gather_rows(data: torch.Tensor) -> torch.Tensor:
    """`data` of every rank concatenated along axis 0 in rank order; the ranks may hold different numbers of rows (padded to the longest for the
    collective, trimmed afterwards -- monai/utils/dist.py:59-130).  Without an initialised process group: `data` itself."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
        return data
    orig = data.device
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    data = data.to(dev)
    world = dist.get_world_size()
    mine = torch.as_tensor([data.shape[0]], device=dev)
    lens = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(lens, mine)
    rows = [int(v.item()) for v in lens]
    longest = max(rows)
    if data.shape[0] < longest:
        data = torch.cat([data, data.new_zeros([longest - data.shape[0]] + list(data.shape[1:]))], dim=0)
    parts = [torch.zeros_like(data) for _ in range(world)]
    dist.all_gather(parts, data.contiguous())
    return torch.cat([p[:r] for p, r in zip(parts, rows)], dim=0).to(orig)


class Cumulative:
    """monai/metrics/metric.py:125-293: local buffers (one per positional item of ``extend`` / ``append``), synchronised over the process group on demand."""

    def __init__(self) -> None:
        self._buffers: list | None = None
        self._synced_tensors: list | None = None
        self._synced: bool = False
        self.reset()

    def reset(self):
        self._buffers = None
        self._synced_tensors = None
        self._synced = False

    def extend(self, *data: Any) -> None:
        """add a batch: every item is a batch-first tensor (or a list of channel-first tensors) whose rows become samples of its buffer"""
        if self._buffers is None:
            self._buffers = [[] for _ in data]
        for buf, d in zip(self._buffers, data):
            d_t = _as_tensor(d)
            try:
                buf.extend([x[0] for x in torch.split(d_t, 1, dim=0)])
            except (AttributeError, IndexError, RuntimeError) as e:
                raise TypeError(f"{e}. `data` should be a batch-first tensor or a list of channel-first tensors, got {type(d_t)}") from e
        self._synced = False

    def append(self, *data: Any) -> None:
        """add one sample per buffer"""
        if self._buffers is None:
            self._buffers = [[] for _ in data]
        for buf, d in zip(self._buffers, data):
            buf.append(_as_tensor(d))
        self._synced = False

    @abstractmethod
    def aggregate(self, *args: Any, **kwargs: Any) -> Any:
        raise NotImplementedError(f"Subclass {self.__class__.__name__} must implement this method.")

    def _sync(self):
        if self._synced or self._buffers is None:
            return
        try:
            self._synced_tensors = [_all_gather_rows(torch.stack(b, dim=0)) for b in self._buffers]
        except (RuntimeError, TypeError, ValueError) as e:
            raise TypeError(f"{e}. unable to sync buffer contents: {self._buffers}.") from e
        self._synced = True

    def __len__(self):
        self._sync()
        if self._synced_tensors is None:
            return 0
        return max(len(x) for x in self._synced_tensors if x is not None)

    def get_buffer(self):
        """the synchronised buffers as tensors (copies): one tensor, or a list when there are several buffers; None before the first sample"""
        self._sync()
        if self._synced_tensors is None:
            return self._synced_tensors
        buffers = [x.detach().clone() if isinstance(x, torch.Tensor) else x for x in self._synced_tensors]
        return buffers[0] if len(buffers) == 1 else buffers


class CumulativeIterationMetric(Cumulative, IterationMetric):
    """monai/metrics/metric.py:296-353: every call computes the batch's values, adds them to the buffers and returns them."""

    def __call__(self, y_pred, y=None, **kwargs: Any):
        ret = super().__call__(y_pred=y_pred, y=y, **kwargs)
        if isinstance(ret, (tuple, list)):
            self.extend(*ret)
        else:
            self.extend(ret)
        return ret
