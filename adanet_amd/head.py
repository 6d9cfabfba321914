"""Heads: loss / predictions / metrics per task type.

The reference delegates to tf.estimator heads (created in user code and
consumed at adanet/core/ensemble_builder.py:571-583). adanet_amd ships its
own minimal heads built on the fused kernels: MultiClassHead runs the K2
fused softmax-xent; metrics run on-device (K10 argmax_correct) and stream
into python accumulators.
"""

from __future__ import annotations

import abc
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from adanet_amd.ops import _extension
from adanet_amd.ops import metrics as metric_ops
from adanet_amd.ops.xent import softmax_xent

_NAN = float("nan")


class StreamingMetrics(abc.ABC):
    """Whole-dataset eval metrics of one head, accumulated batch by batch.

    ``update`` folds a batch in, ``result`` reads the metrics back,
    ``reset`` starts over and ``merge_`` adds another accumulator of the same
    kind (states of shards or ranks combine by summation). ``state`` is what
    is accumulated.
    """

    state = None

    @abc.abstractmethod
    def update(self, logits: torch.Tensor, labels) -> None:
        ...

    @abc.abstractmethod
    def result(self) -> Dict[str, float]:
        ...

    @abc.abstractmethod
    def reset(self) -> None:
        ...

    @abc.abstractmethod
    def merge_(self, other: "StreamingMetrics") -> "StreamingMetrics":
        ...


class _HostMeanStreamingMetrics(StreamingMetrics):
    """Default for heads without a device-side state: ``head.metrics`` per
    batch (which syncs), example-weighted host means. ``state`` maps a metric
    to its weighted sum, under ``"n"`` the example count."""

    def __init__(self, head: "Head"):
        self._head = head
        self.reset()

    def update(self, logits, labels):
        n = int(logits.shape[0])
        for k, v in self._head.metrics(logits, labels).items():
            self.state["sums"][k] = self.state["sums"].get(k, 0.0) \
                + float(v) * n
        self.state["n"] += n

    def result(self):
        n = self.state["n"]
        return {k: (v / n if n else _NAN)
                for k, v in self.state["sums"].items()}

    def reset(self):
        self.state = {"n": 0, "sums": {}}

    def merge_(self, other):
        for k, v in other.state["sums"].items():
            self.state["sums"][k] = self.state["sums"].get(k, 0.0) + v
        self.state["n"] += other.state["n"]
        return self


class _DeviceStreamingMetrics(StreamingMetrics):
    """One flat fp64 device tensor updated by a fused kernel per batch
    (ops/metrics.py): ``update`` never syncs, ``result`` is the one D2H
    read. With ``device=None`` the state is placed on first use, where the
    logits live."""

    def __init__(self, size: int, device=None):
        self._size = int(size)
        self.state = None
        if device is not None:
            self.state = metric_ops.new_state(self._size, device)

    def _state_for(self, logits):
        if self.state is None:
            self.state = metric_ops.new_state(self._size, logits.device)
        return self.state

    def _host_state(self):
        if self.state is None:
            return torch.zeros((self._size,), dtype=torch.float64)
        return self.state.cpu()

    def result(self):
        return self._result_from(self._host_state())

    def reset(self):
        if self.state is not None:
            self.state.zero_()

    def merge_(self, other):
        if type(other) is not type(self) or other._size != self._size:
            raise ValueError("merge_: incompatible streaming metric states")
        if other.state is not None:
            if self.state is None:
                self.state = torch.zeros_like(other.state)
            self.state.add_(other.state.to(self.state.device))
        return self


def _ratio(num: float, den: float) -> float:
    return num / den if den else _NAN


class _MultiClassStreamingMetrics(_DeviceStreamingMetrics):

    def __init__(self, n_classes, label_smoothing, device, k, per_class):
        if int(k) < 1:
            raise ValueError("streaming_metrics: k must be >= 1")
        self._C, self._eps = int(n_classes), float(label_smoothing)
        self._k, self._per_class = int(k), bool(per_class)
        super().__init__(
            metric_ops.multiclass_state_size(self._C, self._per_class),
            device)

    def update(self, logits, labels):
        metric_ops.multiclass_update(
            self._state_for(logits), logits, labels, k=self._k,
            label_smoothing=self._eps, per_class=self._per_class)

    def _result_from(self, s):
        n = float(s[0])
        out = {"accuracy": _ratio(float(s[2]), n),
               "average_loss": _ratio(float(s[1]), n),
               "top_k_accuracy": _ratio(float(s[3]), n)}
        if self._per_class:
            C, o = self._C, metric_ops.MULTICLASS_SLOTS
            seen = s[o:o + C] > 0
            # classes without a labelled example are left out of the mean
            out["mean_per_class_accuracy"] = float(
                (s[o + C:o + 2 * C][seen] / s[o:o + C][seen]).mean()
            ) if bool(seen.any()) else _NAN
        return out


class _BinaryStreamingMetrics(_DeviceStreamingMetrics):

    def __init__(self, device, num_thresholds):
        self._T = int(num_thresholds)
        super().__init__(metric_ops.binary_state_size(self._T), device)

    def update(self, logits, labels):
        metric_ops.binary_update(self._state_for(logits), logits, labels,
                                 num_thresholds=self._T)

    def _result_from(self, s):
        from adanet_amd.core.eval_metrics import binary_metrics_from_histogram
        n = float(s[0])
        out = {"accuracy": _ratio(float(s[2]), n),
               "average_loss": _ratio(float(s[1]), n)}
        if n:
            out.update(binary_metrics_from_histogram(
                s[metric_ops.BINARY_SLOTS:].view(2, self._T)))
        else:
            out.update({"auc": _NAN, "precision": _NAN, "recall": _NAN})
        return out


class _RegressionStreamingMetrics(_DeviceStreamingMetrics):

    def __init__(self, device):
        super().__init__(metric_ops.REGRESSION_SLOTS, device)

    def update(self, logits, labels):
        metric_ops.regression_update(self._state_for(logits), logits, labels)

    def _result_from(self, s):
        n = float(s[0])
        mse = _ratio(float(s[1]), n)
        return {"average_loss": mse,
                "mean_absolute_error": _ratio(float(s[2]), n),
                "root_mean_squared_error": mse ** 0.5}


class _MultiHeadStreamingMetrics(StreamingMetrics):
    """One sub-state per sub-head over the same logits split as
    ``MultiHead.loss``; ``state`` is the tuple of the sub-states' states in
    head-name order."""

    def __init__(self, multi_head: "MultiHead", parts: dict):
        self._head = multi_head
        self._parts = parts

    @property
    def state(self):
        return tuple(self._parts[k].state for k in self._head._order)

    def update(self, logits, labels):
        split = self._head._split(logits)
        for k in self._head._order:
            self._parts[k].update(split[k], labels[k])

    def result(self):
        # one D2H copy for all device-side sub-states together
        order = self._head._order
        dev = [k for k in order
               if isinstance(self._parts[k], _DeviceStreamingMetrics)
               and self._parts[k].state is not None]
        host = {}
        if dev and len({self._parts[k].state.device for k in dev}) == 1:
            flat = torch.cat([self._parts[k].state for k in dev]).cpu()
            off = 0
            for k in dev:
                host[k] = flat[off:off + self._parts[k]._size]
                off += self._parts[k]._size
        out, total = {}, 0.0
        for k in order:
            part = self._parts[k]
            res = part._result_from(host[k]) if k in host else part.result()
            for name, v in res.items():
                out["%s/%s" % (k, name)] = v
            total += res.get("average_loss", _NAN)
        out["average_loss"] = total
        return out

    def reset(self):
        for part in self._parts.values():
            part.reset()

    def merge_(self, other):
        if not isinstance(other, _MultiHeadStreamingMetrics) \
                or other._head._order != self._head._order:
            raise ValueError("merge_: incompatible streaming metric states")
        for k in self._head._order:
            self._parts[k].merge_(other._parts[k])
        return self


class Head(abc.ABC):

    @property
    @abc.abstractmethod
    def logits_dimension(self) -> int:
        ...

    @abc.abstractmethod
    def loss(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """Scalar fp32 training loss."""

    @abc.abstractmethod
    def predictions(self, logits: torch.Tensor) -> Dict[str, torch.Tensor]:
        ...

    def metrics(self, logits: torch.Tensor,
                labels: torch.Tensor) -> Dict[str, float]:
        with torch.no_grad():
            return {
                "average_loss": float(self.loss(logits, labels).detach().cpu())
            }

    def streaming_metrics(self, device=None, **options) -> StreamingMetrics:
        """A whole-dataset accumulator of this head's eval metrics (see
        ``StreamingMetrics``). The built-in heads keep a device-side state
        updated by a fused kernel; this default keeps custom heads working:
        it calls ``self.metrics`` per batch and keeps example-weighted host
        means (weight ``logits.shape[0]``)."""
        if options:
            raise TypeError("streaming_metrics: %s takes no options (got %s)"
                            % (type(self).__name__, sorted(options)))
        return _HostMeanStreamingMetrics(self)


class MultiClassHead(Head):
    """Softmax cross-entropy head with optional label smoothing
    (reference usage: research/improve_nas/trainer/cifar10.py:149-152
    multi-class head with SUM_OVER_BATCH_SIZE reduction = mean)."""

    def __init__(self, n_classes: int, label_smoothing: float = 0.0):
        if n_classes < 2:
            raise ValueError("n_classes must be >= 2")
        self._n_classes = n_classes
        self._label_smoothing = label_smoothing

    @property
    def logits_dimension(self) -> int:
        return self._n_classes

    def loss(self, logits, labels):
        return softmax_xent(logits, labels.long(),
                            label_smoothing=self._label_smoothing,
                            reduction="mean")

    def predictions(self, logits):
        with torch.no_grad():
            probs = torch.softmax(logits.float(), dim=-1)
            return {
                "logits": logits,
                "probabilities": probs,
                "class_ids": probs.argmax(dim=-1),
            }

    def metrics(self, logits, labels):
        with torch.no_grad():
            labels = labels.long()
            if logits.is_cuda:
                ext = _extension.require()
                correct = torch.zeros((1,), device=logits.device,
                                      dtype=torch.int32)
                ext.argmax_correct(logits.to(torch.bfloat16), labels, None,
                                   correct)
                acc = float(correct.item()) / logits.shape[0]
            else:
                acc = float((logits.argmax(dim=-1) == labels).float().mean())
            return {
                "accuracy": acc,
                "average_loss": float(self.loss(logits, labels).detach().cpu()),
            }

    def streaming_metrics(self, device=None, k: int = 5,
                          per_class: bool = False) -> StreamingMetrics:
        """``accuracy``, ``average_loss`` (with this head's label smoothing,
        like ``loss()``), ``top_k_accuracy`` and, with ``per_class``,
        ``mean_per_class_accuracy`` over the classes that have labelled
        examples."""
        return _MultiClassStreamingMetrics(
            self._n_classes, self._label_smoothing, device, k, per_class)


class BinaryClassHead(Head):
    """Single-logit sigmoid head."""

    def __init__(self):
        pass

    @property
    def logits_dimension(self) -> int:
        return 1

    def loss(self, logits, labels):
        return F.binary_cross_entropy_with_logits(
            logits.float().reshape(-1), labels.float().reshape(-1))

    def predictions(self, logits):
        with torch.no_grad():
            p = torch.sigmoid(logits.float()).reshape(-1)
            return {"logits": logits, "probabilities": p,
                    "class_ids": (p > 0.5).long()}

    def metrics(self, logits, labels):
        from adanet_amd.core.eval_metrics import AUCAccumulator
        with torch.no_grad():
            p = torch.sigmoid(logits.float()).reshape(-1)
            y = labels.long().reshape(-1)
            acc = float(((p > 0.5).long() == y).float().mean())
            auc = AUCAccumulator()
            auc.update(p, y)
            out = {"accuracy": acc,
                   "average_loss": float(self.loss(logits, labels).cpu())}
            out.update(auc.value())
            return out

    def streaming_metrics(self, device=None,
                          num_thresholds: int = 200) -> StreamingMetrics:
        """The keys of ``metrics()`` over the whole dataset: one score
        histogram, so ``auc`` is the dataset AUC, not a mean of batch AUCs.
        ``accuracy`` is decided on the sign of the logit; ``metrics()``
        thresholds the fp32 sigmoid at 0.5, which differs only for
        ``0 < x < ~6e-8``."""
        return _BinaryStreamingMetrics(device, num_thresholds)


class MultiHead(Head):
    """Composite head over named sub-heads (the reference's multi-head
    support, adanet/core/estimator_test.py:1517: logits split across heads,
    labels a dict keyed by head name, losses summed)."""

    def __init__(self, heads: dict):
        if not heads:
            raise ValueError("heads must not be empty")
        self._heads = dict(heads)
        self._order = sorted(heads.keys())

    @property
    def logits_dimension(self) -> int:
        return sum(self._heads[k].logits_dimension for k in self._order)

    def _split(self, logits):
        out = {}
        off = 0
        for k in self._order:
            d = self._heads[k].logits_dimension
            out[k] = logits[:, off:off + d]
            off += d
        return out

    def loss(self, logits, labels):
        parts = self._split(logits)
        total = None
        for k in self._order:
            term = self._heads[k].loss(parts[k], labels[k])
            total = term if total is None else total + term
        return total

    def predictions(self, logits):
        parts = self._split(logits)
        out = {}
        for k in self._order:
            for name, v in self._heads[k].predictions(parts[k]).items():
                out["%s/%s" % (k, name)] = v
        return out

    def metrics(self, logits, labels):
        parts = self._split(logits)
        out = {}
        for k in self._order:
            for name, v in self._heads[k].metrics(parts[k],
                                                  labels[k]).items():
                out["%s/%s" % (k, name)] = v
        out["average_loss"] = float(self.loss(logits, labels).detach().cpu())
        return out

    def streaming_metrics(self, device=None, **options) -> StreamingMetrics:
        """One sub-state per sub-head, keys ``"<head>/<metric>"``; the
        top-level ``average_loss`` is the sum of the sub-heads'. ``options``
        maps a sub-head's name to that head's own options."""
        unknown = sorted(set(options) - set(self._order))
        if unknown:
            raise TypeError("streaming_metrics: no sub-head named %s"
                            % unknown)
        return _MultiHeadStreamingMetrics(self, {
            k: self._heads[k].streaming_metrics(device=device,
                                                **options.get(k, {}))
            for k in self._order})


class RegressionHead(Head):
    """Mean-squared-error head (the reference tests' regression head,
    adanet/core/testing_utils.py:236)."""

    def __init__(self, label_dimension: int = 1):
        self._dim = label_dimension

    @property
    def logits_dimension(self) -> int:
        return self._dim

    def loss(self, logits, labels):
        return F.mse_loss(logits.float().reshape(labels.shape),
                          labels.float())

    def predictions(self, logits):
        return {"predictions": logits}

    def metrics(self, logits, labels):
        with torch.no_grad():
            return {"average_loss": float(self.loss(logits, labels).cpu())}

    def streaming_metrics(self, device=None) -> StreamingMetrics:
        """``average_loss`` (MSE), ``mean_absolute_error`` and
        ``root_mean_squared_error`` over every element seen."""
        return _RegressionStreamingMetrics(device)
