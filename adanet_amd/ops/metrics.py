"""Streaming eval-metric updates (K10): fold one batch into a persistent
fp64 state tensor with no host sync.

Each ``*_update(state, logits, labels, ...)`` adds one batch of logits and
labels into ``state`` in place and returns it. On CUDA tensors the update is
one fused HIP kernel plus a one-wave finisher (csrc/eval_metrics.hip) through
``_extension.require()``; there is no eager fallback. On CPU tensors it is the
pure-torch fp64 reference below, which is the GPU-less implementation and the
numerics oracle of the tests.

State layouts (flat fp64; counts are exact integers):

* multiclass  ``[n, loss_sum, correct_1, correct_k]`` and, with
  ``per_class``, ``label_count[C]`` then ``correct_count[C]``
* binary      ``[n, loss_sum, correct, hist[2, T]]``, positives in row 0
* regression  ``[n_elems, sq_err_sum, abs_err_sum]``

States of shards or ranks combine by elementwise addition.

Definitions (identical on both devices):

* multiclass loss of a row is ``lse - (1-eps)*v_y - (eps/C)*sum(v)``. The
  rank of the label is ``#{c : v_c > v_y or (v_c == v_y and c < y)}``; the row
  is top-1 correct iff the rank is 0 (first-index argmax, what
  ``torch.argmax`` on CPU and the argmax_correct kernel do) and top-k correct
  iff the rank is below ``k``. A NaN logit makes ``loss_sum`` NaN; what that
  row adds to the counts is unspecified.
* binary loss is ``max(x,0) - x*y + log1p(exp(-|x|))``; an example is correct
  iff ``(x > 0) == (y != 0)`` - decided on the sign of the logit, so it is
  exact. (``BinaryClassHead.metrics`` thresholds the fp32 sigmoid at 0.5,
  which differs only for ``0 < x < ~6e-8``, where the sigmoid rounds to 0.5.)
  The fp32 sigmoid ``p`` is bucketed as the binary_histogram kernel does it:
  clamp to [0, 1], ``int(p * T)``, clamp to ``T - 1``.
* regression sums ``(x - y)^2`` and ``|x - y|`` over every element.
"""

from __future__ import annotations

import torch

from adanet_amd.ops import _extension

MULTICLASS_SLOTS = 4   # n, loss_sum, correct_1, correct_k
BINARY_SLOTS = 3       # n, loss_sum, correct
REGRESSION_SLOTS = 3   # n_elems, sq_err_sum, abs_err_sum


def multiclass_state_size(n_classes: int, per_class: bool = False) -> int:
    return MULTICLASS_SLOTS + (2 * int(n_classes) if per_class else 0)


def binary_state_size(num_thresholds: int) -> int:
    return BINARY_SLOTS + 2 * int(num_thresholds)


def new_state(size: int, device=None) -> torch.Tensor:
    return torch.zeros((int(size),), dtype=torch.float64, device=device)


def max_blocks() -> int:
    """Grid cap of the update kernels: past ``4 * max_blocks()`` rows a wave
    of the multiclass kernel takes more than one row."""
    return int(_extension.require().metrics_max_blocks())


def _check_state(op, state, logits, size):
    if state.dtype != torch.float64 or state.dim() != 1 \
            or state.shape[0] != size or not state.is_contiguous():
        raise ValueError("%s: state must be a contiguous float64 vector of "
                         "%d elements (got %s %s)"
                         % (op, size, state.dtype, tuple(state.shape)))
    if state.device != logits.device:
        raise ValueError("%s: state lives on %s, logits on %s"
                         % (op, state.device, logits.device))


def _kernel_logits(logits):
    """bf16 and fp32 go to the kernel as they are; other dtypes as fp32."""
    if logits.dtype not in (torch.bfloat16, torch.float32):
        logits = logits.float()
    if logits.dim() == 2 and logits.shape[0] > 0 and logits.stride(1) != 1:
        logits = logits.contiguous()
    return logits


def multiclass_update(state: torch.Tensor, logits: torch.Tensor,
                      labels: torch.Tensor, k: int = 5,
                      label_smoothing: float = 0.0,
                      per_class: bool = False) -> torch.Tensor:
    """Adds a ``[B, C]`` batch into a multiclass state."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("multiclass_update: logits must be [B, C]")
    B, C = logits.shape
    k = int(k)
    if k < 1:
        raise ValueError("multiclass_update: k must be >= 1")
    _check_state("multiclass_update", state, logits,
                 multiclass_state_size(C, per_class))
    labels = labels.detach().reshape(-1).long()
    if labels.shape[0] != B:
        raise ValueError("multiclass_update: %d labels for %d rows"
                         % (labels.shape[0], B))
    logits = logits.detach()
    if logits.is_cuda:
        ext = _extension.require()
        ext.metrics_multiclass_update(state, _kernel_logits(logits),
                                      labels.contiguous(), k,
                                      float(label_smoothing),
                                      bool(per_class))
        return state
    if B == 0:
        return state
    if bool(((labels < 0) | (labels >= C)).any()):
        raise ValueError("multiclass_update: label outside [0, %d)" % C)
    eps = float(label_smoothing)
    v = logits.double()
    y = labels.view(-1, 1)
    vy = v.gather(1, y)
    loss = torch.logsumexp(v, dim=1) - (1.0 - eps) * vy[:, 0] \
        - (eps / C) * v.sum(dim=1)
    cls = torch.arange(C).view(1, C)
    rank = ((v > vy) | ((v == vy) & (cls < y))).sum(dim=1)
    top1 = rank == 0
    state[0] += B
    state[1] += loss.sum()
    state[2] += int(top1.sum())
    state[3] += int((rank < k).sum())
    if per_class:
        s = MULTICLASS_SLOTS
        state[s:s + C] += torch.bincount(labels, minlength=C).double()
        state[s + C:s + 2 * C] += torch.bincount(labels[top1],
                                                 minlength=C).double()
    return state


def binary_update(state: torch.Tensor, logits: torch.Tensor,
                  labels: torch.Tensor,
                  num_thresholds: int = 200) -> torch.Tensor:
    """Adds a ``[B]`` or ``[B, 1]`` batch into a binary state."""
    T = int(num_thresholds)
    if T < 1 or T > 4096:
        raise ValueError("binary_update: need 1 <= num_thresholds <= 4096")
    if logits.dim() == 2 and logits.shape[1] != 1 or logits.dim() > 2:
        raise ValueError("binary_update: logits must be [B] or [B, 1]")
    _check_state("binary_update", state, logits, binary_state_size(T))
    logits = logits.detach().reshape(-1)
    labels = labels.detach().reshape(-1).long()
    B = logits.shape[0]
    if labels.shape[0] != B:
        raise ValueError("binary_update: %d labels for %d examples"
                         % (labels.shape[0], B))
    if logits.is_cuda:
        ext = _extension.require()
        ext.metrics_binary_update(state, _kernel_logits(logits),
                                  labels.contiguous(), T)
        return state
    if B == 0:
        return state
    pos = labels != 0
    x = logits.double()
    loss = x.clamp(min=0) - x * pos.double() + torch.log1p(torch.exp(-x.abs()))
    p = torch.sigmoid(logits.float())
    b = (p.clamp(0, 1) * T).long().clamp(min=0, max=T - 1)
    state[0] += B
    state[1] += loss.sum()
    state[2] += int(((x > 0) == pos).sum())
    s = BINARY_SLOTS
    state[s:s + T] += torch.bincount(b[pos], minlength=T).double()
    state[s + T:s + 2 * T] += torch.bincount(b[~pos], minlength=T).double()
    return state


def regression_update(state: torch.Tensor, logits: torch.Tensor,
                      labels: torch.Tensor) -> torch.Tensor:
    """Adds a ``[B, D]`` batch (labels of as many elements) into a regression
    state."""
    if logits.dim() == 1:
        logits = logits.unsqueeze(1)
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("regression_update: logits must be [B, D]")
    _check_state("regression_update", state, logits, REGRESSION_SLOTS)
    if labels.numel() != logits.numel():
        raise ValueError("regression_update: labels hold %d elements, logits "
                         "%d" % (labels.numel(), logits.numel()))
    logits = logits.detach()
    labels = labels.detach().float().reshape(logits.shape)
    if logits.is_cuda:
        ext = _extension.require()
        ext.metrics_regression_update(state, _kernel_logits(logits),
                                      labels.contiguous())
        return state
    if logits.numel() == 0:
        return state
    d = logits.double() - labels.double()
    state[0] += d.numel()
    state[1] += (d * d).sum()
    state[2] += d.abs().sum()
    return state
