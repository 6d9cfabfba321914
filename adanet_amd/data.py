"""Device-feeding input pipeline: pinned staging + overlapped H2D copies.

The reference rides tf.data's host pipeline; the MI355X-native equivalent
wraps any ``input_fn`` (an iterable of (features, labels) CPU batches) with:

  * pinned-memory staging buffers (reused, no per-batch allocation),
  * async H2D copies on a dedicated copy stream, double-buffered so batch
    i+1 uploads while batch i trains,
  * optional bf16 cast on device.

Synthetic/resident datasets (bench.py) bypass this entirely — tensors are
already in HBM. On CPU the wrapper is pass-through.

``DeviceImageLoader`` is the other shape for image sets that fit in HBM: the
dataset is uploaded once as uint8 and every batch is drawn, augmented,
normalised and cast on the device (csrc/augment.hip), with no host pixel work
at all.
"""

from __future__ import annotations

from typing import Iterable, Iterator, Optional, Tuple

import torch


class DeviceLoader(object):
    """Wraps an input_fn with prefetched device transfer.

    Usage::

        loader = DeviceLoader(input_fn, device="cuda:0")
        estimator.train(loader, max_steps=...)

    (It is itself a valid ``input_fn``: calling it returns a fresh
    iterator.)
    """

    def __init__(self, input_fn, device, dtype: torch.dtype = torch.bfloat16,
                 prefetch: int = 2):
        self._input_fn = input_fn
        self._device = torch.device(device)
        self._dtype = dtype
        self._prefetch = max(1, prefetch)

    def __call__(self):
        if self._device.type != "cuda":
            return iter(self._input_fn())
        return _DeviceIterator(iter(self._input_fn()), self._device,
                               self._dtype, self._prefetch)


class _DeviceIterator(object):

    def __init__(self, src: Iterator, device, dtype, prefetch: int):
        self._src = src
        self._device = device
        self._dtype = dtype
        self._prefetch = prefetch
        self._stream = torch.cuda.Stream(device=device)
        self._queue = []
        # Ring of prefetch+1 pinned buffers per slot: a buffer is only
        # rewritten after ITS async H2D completed (event-synced), so the
        # producer can run ahead without racing in-flight DMA.
        self._pinned = {}
        self._tick = 0
        for _ in range(prefetch):
            self._enqueue()

    def _pin(self, t: torch.Tensor, slot: str) -> torch.Tensor:
        key = (slot, tuple(t.shape), t.dtype,
               self._tick % (self._prefetch + 1))
        entry = self._pinned.get(key)
        if entry is None:
            entry = [torch.empty_like(t, pin_memory=True), None]
            self._pinned[key] = entry
        buf, ev = entry
        if ev is not None:
            ev.synchronize()  # prior H2D from this buffer must be done
        buf.copy_(t)
        entry[1] = self._cur_event
        return buf

    def _to_dev(self, t: torch.Tensor, slot: str) -> torch.Tensor:
        staged = t if t.is_pinned() else self._pin(t, slot)
        d = staged.to(self._device, non_blocking=True)
        if d.is_floating_point() and self._dtype is not None:
            d = d.to(self._dtype)
        return d

    def _enqueue(self):
        try:
            features, labels = next(self._src)
        except StopIteration:
            return
        ev = torch.cuda.Event()
        self._cur_event = ev
        with torch.cuda.stream(self._stream):
            if isinstance(features, dict):
                f = {k: self._to_dev(v, "f:" + k)
                     for k, v in features.items()}
            elif torch.is_tensor(features) and not features.is_cuda:
                f = self._to_dev(features, "f")
            else:
                f = features
            if isinstance(labels, dict):
                l = {k: v.to(self._device, non_blocking=True)
                     for k, v in labels.items()}
            elif torch.is_tensor(labels) and not labels.is_cuda:
                l = self._to_dev(labels, "l").long() if (
                    not labels.is_floating_point()) else self._to_dev(
                        labels, "l")
            else:
                l = labels
            ev.record(self._stream)
        self._tick += 1
        self._queue.append((f, l, ev))

    def __iter__(self):
        return self

    def __next__(self):
        if not self._queue:
            raise StopIteration
        f, l, ev = self._queue.pop(0)
        # Consumer stream waits on the copy (device-side, no host sync).
        ev.wait(torch.cuda.current_stream(self._device))
        self._enqueue()
        return f, l


class DeviceImageLoader(object):
    """Device-resident image dataset with on-device augmentation.

    ``images`` (uint8 or float32 ``[N, C, H, W]``) and ``labels`` (``[N]``)
    are uploaded to ``device`` once, here. After that a training batch is two
    kernel launches (``ops.augment.draw_params`` + ``augment_apply``): no
    host pixel work, no pinned staging, no host-to-device copy. It is itself
    a valid ``input_fn``: calling it returns a fresh iterator that starts at
    ``start_step``.

    Training mode yields an endless stream of ``(bf16 [B, C, H, W], int64
    [B])``, sampled with replacement. Batch ``s`` is a pure function of
    ``(seed, s, shard, data)``: equal loaders yield bit-identical batches
    and ``start_step=k`` resumes the same stream at batch ``k``. ``shard =
    (rank, world)`` gives each rank its own counters. ``augment=False``
    still draws the indices but centres the crop, never flips and turns
    cutout off.

    Evaluation mode (``training=False``) visits every example once, in
    order, unaugmented; the last batch may be short. Its feature tensors
    carry ``adanet_cache_key = ("image-eval", id(loader), batch_index)`` so
    the frozen-logit HBM cache applies; training batches carry none.

    ``normalize``: ``"unit"`` maps uint8 to [-1, 1] (scale 2/255, shift -1;
    pad and cutout pixels, written as 0, are then mid-grey); ``"none"`` maps
    uint8 to [0, 1]; both leave float data as it is. A ``(mean, std)`` pair
    of per-channel sequences gives ``(x - mean) / std`` with ``x`` in [0, 1]
    for uint8 data.
    """

    def __init__(self, images, labels, batch_size: int, device,
                 training: bool = True, augment: bool = True, pad: int = 4,
                 cutout_pad: int = 8, normalize="unit", seed: int = 0,
                 start_step: int = 0, shard: Tuple[int, int] = (0, 1)):
        images = torch.as_tensor(images)
        labels = torch.as_tensor(labels)
        if images.dim() != 4 or images.dtype not in (torch.uint8,
                                                     torch.float32):
            raise ValueError("DeviceImageLoader: images must be uint8 or "
                             "float32 [N, C, H, W] (got %s %s)"
                             % (images.dtype, tuple(images.shape)))
        n = images.shape[0]
        if not (1 <= n < 2 ** 31):
            raise ValueError("DeviceImageLoader: need 1 <= N < 2^31 images")
        if labels.dim() != 1 or labels.shape[0] != n \
                or labels.is_floating_point():
            raise ValueError("DeviceImageLoader: labels must be N integers")
        rank, world = (int(v) for v in shard)
        if batch_size < 1 or pad < 0 or cutout_pad < 0 or start_step < 0 \
                or world < 1 or not (0 <= rank < world):
            raise ValueError("DeviceImageLoader: bad batch_size, pad, "
                             "cutout_pad, start_step or shard")
        self.device = torch.device(device)
        self.images = images.to(self.device).contiguous()
        self.labels = labels.to(self.device, torch.int64).contiguous()
        self.batch_size = int(batch_size)
        self.training = bool(training)
        self.augment = bool(augment)
        self.pad = int(pad)
        self.cutout_pad = int(cutout_pad)
        self.seed = int(seed or 0)
        self.start_step = int(start_step)
        self.shard = (rank, world)
        scale, shift = self._affine(normalize, images.dtype, images.shape[1])
        self.scale = scale.to(self.device)
        self.shift = shift.to(self.device)

    @staticmethod
    def _affine(normalize, dtype, channels: int):
        """Per-channel fp32 (scale, shift) of ``x * scale + shift``."""
        unit = 1.0 / 255.0 if dtype == torch.uint8 else 1.0
        if isinstance(normalize, str):
            if normalize not in ("unit", "none"):
                raise ValueError("DeviceImageLoader: normalize must be "
                                 "'unit', 'none' or (mean, std)")
            if normalize == "unit" and dtype == torch.uint8:
                scale, shift = [2.0 / 255.0] * channels, [-1.0] * channels
            else:
                scale, shift = [unit] * channels, [0.0] * channels
        else:
            mean, std = ([float(v) for v in seq] for seq in normalize)
            if len(mean) != channels or len(std) != channels:
                raise ValueError("DeviceImageLoader: mean and std need one "
                                 "entry per channel")
            scale = [unit / s for s in std]
            shift = [-m / s for m, s in zip(mean, std)]
        return (torch.tensor(scale, dtype=torch.float32),
                torch.tensor(shift, dtype=torch.float32))

    def __len__(self):
        if self.training:
            raise TypeError("a training DeviceImageLoader is endless")
        return -(-self.images.shape[0] // self.batch_size)

    def __call__(self):
        return self._train_iter() if self.training else self._eval_iter()

    def _train_iter(self):
        from adanet_amd.ops import augment as A
        n, _, h, w = self.images.shape
        cut = self.cutout_pad if self.augment else 0
        step = self.start_step
        while True:
            params, y = A.draw_params(
                self.seed, step, self.batch_size, n, h, w, self.pad,
                self.labels, rank=self.shard[0], world=self.shard[1],
                augment=self.augment)
            x = A.augment_apply(self.images, params, self.scale, self.shift,
                                self.pad, cut)
            yield x, y
            step += 1

    def _eval_iter(self):
        from adanet_amd.ops import augment as A
        n = self.images.shape[0]
        for i in range(self.start_step, len(self)):
            lo = i * self.batch_size
            hi = min(n, lo + self.batch_size)
            # index = lo..hi-1, zero crop offset against zero padding, no
            # flip, cutout off: the image itself, normalised.
            params = torch.zeros((hi - lo, A.FIELDS), device=self.device,
                                 dtype=torch.int32)
            params[:, 0] = torch.arange(lo, hi, device=self.device,
                                        dtype=torch.int32)
            x = A.augment_apply(self.images, params, self.scale, self.shift,
                                0, 0)
            x.adanet_cache_key = ("image-eval", id(self), i)
            yield x, self.labels[lo:hi]
