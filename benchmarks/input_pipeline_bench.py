"""Input pipeline throughput: host augmentation + DeviceLoader against the
device-resident pipeline, on the same data in the same run.

50,000 synthetic CIFAR-shaped uint8 images, batch 256, augmentation on:

  (a) host    Provider.get_input_fn (Python crop/flip/cutout on fp32) wrapped
              in data.DeviceLoader (pinned staging, H2D copy, bf16 cast);
  (b) device  Provider.get_device_input_fn (data.DeviceImageLoader: uint8
              resident in HBM, augment_draw + augment_apply per batch).

Every timed step reads the first label back to the host, so both paths have
to finish the batch. Nothing consumes the batches: this is the cost of
producing them, not how much of it a training step would hide.

python benchmarks/input_pipeline_bench.py [--steps 50 --warmup 5] [--out f]
"""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")
from adanet_amd.data import DeviceLoader
from adanet_amd.models.cifar import Provider


class SyntheticBytesProvider(Provider):
    """CIFAR-sized random uint8 images; the host path sees them as the real
    providers present bytes to it, floats in [0, 1]."""

    def __init__(self, n_examples: int, **kwargs):
        super().__init__(n_classes=10, **kwargs)
        g = torch.Generator().manual_seed(self.seed or 0)
        self._raw = torch.randint(0, 256, (n_examples,) + tuple(
            self.image_shape), generator=g, dtype=torch.uint8)
        self._Y = torch.randint(0, 10, (n_examples,), generator=g)
        self._X = None

    def _data(self, training: bool):
        if self._X is None:
            self._X = self._raw.float() / 255.0
        return self._X, self._Y

    def _raw_data(self, training: bool):
        return self._raw, self._Y


def _time(input_fn, steps: int, warmup: int, sync) -> float:
    it = iter(input_fn())
    for _ in range(warmup):
        x, y = next(it)
        int(y[0])
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        x, y = next(it)
        int(y[0])  # forces the batch to complete on either path
    sync()
    return (time.perf_counter() - t0) / steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--examples", type=int, default=50000)
    p.add_argument("--only", choices=["host", "device"], default=None,
                   help="time one path alone (e.g. under a profiler)")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    use_gpu = torch.cuda.is_available()
    dev = torch.device("cuda:0") if use_gpu else torch.device("cpu")
    sync = torch.cuda.synchronize if use_gpu else (lambda: None)

    provider = SyntheticBytesProvider(args.examples, batch_size=args.batch,
                                      seed=3)
    paths = {}
    if args.only in (None, "host"):
        host_fn = DeviceLoader(provider.get_input_fn(), dev)
        paths["host"] = _time(host_fn, args.steps, args.warmup, sync)
    if args.only in (None, "device"):
        device_fn = provider.get_device_input_fn(dev)
        paths["device"] = _time(device_fn, args.steps, args.warmup, sync)

    out = {
        "metric": "input_pipeline_batches_per_second",
        "unit": "batches/s",
        "higher_is_better": True,
        "device": torch.cuda.get_device_name(0) if use_gpu else "cpu",
        "batch": args.batch,
        "examples": args.examples,
        "steps": args.steps,
        "warmup": args.warmup,
        "torch_threads": torch.get_num_threads(),
    }
    for name, secs in paths.items():
        out[name + "_batches_per_s"] = 1.0 / secs
        out[name + "_ms_per_batch"] = secs * 1000.0
    if len(paths) == 2:
        out["device_over_host"] = paths["host"] / paths["device"]
    print(json.dumps(out))
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
