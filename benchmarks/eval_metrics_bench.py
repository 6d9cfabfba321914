"""Estimator.evaluate per batch: streaming=True (device-resident head state,
csrc/eval_metrics.hip, one read-back at the end) against the default path
(head.loss + head.metrics per batch, each ending in a host sync).

A small DNN ensemble is trained for a few steps and frozen; both paths then
evaluate the same device-resident batches of 1024 examples x 10 classes.
The host clock runs around whole evaluate() calls, which end in a D2H read,
so the time covers all queued device work. After a warm-up of each path the
two are alternated inside one process; the medians are reported.

python benchmarks/eval_metrics_bench.py [--batches 200 --rounds 7] [--out f]
"""
import argparse
import itertools
import json
import sys
import tempfile
import time

import torch

sys.path.insert(0, ".")
import adanet_amd
from adanet_amd.head import MultiClassHead
from adanet_amd.models import simple_dnn

BATCH, DIM, CLASSES = 1024, 64, 10


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, default=200)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--layer-size", type=int, default=256)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "eval_metrics_bench needs a GPU"
    dev = torch.device("cuda:0")

    g = torch.Generator().manual_seed(0)
    n = BATCH * 8
    X = torch.randn(n, DIM, generator=g)
    Y = (X @ torch.randn(DIM, CLASSES, generator=g)).argmax(dim=1)
    Xd, Yd = X.to(dev), Y.to(dev)
    batches = [(Xd[(i % 8) * BATCH:(i % 8 + 1) * BATCH],
                Yd[(i % 8) * BATCH:(i % 8 + 1) * BATCH])
               for i in range(args.batches)]

    def train_fn():
        return itertools.cycle(batches[:8])

    with tempfile.TemporaryDirectory() as model_dir:
        est = adanet_amd.Estimator(
            head=MultiClassHead(CLASSES),
            subnetwork_generator=simple_dnn.Generator(
                layer_size=args.layer_size),
            max_iteration_steps=10, model_dir=model_dir,
            config=adanet_amd.RunConfig(tf_random_seed=42))
        est.train(train_fn, max_steps=10)

        def run(streaming):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = est.evaluate(lambda: iter(batches), streaming=streaming)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / len(batches), res

        for streaming in (False, True):     # warm-up of both paths
            run(streaming)
        times = {False: [], True: []}
        for _ in range(args.rounds):        # alternate the variants
            for streaming in (False, True):
                ms, res = run(streaming)
                times[streaming].append(ms)
                last = res if streaming else None
        _, plain = run(False)

    out = {
        "bench": "Estimator.evaluate per batch, default vs streaming",
        "device": torch.cuda.get_device_name(0),
        "batch": BATCH, "classes": CLASSES, "batches": len(batches),
        "rounds": args.rounds,
        "default_ms_per_batch": _median(times[False]),
        "streaming_ms_per_batch": _median(times[True]),
        "default_all": times[False], "streaming_all": times[True],
        "speedup": _median(times[False]) / _median(times[True]),
        "accuracy": {"default": plain["accuracy"],
                     "streaming": last["accuracy"]},
        "average_loss": {"default": plain["average_loss"],
                         "streaming": last["average_loss"]},
    }
    print("default %.4f ms/batch, streaming %.4f ms/batch (x%.2f)" % (
        out["default_ms_per_batch"], out["streaming_ms_per_batch"],
        out["speedup"]))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
