"""Training-step time of a NasNetCIFAR at the reference's own filter counts
(off the 32 grid), native pointwise convs against ADANET_CONV_RAGGED=0 (the
library convolution), alternated in one process on one model. A step is
forward, cross-entropy, backward and a torch SGD update, eager, batch 256;
a round is `--steps` steps between two device synchronisations on the host
clock. Prints one JSON line per filter count: median ms per step and
interquartile range per path.

    python benchmarks/nasnet_ragged_step_bench.py [--filters 10 20]
                                                  [--steps 30] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    from adanet_amd.models.nasnet import NasNetCIFAR
    from adanet_amd.ops import _extension
    from adanet_amd.ops.linear import HipLinear
    _extension.require()
    dev = "cuda:0"
    for f in args.filters:
        torch.manual_seed(0)
        m = NasNetCIFAR(num_cells=3, num_conv_filters=f).to(dev).to(
            torch.bfloat16)
        for mod in m.modules():
            if isinstance(mod, HipLinear) and mod.bias is not None:
                mod.bias.data = mod.bias.data.float()
        m.train()
        opt = torch.optim.SGD(m.parameters(), lr=0.01)
        x = torch.randn(args.batch, 3, 32, 32, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 10, (args.batch,), device=dev)

        def run(ragged, steps):
            os.environ["ADANET_CONV_RAGGED"] = ragged
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                _, logits = m(x)
                loss = torch.nn.functional.cross_entropy(logits.float(), y)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        for ragged in ("1", "0"):
            run(ragged, 5)
        t = {"1": [], "0": []}
        for _ in range(args.rounds):
            for ragged in ("0", "1"):
                t[ragged].append(run(ragged, args.steps))
        row = {"filters": f, "batch": args.batch, "steps": args.steps,
               "rounds": args.rounds}
        for ragged, name in (("1", "native"), ("0", "library")):
            q = statistics.quantiles(t[ragged], n=4)
            row[name + "_ms"] = round(statistics.median(t[ragged]), 2)
            row[name + "_iqr"] = round(q[2] - q[0], 2)
        row["speedup"] = round(row["library_ms"] / row["native_ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
