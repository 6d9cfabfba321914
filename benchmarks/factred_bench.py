"""FactorizedReduction: the fused kernels (csrc/factred.hip) against the
unfused chain, eval forward and training forward + backward.

Both paths live in the module (ADANET_FUSED_FACTRED / ADANET_FACTRED_TRAIN
select them), so one process times them on the same inputs, alternating
fused and chain windows; each figure is the median over the rounds of a
device-event window's mean, in microseconds per call.

    python benchmarks/factred_bench.py [--iters 2000] [--rounds 5]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(128, 96, 64, 32, 32), (128, 320, 128, 16, 16),
          (128, 96, 32, 32, 32)]


def window(fn, iters):
    start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "factred_bench needs a GPU"
    from adanet_amd.models.nasnet import FactorizedReduction

    for B, ci, co, H, W in SHAPES:
        torch.manual_seed(0)
        m = FactorizedReduction(ci, co).to(torch.bfloat16).cuda()
        x = torch.randn(B, ci, H, W, device="cuda").to(torch.bfloat16)

        def evalfwd():
            with torch.no_grad():
                m(x)

        def train():
            xi = x.detach().requires_grad_()
            y = m(xi)
            y.backward(y)
            m.zero_grad(set_to_none=True)

        for mode, fn, var in (("eval_fwd", evalfwd, "ADANET_FUSED_FACTRED"),
                              ("train_fwd_bwd", train,
                               "ADANET_FACTRED_TRAIN")):
            m.train(mode != "eval_fwd")
            # with the eval kernel off, or the training switch off, the
            # module runs the chain
            times = {"1": [], "0": []}
            for rnd in range(args.rounds + 1):
                for flag in ("1", "0"):
                    os.environ[var] = flag
                    t = window(fn, args.iters)
                    if rnd:             # round 0 warms both paths up
                        times[flag].append(t)
            os.environ.pop(var)
            fused, chain = (statistics.median(times[f]) for f in "10")
            print(json.dumps({
                "shape": [B, ci, co, H, W], "mode": mode,
                "fused_us": round(fused, 1), "chain_us": round(chain, 1),
                "fused_range_us": [round(min(times["1"]), 1),
                                   round(max(times["1"]), 1)],
                "chain_range_us": [round(min(times["0"]), 1),
                                   round(max(times["0"]), 1)],
                "speedup": round(chain / fused, 2)}), flush=True)


if __name__ == "__main__":
    main()
