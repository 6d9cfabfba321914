"""Pointwise conv at channel counts off the 32 grid: the native kernels
(csrc/conv1x1_ragged.hip forward and dX, conv1x1_dw) against the library
convolution that ADANET_CONV_RAGGED=0 restores, per direction, at the
shapes a 10-, 20-, 30- and 42-filter 3-cell NASNet produces: per stage
(c = f, 2f, 4f on 32x32, 16x16, 8x8) the separable convs' c -> c and the
cell adaptors' 6c -> c. Both paths go through `conv1x1` and autograd, are
alternated in one process and timed with device events; the figures are
medians over rounds with the interquartile range.

    python benchmarks/conv1x1_ragged_bench.py [--iters 1000] [--rounds 7]
                                              [--only Ci,Co,HW]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")

B = 256
SHAPES = [(ci, c, hw) for f in (10, 20, 30, 42)
          for c, hw in ((f, 1024), (2 * f, 256), (4 * f, 64))
          for ci in (c, 6 * c)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default=None, metavar="Ci,Co,HW",
                    help="one shape, for a kernel trace of its own")
    args = ap.parse_args()
    shapes = SHAPES
    if args.only:
        shapes = [tuple(int(v) for v in args.only.split(","))]
    from adanet_amd.ops import _extension
    from adanet_amd.ops.conv import conv1x1
    _extension.require()
    dev = "cuda:0"
    torch.manual_seed(0)

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.iters * 1e3  # us

    for ci, co, hw in shapes:
        side = int(hw ** 0.5)
        x = torch.randn(B, ci, side, side, device=dev).to(
            torch.bfloat16).requires_grad_(True)
        w = torch.randn(co, ci, device=dev).mul(0.1).to(
            torch.bfloat16).requires_grad_(True)
        dy = torch.randn(B, co, side, side, device=dev).to(torch.bfloat16)

        def calls(ragged):
            os.environ["ADANET_CONV_RAGGED"] = ragged
            # A graph keeps the path it was built on. One graph per gradient:
            # a custom Function computes every gradient its inputs require,
            # whichever of them autograd.grad asks for.
            y_x = conv1x1(x, w.detach())
            y_w = conv1x1(x.detach(), w)

            def fwd():
                os.environ["ADANET_CONV_RAGGED"] = ragged
                with torch.no_grad():
                    conv1x1(x, w)
            return {"fwd": fwd,
                    "dx": lambda: torch.autograd.grad(y_x, x, dy,
                                                      retain_graph=True),
                    "dw": lambda: torch.autograd.grad(y_w, w, dy,
                                                      retain_graph=True)}

        paths = {"native": calls("1"), "library": calls("0")}
        row = {"Ci": ci, "Co": co, "HW": hw, "B": B}
        for d in ("fwd", "dx", "dw"):
            for fn in (paths["native"][d], paths["library"][d]):
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            t = {"native": [], "library": []}
            for _ in range(args.rounds):
                for name in ("library", "native"):
                    t[name].append(timed(paths[name][d]))
            for name in t:
                q = statistics.quantiles(t[name], n=4)
                row["%s_%s_us" % (d, name)] = round(
                    statistics.median(t[name]), 1)
                row["%s_%s_iqr" % (d, name)] = round(q[2] - q[0], 1)
            row["%s_speedup" % d] = round(
                row["%s_library_us" % d] / row["%s_native_us" % d], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
