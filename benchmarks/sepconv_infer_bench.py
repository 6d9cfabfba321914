"""Fused eval-mode separable-conv half-stack (csrc/sepconv_infer.hip) against
the four-launch chain it replaces (clamp, depthwise_fwd, gemm_tr_batched,
bn_norm), in one process on one GPU.

Shapes are the NASNet cell ones: C in {32, 64, 128} at 32x32 / 16x16 / 8x8,
K in {3, 5, 7} at stride 1 and 2, plus K = 1 (ReLU-Conv-BN), at
improve_nas_bench's batch of 256. Per shape the two paths are timed in
alternating windows of device-event time (--rounds windows of --iters calls
each, after a warm-up of both); the table gives the median window of each and
their ratio, and the last column the spread (max/min window) of the fused
path. Prints a markdown table; --json also writes the rows to a file.
"""

import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from adanet_amd.ops import conv  # noqa: E402
from adanet_amd.ops.batchnorm import HipBatchNorm2d  # noqa: E402


def _window(fn, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters     # us per call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    print("| C | HxW | K | stride | chain us | fused us | chain/fused | "
          "fused spread | max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    for c, hw in ((32, 32), (64, 16), (128, 8), (32, 16), (64, 32),
                  (128, 16), (64, 8), (128, 32), (32, 8)):
        for k, stride in ((1, 1), (3, 1), (3, 2), (5, 1), (5, 2), (7, 1),
                          (7, 2)):
            bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
            x = bf(args.batch, c, hw, hw)
            dw = bf(c, 1, k, k) if k > 1 else None
            pw = bf(c, c) / 8
            bn = HipBatchNorm2d(c).to(dev).eval()
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
            pad = k // 2
            if not conv.sepconv_infer_supported(x, dw, pw, stride, pad):
                print("| %d | %dx%d | %d | %d | routed to the chain |||||"
                      % (c, hw, hw, k, stride))
                continue

            def chain():
                y = torch.relu(x)
                if dw is not None:
                    y = conv.depthwise_conv2d(y, dw, stride, pad)
                return bn.infer(conv.conv1x1(y, pw))

            def fused():
                return conv.sepconv_bn_infer(x, dw, pw, bn, stride, pad)

            with torch.no_grad():
                diff = (chain().float() - fused().float()).abs().max().item()
                for fn in (chain, fused):
                    _window(fn, 10)
                tc, tf = [], []
                for _ in range(args.rounds):
                    tc.append(_window(chain, args.iters))
                    tf.append(_window(fused, args.iters))
            row = dict(C=c, HW=hw, K=k, stride=stride,
                       chain_us=statistics.median(tc),
                       fused_us=statistics.median(tf),
                       fused_spread=max(tf) / min(tf), max_abs_diff=diff)
            rows.append(row)
            print("| %d | %dx%d | %d | %d | %.1f | %.1f | %.2f | %.2f | %g |"
                  % (c, hw, hw, k, stride, row["chain_us"], row["fused_us"],
                     row["chain_us"] / row["fused_us"], row["fused_spread"],
                     diff), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
