"""Time the fused ReLU -> depthwise kernels against the chain they replace.

forward   relu_depthwise_fwd           vs  torch.relu + depthwise_fwd
backward  relu_depthwise_bwd (dx, dw)  vs  depthwise_bwd_dw + depthwise_bwd_dx
                                           + threshold_backward
and, where the strip-tiled kernels take the shape, against both
strip     relu_depthwise_strip_fwd;  relu_depthwise_strip_bwd_dx (strip_dx)
          + relu_depthwise_bwd's dW-only launch and reduce (strip_dw),
          and relu_depthwise_strip_bwd_dw in its place (strip_dw_new)
at the NASNet(filters=32) depthwise shapes of depthwise_bench.py. Each sample
is one pass over a ring of buffer sets larger than the caches, timed with
device events; fused and chain samples alternate, and the medians and the
quartile spread of the same run are reported. Outputs are compared first.

python benchmarks/relu_depthwise_bench.py [--out relu_dw.json]
"""

import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from adanet_amd.ops import _extension  # noqa: E402

# (B, C, H, KS, stride), as depthwise_bench.SHAPES (importing that module
# would run its device set-up twice).
SHAPES = [
    (256, 32, 32, 5, 1), (256, 32, 32, 3, 1), (256, 64, 16, 5, 1),
    (256, 64, 16, 3, 1), (256, 160, 8, 5, 1), (256, 32, 32, 5, 2),
    (256, 64, 16, 7, 2), (256, 64, 16, 7, 1), (64, 48, 17, 5, 1),
]
RING_BYTES = 512 << 20      # above the 256 MB last-level cache


def _sample(fn, sets):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    passes = max(1, 64 // len(sets))        # at least 64 calls per sample
    start.record()
    for _ in range(passes):
        for s in sets:
            fn(s)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / (passes * len(sets))  # us / call


def _compare(fns, sets, samples, warmup):
    """Median and interquartile range, in us per call, of each of `fns`
    (name -> callable), their samples interleaved."""
    for _ in range(warmup):
        for f in fns.values():
            _sample(f, sets)
    t = {k: [] for k in fns}
    for _ in range(samples):
        for k, f in fns.items():
            t[k].append(_sample(f, sets))
    out = {}
    for k, v in t.items():
        q = statistics.quantiles(v, n=4)
        out[k + "_us"] = round(statistics.median(v), 2)
        out[k + "_iqr_us"] = round(q[2] - q[0], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ext = _extension.require()
    dev = "cuda:0"
    rows = []
    for (B, C, H, KS, stride) in SHAPES:
        pad = KS // 2
        OH = (H + 2 * pad - KS) // stride + 1
        torch.manual_seed(B + C + H + KS + stride)
        bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
        per_set = 2 * (4 * B * C * H * H + 3 * B * C * OH * OH)
        sets = []
        for _ in range(max(2, RING_BYTES // per_set)):
            x, dy = bf(B, C, H, H), bf(B, C, OH, OH)
            sets.append(dict(
                x=x, dy=dy, w=bf(C, 1, KS, KS), r=torch.empty_like(x),
                dr=torch.empty_like(x), dx=torch.empty_like(x),
                y=torch.empty_like(dy), y2=torch.empty_like(dy),
                dw=torch.empty(C * KS * KS, device=dev),
                dw2=torch.empty(C * KS * KS, device=dev)))

        def fwd_fused(s):
            ext.relu_depthwise_fwd(s["x"], s["w"], s["y"], stride, pad)

        def fwd_chain(s):
            s["r"] = torch.relu(s["x"])
            ext.depthwise_fwd(s["r"], s["w"], s["y2"], stride, pad)

        def bwd_fused(s):
            ext.relu_depthwise_bwd(s["x"], s["dy"], s["w"], s["dx"], s["dw"],
                                   stride, pad)

        def bwd_split(s):       # the same kernel, one half per launch
            ext.relu_depthwise_bwd(s["x"], s["dy"], s["w"], s["dx"], None,
                                   stride, pad)
            ext.relu_depthwise_bwd(s["x"], s["dy"], s["w"], None, s["dw"],
                                   stride, pad)

        def bwd_chain(s):
            ext.depthwise_bwd_dw(s["r"], s["dy"], s["dw2"], stride, pad)
            ext.depthwise_bwd_dx(s["dy"], s["w"], s["dr"], stride, pad)
            s["dx2"] = torch.ops.aten.threshold_backward(s["dr"], s["r"], 0)

        def fwd_strip(s):
            ext.relu_depthwise_strip_fwd(s["x"], s["w"], s["y"], stride, pad)

        def bwd_strip_dx(s):
            ext.relu_depthwise_strip_bwd_dx(s["x"], s["dy"], s["w"], s["dx"],
                                            stride, pad)

        def bwd_strip_dw(s):
            ext.relu_depthwise_bwd(s["x"], s["dy"], s["w"], None, s["dw"],
                                   stride, pad)

        def bwd_strip_dw_new(s):
            ext.relu_depthwise_strip_bwd_dw(s["x"], s["dy"], s["dw"], stride,
                                            pad)

        def bwd_strip(s):
            bwd_strip_dx(s)
            bwd_strip_dw(s)

        s = sets[0]
        for f in (fwd_fused, fwd_chain, bwd_fused, bwd_chain):
            f(s)
        same = bool(torch.equal(s["y"], s["y2"]) and
                    torch.equal(s["dx"], s["dx2"]) and
                    torch.equal(s["dw"], s["dw2"]))
        fwd = {"fused": fwd_fused, "chain": fwd_chain}
        bwd = {"fused": bwd_fused, "split": bwd_split, "chain": bwd_chain}
        if ext.relu_depthwise_strip_supported(C, H, H, KS, stride, pad):
            for t in (s["y"], s["dx"], s["dw"]):
                t.fill_(3.0)
            fwd_strip(s)
            bwd_strip(s)
            same = bool(same and torch.equal(s["y"], s["y2"]) and
                        torch.equal(s["dx"], s["dx2"]) and
                        torch.equal(s["dw"], s["dw2"]))
            s["dw"].fill_(3.0)
            bwd_strip_dw_new(s)
            same = bool(same and torch.equal(s["dw"], s["dw2"]))
            fwd["strip"] = fwd_strip
            bwd.update(strip=bwd_strip, strip_dx=bwd_strip_dx,
                       strip_dw=bwd_strip_dw, strip_dw_new=bwd_strip_dw_new)
        row = {"shape": [B, C, H, KS, stride], "bit_identical": same,
               "ring": len(sets),
               "fwd": _compare(fwd, sets, args.samples, args.warmup),
               "bwd": _compare(bwd, sets, args.samples, args.warmup)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del sets
        torch.cuda.empty_cache()
    if args.out:
        json.dump(rows, open(args.out, "w"), indent=1)
    if not all(r["bit_identical"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
