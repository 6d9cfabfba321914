"""Time the fused ReLU -> pointwise kernels against the chain they replace.

forward   relu_pointwise_fwd                       vs  torch.relu + gemm_tr_batched
backward  relu_pointwise_bwd_dx + relu_conv1x1_dw  vs  gemm_tr_batched (dX)
                                                       + threshold_backward
                                                       + conv1x1_dw
at the ReluConvBN shapes of NASNet(filters=32, batch 256, 3 cells). Each
sample is one pass over a ring of buffer sets larger than the caches, timed
with device events; fused and chain samples alternate, and the medians and
the quartile spread of the same run are reported. Outputs are compared first.

python benchmarks/relu_pointwise_bench.py [--out relu_pw.json]
"""

import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "benchmarks")
from adanet_amd.ops import _extension  # noqa: E402
from relu_depthwise_bench import RING_BYTES, _compare  # noqa: E402

# (B, Ci, Co, H): pre0/pre1 of the normal and reduction cells, then two
# narrower 8x8 classes that the routing rule of ops/conv.py also admits
SHAPES = [
    (256, 96, 32, 32), (256, 96, 64, 32), (256, 160, 64, 32),
    (256, 320, 64, 16), (256, 320, 128, 16), (256, 640, 128, 8),
    (256, 640, 64, 8), (256, 96, 32, 8),
]


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
    for (B, Ci, Co, H) in SHAPES:
        HW = H * H
        torch.manual_seed(B + Ci + Co + H)
        bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
        # the ring is sized by the least a variant touches per set (the
        # fused forward: x and y), so that no variant runs from the cache
        touched = 2 * B * HW * (Ci + Co)
        sets = []
        for _ in range(max(2, -(-RING_BYTES // touched))):
            x, dy = bf(B, Ci, H, H), bf(B, Co, H, H)
            sets.append(dict(
                x=x, dy=dy, w=bf(Co, Ci) / 8, r=torch.empty_like(x),
                dr=torch.empty_like(x), dx=torch.empty_like(x),
                y=torch.empty_like(dy), y2=torch.empty_like(dy),
                dw=torch.empty(Co, Ci, device=dev, dtype=torch.bfloat16),
                dw2=torch.empty(Co, Ci, device=dev, dtype=torch.bfloat16)))
        v3 = lambda t: t.view(B, -1, HW)

        def fwd_fused(s):
            ext.relu_pointwise_fwd(s["x"], s["w"], s["y"])

        def fwd_chain(s):
            s["r"] = torch.relu(s["x"])
            ext.gemm_tr_batched(s["w"], v3(s["r"]), v3(s["y2"]), None, 0, 0, 1)

        def bwd_fused(s):
            ext.relu_pointwise_bwd_dx(s["dy"], s["x"], s["w"], s["dx"])
            ext.relu_conv1x1_dw(v3(s["dy"]), v3(s["x"]), s["dw"])

        def bwd_chain(s):
            ext.gemm_tr_batched(s["w"], v3(s["dy"]), v3(s["dr"]), None, 0, 1,
                                1)
            s["dx2"] = torch.ops.aten.threshold_backward(s["dr"], s["r"], 0)
            ext.conv1x1_dw(v3(s["dy"]), v3(s["r"]), s["dw2"])

        s = sets[0]
        for f in (fwd_fused, fwd_chain, bwd_fused, bwd_chain):
            f(s)
        same = bool(torch.equal(s["y"], s["y2"]) and
                    torch.equal(s["dx"], s["dx2"]) and
                    torch.equal(s["dw"], s["dw2"]))
        for t in sets:          # the chain's backward reads the forward's r
            fwd_chain(t)
        row = {"shape": [B, Ci, Co, H], "bit_identical": same,
               "ring": len(sets),
               "fwd": _compare({"fused": fwd_fused, "chain": fwd_chain},
                               sets, args.samples, args.warmup),
               "bwd": _compare({"fused": bwd_fused, "chain": bwd_chain},
                               sets, args.samples, args.warmup)}
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
