"""Fused cell combine (ops/combine.py, csrc/combine.hip) against the unfused
torch composition, forward + backward, at the NAS bench's cell shapes.

Two things are measured, both with device events after a warm-up and with
the variants alternated inside one process:

* op level: ``cell_combine`` (ADANET_FUSED_COMBINE=1) vs the same call with
  the toggle off (x*scale, left+right, torch.cat and autograd's backward),
  drop-path keep 0.9 and 1.0;
* kernel level: the two kernels' host entry points on preallocated buffers,
  with bytes moved computed from the shapes (forward: read left, read
  right, write out; backward: read dy, write dleft, write dright — three
  2-byte passes over n*B*F*H*W elements each) and the achieved GB/s set
  against the HBM3E peak. Both kernels do one multiply-add per 6 bytes, so
  memory bandwidth is the bound. A working set under the 256 MiB Infinity
  Cache can be served from it; the output says so per shape.

python benchmarks/combine_bench.py [--iters 50 --warmup 10] [--out f.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, ".")
from adanet_amd.ops import _extension, combine

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak
HBM_ACHIEVABLE_GBS = 6290.0  # measured float4 copy on the same part
INFINITY_CACHE_BYTES = 256 << 20

# (B, F, H, W, n): the three resolutions of the 3-cell, 32-filter search
SHAPES = [(256, 32, 32, 32, 5), (256, 64, 16, 16, 5), (256, 128, 8, 8, 5)]
KEEPS = [0.9, 1.0]


def _time(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters  # ms


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def bench_shape(shape, keep, iters, warmup, rounds):
    B, F, H, W, n = shape
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)

    def rnd(*s):
        return torch.randn(*s, device=dev, generator=gen).to(torch.bfloat16)

    lefts = [rnd(B, F, H, W).requires_grad_(True) for _ in range(n)]
    rights = [rnd(B, F, H, W).requires_grad_(True) for _ in range(n)]
    dy = rnd(B, n * F, H, W)
    sl = sr = None
    if keep < 1.0:
        def scale():
            return ((torch.rand(B, 1, 1, 1, device=dev, generator=gen) < keep)
                    .to(torch.bfloat16) * (1.0 / keep))
        sl = [scale() for _ in range(n)]
        sr = [scale() for _ in range(n)]

    def op_step():
        out = combine.cell_combine(lefts, rights, sl, sr)
        torch.autograd.grad(out, lefts + rights, dy)

    def run(toggle):
        os.environ["ADANET_FUSED_COMBINE"] = toggle
        return _time(op_step, iters)

    for toggle in ("1", "0"):
        os.environ["ADANET_FUSED_COMBINE"] = toggle
        for _ in range(warmup):
            op_step()
    fused, unfused = [], []
    for _ in range(rounds):  # alternate the variants
        fused.append(run("1"))
        unfused.append(run("0"))
    os.environ["ADANET_FUSED_COMBINE"] = "1"

    # kernel level
    ext = _extension.require()
    elems = n * B * F * H * W
    bytes_pass3 = 3 * 2 * elems
    out = torch.empty(B, n * F, H, W, device=dev, dtype=torch.bfloat16)
    ls = [t.detach() for t in lefts]
    rs = [t.detach() for t in rights]
    k_sl, k_sr = (sl, sr) if sl is not None else ([], [])

    def k_fwd():
        ext.cell_combine_fwd(ls, rs, k_sl, k_sr, out, 0)

    res = {
        "shape": {"B": B, "F": F, "H": H, "W": W, "n": n}, "keep": keep,
        "op_fwd_bwd_ms": {"fused": _median(fused), "unfused": _median(unfused),
                          "fused_all": fused, "unfused_all": unfused},
        "speedup": _median(unfused) / _median(fused),
        "bytes_per_kernel": bytes_pass3,
        "fits_infinity_cache": bytes_pass3 <= INFINITY_CACHE_BYTES,
    }
    for _ in range(warmup):
        k_fwd()
    t = _median([_time(k_fwd, iters) for _ in range(rounds)])
    res["fwd_kernel"] = _rate(t, bytes_pass3)
    if sl is not None:
        dl = [torch.empty_like(t) for t in ls]
        dr = [torch.empty_like(t) for t in rs]

        def k_bwd():
            ext.cell_combine_bwd(dy, sl, sr, dl, dr, 0)

        for _ in range(warmup):
            k_bwd()
        t = _median([_time(k_bwd, iters) for _ in range(rounds)])
        res["bwd_kernel"] = _rate(t, bytes_pass3)
    else:
        res["bwd_kernel"] = None  # no kernel: gradients are slices of dy
    return res


def _rate(ms, nbytes):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"ms": ms, "GBps": gbs, "bound": "memory bandwidth",
            "share_of_hbm_peak": gbs / HBM_PEAK_GBS,
            "share_of_hbm_achievable": gbs / HBM_ACHIEVABLE_GBS}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "combine_bench needs a GPU"
    rows = [bench_shape(s, k, args.iters, args.warmup, args.rounds)
            for s in SHAPES for k in KEEPS]
    out = {"bench": "cell_combine fused vs unfused, fwd+bwd",
           "device": torch.cuda.get_device_name(0),
           "hbm_peak_GBps": HBM_PEAK_GBS,
           "hbm_achievable_GBps": HBM_ACHIEVABLE_GBS, "rows": rows}
    for r in rows:
        s = r["shape"]
        bwd = r["bwd_kernel"]
        print("B%d F%d %dx%d n%d keep %.1f: fused %.3f ms unfused %.3f ms "
              "(x%.2f) | fwd %.0f GB/s (%.0f%% of HBM peak) bwd %s" % (
                  s["B"], s["F"], s["H"], s["W"], s["n"], r["keep"],
                  r["op_fwd_bwd_ms"]["fused"], r["op_fwd_bwd_ms"]["unfused"],
                  r["speedup"], r["fwd_kernel"]["GBps"],
                  100 * r["fwd_kernel"]["share_of_hbm_peak"],
                  "%.0f GB/s (%.0f%%)" % (bwd["GBps"],
                                          100 * bwd["share_of_hbm_peak"])
                  if bwd else "no kernel"))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
