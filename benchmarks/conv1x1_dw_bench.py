"""Pointwise-conv weight gradient: conv1x1_dw (reads dy and x in [B, C, HW])
vs the copy path (two channel-major permute copies + gemm_nt_bf16), at the
NASNet pointwise shapes. Device-event timing, both paths alternated in one
process; bytes are the compulsory traffic of each path, from shapes alone.

    python benchmarks/conv1x1_dw_bench.py [--iters 200] [--rounds 5]
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")

B = 96
# (Co, Ci, HW): NASNet(filters=32) pointwise convs per stage, plus the 3x3
# stem as it reaches the GEMM (im2col, Ci*9 = 27 zero-padded to 32).
SHAPES = [(co, ci, hw) for hw in (1024, 256, 64)
          for co in (32, 64, 128) for ci in (32, 64, 128)]
SHAPES.append((96, 32, 1024))


def bytes_moved(co, ci, hw):
    """(direct, copy) bytes: operands read once, dW written once, the fp32
    split-K slots written and read once; the copy path also reads and writes
    each operand once more."""
    k = B * hw
    t64 = ((co + 63) // 64) * ((ci + 63) // 64)
    ksplit = max(1, min(512 // t64, k // 256))
    per = -(-(k // 32) // ksplit)
    ksplit = -(-(k // 32) // per)
    gemm = 2 * k * (co + ci) + 2 * co * ci
    if ksplit > 1:
        gemm += 2 * 4 * ksplit * co * ci
    return gemm, gemm + 2 * 2 * k * (co + ci)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from adanet_amd.ops import _extension
    ext = _extension.require()
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

    for co, ci, hw in SHAPES:
        dy3 = torch.randn(B, co, hw, device=dev).to(torch.bfloat16)
        x3 = torch.randn(B, ci, hw, device=dev).to(torch.bfloat16)
        dw_d = torch.empty(co, ci, device=dev, dtype=torch.bfloat16)
        dw_c = torch.empty(co, ci, device=dev, dtype=torch.bfloat16)

        def direct():
            ext.conv1x1_dw(dy3, x3, dw_d)

        def copy():
            dz = dy3.permute(1, 0, 2).reshape(co, B * hw).contiguous()
            xf = x3.permute(1, 0, 2).reshape(ci, B * hw).contiguous()
            ext.gemm_nt_bf16(dz, xf, dw_c, None, 0)

        for _ in range(20):
            direct()
            copy()
        torch.cuda.synchronize()
        t_d, t_c = [], []
        for _ in range(args.rounds):
            t_c.append(timed(copy))
            t_d.append(timed(direct))
        by_d, by_c = bytes_moved(co, ci, hw)
        print(json.dumps({
            "Co": co, "Ci": ci, "HW": hw, "K": B * hw,
            "copy_us": round(min(t_c), 2), "copy_us_max": round(max(t_c), 2),
            "direct_us": round(min(t_d), 2),
            "direct_us_max": round(max(t_d), 2),
            "copy_MB": round(by_c / 1e6, 2), "direct_MB": round(by_d / 1e6, 2),
            "bit_identical": bool(torch.equal(dw_d, dw_c))}))


if __name__ == "__main__":
    main()
