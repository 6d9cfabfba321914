"""Bit-exact regression of the two-stage reduction kernels (colsum,
relu_bwd_colsum, BatchNorm stats/backward, mixer, depthwise dW) against
hashes recorded from the kernels as they stood before they were rebuilt on
the shared block-sum / slot-sum helpers (tests/golden/reduction_bits.json).

Inputs come from integer arithmetic on the CPU (no torch RNG), so the
recording is reproducible anywhere: `python tests/test_gpu_reduction_bits.py
--record` on an MI355X rewrites the JSON.
"""

import hashlib
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "reduction_bits.json")
DEV = "cuda:0"


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _ints(shape, salt):
    """k in [-128, 127] from a multiplicative hash of the flat index."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    return (((i * 2654435761 + salt) >> 8) % 256 - 128).reshape(shape)


def _bf16(shape, salt):
    # k/64 is exact in bf16 (8 significant bits).
    return (_ints(shape, salt).float() / 64).to(torch.bfloat16).to(DEV)


def _f32(shape, salt, scale=1.0 / 64, shift=0.0):
    return (_ints(shape, salt).float() * scale + shift).to(DEV)


def _sha(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------ cases
def _colsum(B, C, sliced, accum):
    def run(ext):
        x = _bf16((B, C + 6), 11)[:, :C] if sliced else _bf16((B, C), 11)
        out = _f32((C,), 12)
        ext.colsum_bf16(x, out, accum)
        return {"out": out}
    return run


def _relu_bwd_colsum(B, C, scale):
    def run(ext):
        dy, y = _bf16((B, C), 21), _bf16((B, C), 22)
        dz = torch.empty_like(dy)
        db = _f32((C,), 23)
        ext.relu_bwd_colsum(dy, y, dz, db, scale)
        return {"dz": dz, "db": db}
    return run


def _bn_stats(shape, running):
    def run(ext):
        C = shape[1]
        x = _bf16(shape, 31)
        mean = torch.empty(C, device=DEV)
        rstd = torch.empty(C, device=DEV)
        out = {"mean": mean, "rstd": rstd}
        rm = rv = None
        if running:
            rm = _f32((C,), 32)
            rv = _f32((C,), 33, shift=2.5)
            out.update(running_mean=rm, running_var=rv)
        ext.batchnorm_stats(x, mean, rstd, rm, rv, 1e-3, 0.1)
        return out
    return run


def _bn_bwd(shape, with_gamma):
    def run(ext):
        C = shape[1]
        x, dy = _bf16(shape, 41), _bf16(shape, 42)
        mean = _f32((C,), 43, scale=1.0 / 512)
        rstd = _f32((C,), 44, scale=1.0 / 256, shift=1.0)
        gamma = _f32((C,), 45, shift=2.5) if with_gamma else None
        dx = torch.empty_like(x)
        sdy = torch.empty(C, device=DEV)
        sdyx = torch.empty(C, device=DEV)
        ext.batchnorm_bwd(x, dy, dx, mean, rstd, gamma, sdy, sdyx)
        return {"dx": dx, "sdy": sdy, "sdyx": sdyx}
    return run


def _mixer(J, B, C, vector_mode):
    def run(ext):
        members = [_bf16((B, C), 50 + j) for j in range(J)]
        # one member is a row-strided view (ld != C)
        members[1] = _bf16((B, C + 6), 70)[:, :C]
        wshape = (J, C) if vector_mode else (J,)
        w = _f32(wshape, 71)
        bias = _f32((C,), 72)
        out = torch.empty(B, C, device=DEV, dtype=torch.bfloat16)
        ext.mixer_fwd_direct(members, w, bias, out, vector_mode)
        dY = _bf16((B, C), 73)
        dw = _f32(wshape, 74)  # accumulated into, so start non-zero
        ext.mixer_bwd_dw_direct(members, dY, dw, vector_mode)
        dL = torch.empty(B, C, device=DEV, dtype=torch.bfloat16)
        ext.mixer_bwd_dlogits(dY, w, dL, J - 1, vector_mode)
        return {"out": out, "dw": dw, "dL": dL}
    return run


def _depthwise_dw(B, C, H, KS):
    def run(ext):
        x, dy = _bf16((B, C, H, H), 81), _bf16((B, C, H, H), 82)
        dw = torch.empty(C, KS * KS, device=DEV)
        ext.depthwise_bwd_dw(x, dy, dw, 1, KS // 2)
        return {"dw": dw}
    return run


BN_CHUNKED = [(8, 32, 16, 16),   # vectorised, 8 chunks
              (4, 8, 5, 3),      # scalar, chunked
              (70, 4, 8, 8)]     # 64 chunks, uneven image ranges
BN_DIRECT = [(1, 16, 8, 8),      # direct, vectorised
             (1, 8, 5, 3),       # direct, scalar
             (2, 1100, 4, 4)]    # direct because C > 1024


def _cases():
    cases = {}
    for accum in (0, 1):
        # 8 chunks / single chunk, no workspace / 125 chunks (lane loop
        # wraps) over 3 stripes / ldx != C
        for B, C, sliced in [(64, 10, False), (5, 300, False),
                             (1000, 513, False), (64, 10, True)]:
            cases["colsum-%dx%d%s-accum%d" % (
                B, C, "-sliced" if sliced else "", accum)] = _colsum(
                    B, C, sliced, accum)
    for B, C in [(64, 10), (1000, 513)]:
        for scale in (1.0, 1.25):
            cases["relu_bwd_colsum-%dx%d-scale%g" % (B, C, scale)] = (
                _relu_bwd_colsum(B, C, scale))
    for shape in BN_CHUNKED + BN_DIRECT:
        for running in (True, False):
            cases["bn_stats-%s-%s" % (
                "x".join(map(str, shape)),
                "running" if running else "norunning")] = _bn_stats(
                    shape, running)
    for shape in BN_CHUNKED:
        for with_gamma in (True, False):
            cases["bn_bwd-%s-%s" % (
                "x".join(map(str, shape)),
                "gamma" if with_gamma else "nogamma")] = _bn_bwd(
                    shape, with_gamma)
    # 11 members: two launches (8+3), the accum path; B=512: grid.x = 3 in
    # the scalar dW kernel
    for J, B, C in [(5, 128, 10), (11, 128, 10), (3, 512, 10)]:
        for vm in (0, 1):
            cases["mixer-%dx%dx%d-%s" % (
                J, B, C, "vector" if vm else "scalar")] = _mixer(J, B, C, vm)
    # the two shapes of test_depthwise_dw_bitrepeat: both dispatch to the
    # deterministic (slot-reduced) dW kernel
    for B, C, H, KS in [(5, 7, 16, 3), (64, 32, 32, 5)]:
        cases["depthwise_dw-%dx%dx%d-k%d" % (B, C, H, KS)] = _depthwise_dw(
            B, C, H, KS)
    return cases


CASES = _cases()


def _run(name):
    out = CASES[name](_ext())
    torch.cuda.synchronize()
    return {k: _sha(v) for k, v in sorted(out.items())}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_reduction_bits(name, golden):
    got = _run(name)
    for k in got:
        print(name, k, got[k])
    assert got == golden[name]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    if "--record" not in sys.argv[1:]:
        sys.exit("usage: test_gpu_reduction_bits.py --record")
    out_path = GOLDEN
    for a in sys.argv[1:]:
        if a.startswith("--out="):
            out_path = a[len("--out="):]
    rec = {name: _run(name) for name in sorted(CASES)}
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases to %s" % (len(rec), out_path))
