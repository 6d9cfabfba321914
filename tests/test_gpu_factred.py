"""factred: the fused factorized-reduction forward, dX and dW kernels against
exact arithmetic, through the NASNet module, and their argument checks."""

import collections
import copy

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 32, 32, 8, 8),      # one chunk, a partial tile, 16-row halves
    (1, 64, 64, 16, 16),    # two chunks
    (2, 32, 128, 32, 32),   # several pixel tiles, the widest wave grid
    (1, 96, 96, 9, 9),      # odd size: zero column and row on the 2nd path
    (2, 32, 64, 7, 10),     # W % 8 != 0: scalar staging, non-square
    (5, 32, 32, 17, 24),    # odd H on the vector path, ragged second tile
]


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _compose(x, w1, w2):
    r = F.relu(x)
    shifted = F.pad(r, (0, 1, 0, 1))[:, :, 1::2, 1::2]
    return torch.cat([torch.einsum("oi,bihw->bohw", w1, r[:, :, ::2, ::2]),
                      torch.einsum("oi,bihw->bohw", w2, shifted)], dim=1)


def _eighths(B, Ci, Co, H, W):
    # n/8 with n in [-8, 8): products are multiples of 1/64 and every fp32
    # partial sum stays far below 2^24 of them, so any summation order is
    # exact; mean, beta in quarters and rstd, gamma powers of two keep
    # BatchNorm exact too. No tolerance anywhere.
    g = torch.Generator().manual_seed(B + Ci + Co + H * W)
    e = lambda *s: torch.randint(-8, 8, s, generator=g).double() / 8
    return g, e, e(B, Ci, H, W), e(Co // 2, Ci), e(Co // 2, Ci)


def _bf(t):
    return t.to(DEV, torch.bfloat16)


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("B,Ci,Co,H,W", SHAPES)
def test_factred_fwd_exact(B, Ci, Co, H, W, bn):
    g, e, x, w1, w2 = _eighths(B, Ci, Co, H, W)
    want = _compose(x, w1, w2).bfloat16()
    stats = [None] * 4
    if bn:
        pick = lambda: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[
            torch.randint(0, 3, (Co,), generator=g)]
        mean, rstd, gamma, beta = e(Co) * 2, pick(), pick(), e(Co) * 2
        c = lambda t: t.view(1, -1, 1, 1)
        want = ((want.double() - c(mean)) * c(rstd) * c(gamma)
                + c(beta)).bfloat16()
        stats = [t.to(DEV, torch.float32) for t in (mean, rstd, gamma, beta)]
    y = torch.empty(want.shape, device=DEV, dtype=torch.bfloat16)
    _ext().factred_fwd(_bf(x), _bf(w1), _bf(w2), *stats, y)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("B,Ci,Co,H,W,split,slots", [
    s + (0, None) for s in SHAPES] + [
    (5, 32, 32, 17, 24, 4, 4),   # 10 K tiles in slots of 3, 3, 3, 1
    (2, 32, 32, 8, 8, 8, 2),     # split beyond the 2 K tiles: clamped
])
def test_factred_bwd_exact(B, Ci, Co, H, W, split, slots):
    ext = _ext()
    _, e, x, w1, w2 = _eighths(B, Ci, Co, H, W)
    leaves = [t.requires_grad_() for t in (x, w1, w2)]
    y = _compose(*leaves)
    dy = e(*y.shape)
    y.backward(dy)       # relu's backward masks with x > 0; many x are 0
    want = [t.grad.bfloat16() for t in leaves]

    n = ext.factred_dw_slots(B, Ci, H, W, split)
    assert slots is None or n == slots
    xd, w1d, w2d, dyd = (_bf(t.detach()) for t in (x, w1, w2, dy))

    def backward():
        dx = torch.empty_like(xd)
        dw = torch.empty(Co, Ci, device=DEV, dtype=torch.bfloat16)
        wsp = torch.empty(n, Co, Ci, device=DEV, dtype=torch.float32)
        ext.factred_bwd_dx(dyd, xd, w1d, w2d, dx)
        ext.factred_bwd_dw(xd, dyd, dw, wsp, split)
        return [dx.cpu(), dw[:Co // 2].cpu(), dw[Co // 2:].cpu()]

    first, second = backward(), backward()
    for got, again, ref in zip(first, second, want):
        assert torch.equal(got, ref) and torch.equal(got, again)


@pytest.mark.parametrize("ci,co,size", [(64, 64, 16), (96, 32, 9)])
def test_module_routing(ci, co, size, monkeypatch):
    from adanet_amd.models.nasnet import FactorizedReduction
    torch.manual_seed(ci + co + size)
    m = FactorizedReduction(ci, co)
    m.bn.bn.running_mean.normal_()
    m.bn.bn.running_var.uniform_(0.5, 2.0)
    m.bn.bn.weight.data.uniform_(0.5, 1.5)
    m.bn.bn.bias.data.normal_()
    m.to(torch.bfloat16)        # weights bf16-exact; BN pins itself to fp32
    x = torch.randn(4, ci, size, size).to(torch.bfloat16)
    ref_m, m = copy.deepcopy(m).double(), m.to(DEV)

    ext, calls = _ext(), collections.Counter()
    for name in ("factred_fwd", "factred_bwd_dx", "factred_bwd_dw"):
        monkeypatch.setattr(ext, name, lambda *a, _n=name, _r=getattr(
            ext, name): (calls.update([_n]), _r(*a))[1])

    def run(mod, xin, train, grad, fused="1", fused_train="0", fwd=None):
        monkeypatch.setenv("ADANET_FUSED_FACTRED", fused)
        monkeypatch.setenv("ADANET_FACTRED_TRAIN", fused_train)
        mod.train(train)
        mod.zero_grad()
        xi = xin.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            y = (fwd or mod)(xi)
        if grad:
            y.double().square().sum().backward()
        return [t if t is None else t.detach().cpu().double().flatten() for t
                in (y, xi.grad, mod.p1.weight.grad, mod.p2.weight.grad)]

    def check(fused, chain, ref, what):
        # same rounding points, another fp32 order: within twice the
        # chain's own error, the contract of the sepconv test
        for f, c, r, part in zip(fused, chain, ref, ("y", "dx", "dw1", "dw2")):
            if r is not None:
                ef, ec = (f - r).abs().max().item(), (c - r).abs().max().item()
                print("%s %s: fused err %.4g chain err %.4g" %
                      (what, part, ef, ec))
                assert ef <= 2 * ec

    ref = run(ref_m, x.double(), False, False)
    fused = run(m, x.to(DEV), False, False)
    assert calls == {"factred_fwd": 1}          # one launch, Co = 32 included
    chain = run(m, x.to(DEV), False, False, fused="0")
    assert calls == {"factred_fwd": 1}
    check(fused, chain, ref, "eval")

    # training keeps the chain by default, exactly
    ref = run(ref_m, x.double(), True, True)
    chain = run(m, x.to(DEV), True, True)
    parent = run(m, x.to(DEV), True, True, fwd=lambda t: (
        lambda r: m.bn(torch.cat([m.p1(r), m.p2(
            F.pad(r, (0, 1, 0, 1))[:, :, 1:, 1:])], dim=1)))(m.relu(t)))
    assert calls == {"factred_fwd": 1}
    assert all(torch.equal(a, b) for a, b in zip(chain, parent))
    fused = run(m, x.to(DEV), True, True, fused_train="1")
    assert calls == {"factred_fwd": 2, "factred_bwd_dx": 1,
                     "factred_bwd_dw": 1}
    check(fused, chain, ref, "train")


def test_argument_checks():
    from adanet_amd.ops.conv import (conv_nxn, factorized_reduction,
                                     factorized_reduction_bn_infer,
                                     factorized_reduction_supported)
    ext = _ext()
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    out = lambda *s: torch.empty(*s, device=DEV, dtype=torch.bfloat16)
    x, w = bf(2, 32, 8, 8), bf(16, 32)
    with pytest.raises(RuntimeError, match="y must be"):
        ext.factred_fwd(x, w, w, None, None, None, None, out(2, 32, 4, 5))
    assert factorized_reduction_supported(x, w, w)
    for xs, ws, msg in ((bf(2, 48, 8, 8), bf(32, 48), "Ci%32==0"),
                        (x, bf(96, 32), "Co<=128")):
        with pytest.raises(RuntimeError, match="unsupported shape.*" + msg):
            ext.factred_fwd(xs, ws, ws, None, None, None, None,
                            out(2, 2 * ws.shape[0], 4, 4))
        assert not factorized_reduction_supported(xs, ws, ws)
        r, w4 = xs.relu(), ws.reshape(*ws.shape, 1, 1)
        want = torch.cat([conv_nxn(r, w4, None, 2, 0), conv_nxn(
            F.pad(r, (0, 1, 0, 1))[:, :, 1:, 1:], w4, None, 2, 0)], dim=1)
        assert torch.equal(factorized_reduction(xs, ws, ws), want)
    with pytest.raises(RuntimeError, match="no backward"):
        factorized_reduction_bn_infer(x.requires_grad_(), w, w)
