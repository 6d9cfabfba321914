"""sepconv_infer: the fused eval-mode relu -> depthwise -> pointwise -> BN
kernel against exact arithmetic, through the NASNet modules, and its
argument checks."""

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _out(B, Co, H, W, K, stride):
    pad = K // 2
    return torch.empty(B, Co, (H + 2 * pad - K) // stride + 1,
                       (W + 2 * pad - K) // stride + 1, device=DEV,
                       dtype=torch.bfloat16)


@pytest.mark.parametrize("B,Ci,Co,H,W,K,stride,bn", [
    (2, 32, 32, 8, 8, 3, 1, True),      # one chunk, one 64 tile, Co=32 waves
    (1, 64, 32, 8, 8, 5, 1, True),      # two chunks: accumulate, restage
    (2, 32, 64, 16, 16, 3, 1, True),    # two tiles: halo rows, top/bottom clip
    (1, 32, 128, 12, 10, 7, 1, True),   # W%8 != 0, ragged tile, Co=128
    (2, 64, 64, 16, 16, 5, 2, True),    # stride 2
    (1, 128, 128, 9, 9, 7, 2, True),    # odd size at stride 2, four chunks
    (3, 96, 96, 8, 8, 1, 1, True),      # no depthwise stage, Co=Ci=96
    (2, 32, 32, 8, 8, 3, 1, False),     # no BN
])
def test_sepconv_infer_exact(B, Ci, Co, H, W, K, stride, bn):
    # x, dw, pw are n/8 with n in [-8, 8): depthwise sums are multiples of
    # 1/64 below 2^6 and pointwise partial sums multiples of 1/512 below
    # 2^15, so every fp32 sum is exact in any order; mean, beta in quarters
    # and rstd, gamma powers of two keep BN exact too. No tolerance.
    g = torch.Generator().manual_seed(B + Ci + Co + H * W + K)
    eighths = lambda *s: torch.randint(-8, 8, s, generator=g).double() / 8
    pick = lambda n: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[
        torch.randint(0, 3, (n,), generator=g)]
    x, pw = eighths(B, Ci, H, W), eighths(Co, Ci)
    dw = eighths(Ci, 1, K, K) if K > 1 else None
    mean, beta = (torch.randint(-8, 8, (Co,), generator=g).double() / 4
                  for _ in range(2))
    rstd, gamma = pick(Co), pick(Co)

    u = x.clamp_min(0)
    if K > 1:
        u = F.conv2d(u, dw, None, stride, K // 2, groups=Ci)
    u = u.bfloat16().double()
    want = torch.einsum("oi,bihw->bohw", pw, u).bfloat16()
    if bn:
        c = lambda t: t.view(1, -1, 1, 1)
        want = ((want.double() - c(mean)) * c(rstd) * c(gamma)
                + c(beta)).bfloat16()

    dev = lambda t, ty: None if t is None else t.to(DEV, ty)
    stats = [dev(t if bn else None, torch.float32)
             for t in (mean, rstd, gamma, beta)]
    y = _out(B, Co, H, W, K, stride)
    _ext().sepconv_infer(dev(x, torch.bfloat16), dev(dw, torch.bfloat16),
                         dev(pw, torch.bfloat16), *stats, y, stride,
                         K // 2 if K > 1 else 0)
    assert torch.equal(y.cpu(), want)


def _stack(kind, filters, kernel, stride):
    from adanet_amd.models.nasnet import ReluConvBN, SepConv
    torch.manual_seed(filters + kernel + stride)
    m = (SepConv(filters, filters, kernel, stride) if kind == "sep"
         else ReluConvBN(filters, filters))
    for mod in m.modules():
        if hasattr(mod, "running_mean"):
            mod.running_mean.normal_()
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_()
    m.to(torch.bfloat16)        # weights bf16-exact; BN pins itself to fp32
    return m


@pytest.mark.parametrize("kind,filters,kernel,stride,size", [
    ("sep", 32, 3, 1, 16), ("sep", 64, 5, 2, 16), ("relu", 64, 1, 1, 8)])
def test_module_routing(kind, filters, kernel, stride, size, monkeypatch):
    m = _stack(kind, filters, kernel, stride)
    x = torch.randn(2, filters, size, size).to(torch.bfloat16)
    with torch.no_grad():
        ref = m.double().eval()(x.double())
    m = m.to(torch.bfloat16).to(DEV)
    xd = x.to(DEV)

    calls = []
    ext = _ext()
    real = ext.sepconv_infer
    monkeypatch.setattr(ext, "sepconv_infer",
                        lambda *a: (calls.append(1), real(*a))[1])

    def run(switch, train=False, grad=False):
        monkeypatch.setenv("ADANET_FUSED_SEPCONV", switch)
        m.train(train)
        xi = xd.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            y = m(xi)
        if grad:
            y.float().square().sum().backward()
        return y.detach(), xi.grad

    fused, _ = run("1")
    assert len(calls) == (2 if kind == "sep" else 1)   # the kernel ran
    unfused, _ = run("0")
    assert len(calls) == (2 if kind == "sep" else 1)   # and here it did not
    # The two paths round at the same points and both GEMMs walk the
    # channels in 32-wide MFMA steps in the same order, so on the MI355X they
    # agreed bit for bit: max abs errors 0.01825, 0.01677, 0.01601 for the
    # three cases, fused / unfused ratio 1.0 each. That is why the call
    # count above, not a difference in output, shows which path ran; the
    # bound of twice the unfused path's own error is the contract.
    err = lambda y: (y.cpu().double() - ref).abs().max().item()
    print("fused err %.4g unfused err %.4g equal %s"
          % (err(fused), err(unfused), torch.equal(fused, unfused)))
    assert err(fused) <= 2 * err(unfused)

    # training, and eval with autograd on, keep the unfused path
    for train in (True, False):
        m.zero_grad()
        y1, g1 = run("1", train, True)
        m.zero_grad()
        y0, g0 = run("0", train, True)
        assert torch.equal(y1, y0) and torch.equal(g1, g0)
    assert len(calls) == (2 if kind == "sep" else 1)


def test_argument_checks():
    from adanet_amd.ops.conv import (conv1x1, depthwise_conv2d,
                                     sepconv_bn_infer,
                                     sepconv_infer_supported)
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    x, dw, pw = bf(2, 32, 8, 8), bf(32, 1, 3, 3), bf(32, 32)
    with pytest.raises(RuntimeError, match="y must be"):
        _ext().sepconv_infer(x, dw, pw, None, None, None, None,
                             _out(2, 32, 8, 9, 3, 1), 1, 1)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _ext().sepconv_infer(bf(2, 48, 8, 8), bf(48, 1, 3, 3), bf(32, 48),
                             None, None, None, None, _out(2, 32, 8, 8, 3, 1),
                             1, 1)
    pw160 = bf(160, 32)
    assert sepconv_infer_supported(x, dw, pw, 1, 1)
    assert not sepconv_infer_supported(x, dw, pw160, 1, 1)
    with torch.no_grad():
        got = sepconv_bn_infer(x, dw, pw160, None, 1, 1)
        want = conv1x1(depthwise_conv2d(x.relu(), dw, 1, 1), pw160)
    assert torch.equal(got, want)
