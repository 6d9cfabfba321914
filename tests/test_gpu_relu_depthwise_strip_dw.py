"""relu_depthwise_strip_bwd_dw: the strip-tiled weight gradient against exact
arithmetic, against the one-launch kernel's dW-only instance bit for bit,
outside its class and through SepConv."""

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

SHAPES = [                      # (B, C, H, W, K, stride)
    (2, 3, 8, 8, 3, 1),         # one image per chunk; 64 outputs: one wave
    (2, 3, 4, 8, 7, 1),         # lower than the window
    (9, 1024, 8, 8, 5, 1),      # one group of 9: passes cross images, ragged
    (9, 1024, 32, 32, 5, 1),    # groups of 4, 4, 1; four passes per group
    (5, 512, 16, 16, 7, 1),     # chunks of 3 and 2 images
    (5, 512, 32, 32, 5, 2),     # stride 2; G limited by x, not dy
    (3, 1024, 16, 16, 7, 2),    # OW = 8; 192 outputs in one partial pass
    (3, 1024, 6, 16, 3, 2),     # 24 outputs per plane: strips start mid-pass
    (1, 2, 64, 64, 3, 1),       # the upper edge of the class; 16 passes
]


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _exact(B, C, H, W, KS, stride):
    """x, w, dy = n/8 with n in [-8, 8), as test_gpu_relu_depthwise_strip's:
    every fp32 sum is exact in any order (at most 9 x 1024 terms of magnitude
    at most 1 in steps of 1/64), so the float64 autograd, rounded once, is
    the expected bits."""
    g = torch.Generator().manual_seed(B + C + H * W + KS + stride)
    e = lambda *s: torch.randint(-8, 8, s, generator=g).double() / 8
    x, w = e(B, C, H, W), e(C, 1, KS, KS).requires_grad_()
    y = F.conv2d(F.relu(x), w, None, stride, KS // 2, groups=C)
    dy = e(*y.shape)
    y.backward(dy)
    bf = lambda t: t.detach().to(DEV, torch.bfloat16)
    return bf(x), bf(dy), w.grad.float().bfloat16()


@pytest.mark.parametrize("shape", SHAPES)
def test_exact(shape):
    _, C, _, _, KS, stride = shape
    x, dy, dw_ref = _exact(*shape)
    dw = torch.full((C * KS * KS,), 3.0, device=DEV)
    _ext().relu_depthwise_strip_bwd_dw(x, dy, dw, stride, KS // 2)
    assert torch.equal(dw.cpu().bfloat16().reshape(dw_ref.shape), dw_ref)


@pytest.mark.parametrize("B,C,H,W,KS,stride", SHAPES)
def test_bit_identical_to_one_launch(B, C, H, W, KS, stride):
    torch.manual_seed(B + C + H + KS)
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    pad = KS // 2
    x, w = bf(B, C, H, W), bf(C, 1, KS, KS)
    dy = bf(B, C, (H + 2 * pad - KS) // stride + 1,
            (W + 2 * pad - KS) // stride + 1)
    new, old = (torch.full((C * KS * KS,), 3.0, device=DEV) for _ in range(2))
    _ext().relu_depthwise_strip_bwd_dw(x, dy, new, stride, pad)
    _ext().relu_depthwise_bwd(x, dy, w, None, old, stride, pad)
    assert torch.equal(new, old)


@pytest.mark.parametrize("W,KS,pad", [(20, 3, 1), (16, 5, 1)])
def test_outside_the_class(W, KS, pad):
    from adanet_amd.ops.conv import depthwise_conv2d, relu_depthwise_conv2d
    torch.manual_seed(W + pad)
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    x, w = bf(2, 3, 32, W), bf(3, 1, KS, KS)
    y = relu_depthwise_conv2d(x, w, 1, pad)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _ext().relu_depthwise_strip_bwd_dw(
            x, torch.empty_like(y), torch.empty(3 * KS * KS, device=DEV), 1,
            pad)
    assert torch.equal(y, depthwise_conv2d(F.relu(x), w, 1, pad))


def test_through_sepconv(monkeypatch):
    from adanet_amd.models.nasnet import SepConv
    torch.manual_seed(5)
    m = SepConv(32, 32, 5, 1).to(torch.bfloat16).to(DEV).train()
    x = torch.randn(2, 32, 32, 32, device=DEV).to(torch.bfloat16)
    ext, calls = _ext(), []
    real = ext.relu_depthwise_strip_bwd_dw
    monkeypatch.setattr(ext, "relu_depthwise_strip_bwd_dw",
                        lambda *a: (calls.append(1), real(*a))[1])

    def run(switch):
        monkeypatch.setenv("ADANET_RELU_DW_STRIP_DW", switch)
        m.zero_grad()
        xi = x.clone().requires_grad_()
        y = m(xi)
        y.float().square().sum().backward()
        return [y.detach(), xi.grad] + [p.grad.clone() for p in m.parameters()]

    old = run("0")
    assert not calls
    new = run("1")
    assert len(calls) == 2
    assert all(torch.equal(a, b) for a, b in zip(new, old))
