"""relu_depthwise_strip: the strip-tiled ReLU -> depthwise forward and masked
dX against exact arithmetic, against the chain they replace, outside their
class and through SepConv."""

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

SHAPES = [                      # (B, C, H, W, K, stride)
    (2, 3, 4, 8, 7, 1),         # lower than the window; one strip per row
    (3, 5, 8, 16, 5, 1),        # a left-edge and a right-edge strip
    (2, 2, 16, 24, 7, 1),       # interior strip reaching both neighbours
    (1, 23, 32, 32, 3, 1),      # prime plane count: a partial last group
    (2, 3, 32, 32, 5, 2),       # stride 2
    (2, 2, 16, 16, 7, 2),
    (1, 2, 6, 16, 3, 2),        # 3 output rows, 6 dx rows: ragged strips
    (1, 2, 64, 64, 3, 1),       # the upper edge of the class
    (1, 2, 9, 8, 5, 1),         # rows no multiple of the strip height
]


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _exact(B, C, H, W, KS, stride):
    """x, w, dy = n/8 with n in [-8, 8), as test_gpu_relu_depthwise._exact:
    every fp32 sum is exact in any order, so the float64 conv and its
    autograd, rounded once, are the expected bits."""
    g = torch.Generator().manual_seed(B + C + H * W + KS + stride)
    e = lambda *s: torch.randint(-8, 8, s, generator=g).double() / 8
    x, w = e(B, C, H, W).requires_grad_(), e(C, 1, KS, KS).requires_grad_()
    y = F.conv2d(F.relu(x), w, None, stride, KS // 2, groups=C)
    dy = e(*y.shape)
    y.backward(dy)
    bf = lambda t: t.detach().to(DEV, torch.bfloat16)
    return (bf(x), bf(w), bf(dy), y.detach().bfloat16(), x.grad.bfloat16(),
            w.grad.float().bfloat16())


@pytest.mark.parametrize("shape", SHAPES)
def test_exact(shape):
    from adanet_amd.ops.conv import _ReluDepthwiseStripFn
    _, C, H, W, KS, stride = shape
    x, w, dy, y_ref, dx_ref, dw_ref = _exact(*shape)
    assert _ext().relu_depthwise_strip_supported(C, H, W, KS, stride, KS // 2)
    y, dx = torch.full_like(dy, 3.0), torch.full_like(x, 3.0)
    _ext().relu_depthwise_strip_fwd(x, w, y, stride, KS // 2)
    _ext().relu_depthwise_strip_bwd_dx(x, dy, w, dx, stride, KS // 2)
    assert torch.equal(y.cpu(), y_ref)
    assert torch.equal(dx.cpu(), dx_ref)
    x.requires_grad_(), w.requires_grad_()
    y = _ReluDepthwiseStripFn.apply(x, w, stride, KS // 2)
    y.backward(dy)
    assert torch.equal(y.detach().cpu(), y_ref)
    assert torch.equal(x.grad.cpu(), dx_ref)
    assert torch.equal(w.grad.cpu(), dw_ref)


@pytest.mark.parametrize("B,C,H,W,KS,stride", SHAPES)
def test_bit_identical_to_chain(B, C, H, W, KS, stride):
    from adanet_amd.ops.conv import _ReluDepthwiseStripFn, depthwise_conv2d
    torch.manual_seed(B + C + H + KS)
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    x, w = bf(B, C, H, W), bf(C, 1, KS, KS)
    dy = None
    runs = []
    for fn in (_ReluDepthwiseStripFn.apply,
               lambda x, w, s, p: depthwise_conv2d(F.relu(x), w, s, p)):
        xi, wi = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = fn(xi, wi, stride, KS // 2)
        dy = bf(*y.shape) if dy is None else dy
        y.backward(dy)
        runs.append((y.detach(), xi.grad, wi.grad))
    for strip, chain in zip(*runs):
        assert torch.equal(strip, chain)


@pytest.mark.parametrize("W,KS,pad", [(20, 3, 1), (16, 5, 1)])
def test_outside_the_class(W, KS, pad):
    from adanet_amd.ops.conv import depthwise_conv2d, relu_depthwise_conv2d
    torch.manual_seed(W + pad)
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    x, w = bf(2, 3, 32, W), bf(3, 1, KS, KS)
    y = relu_depthwise_conv2d(x, w, 1, pad)
    assert not _ext().relu_depthwise_strip_supported(3, 32, W, KS, 1, pad)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _ext().relu_depthwise_strip_fwd(x, w, torch.empty_like(y), 1, pad)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _ext().relu_depthwise_strip_bwd_dx(x, torch.empty_like(y), w,
                                           torch.empty_like(x), 1, pad)
    assert torch.equal(y, depthwise_conv2d(F.relu(x), w, 1, pad))


def test_through_sepconv(monkeypatch):
    from adanet_amd.models.nasnet import SepConv
    torch.manual_seed(5)
    m = SepConv(32, 32, 5, 1).to(torch.bfloat16).to(DEV).train()
    x = torch.randn(2, 32, 32, 32, device=DEV).to(torch.bfloat16)
    ext, calls = _ext(), []
    real = ext.relu_depthwise_strip_fwd
    monkeypatch.setattr(ext, "relu_depthwise_strip_fwd",
                        lambda *a: (calls.append(1), real(*a))[1])

    def run(switch):
        monkeypatch.setenv("ADANET_RELU_DW_STRIP", switch)
        m.zero_grad()
        xi = x.clone().requires_grad_()
        y = m(xi)
        y.float().square().sum().backward()
        return [y.detach(), xi.grad] + [p.grad.clone() for p in m.parameters()]

    chain = run("0")
    assert not calls
    strip = run("1")
    assert len(calls) == 2
    assert all(torch.equal(a, b) for a, b in zip(strip, chain))
