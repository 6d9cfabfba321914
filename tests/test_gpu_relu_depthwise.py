"""relu_depthwise: the fused ReLU -> depthwise forward and one-launch dX+dW
backward against exact arithmetic, against the chain they replace, through
SepConv, and their argument checks."""

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

SUPPORTED = [
    (2, 3, 8, 8, 3, 1),      # flat small-image loop, one group
    (5, 4, 16, 16, 5, 1),    # image-outer loop, one image per chunk
    (3, 2, 32, 32, 7, 2),    # stride 2, 7x7, G < B
    (2, 5, 7, 10, 3, 2),     # spans not multiples of 8, odd sizes
    (3, 520, 48, 48, 3, 1),  # one chunk, G = 1, three groups in one block
    (1, 2, 64, 64, 5, 1),    # the upper edge of the supported class
]
OUTSIDE = (1, 2, 64, 72, 3, 1)   # just outside: takes the fallback


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _exact(B, C, H, W, KS, stride):
    """x, w, dy = n/8 with n in [-8, 8): products are multiples of 1/64 and
    every fp32 sum (at most 3*48*48 terms below 1) is exact in any order, so
    the float64 conv and its autograd, rounded once, are the expected bits.
    Many x are 0 or negative: the mask is exercised."""
    g = torch.Generator().manual_seed(B + C + H * W + KS + stride)
    e = lambda *s: torch.randint(-8, 8, s, generator=g).double() / 8
    x, w = e(B, C, H, W).requires_grad_(), e(C, 1, KS, KS).requires_grad_()
    y = F.conv2d(F.relu(x), w, None, stride, KS // 2, groups=C)
    dy = e(*y.shape)
    y.backward(dy)
    bf = lambda t: t.detach().to(DEV, torch.bfloat16)
    return (bf(x), bf(w), bf(dy), y.detach().bfloat16(), x.grad.bfloat16(),
            w.grad.float().bfloat16())


@pytest.mark.parametrize("shape", SUPPORTED + [OUTSIDE])
def test_exact(shape):
    from adanet_amd.ops.conv import _ReluDepthwiseFn, relu_depthwise_conv2d
    _, C, H, W, KS, stride = shape
    x, w, dy, y_ref, dx_ref, dw_ref = _exact(*shape)
    inside = _ext().relu_depthwise_supported(C, H, W, KS, stride, KS // 2)
    assert inside == (shape != OUTSIDE)
    x.requires_grad_(), w.requires_grad_()
    # the kernels over their whole class; outside it the public fallback
    y = (_ReluDepthwiseFn.apply if inside else relu_depthwise_conv2d)(
        x, w, stride, KS // 2)
    y.backward(dy)
    assert torch.equal(y.detach().cpu(), y_ref)
    assert torch.equal(x.grad.cpu(), dx_ref)
    assert torch.equal(w.grad.cpu(), dw_ref)


def test_skipped_halves():
    B, C, H, W, KS, stride = SUPPORTED[2]
    x, w, dy, _, dx_ref, dw_ref = _exact(B, C, H, W, KS, stride)
    dx = torch.full_like(x, 3.0)
    dw = torch.full((C * KS * KS,), 3.0, device=DEV)
    _ext().relu_depthwise_bwd(x, dy, w, dx, None, stride, KS // 2)
    assert torch.equal(dx.cpu(), dx_ref)
    _ext().relu_depthwise_bwd(x, dy, w, None, dw, stride, KS // 2)
    assert torch.equal(dw.bfloat16().cpu().view_as(dw_ref), dw_ref)
    assert torch.equal(dx.cpu(), dx_ref)        # untouched by the dW launch


@pytest.mark.parametrize("B,C,H,W,KS,stride", SUPPORTED)
def test_bit_identical_to_chain(B, C, H, W, KS, stride):
    from adanet_amd.ops.conv import _ReluDepthwiseFn, depthwise_conv2d
    torch.manual_seed(B + C + H + KS)
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    x, w = bf(B, C, H, W), bf(C, 1, KS, KS)
    dy = None
    runs = []
    for fn in (_ReluDepthwiseFn.apply,
               lambda x, w, s, p: depthwise_conv2d(F.relu(x), w, s, p)):
        xi, wi = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = fn(xi, wi, stride, KS // 2)
        dy = bf(*y.shape) if dy is None else dy
        y.backward(dy)
        runs.append((y.detach(), xi.grad, wi.grad))
    for fused, chain in zip(*runs):
        assert torch.equal(fused, chain)


def test_through_sepconv(monkeypatch):
    from adanet_amd.models.nasnet import SepConv
    torch.manual_seed(5)
    m = SepConv(32, 32, 5, 1).to(torch.bfloat16).to(DEV).train()
    x = torch.randn(2, 32, 8, 8, device=DEV).to(torch.bfloat16)
    ext, calls = _ext(), []
    real = ext.relu_depthwise_fwd
    monkeypatch.setattr(ext, "relu_depthwise_fwd",
                        lambda *a: (calls.append(1), real(*a))[1])

    def run(switch):
        monkeypatch.setenv("ADANET_FUSED_RELU_DW", switch)
        m.zero_grad()
        xi = x.clone().requires_grad_()
        y = m(xi)
        y.float().square().sum().backward()
        return [y.detach(), xi.grad] + [p.grad.clone() for p in m.parameters()]

    chain = run("0")
    assert not calls
    fused = run("1")
    assert len(calls) == 2
    assert all(torch.equal(a, b) for a, b in zip(fused, chain))


def test_argument_checks():
    ext = _ext()
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    x, w = bf(2, 4, 8, 8), bf(4, 1, 3, 3)
    dx, dw = torch.empty_like(x), torch.empty(36, device=DEV)
    with pytest.raises(RuntimeError, match="does not match"):
        ext.relu_depthwise_bwd(x, bf(2, 4, 8, 9), w, dx, dw, 1, 1)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.relu_depthwise_fwd(x.float(), w, torch.empty_like(x), 1, 1)
    with pytest.raises(RuntimeError, match="dw must be"):
        ext.relu_depthwise_bwd(x, bf(2, 4, 8, 8), w, dx, dw[:35], 1, 1)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.relu_depthwise_fwd(bf(1, 2, 64, 72), bf(2, 1, 3, 3),
                               torch.empty(1, 2, 64, 72, device=DEV,
                                           dtype=torch.bfloat16), 1, 1)
    from adanet_amd.ops.conv import relu_depthwise_supported
    # routed to the kernels only where they measured no slower than the chain
    assert relu_depthwise_supported(bf(2, 64, 16, 16), bf(64, 1, 3, 3), 1, 1)
    assert not relu_depthwise_supported(bf(2, 32, 32, 32), bf(32, 1, 5, 5),
                                        1, 2)
    assert ext.relu_depthwise_supported(2, 64, 64, 7, 2, 3)
    assert not ext.relu_depthwise_supported(2, 64, 64, 4, 1, 2)
    assert not ext.relu_depthwise_supported(2, 64, 64, 3, 3, 1)
