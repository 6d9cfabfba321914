"""relu_pointwise: the fused ReLU -> 1x1 conv forward, masked dX and dW
against exact arithmetic and against the chain, through the NASNet module,
and their argument checks."""

import collections

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 32, 32, 8, 8),      # one K chunk, one 64-pixel tile
    (1, 96, 64, 16, 16),    # odd chunk count (buffer parity), two tiles
    (2, 160, 128, 8, 8),    # widest Co, dX loop over 5 chunks
    (3, 64, 96, 4, 6),      # HW = 24: ragged 16-pixel fragment; Co = 96
    (1, 32, 32, 32, 32),    # eight tiles per image
    (8, 32, 32, 2, 4),      # HW = 8 < 32: dW K tiles straddle four images
    (2, 32, 32, 12, 12),    # HW = 144: a 128-pixel tile with 16 live pixels
]
FUSED = ("relu_pointwise_fwd", "relu_pointwise_bwd_dx", "relu_conv1x1_dw")


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _run(fn, x, w, dy):
    xi, wi = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = fn(xi, wi)
    y.backward(dy)
    return [t.detach().cpu() for t in (y, xi.grad, wi.grad)]


@pytest.mark.parametrize("B,Ci,Co,H,W", SHAPES)
def test_exact(B, Ci, Co, H, W):
    # n/8 with n in [-8, 8): products are multiples of 1/64 and every fp32
    # partial sum stays far below 2^24 of them, so any summation order is
    # exact, and many x are exactly 0 (the mask boundary). No tolerance.
    from adanet_amd.ops.conv import _ReluConv1x1Fn
    g = torch.Generator().manual_seed(B + Ci + Co + H * W)
    e = lambda *s: torch.randint(-8, 8, s, generator=g).double() / 8
    x, w, dy = e(B, Ci, H, W), e(Co, Ci), e(B, Co, H, W)
    want = _run(lambda a, b: torch.einsum("oi,bihw->bohw", b, F.relu(a)),
                x, w, dy)
    xd, wd, dyd = (t.to(DEV, torch.bfloat16) for t in (x, w, dy))
    # the kernels' whole class, also where the routing keeps the chain
    assert _ext().relu_pointwise_supported(Ci, Co, H, W)
    first, second = (_run(_ReluConv1x1Fn.apply, xd, wd, dyd)
                     for _ in range(2))
    for got, again, ref in zip(first, second, want):
        assert torch.equal(got, ref.bfloat16()) and torch.equal(got, again)


@pytest.mark.parametrize("B,Ci,Co,H,W", SHAPES)
def test_bit_identical_to_chain(B, Ci, Co, H, W):
    from adanet_amd.ops.conv import _ReluConv1x1Fn, conv1x1
    torch.manual_seed(B + Ci + Co + H * W)
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    x, w, dy = bf(B, Ci, H, W), bf(Co, Ci), bf(B, Co, H, W)
    fused = _run(_ReluConv1x1Fn.apply, x, w, dy)
    chain = _run(lambda a, b: conv1x1(F.relu(a), b), x, w, dy)
    for f, c in zip(fused, chain):
        assert torch.equal(f, c)


def test_module_routing(monkeypatch):
    from adanet_amd.models.nasnet import ReluConvBN
    torch.manual_seed(0)
    m = ReluConvBN(96, 32).to(torch.bfloat16).to(DEV)
    x = torch.randn(2, 96, 8, 8, device=DEV).to(torch.bfloat16)
    ext, calls = _ext(), collections.Counter()
    for name in FUSED + ("sepconv_infer",):
        monkeypatch.setattr(ext, name, lambda *a, _n=name, _r=getattr(
            ext, name): (calls.update([_n]), _r(*a))[1])
    start = {k: v.clone() for k, v in m.state_dict().items()}

    def train(switch):
        monkeypatch.setenv("ADANET_FUSED_RELU_PW", switch)
        m.load_state_dict(start)
        m.train()
        m.zero_grad()
        xi = x.clone().requires_grad_()
        y = m(xi)
        y.float().square().sum().backward()
        bn = m.op[2].bn
        return [t.detach().clone() for t in (
            y, xi.grad, m.op[1].weight.grad, bn.weight.grad, bn.bias.grad,
            bn.running_mean, bn.running_var)]

    fused = train("1")
    assert calls == dict.fromkeys(FUSED, 1)
    chain = train("0")
    assert calls == dict.fromkeys(FUSED, 1)
    assert all(torch.equal(f, c) for f, c in zip(fused, chain))
    m.eval()
    monkeypatch.setenv("ADANET_FUSED_RELU_PW", "1")
    with torch.no_grad():
        m(x)
    assert calls == dict(dict.fromkeys(FUSED, 1), sepconv_infer=1)


def test_argument_checks():
    from adanet_amd.ops.conv import (conv1x1, relu_conv1x1,
                                     relu_conv1x1_supported)
    ext = _ext()
    bf = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)
    out = lambda *s: torch.empty(*s, device=DEV, dtype=torch.bfloat16)
    x, w = bf(2, 32, 8, 8), bf(32, 32)
    assert relu_conv1x1_supported(x, w)
    with pytest.raises(RuntimeError, match="y must be"):
        ext.relu_pointwise_fwd(x, w, out(2, 32, 8, 4))
    with pytest.raises(RuntimeError, match="dx must be"):
        ext.relu_pointwise_bwd_dx(out(2, 32, 8, 8), x, w, out(2, 64, 8, 8))
    for xs, ws, msg in ((bf(2, 48, 8, 8), bf(32, 48), "Ci%32==0"),
                        (x, bf(160, 32), "Co<=128"),
                        (bf(2, 32, 7, 10), w, r"\(H\*W\)%8==0")):
        co = ws.shape[0]
        with pytest.raises(RuntimeError, match="unsupported.*" + msg):
            ext.relu_pointwise_fwd(xs, ws, out(2, co, *xs.shape[2:]))
        with pytest.raises(RuntimeError, match="unsupported.*" + msg):
            ext.relu_pointwise_bwd_dx(out(2, co, *xs.shape[2:]), xs, ws,
                                      torch.empty_like(xs))
        assert not relu_conv1x1_supported(xs, ws)
        assert torch.equal(relu_conv1x1(xs, ws), conv1x1(F.relu(xs), ws))
