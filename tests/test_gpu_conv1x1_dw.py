"""conv1x1_dw: the pointwise-conv weight gradient read straight from the
[B, C, HW] layout, against exact integer arithmetic, against the permute-copy
+ gemm_nt_bf16 path it replaces, and through the public conv modules."""

import pytest
import torch

DEV = "cuda:0"


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _inputs(B, Co, Ci, H, W, kind):
    """dy [B,Co,H,W] and x [B,Ci,H,W], bf16 on the CPU. "eighths": n/8 with
    integer n in [-8, 8); "randn": normal."""
    g = torch.Generator().manual_seed(B * 1000 + Co + Ci + H * W)
    if kind == "eighths":
        draw = lambda *s: torch.randint(-8, 8, s, generator=g).float() / 8
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
    return (draw(B, Co, H, W).to(torch.bfloat16),
            draw(B, Ci, H, W).to(torch.bfloat16))


def _direct(dy, x):
    B, Co, H, W = dy.shape
    dw = torch.empty(Co, x.shape[1], device=DEV, dtype=torch.bfloat16)
    _ext().conv1x1_dw(dy.to(DEV).reshape(B, Co, H * W),
                      x.to(DEV).reshape(B, -1, H * W), dw)
    return dw


@pytest.mark.gpu
@pytest.mark.parametrize("B,Co,Ci,H,W", [
    (2, 32, 32, 8, 8),      # one tile, one split, row clamping in a 64 tile
    (4, 32, 32, 2, 4),      # HW = 8: every K tile spans four images
    (4, 64, 32, 4, 6),      # HW = 24: tiles straddle images off-tile
    (4, 32, 64, 5, 8),      # HW = 40
    (2, 96, 160, 8, 8),     # several tiles, ragged last tile on both axes
    (7, 64, 64, 16, 20),    # K = 2240: 70 K-tiles over 8 splits, short last
    (8, 32, 128, 16, 16),   # K = 2048, two tiles
])
def test_conv1x1_dw_exact(B, Co, Ci, H, W):
    # Products are multiples of 1/64 with magnitude <= 1 and K <= 2^17, so
    # every fp32 partial sum is exact in any order: no tolerance.
    dy, x = _inputs(B, Co, Ci, H, W, "eighths")
    n = torch.einsum("bohw,bihw->oi", (dy.float() * 8).long(),
                     (x.float() * 8).long())
    exact = (n.double() / 64).to(torch.bfloat16)
    assert torch.equal(_direct(dy, x).cpu(), exact)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Co,Ci,H,W", [(7, 64, 64, 16, 20),
                                         (8, 32, 128, 16, 16)])
def test_conv1x1_dw_bit_identical_to_copy_path(B, Co, Ci, H, W):
    dy, x = _inputs(B, Co, Ci, H, W, "randn")
    K = B * H * W
    dz_flat = dy.to(DEV).reshape(B, Co, H * W).permute(1, 0, 2).reshape(
        Co, K).contiguous()
    x_flat = x.to(DEV).reshape(B, Ci, H * W).permute(1, 0, 2).reshape(
        Ci, K).contiguous()
    want = torch.empty(Co, Ci, device=DEV, dtype=torch.bfloat16)
    _ext().gemm_nt_bf16(dz_flat, x_flat, want, None, 0)
    got = _direct(dy, x)
    assert torch.equal(got, want)
    assert torch.equal(_direct(dy, x), got)


@pytest.mark.gpu
@pytest.mark.parametrize("name,xshape", [
    ("1x1", (2, 32, 8, 8)),
    ("3x3", (2, 16, 8, 8)),
    ("1x1", (3, 32, 2, 4)),     # K = 24: outside the contract, copy path
])
def test_module_weight_grad_vs_fp32(name, xshape):
    from adanet_amd.ops.conv import HipConv1x1, HipConvNxN
    torch.manual_seed(11)
    m = (HipConv1x1(32, 64) if name == "1x1" else
         HipConvNxN(16, 32, 3, padding=1)).to(DEV)
    m.weight.data = m.weight.data.to(torch.bfloat16)
    x = torch.randn(*xshape, device=DEV).to(torch.bfloat16)
    y = m(x)
    up = torch.randn(y.shape, device=DEV).to(torch.bfloat16)
    y.backward(up)
    wf = m.weight.detach().float().requires_grad_(True)
    ref = torch.nn.functional.conv2d(x.float(), wf, m.bias.detach(),
                                     padding=m.weight.shape[-1] // 2)
    ref.backward(up.float())
    rel = (m.weight.grad.float() - wf.grad).abs().mean() / (
        wf.grad.abs().mean() + 1e-6)
    assert rel < 0.03, rel


def test_conv1x1_weight_grad_cpu():
    from adanet_amd.ops.conv import conv1x1_weight_grad
    dy, x = _inputs(3, 5, 7, 3, 4, "randn")
    dy, x = dy.float(), x.float()
    want = torch.einsum("bohw,bihw->oi", dy, x)
    assert torch.equal(conv1x1_weight_grad(dy, x), want)
