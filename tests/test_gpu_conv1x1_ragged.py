"""Pointwise conv at channel counts off the 32 grid (csrc/conv1x1_ragged.hip
for forward and dX, conv1x1_dw for dW): against exact integer arithmetic,
with non-finite neighbours, against the aligned path on zero-padded
operands, and through the public conv modules."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [               # (B, Ci, Co, H, W)
    (2, 10, 10, 8, 8),      # one partial K chunk, 64-pixel tile
    (3, 33, 7, 8, 8),       # odd counts, one-element K tail, 2-byte W loads
    (2, 42, 84, 16, 16),    # full chunk + tail of 10, several fragments
    (1, 252, 168, 8, 8),    # many chunks, more than one 128-channel tile
    (2, 64, 20, 8, 8),      # one axis on the grid (conv_nxn) ...
    (2, 20, 64, 8, 8),      # ... and its transpose
    (3, 20, 40, 5, 8),      # HW = 40: the pixel tile ends inside the block
    (4, 10, 20, 2, 4),      # HW = 8: tile much wider than the image
]


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _eighths(*shape, seed):
    """n/8 with integer n in [-8, 8): products are multiples of 1/64 with
    magnitude <= 1 and every K here is below 2^17, so each fp32 partial sum
    is exact in any order and the tests below need no tolerance."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 8, shape, generator=g).float() / 8).to(
        torch.bfloat16)


def _exact(eq, a, b):
    n = torch.einsum(eq, (a.float() * 8).long(), (b.float() * 8).long())
    return (n.double() / 64).to(torch.bfloat16)


def _run(direction, w, act):
    """act [B, C, HW] on the GPU (any batch stride) -> the new kernel's out"""
    co, ci = w.shape
    out = torch.empty(act.shape[0], co if direction == "fwd" else ci,
                      act.shape[2], device=DEV, dtype=torch.bfloat16)
    fn = _ext().conv1x1_ragged_fwd if direction == "fwd" \
        else _ext().conv1x1_ragged_dx
    fn(act, w.to(DEV), out)
    return out.cpu()


def _operands(direction, B, Ci, Co, H, W):
    w = _eighths(Co, Ci, seed=Ci * 1000 + Co)
    act = _eighths(B, Ci if direction == "fwd" else Co, H * W, seed=B + H * W)
    eq = "oi,bip->bop" if direction == "fwd" else "oi,bop->bip"
    return w, act, _exact(eq, w, act)


@pytest.mark.parametrize("direction", ["fwd", "dx"])
@pytest.mark.parametrize("B,Ci,Co,H,W", CASES)
def test_exact(direction, B, Ci, Co, H, W):
    w, act, want = _operands(direction, B, Ci, Co, H, W)
    assert torch.equal(_run(direction, w, act.to(DEV)), want)


@pytest.mark.parametrize("B,Ci,Co,H,W", CASES)
def test_weight_grad_exact(B, Ci, Co, H, W):
    # conv1x1_dw where B*HW % 32 == 0, the permute-copy path at HW = 40
    from adanet_amd.ops.conv import conv1x1_weight_grad
    dy = _eighths(B, Co, H, W, seed=1 + B + Co)
    x = _eighths(B, Ci, H, W, seed=2 + B + Ci)
    got = conv1x1_weight_grad(dy.to(DEV), x.to(DEV))
    assert torch.equal(got.cpu(), _exact("bohw,bihw->oi", dy, x))


@pytest.mark.parametrize("direction,case", [("fwd", CASES[1]),
                                            ("dx", CASES[2])])
def test_tail_is_zero_in_lds_not_in_the_weights(direction, case):
    # The images are the leading channels of the middle images of a larger
    # buffer: the channels behind each image and the images around the batch
    # hold inf and nan, which 0 * would turn into nan.
    w, act, want = _operands(direction, *case)
    B, C, HW = act.shape
    big = torch.full((B + 2, C + 3, HW), float("inf"), dtype=torch.bfloat16)
    big[:, :, ::2] = float("nan")
    big[1:1 + B, :C] = act
    got = _run(direction, w, big.to(DEV)[1:1 + B, :C])
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)


def test_bits_match_padded_aligned_path_and_dw_repeats():
    from adanet_amd.ops.conv import _Conv1x1Fn
    B, Ci, Co, H, W = CASES[2]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, Ci, H, W, generator=g).to(torch.bfloat16).to(DEV)
    w = torch.randn(Co, Ci, generator=g).mul(0.1).to(torch.bfloat16).to(DEV)
    up = torch.randn(B, Co, H, W, generator=g).to(torch.bfloat16).to(DEV)
    pad = torch.nn.functional.pad
    res = []
    for xi, wi, ui in [(x, w, up),
                       (pad(x, (0, 0, 0, 0, 0, 64 - Ci)),
                        pad(w, (0, 64 - Ci, 0, 96 - Co)),
                        pad(up, (0, 0, 0, 0, 0, 96 - Co)))]:
        xi = xi.contiguous().requires_grad_(True)
        y = _Conv1x1Fn.apply(xi, wi.contiguous(), None)
        y.backward(ui.contiguous())
        res.append((y.detach()[:, :Co], xi.grad[:, :Ci]))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    # dW run to run: these fp32 sums are inexact, so a slot order that
    # changed between calls would change bits
    from adanet_amd.ops.conv import conv1x1_weight_grad
    dw = conv1x1_weight_grad(up, x)
    assert torch.equal(conv1x1_weight_grad(up, x), dw)


@pytest.mark.parametrize("ragged", ["1", "0"])
@pytest.mark.parametrize("kind", ["1x1", "3x3"])
def test_modules_vs_fp32(kind, ragged, monkeypatch):
    from adanet_amd.ops.conv import HipConv1x1, HipConvNxN
    monkeypatch.setenv("ADANET_CONV_RAGGED", ragged)
    torch.manual_seed(6)
    if kind == "1x1":
        m, ci = HipConv1x1(42, 84, bias=False), 42
    else:
        m, ci = HipConvNxN(3, 30, 3, padding=1, bias=False), 3
    m = m.to(DEV).to(torch.bfloat16)
    x = torch.randn(2, ci, 16, 16, device=DEV).to(
        torch.bfloat16).requires_grad_(True)
    y = m(x)
    xf = x.detach().float().requires_grad_(True)
    wf = m.weight.detach().float().requires_grad_(True)
    ref = torch.nn.functional.conv2d(xf, wf, padding=wf.shape[-1] // 2)
    rel = (y.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.02, rel
    up = torch.randn_like(ref)
    y.backward(up.to(torch.bfloat16))
    ref.backward(up)
    for got, want in [(x.grad.float(), xf.grad),
                      (m.weight.grad.float(), wf.grad)]:
        rel = (got - want).abs().mean() / (want.abs().mean() + 1e-6)
        assert rel < 0.03, rel
