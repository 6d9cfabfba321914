"""cell_combine off the GPU: the fallback IS the unfused composition, the
error paths, and the cell wiring (RNG draw order, block grouping) pinned
against the pre-fusion cell loop."""

import pytest
import torch

from adanet_amd.models import nasnet
from adanet_amd.ops import combine


def _compose(lefts, rights, sl=None, sr=None):
    outs = []
    for i in range(len(lefts)):
        left, right = lefts[i], rights[i]
        if sl is not None:
            left = left * sl[i]
            right = right * sr[i]
        outs.append(left + right)
    return torch.cat(outs, dim=1)


def _scales(n, B, keep, dtype, gen):
    return [(torch.rand(B, 1, 1, 1, generator=gen) < keep).to(dtype)
            * (1.0 / keep) for _ in range(n)]


def _inputs(n, shape, dtype, gen, requires_grad=False):
    return [(torch.randn(shape, generator=gen) * 3).to(dtype)
            .requires_grad_(requires_grad) for _ in range(n)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("scaled", [False, True])
def test_cpu_equals_composition_bitwise(dtype, scaled):
    gen = torch.Generator().manual_seed(3)
    n, shape = 3, (4, 3, 5, 5)
    lefts = _inputs(n, shape, dtype, gen)
    rights = _inputs(n, shape, dtype, gen)
    sl = _scales(n, 4, 0.6, dtype, gen) if scaled else None
    sr = _scales(n, 4, 0.6, dtype, gen) if scaled else None
    got = combine.cell_combine(lefts, rights, sl, sr)
    want = _compose(lefts, rights, sl, sr)
    assert got.shape == (4, 9, 5, 5) and got.dtype == dtype
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("scaled", [False, True])
def test_cpu_gradients_equal_composition(dtype, scaled):
    gen = torch.Generator().manual_seed(4)
    n, shape = 3, (4, 2, 3, 3)
    sl = _scales(n, 4, 0.6, dtype, gen) if scaled else None
    sr = _scales(n, 4, 0.6, dtype, gen) if scaled else None
    base_l = _inputs(n, shape, dtype, gen)
    base_r = _inputs(n, shape, dtype, gen)
    dy = torch.randn((4, 2 * n, 3, 3), generator=gen).to(dtype)
    grads = []
    for fn in (combine.cell_combine, _compose):
        lefts = [t.clone().requires_grad_(True) for t in base_l]
        rights = [t.clone().requires_grad_(True) for t in base_r]
        rights[0] = lefts[1]  # one tensor feeding two blocks
        fn(lefts, rights, sl, sr).backward(dy)
        grads.append([t.grad for t in lefts + rights[1:]])
    for got, want in zip(*grads):
        assert torch.equal(got, want)


def test_mismatched_list_lengths_raise():
    x = torch.zeros(2, 1, 2, 2)
    with pytest.raises((ValueError, AssertionError)):
        combine.cell_combine([x, x], [x])
    with pytest.raises((ValueError, AssertionError)):
        combine.cell_combine([], [])
    s = torch.ones(2, 1, 1, 1)
    with pytest.raises((ValueError, AssertionError)):
        combine.cell_combine([x, x], [x, x], [s], [s, s])


def test_one_scale_list_without_the_other_raises():
    x = torch.zeros(2, 1, 2, 2)
    s = torch.ones(2, 1, 1, 1)
    with pytest.raises((ValueError, AssertionError)):
        combine.cell_combine([x], [x], [s], None)
    with pytest.raises((ValueError, AssertionError)):
        combine.cell_combine([x], [x], None, [s])


def test_drop_path_scale_is_drop_path_unapplied():
    x = torch.randn(6, 2, 3, 3)
    torch.manual_seed(11)
    want = nasnet.drop_path(x, 0.5, True)
    torch.manual_seed(11)
    scale = nasnet.drop_path_scale(x, 0.5, True)
    assert scale.shape == (6, 1, 1, 1)
    assert torch.equal(x * scale, want)
    assert nasnet.drop_path_scale(x, 0.5, False) is None
    assert nasnet.drop_path_scale(x, 1.0, True) is None
    assert nasnet.drop_path(x, 1.0, True) is x


def _unfused_cell_forward(self, h_prev_prev, h_prev):
    """NasNetACell.forward as it stood before the fused combine."""
    states = [self.pre0(h_prev_prev), self.pre1(h_prev)]
    for i, (op_l, op_r) in enumerate(zip(self.ops_left, self.ops_right)):
        in_l, in_r = self.idx[i]
        left = op_l(states[in_l])
        right = op_r(states[in_r])
        left = nasnet.drop_path(left, self.drop_path_keep, self.training)
        right = nasnet.drop_path(right, self.drop_path_keep, self.training)
        states.append(left + right)
    return torch.cat(states[2:], dim=1)


def _model_run(keep=0.8):
    torch.manual_seed(5)
    model = nasnet.NasNetCIFAR(num_cells=3, num_conv_filters=4,
                               drop_path_keep=keep)
    model.train()
    x = torch.randn(4, 3, 32, 32)
    torch.manual_seed(6)
    _, logits = model(x)
    logits.square().sum().backward()
    return logits.detach(), {k: p.grad for k, p in model.named_parameters()}


def _assert_same_run(a, b):
    assert torch.equal(a[0], b[0])
    assert a[1].keys() == b[1].keys()
    for k in a[1]:
        assert a[1][k] is not None, k
        assert torch.equal(a[1][k], b[1][k]), k


def test_model_toggle_on_equals_off(monkeypatch):
    monkeypatch.setenv("ADANET_FUSED_COMBINE", "1")
    on = _model_run()
    monkeypatch.setenv("ADANET_FUSED_COMBINE", "0")
    off = _model_run()
    _assert_same_run(on, off)


@pytest.mark.parametrize("keep", [0.8, 1.0])
def test_model_equals_unfused_cell_loop(monkeypatch, keep):
    """Same masks, same block wiring, same gradient accumulation order as
    the loop the fused combine replaced — reduction cells included."""
    new = _model_run(keep)
    monkeypatch.setattr(nasnet.NasNetACell, "forward", _unfused_cell_forward)
    old = _model_run(keep)
    _assert_same_run(new, old)


def test_cells_call_cell_combine_through_the_module(monkeypatch):
    calls = []
    real = combine.cell_combine

    def counting(lefts, rights, scales_l=None, scales_r=None):
        calls.append((len(lefts), scales_l is not None))
        return real(lefts, rights, scales_l, scales_r)

    monkeypatch.setattr(combine, "cell_combine", counting)
    torch.manual_seed(0)
    normal = nasnet.NasNetACell(8, 8, 4, reduction=False,
                                prev_reduction=False, drop_path_keep=0.8)
    reduce_ = nasnet.NasNetACell(8, 8, 4, reduction=True,
                                 prev_reduction=False, drop_path_keep=0.8)
    x = torch.randn(2, 8, 8, 8)
    assert normal.train()(x, x).shape == (2, 20, 8, 8)
    assert calls == [(5, True)]
    del calls[:]
    assert reduce_.train()(x, x).shape == (2, 20, 4, 4)
    assert calls == [(1, True), (1, True), (3, True)]
    del calls[:]
    normal.eval()(x, x)
    assert calls == [(5, False)]
