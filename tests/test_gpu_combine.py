"""Fused cell combine on the GPU (csrc/combine.hip): bit-for-bit parity with
the unfused torch composition on the same device — forward, backward,
aliased and misaligned inputs, non-finite values, hipGraph replay — and the
NASNet wiring around it."""

import pytest
import torch

from adanet_amd.models import nasnet
from adanet_amd.ops import combine, conv
from adanet_amd.ops.linear import restore_fp32_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEEP = 0.6

# (B, F, H, W, n)
SHAPES = [
    (1, 1, 1, 1, 1),      # single element
    (5, 2, 2, 2, 3),      # chunk = exactly one 8-wide vector
    (2, 3, 5, 5, 5),      # chunk 75: scalar variant
    (2, 5, 4, 2, 1),      # chunk 40
    (3, 8, 4, 4, 5),      # chunk 128
    (32, 32, 32, 32, 5),  # the workload's own layout
    # Grid-stride loops run twice. The grid is capped at 2048 // n blocks of
    # 256 threads per block pair, so with n = 8 one pass covers 256 * 256
    # work items per pair: 65,536 elements on the scalar variant, 524,288
    # (8 per lane) on the vector one. These give 73,101 (odd chunk 24,367)
    # and 552,960 elements per pair.
    (3, 7, 59, 59, 8),
    (3, 24, 96, 80, 8),
]


def _compose(lefts, rights, sl=None, sr=None):
    outs = []
    for i in range(len(lefts)):
        left, right = lefts[i], rights[i]
        if sl is not None:
            left = left * sl[i]
            right = right * sr[i]
        outs.append(left + right)
    return torch.cat(outs, dim=1)


def _draw_scales(n, B, gen):
    return [((torch.rand(B, 1, 1, 1, generator=gen) < KEEP)
             .to(torch.bfloat16) * (1.0 / KEEP)) for _ in range(n)]


_CASES = {}


def _case(shape):
    """Inputs, scales, dy and the composition's outputs and gradients for
    one shape: built once, shared by the tests, never written to."""
    if shape in _CASES:
        return _CASES[shape]
    B, F, H, W, n = shape
    gen = torch.Generator().manual_seed(1234 + sum(shape))

    def rnd(*s):  # asymmetric: shifted off zero, scaled by 3
        return ((torch.randn(*s, generator=gen) + 0.25) * 3).to(
            torch.bfloat16).to(DEV)

    c = {
        "lefts": [rnd(B, F, H, W) for _ in range(n)],
        "rights": [rnd(B, F, H, W) for _ in range(n)],
        "sl": [s.to(DEV) for s in _draw_scales(n, B, gen)],
        "sr": [s.to(DEV) for s in _draw_scales(n, B, gen)],
        "dy": rnd(B, n * F, H, W),
    }
    if B >= 2:
        flat = torch.cat([s.flatten() for s in c["sl"] + c["sr"]])
        assert bool((flat == 0).any()) and bool((flat != 0).any())
    for scaled in (False, True):
        sl = c["sl"] if scaled else None
        sr = c["sr"] if scaled else None
        ls = [t.clone().requires_grad_(True) for t in c["lefts"]]
        rs = [t.clone().requires_grad_(True) for t in c["rights"]]
        out = _compose(ls, rs, sl, sr)
        out.backward(c["dy"])
        c["ref", scaled] = (out.detach(), [t.grad for t in ls + rs])
    _CASES[shape] = c
    return c


@pytest.fixture(autouse=True)
def _fused_on(monkeypatch):
    monkeypatch.setenv("ADANET_FUSED_COMBINE", "1")


@pytest.fixture
def native_calls(monkeypatch):
    """Counts launches of the two kernels' host entry points."""
    calls = {"fwd": 0, "bwd": 0}
    ext = combine._extension.require()

    class Spy:
        def __getattr__(self, name):
            return getattr(ext, name)

        def cell_combine_fwd(self, *a):
            calls["fwd"] += 1
            return ext.cell_combine_fwd(*a)

        def cell_combine_bwd(self, *a):
            calls["bwd"] += 1
            return ext.cell_combine_bwd(*a)

    monkeypatch.setattr(combine._extension, "require", lambda: Spy())
    return calls


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_parity(shape, scaled, native_calls):
    c = _case(shape)
    out = combine.cell_combine(c["lefts"], c["rights"],
                               c["sl"] if scaled else None,
                               c["sr"] if scaled else None)
    assert native_calls["fwd"] == 1  # n <= 8: one launch whatever n is
    assert out.is_contiguous() and out.dtype == torch.bfloat16
    assert torch.equal(out, c["ref", scaled][0])


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_parity(shape, scaled, native_calls):
    c = _case(shape)
    ls = [t.clone().requires_grad_(True) for t in c["lefts"]]
    rs = [t.clone().requires_grad_(True) for t in c["rights"]]
    out = combine.cell_combine(ls, rs, c["sl"] if scaled else None,
                               c["sr"] if scaled else None)
    out.backward(c["dy"])
    # one launch with scales; none without (gradients are slices of dy)
    assert native_calls["bwd"] == (1 if scaled else 0)
    for got, want in zip([t.grad for t in ls + rs], c["ref", scaled][1]):
        assert torch.equal(got, want)


@pytest.mark.parametrize("scaled", [False, True])
def test_input_without_grad_gets_none(scaled):
    c = _case((3, 8, 4, 4, 5))
    ls = [t.clone().requires_grad_(True) for t in c["lefts"]]
    rs = [t.clone().requires_grad_(True) for t in c["rights"]]
    ls[0].requires_grad_(False)
    out = combine.cell_combine(ls, rs, c["sl"] if scaled else None,
                               c["sr"] if scaled else None)
    out.backward(c["dy"])
    assert ls[0].grad is None
    want = c["ref", scaled][1]
    for got, ref in list(zip([t.grad for t in ls + rs], want))[1:]:
        assert torch.equal(got, ref)


@pytest.mark.parametrize("scaled", [False, True])
def test_aliased_inputs_accumulate(scaled):
    c = _case((3, 8, 4, 4, 5))
    sl = c["sl"] if scaled else None
    sr = c["sr"] if scaled else None
    res = []
    for fn in (combine.cell_combine, _compose):
        ls = [t.clone().requires_grad_(True) for t in c["lefts"]]
        rs = [t.clone().requires_grad_(True) for t in c["rights"]]
        rs[0] = ls[1]
        out = fn(ls, rs, sl, sr)
        out.backward(c["dy"])
        res.append((out.detach(), [t.grad for t in ls + rs[1:]]))
    assert torch.equal(res[0][0], res[1][0])
    for got, want in zip(res[0][1], res[1][1]):
        assert torch.equal(got, want)


@pytest.mark.parametrize("scaled", [False, True])
def test_misaligned_base_takes_scalar_variant(scaled, native_calls):
    """A dense input 2 bytes off 16-byte alignment, chunk a multiple of 8."""
    c = _case((3, 8, 4, 4, 5))
    numel = c["lefts"][2].numel()
    buf = torch.zeros(numel + 8, device=DEV, dtype=torch.bfloat16)
    off = buf[1:1 + numel].view(3, 8, 4, 4)
    off.copy_(c["lefts"][2])
    assert off.is_contiguous() and off.data_ptr() % 16 == 2
    ls = list(c["lefts"])
    ls[2] = off
    out = combine.cell_combine(ls, c["rights"], c["sl"] if scaled else None,
                               c["sr"] if scaled else None)
    assert native_calls["fwd"] == 1
    assert torch.equal(out, c["ref", scaled][0])


def _bits(t):
    return t.view(torch.int16)


def test_non_finite_values_multiply_through():
    """inf * 0 is NaN and -x * 0 is -0: the scale multiplies, never selects."""
    B, F, H, W, n = 4, 2, 4, 4, 2
    gen = torch.Generator().manual_seed(77)
    specials = [float("inf"), float("-inf"), float("nan"), -0.0]

    def make():
        t = ((torch.randn(B, F, H, W, generator=gen) + 0.25) * 3).to(
            torch.bfloat16)
        flat = t.view(B, -1)
        for k, v in enumerate(specials):
            flat[:, 3 * k + 1] = v  # every sample, dropped and kept alike
        return t.to(DEV)

    lefts = [make() for _ in range(n)]
    rights = [make() for _ in range(n)]
    # a negative finite opposite a special, and specials opposite each other
    rights[0].view(B, -1)[:, 1] = -2.0
    on = 1.0 / KEEP
    sl = [torch.tensor([0, 0, on, on]), torch.tensor([0, on, 0, on])]
    sr = [torch.tensor([0, on, 0, on]), torch.tensor([on, 0, 0, on])]
    sl = [s.to(torch.bfloat16).view(B, 1, 1, 1).to(DEV) for s in sl]
    sr = [s.to(torch.bfloat16).view(B, 1, 1, 1).to(DEV) for s in sr]
    dy = torch.cat([make() for _ in range(n)], dim=1)
    res = []
    for fn in (combine.cell_combine, _compose):
        ls = [t.clone().requires_grad_(True) for t in lefts]
        rs = [t.clone().requires_grad_(True) for t in rights]
        out = fn(ls, rs, sl, sr)
        out.backward(dy)
        res.append([out.detach()] + [t.grad for t in ls + rs])
    assert bool(torch.isnan(res[1][0]).any())
    assert bool((_bits(res[1][0]) == -32768).any())  # a -0.0 survives
    for got, want in zip(*res):
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def test_hipgraph_replay_matches_eager():
    shape = (3, 8, 4, 4, 5)
    B, F, H, W, n = shape
    c = _case(shape)
    ls = [torch.zeros_like(t).requires_grad_(True) for t in c["lefts"]]
    rs = [torch.zeros_like(t).requires_grad_(True) for t in c["rights"]]
    sl = [torch.ones_like(s) for s in c["sl"]]
    sr = [torch.ones_like(s) for s in c["sr"]]
    dy = torch.zeros_like(c["dy"])

    def step():
        out = combine.cell_combine(ls, rs, sl, sr)
        return out, torch.autograd.grad(out, ls + rs, dy)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one capture stream, no parallel branches
        out, grads = step()
    with torch.no_grad():
        for dst, src in zip(ls + rs + sl + sr + [dy],
                            c["lefts"] + c["rights"] + c["sl"] + c["sr"]
                            + [c["dy"]]):
            dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    want_out, want_grads = c["ref", True]
    assert torch.equal(out, want_out)
    for got, want in zip(grads, want_grads):
        assert torch.equal(got, want)


def test_more_than_eight_blocks_chunk_into_one_output(native_calls):
    c = _case((5, 2, 2, 2, 3))
    ls, rs = c["lefts"] * 4, c["rights"] * 4  # 12 blocks
    sl, sr = c["sl"] * 4, c["sr"] * 4
    lg = [t.clone().requires_grad_(True) for t in ls]
    out = combine.cell_combine(lg, rs, sl, sr)
    assert native_calls["fwd"] == 2
    assert torch.equal(out, c["ref", True][0].repeat(1, 4, 1, 1))
    out.backward(c["dy"].repeat(1, 4, 1, 1))
    for k, t in enumerate(lg):
        assert torch.equal(t.grad, c["ref", True][1][k % 3])


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


def _model_run():
    torch.manual_seed(5)
    model = nasnet.NasNetCIFAR(num_cells=3, num_conv_filters=32,
                               drop_path_keep=0.8)
    model = model.to(DEV).to(torch.bfloat16)
    restore_fp32_params(model)  # BN/bias parameters stay fp32, as in training
    model.train()
    gen = torch.Generator().manual_seed(8)
    x = (torch.randn(8, 3, 32, 32, generator=gen) / 4).to(
        torch.bfloat16).to(DEV)
    torch.manual_seed(6)
    _, logits = model(x)
    logits.float().square().sum().backward()
    torch.cuda.synchronize()
    return (model, logits.detach(),
            {k: p.grad for k, p in model.named_parameters()})


def _assert_same_run(a, b):
    assert torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert a[2][k] is not None, k
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.fixture(scope="module")
def model_runs():
    """One seeded forward+backward of the bf16 model per variant: fused
    (with call counters and the contiguity guard), toggle off, and the
    pre-fusion cell loop."""
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("ADANET_FUSED_COMBINE", "1")
        seen = {"combine": [], "native": 0, "strided": []}
        real = combine.cell_combine
        real_apply = combine._CellCombineFn.apply

        def counting(lefts, rights, scales_l=None, scales_r=None):
            seen["combine"].append(len(lefts))
            return real(lefts, rights, scales_l, scales_r)

        def counting_apply(*a):
            seen["native"] += 1
            return real_apply(*a)

        def guard(cls):
            fwd = cls.forward

            def forward(self, x):
                if not x.is_contiguous():
                    seen["strided"].append(type(self).__name__)
                return fwd(self, x)
            mp.setattr(cls, "forward", forward)

        mp.setattr(combine, "cell_combine", counting)
        mp.setattr(combine._CellCombineFn, "apply", counting_apply)
        guard(conv.HipDepthwiseConv2d)
        guard(conv.HipConv1x1)
        fused = _model_run()
        mp.undo()
        mp.setenv("ADANET_FUSED_COMBINE", "0")
        off = _model_run()
        mp.setenv("ADANET_FUSED_COMBINE", "1")
        mp.setattr(nasnet.NasNetACell, "forward", _unfused_cell_forward)
        old = _model_run()
    finally:
        mp.undo()
    return {"fused": fused, "off": off, "old": old, "seen": seen}


def test_model_toggle_on_equals_off(model_runs):
    _assert_same_run(model_runs["fused"], model_runs["off"])


def test_model_equals_unfused_cell_loop(model_runs):
    """Bit-identical to the cell loop the fused combine replaced, gradient
    accumulation order included."""
    _assert_same_run(model_runs["fused"], model_runs["old"])


def test_model_takes_native_path_once_per_normal_cell(model_runs):
    cells = list(model_runs["fused"][0].cells)
    seen = model_runs["seen"]
    normal = sum(not c.reduction for c in cells)
    reduction = len(cells) - normal
    assert normal == 3 and reduction == 2
    assert len(seen["combine"]) >= len(cells)
    # a normal cell: all five blocks in one call; a reduction cell: blocks
    # 0 and 1 (read again later) alone, then 2-4 together
    assert seen["combine"].count(5) == normal
    assert sorted(seen["combine"]) == [1] * (2 * reduction) + \
        [3] * reduction + [5] * normal
    assert seen["native"] == len(seen["combine"])  # every call went native


def test_model_conv_inputs_stay_contiguous(model_runs):
    assert model_runs["seen"]["strided"] == []
