"""HIP kernel numerics vs plain PyTorch fp32 references (MI355X only).

Every kernel in adanet_amd/csrc is compared against an fp32 torch
computation of the same op on random (asymmetric) data — the guide's G9
rule: transpose-detecting inputs, no symmetric matrices.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from adanet_amd.ops import _extension
    return _extension.require()


def _rand_bf16(*shape, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return torch.randn(*shape, device=DEV).to(torch.bfloat16)


def test_extension_is_native_and_loaded():
    import adanet_amd
    m = _ext()
    assert m.__file__.endswith(".so")
    assert "adanet_amd" in m.__file__


# ------------------------------------------------------------------ GEMM K1
@pytest.mark.parametrize("M,N,K", [
    (128, 128, 32),
    (256, 512, 384),
    (1024, 2048, 3072),   # bench fwd shape
    (100, 130, 64),       # M,N tails
    (64, 16, 96),         # small N
    (513, 255, 160),      # odd tails
])
def test_gemm_nt_vs_fp32(M, N, K):
    ext = _ext()
    a = _rand_bf16(M, K, seed=M + N)
    b = _rand_bf16(N, K)
    c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    ext.gemm_nt_bf16(a, b, c, None, 0)
    ref = a.float() @ b.float().t()
    err = (c.float() - ref).abs()
    scale = ref.abs().mean() + 1e-3
    assert (err.mean() / scale) < 0.01, "mean rel err %.4f" % (
        err.mean() / scale)


def test_gemm_bias_relu_epilogue():
    ext = _ext()
    M, N, K = 256, 256, 128
    a = _rand_bf16(M, K, seed=1)
    b = _rand_bf16(N, K)
    bias = torch.randn(N, device=DEV, dtype=torch.float32)
    c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    ext.gemm_nt_bf16(a, b, c, bias, 1)
    ref = torch.relu(a.float() @ b.float().t() + bias)
    err = (c.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert err < 0.01
    assert (c.float() >= 0).all()


def test_gemm_generic_fallback_odd_stride():
    ext = _ext()
    # lda not 8-aligned -> generic kernel path
    M, N, K = 33, 7, 10
    a = _rand_bf16(M, K, seed=3)
    b = _rand_bf16(N, K)
    c = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    ext.gemm_nt_bf16(a, b, c, None, 0)
    ref = a.float() @ b.float().t()
    assert (c.float() - ref).abs().max() < 0.1


# ------------------------------------------------------------- transpose
@pytest.mark.parametrize("M,N", [(64, 64), (128, 192), (1000, 513),
                                 (3072, 2048)])
def test_transpose(M, N):
    ext = _ext()
    x = _rand_bf16(M, N, seed=M)
    y = torch.empty(N, M, device=DEV, dtype=torch.bfloat16)
    ext.transpose_bf16(x, y)
    assert torch.equal(y, x.t().contiguous())


# ------------------------------------------------------------- xent K2
@pytest.mark.parametrize("B,C,eps", [(128, 10, 0.0), (256, 100, 0.0),
                                     (64, 10, 0.1), (32, 1000, 0.0)])
def test_softmax_xent_fwd_bwd(B, C, eps):
    ext = _ext()
    torch.manual_seed(B + C)
    logits = torch.randn(B, C, device=DEV).to(torch.bfloat16)
    labels = torch.randint(0, C, (B,), device=DEV)
    loss = torch.empty(B, device=DEV, dtype=torch.float32)
    probs = torch.empty(B, C, device=DEV, dtype=torch.bfloat16)
    ext.softmax_xent_fwd(logits, labels, loss, probs, eps, None)
    ref = torch.nn.functional.cross_entropy(logits.float(), labels,
                                            label_smoothing=eps,
                                            reduction="none")
    assert (loss - ref).abs().max() < 0.02
    ref_probs = torch.softmax(logits.float(), dim=-1)
    assert (probs.float() - ref_probs).abs().max() < 0.01

    grad_rows = torch.full((B,), 1.0 / B, device=DEV, dtype=torch.float32)
    dlogits = torch.empty(B, C, device=DEV, dtype=torch.bfloat16)
    ext.softmax_xent_bwd(probs, labels, grad_rows, dlogits, eps, None)
    lf = logits.float().requires_grad_(True)
    torch.nn.functional.cross_entropy(lf, labels, label_smoothing=eps,
                                      reduction="mean").backward()
    assert (dlogits.float() - lf.grad).abs().max() < 0.01


def test_softmax_xent_fused_mean_autograd():
    """The scalar-mean fused path vs torch CE (fwd + bwd)."""
    from adanet_amd.ops.xent import softmax_xent
    torch.manual_seed(2)
    logits = torch.randn(128, 10, device=DEV).to(
        torch.bfloat16).requires_grad_(True)
    labels = torch.randint(0, 10, (128,), device=DEV)
    loss = softmax_xent(logits, labels, reduction="mean")
    lf = logits.detach().float().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lf, labels)
    assert abs(float(loss) - float(ref)) < 0.02
    loss.backward()
    ref.backward()
    assert (logits.grad.float() - lf.grad).abs().max() < 0.01


def test_softmax_xent_strided_view():
    """Padded logits: kernel must honor row stride (narrow view)."""
    ext = _ext()
    torch.manual_seed(0)
    full = torch.randn(64, 16, device=DEV).to(torch.bfloat16)
    logits = full[:, :10]
    labels = torch.randint(0, 10, (64,), device=DEV)
    loss = torch.empty(64, device=DEV, dtype=torch.float32)
    probs = torch.empty(64, 16, device=DEV, dtype=torch.bfloat16)[:, :10]
    ext.softmax_xent_fwd(logits, labels, loss, probs, 0.0, None)
    ref = torch.nn.functional.cross_entropy(logits.float(), labels,
                                            reduction="none")
    assert (loss - ref).abs().max() < 0.02


# ------------------------------------------------------------- mixer K5
@pytest.mark.parametrize("J", [5, 11])  # 11: two launches, 8 + 3 members
@pytest.mark.parametrize("vector_mode", [False, True])
def test_mixer_fwd_bwd(vector_mode, J):
    from adanet_amd.ops.mixer import weighted_sum_logits
    torch.manual_seed(0)
    B, C = 128, 10
    logits = [torch.randn(B, C, device=DEV).to(torch.bfloat16)
              for _ in range(J)]
    logits[-1].requires_grad_(True)
    shape = (C,) if vector_mode else ()
    weights = [torch.randn(shape, device=DEV, dtype=torch.float32,
                           requires_grad=True) for _ in range(J)]
    bias = torch.randn(C, device=DEV, dtype=torch.float32,
                       requires_grad=True)
    out = weighted_sum_logits(logits, weights, bias)
    ref = bias.float() + sum(w * l.float() for w, l in zip(weights, logits))
    assert (out.float() - ref).abs().max() < 0.05

    upstream = torch.randn(B, C, device=DEV).to(torch.bfloat16)
    out.backward(upstream)
    refs = torch.autograd.grad(
        (bias.float() + sum(w * l.float()
                            for w, l in zip(weights, logits))),
        [*weights, bias, logits[-1]], grad_outputs=upstream.float(),
        allow_unused=True)
    for i, w in enumerate(weights):
        rel = (w.grad - refs[i]).abs().max() / (refs[i].abs().max() + 1e-3)
        assert rel < 0.02, (i, rel)
    assert (bias.grad - refs[J]).abs().max() / (
        refs[J].abs().max() + 1e-3) < 0.02
    dl = logits[-1].grad.float()
    assert (dl - refs[J + 1]).abs().max() / (
        refs[J + 1].abs().max() + 1e-3) < 0.02


# ------------------------------------------------------------- optim K4
def test_fused_sgd_momentum_vs_fp32():
    ext = _ext()
    torch.manual_seed(0)
    n = 4097
    master = torch.randn(n, device=DEV, dtype=torch.float32)
    ref = master.clone()
    param = master.to(torch.bfloat16)
    mom = torch.zeros(n, device=DEV, dtype=torch.float32)
    ref_mom = torch.zeros_like(mom)
    for step in range(5):
        grad = torch.randn(n, device=DEV).to(torch.bfloat16)
        ext.fused_sgd(master, param, grad, mom, 0.1, 0.9, 0.0, 0.01, False,
                      1.0)
        g = grad.float() + 0.01 * ref
        ref_mom.mul_(0.9).add_(g)
        ref.add_(ref_mom, alpha=-0.1)
    assert (master - ref).abs().max() < 1e-4
    assert torch.equal(param, master.to(torch.bfloat16))


def test_fused_adam_vs_fp32():
    ext = _ext()
    torch.manual_seed(0)
    n = 1000
    master = torch.randn(n, device=DEV, dtype=torch.float32)
    p_ref = torch.nn.Parameter(master.clone())
    opt_ref = torch.optim.Adam([p_ref], lr=0.01)
    param = master.to(torch.bfloat16)
    m = torch.zeros(n, device=DEV, dtype=torch.float32)
    v = torch.zeros(n, device=DEV, dtype=torch.float32)
    for step in range(1, 6):
        grad = torch.randn(n, device=DEV).to(torch.bfloat16)
        ext.fused_adam(master, param, grad, m, v, 0.01, 0.9, 0.999, 1e-8,
                       0.0, step, 1.0)
        p_ref.grad = grad.float()
        opt_ref.step()
    assert (master - p_ref.detach()).abs().max() < 1e-3


def test_fused_sgd_fp32_matches_torch():
    ext = _ext()
    torch.manual_seed(0)
    p = torch.randn(513, device=DEV, dtype=torch.float32)
    p_ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.SGD([p_ref], lr=0.1, momentum=0.9, weight_decay=0.01)
    mom = torch.zeros_like(p)
    for _ in range(4):
        g = torch.randn(513, device=DEV, dtype=torch.float32)
        ext.fused_sgd_fp32(p, g, mom, 0.1, 0.9, 0.0, 0.01, False, 1.0)
        p_ref.grad = g.clone()
        opt.step()
    assert (p - p_ref.detach()).abs().max() < 1e-5


def test_fused_adam_fp32_matches_torch():
    ext = _ext()
    torch.manual_seed(0)
    p = torch.randn(257, device=DEV, dtype=torch.float32)
    p_ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([p_ref], lr=0.01)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for t in range(1, 5):
        g = torch.randn(257, device=DEV, dtype=torch.float32)
        ext.fused_adam_fp32(p, g, m, v, 0.01, 0.9, 0.999, 1e-8, 0.0, t, 1.0)
        p_ref.grad = g.clone()
        opt.step()
    assert (p - p_ref.detach()).abs().max() < 1e-5


def test_colsum_two_stage_large_B():
    ext = _ext()
    torch.manual_seed(1)
    x = torch.randn(4096, 32, device=DEV).to(torch.bfloat16)
    out = torch.empty(32, device=DEV, dtype=torch.float32)
    ext.colsum_bf16(x, out)
    ref = x.float().sum(dim=0)
    assert (out - ref).abs().max() / (ref.abs().max() + 1e-3) < 0.01


# ------------------------------------------------------------- layernorm K8
def test_layernorm_fwd_bwd():
    from adanet_amd.ops.layernorm import HipLayerNorm
    torch.manual_seed(0)
    B, D = 256, 2048
    ln = HipLayerNorm(D).to(DEV)
    x = torch.randn(B, D, device=DEV).to(torch.bfloat16).requires_grad_(True)
    y = ln(x)
    ref = torch.nn.functional.layer_norm(x.float(), (D,), ln.weight,
                                         ln.bias)
    assert (y.float() - ref).abs().max() < 0.05
    up = torch.randn(B, D, device=DEV).to(torch.bfloat16)
    y.backward(up)
    xf = x.detach().float().requires_grad_(True)
    wf = ln.weight.detach().clone().requires_grad_(True)
    bf = ln.bias.detach().clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xf, (D,), wf, bf).backward(up.float())
    assert (x.grad.float() - xf.grad).abs().max() < 0.05
    rel_g = (ln.weight.grad - wf.grad).abs().max() / (
        wf.grad.abs().max() + 1e-3)
    assert rel_g < 0.05


# ------------------------------------------------------------- dropout K3
def test_dropout_stats_and_bwd_mask_match():
    ext = _ext()
    x = torch.ones(1 << 20, device=DEV, dtype=torch.bfloat16)
    y = torch.empty_like(x)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    ext.dropout_fwd(x, y, 0.25, seed)
    kept = (y != 0).float().mean().item()
    assert abs(kept - 0.75) < 0.01
    assert abs(y.float().mean().item() - 1.0) < 0.02  # scaled to E[x]
    dy = torch.ones_like(x)
    dx = torch.empty_like(x)
    ext.dropout_bwd(dy, dx, 0.25, seed)
    # identical mask in fwd and bwd
    assert torch.equal((y != 0), (dx != 0))


def test_dropout_module_fresh_masks_and_autograd():
    from adanet_amd.ops.dropout import HipDropout
    torch.manual_seed(0)
    d = HipDropout(0.5).to(DEV)
    d.train()
    x = torch.ones(1 << 16, device=DEV, dtype=torch.bfloat16,
                   requires_grad=True)
    y1 = d(x)
    y2 = d(x)
    # device counter advanced -> different masks across calls
    assert not torch.equal(y1, y2)
    y1.sum().backward()
    assert torch.equal((x.grad != 0), (y1 != 0))


def test_relu_bwd():
    ext = _ext()
    torch.manual_seed(0)
    y = torch.randn(4096, device=DEV).to(torch.bfloat16)
    dy = torch.randn(4096, device=DEV).to(torch.bfloat16)
    dx = torch.empty_like(dy)
    ext.relu_bwd(dy, y, dx)
    ref = torch.where(y.float() > 0, dy.float(), torch.zeros(()).to(DEV))
    assert torch.equal(dx.float(), ref.float())


# ------------------------------------------------------------- reduce K10
def test_colsum():
    ext = _ext()
    torch.manual_seed(0)
    x = torch.randn(1024, 300, device=DEV).to(torch.bfloat16)
    out = torch.empty(300, device=DEV, dtype=torch.float32)
    ext.colsum_bf16(x, out)
    ref = x.float().sum(dim=0)
    assert (out - ref).abs().max() / (ref.abs().max() + 1e-3) < 0.01


def test_argmax_correct():
    ext = _ext()
    torch.manual_seed(0)
    logits = torch.randn(512, 10, device=DEV).to(torch.bfloat16)
    labels = torch.randint(0, 10, (512,), device=DEV)
    pred = torch.empty(512, device=DEV, dtype=torch.int64)
    correct = torch.zeros(1, device=DEV, dtype=torch.int32)
    ext.argmax_correct(logits, labels, pred, correct)
    ref_pred = logits.float().argmax(dim=1)
    assert torch.equal(pred, ref_pred)
    assert correct.item() == (ref_pred == labels).sum().item()


# ------------------------------------------------------------- HipLinear e2e
def test_hip_linear_autograd_vs_fp32():
    from adanet_amd.ops.linear import HipLinear
    torch.manual_seed(0)
    B, K, N = 256, 512, 384
    lin = HipLinear(K, N, activation="relu").to(DEV)
    x = torch.randn(B, K, device=DEV).to(torch.bfloat16).requires_grad_(True)
    y = lin(x)
    w = lin.weight.detach().float().requires_grad_(True)
    b = lin.bias.detach().float().requires_grad_(True)
    xf = x.detach().float().requires_grad_(True)
    ref = torch.relu(xf @ w.t() + b)
    rel = (y.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.01
    up = torch.randn(B, N, device=DEV).to(torch.bfloat16)
    y.backward(up)
    ref.backward(up.float())
    for got, want in [(x.grad.float(), xf.grad), (lin.weight.grad.float(),
                                                  w.grad),
                      (lin.bias.grad, b.grad)]:
        rel = (got - want).abs().mean() / (want.abs().mean() + 1e-3)
        assert rel < 0.02, rel


def test_arena_flattened_sgd_matches_unflattened_training():
    """FusedSGD's parameter-arena flattening must not change training
    numerics: same module trained with arena (multi-param, GPU) vs the
    fp32 per-tensor reference math."""
    from adanet_amd.ops.linear import HipLinear
    from adanet_amd.ops.optim import FusedSGD
    torch.manual_seed(0)
    model = torch.nn.Sequential(
        HipLinear(64, 64, activation="relu"),
        HipLinear(64, 32),
    ).to(DEV)
    # fp32 mirror
    w = [p.detach().float().clone() for p in model.parameters()]
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9)
    mom = [torch.zeros_like(x) for x in w]
    for step in range(5):
        x = torch.randn(32, 64, device=DEV).to(torch.bfloat16)
        y = model(x)
        opt.zero_grad(set_to_none=True)
        y.float().pow(2).mean().backward()
        grads = [p.grad.detach().float().clone()
                 for p in model.parameters()]
        opt.step()
        for i in range(len(w)):
            mom[i].mul_(0.9).add_(grads[i].view_as(mom[i]))
            w[i].add_(mom[i], alpha=-0.05)
    assert opt._arenas, "arena flattening did not engage"
    for p, ref in zip(model.parameters(), w):
        err = (p.detach().float() - ref).abs().max()
        assert err < 0.05, err
    # flat grad buffers exposed for DP all-reduce
    bufs = opt.flat_grad_buffers()
    assert sum(b.numel() for b in bufs) == sum(
        p.numel() for p in model.parameters())


def test_direct_grad_writes_match_autograd():
    """direct_grad_writes (accumulate epilogue into .grad views) must
    produce the same dW/db as the standard autograd accumulate path,
    including double-use accumulation within one backward."""
    from adanet_amd.ops.linear import HipLinear, direct_grad_writes
    torch.manual_seed(1)
    B, K, N = 128, 256, 96
    lin = HipLinear(K, N, activation="relu").to(DEV)
    x = torch.randn(B, K, device=DEV).to(torch.bfloat16)

    # reference: plain autograd
    lin.zero_grad(set_to_none=True)
    (lin(x).float().mean() + lin(x * 0.5).float().mean()).backward()
    ref_w = lin.weight.grad.detach().clone()
    ref_b = lin.bias.grad.detach().clone()

    # direct: pre-pinned zeroed grads + context
    lin.weight.grad = torch.zeros_like(lin.weight)
    lin.bias.grad = torch.zeros_like(lin.bias)
    with direct_grad_writes():
        (lin(x).float().mean() + lin(x * 0.5).float().mean()).backward()
    for got, want in [(lin.weight.grad.float(), ref_w.float()),
                      (lin.bias.grad, ref_b)]:
        rel = (got - want).abs().mean() / (want.abs().mean() + 1e-6)
        assert rel < 0.02, rel


def test_gemm_accumulate_epilogue():
    """act=2 adds into C for both the NT and transposed-staging GEMMs."""
    ext = _ext()
    torch.manual_seed(2)
    M, N, K = 256, 128, 64
    A = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    Bm = torch.randn(N, K, device=DEV).to(torch.bfloat16)
    C0 = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    C = C0.clone()
    ext.gemm_nt_bf16(A, Bm, C, None, 2)
    ref = (C0.float() + A.float() @ Bm.float().t())
    rel = (C.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.02, rel
    # tr (both transposed), accumulate
    At = A.t().contiguous()
    Bt = Bm.t().contiguous()
    C = C0.clone()
    ext.gemm_tr_bf16(At, Bt, C, None, 2, 1, 1)
    rel = (C.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.02, rel
    # colsum accumulate mode
    out0 = torch.randn(K, device=DEV, dtype=torch.float32)
    out = out0.clone()
    ext.colsum_bf16(A, out, 1)
    refc = out0 + A.float().sum(dim=0)
    assert (out - refc).abs().max() < 0.5


def test_binary_histogram_kernel_matches_cpu():
    from adanet_amd.core.eval_metrics import AUCAccumulator
    torch.manual_seed(3)
    s = torch.rand(4096)
    y = (torch.rand(4096) > 0.5).long()
    cpu = AUCAccumulator(200)
    cpu.update(s, y)
    gpu = AUCAccumulator(200)
    gpu.update(s.to(DEV), y.to(DEV))
    assert torch.equal(cpu._hist.cpu(), gpu._hist.cpu())
    g, c = gpu.value(), cpu.value()
    assert abs(g["auc"] - c["auc"]) < 1e-9


@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemm_gemv_path_small_m(M):
    """M<=8 dispatches to the wave-per-column GEMV kernel."""
    ext = _ext()
    torch.manual_seed(4)
    N, K = 2048, 3072
    A = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    Bm = torch.randn(N, K, device=DEV).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV, dtype=torch.float32)
    C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    ext.gemm_nt_bf16(A, Bm, C, bias, 1)
    ref = torch.relu(A.float() @ Bm.float().t() + bias)
    rel = (C.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.02, rel


def test_overwrite_grad_mode_matches_standard():
    """_overwrite_grads (skip arena memset + overwrite epilogue) must
    train identically to the standard accumulate path."""
    from adanet_amd.ops.linear import HipLinear, direct_grad_writes
    from adanet_amd.ops.optim import FusedSGD
    torch.manual_seed(5)

    def build():
        torch.manual_seed(5)
        return torch.nn.Sequential(
            HipLinear(64, 96, activation="relu"),
            HipLinear(96, 32),
        ).to(DEV)

    outs = []
    for overwrite in (False, True):
        model = build()
        opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9)
        if overwrite:
            opt._overwrite_grads = True
        torch.manual_seed(7)
        for _ in range(4):
            x = torch.randn(128, 64, device=DEV).to(torch.bfloat16)
            opt.zero_grad(set_to_none=True)
            with direct_grad_writes():
                model(x).float().pow(2).mean().backward()
            opt.step()
        outs.append([p.detach().float().clone() for p in model.parameters()])
        if overwrite:
            assert any(a["all_single_write"] is False or True
                       for a in opt._arenas)  # arenas engaged
            assert any(a["all_single_write"] for a in opt._arenas), \
                "weight arena should be single-write"
    for a, b in zip(*outs):
        # not bit-exact: the bias-grad colsum accumulates via fp32 atomics
        # whose order varies run-to-run (within EITHER mode); compare with
        # a tight tolerance instead.
        rel = (a - b).abs().max() / (b.abs().max() + 1e-6)
        assert rel < 5e-3, rel


def test_conv1x1_native_fwd_bwd_vs_fp32():
    from adanet_amd.ops.conv import _Conv1x1Fn
    torch.manual_seed(6)
    B, Ci, Co, H, W = 4, 64, 32, 16, 16
    x = torch.randn(B, Ci, H, W, device=DEV).to(
        torch.bfloat16).requires_grad_(True)
    w = torch.randn(Co, Ci, device=DEV).mul(0.1).to(
        torch.bfloat16).requires_grad_(True)
    b = torch.randn(Co, device=DEV, dtype=torch.float32).requires_grad_(True)
    y = _Conv1x1Fn.apply(x, w, b)
    xf = x.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    bf = b.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.conv2d(xf, wf.reshape(Co, Ci, 1, 1), bf)
    rel = (y.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.02, rel
    up = torch.randn_like(ref)
    y.backward(up.to(torch.bfloat16))
    ref.backward(up)
    for got, want in [(x.grad.float(), xf.grad), (w.grad.float(), wf.grad),
                      (b.grad, bf.grad)]:
        rel = (got - want).abs().mean() / (want.abs().mean() + 1e-6)
        assert rel < 0.03, rel


def test_hip_conv1x1_module_native_and_fallback():
    from adanet_amd.ops.conv import HipConv1x1
    torch.manual_seed(7)
    # aligned -> native path
    m = HipConv1x1(32, 64, bias=False).to(DEV).to(torch.bfloat16)
    x = torch.randn(2, 32, 8, 8, device=DEV).to(torch.bfloat16)
    y = m(x)
    ref = torch.nn.functional.conv2d(x.float(), m.weight.float())
    assert (y.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3) < 0.02
    # unaligned channels -> torch fallback, still correct
    m2 = HipConv1x1(12, 20, bias=False).to(DEV).to(torch.bfloat16)
    x2 = torch.randn(2, 12, 8, 8, device=DEV).to(torch.bfloat16)
    y2 = m2(x2)
    ref2 = torch.nn.functional.conv2d(x2.float(), m2.weight.float())
    assert (y2.float() - ref2).abs().mean() / (ref2.abs().mean() + 1e-3) < 0.03


def test_multi_copy_bf16():
    ext = _ext()
    torch.manual_seed(8)
    srcs = [torch.randn(37 + 100 * i, device=DEV).to(torch.bfloat16)
            for i in range(10)]
    dsts = [torch.zeros_like(s) for s in srcs]
    ext.multi_copy_bf16(srcs, dsts)
    torch.cuda.synchronize()
    for s, d in zip(srcs, dsts):
        assert torch.equal(s, d)


@pytest.mark.parametrize("B,C,H,W,KS,stride,pad", [
    # 289 px is no multiple of 8: scalar LDS staging everywhere. These
    # three keep the ids they had as (C, KS, stride).
    pytest.param(3, 24, 17, 17, 3, 1, 1, id="24-3-1"),
    pytest.param(3, 32, 17, 17, 5, 2, 2, id="32-5-2"),
    pytest.param(3, 7, 17, 17, 3, 2, 1, id="7-3-2"),
    # LDS fwd/dX image-outer, vectorised staging, ragged last group
    # (21 images, P = 16); LDS dW with 3 chunks.
    (3, 7, 16, 16, 3, 1, 1),
    # LDS fwd flat branch (8x8 outputs); LDS dX<5,2> with vector staging.
    (3, 7, 16, 16, 5, 2, 2),
    # KS = 7 on a non-square image (catches H/W swaps); LDS dX<7,1>, <7,2>.
    (2, 5, 16, 24, 7, 1, 3), (2, 5, 16, 24, 7, 2, 3),
    (2, 4, 16, 16, 3, 1, 0),  # pad = 0
    (2, 4, 13, 13, 3, 3, 1),  # stride 3: runtime dX kernel
    # KS = 9: runtime fwd and dX, tap-per-block dW.
    (2, 4, 12, 12, 9, 1, 4),
    # 9216 px > 8192: fwd_tmpl<3>, dx_tmpl<3,1>, dw_fused<3> (64 chunks).
    (1, 3, 96, 96, 3, 1, 1),
    # fwd_tmpl<5>; 48x48 dy fits, so LDS dX with P = 1; dw_fused<5>.
    (1, 3, 96, 96, 5, 2, 2),
    # runtime fwd (there is no fwd_tmpl<7>), dx_tmpl<7,1>, dw_fused<7>.
    (1, 2, 96, 96, 7, 1, 3),
    # 92x92 outputs > 8192 px: dx_tmpl<3,2> and dx_tmpl<7,2>.
    (1, 2, 184, 184, 3, 2, 1), (1, 2, 184, 184, 7, 2, 3),
])
def test_depthwise_conv_fwd_bwd_vs_fp32(B, C, H, W, KS, stride, pad):
    """Every dispatch tier of csrc/depthwise.hip against torch's fp32 grouped
    convolution. The one route left uncovered is B*C > 65535 (the grid-y
    limit, which sends templated tap sizes to the runtime-KS kernels): with
    images too large for the LDS tiers it needs over half a billion
    elements."""
    from adanet_amd.ops.conv import _DepthwiseFn
    torch.manual_seed(9)
    x = torch.randn(B, C, H, W, device=DEV).to(
        torch.bfloat16).requires_grad_(True)
    w = torch.randn(C, 1, KS, KS, device=DEV).mul(0.2).to(
        torch.bfloat16).requires_grad_(True)
    y = _DepthwiseFn.apply(x, w, stride, pad)
    xf = x.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    ref = torch.nn.functional.conv2d(xf, wf, None, stride, pad, groups=C)
    rel = (y.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.02, rel
    up = torch.randn_like(ref)
    y.backward(up.to(torch.bfloat16))
    ref.backward(up)
    for got, want in [(x.grad.float(), xf.grad), (w.grad.float(), wf.grad)]:
        rel = (got - want).abs().mean() / (want.abs().mean() + 1e-6)
        assert rel < 0.03, rel


def test_depthwise_rejects_bad_arguments():
    ext = _ext()
    bf = dict(device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(4, 1, 3, 3, **bf)
    dy = torch.zeros(2, 4, 8, 8, **bf)
    x_strided = torch.zeros(2, 4, 8, 16, **bf)[..., ::2]
    assert x_strided.shape == dy.shape and not x_strided.is_contiguous()
    with pytest.raises(RuntimeError):
        ext.depthwise_bwd_dw(x_strided, dy, torch.empty(36, device=DEV), 1, 1)
    with pytest.raises(RuntimeError):  # 3x3, stride 1, pad 1 keeps 8x8
        ext.depthwise_bwd_dx(torch.zeros(2, 4, 7, 7, **bf), w,
                             torch.empty(2, 4, 8, 8, **bf), 1, 1)


def test_conv_nxn_unfold_gemm_vs_fp32():
    from adanet_amd.ops.conv import HipConvNxN
    torch.manual_seed(11)
    m = HipConvNxN(3, 32, 3, padding=1).to(DEV).to(torch.bfloat16)
    from adanet_amd.ops.linear import restore_fp32_params
    restore_fp32_params(m)
    x = torch.randn(4, 3, 16, 16, device=DEV).to(
        torch.bfloat16).requires_grad_(True)
    y = m(x)
    xf = x.detach().float().requires_grad_(True)
    wf = m.weight.detach().float().requires_grad_(True)
    bf = m.bias.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.conv2d(xf, wf, bf, 1, 1)
    rel = (y.float() - ref).abs().mean() / (ref.abs().mean() + 1e-3)
    assert rel < 0.02, rel
    up = torch.randn_like(ref)
    y.backward(up.to(torch.bfloat16))
    ref.backward(up)
    for got, want in [(x.grad.float(), xf.grad),
                      (m.weight.grad.float(), wf.grad),
                      (m.bias.grad, bf.grad)]:
        rel = (got - want).abs().mean() / (want.abs().mean() + 1e-6)
        assert rel < 0.05, rel
    # stride-2 1x1 variant (FactorizedReduction path)
    m2 = HipConvNxN(32, 32, 1, stride=2, bias=False).to(DEV).to(
        torch.bfloat16)
    x2 = torch.randn(2, 32, 16, 16, device=DEV).to(torch.bfloat16)
    y2 = m2(x2)
    ref2 = torch.nn.functional.conv2d(x2.float(), m2.weight.float(),
                                      None, 2, 0)
    assert (y2.float() - ref2).abs().mean() / (
        ref2.abs().mean() + 1e-3) < 0.02


# ------------------------------------------------------------ batchnorm K8
@pytest.mark.parametrize("N,C,H,W", [
    (8, 32, 16, 16),   # 8 image chunks per channel + finalize
    (1, 16, 8, 8),     # one image: a single chunk finishes in place
    (2, 1100, 4, 4),   # C > 1024: a single chunk as well
])
def test_batchnorm_train_fwd_bwd_vs_fp32(N, C, H, W):
    """Native BN (csrc/batchnorm.hip) vs torch fp32 BatchNorm2d: forward,
    running stats, and dx/dgamma/dbeta in train mode."""
    from adanet_amd.ops.batchnorm import HipBatchNorm2d
    torch.manual_seed(11)
    x = torch.randn(N, C, H, W, device=DEV)
    bn = HipBatchNorm2d(C, momentum=0.1, eps=1e-3).to(DEV)
    ref = torch.nn.BatchNorm2d(C, momentum=0.1, eps=1e-3).to(DEV)
    with torch.no_grad():
        ref.weight.copy_(torch.rand(C) + 0.5)
        ref.bias.copy_(torch.randn(C) * 0.1)
        bn.weight.copy_(ref.weight)
        bn.bias.copy_(ref.bias)
    xb = x.to(torch.bfloat16).requires_grad_(True)
    xf = x.clone().requires_grad_(True)
    y = bn(xb)
    yr = ref(xf)
    assert (y.float() - yr).abs().max().item() < 0.05
    assert torch.allclose(bn.running_mean, ref.running_mean, atol=1e-2)
    assert torch.allclose(bn.running_var, ref.running_var, atol=1e-2)
    g = torch.randn_like(yr)
    y.backward(g.to(torch.bfloat16))
    yr.backward(g)
    assert (xb.grad.float() - xf.grad).abs().max().item() < 0.05
    assert torch.allclose(bn.weight.grad, ref.weight.grad, atol=0.3,
                          rtol=0.05)
    assert torch.allclose(bn.bias.grad, ref.bias.grad, atol=0.3, rtol=0.05)


def test_batchnorm_eval_mode_uses_running_stats():
    from adanet_amd.ops.batchnorm import HipBatchNorm2d
    torch.manual_seed(12)
    C = 16
    bn = HipBatchNorm2d(C, eps=1e-3).to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C) * 0.3)
        bn.running_var.copy_(torch.rand(C) + 0.5)
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.1)
    bn.eval()
    x = torch.randn(4, C, 8, 8, device=DEV)
    y = bn(x.to(torch.bfloat16))
    ref = torch.nn.functional.batch_norm(
        x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False,
        0.1, 1e-3)
    assert (y.float() - ref).abs().max().item() < 0.05


def test_batchnorm_odd_hw_scalar_path():
    """HW % 8 != 0 exercises the scalar stats loop."""
    from adanet_amd.ops.batchnorm import HipBatchNorm2d
    torch.manual_seed(13)
    x = torch.randn(4, 8, 5, 3, device=DEV)
    bn = HipBatchNorm2d(8, eps=1e-3).to(DEV)
    y = bn(x.to(torch.bfloat16))
    ref = torch.nn.functional.batch_norm(
        x, None, None, bn.weight, bn.bias, True, 0.1, 1e-3)
    assert (y.float() - ref).abs().max().item() < 0.05


# --------------------------------------------------------------- pool3 K9
@pytest.mark.parametrize("kind,stride", [("avg", 1), ("avg", 2),
                                         ("max", 1), ("max", 2)])
def test_pool3_fwd_bwd_vs_fp32(kind, stride):
    from adanet_amd.ops.conv import HipPool2d
    torch.manual_seed(21)
    x = torch.randn(4, 12, 15, 15, device=DEV)   # odd HW: edge windows
    xb = x.to(torch.bfloat16).requires_grad_(True)
    # reference on the bf16-ROUNDED values: max-pool tie-breaks must see
    # the same inputs or the argmax (and thus the routed gradient) differs
    xf = x.to(torch.bfloat16).float().requires_grad_(True)
    pool = HipPool2d(kind, stride)
    y = pool(xb)
    if kind == "avg":
        yr = torch.nn.functional.avg_pool2d(xf, 3, stride, 1,
                                            count_include_pad=False)
    else:
        yr = torch.nn.functional.max_pool2d(xf, 3, stride, 1)
    assert y.shape == yr.shape
    assert (y.float() - yr).abs().max().item() < 0.03
    g = torch.randn_like(yr)
    y.backward(g.to(torch.bfloat16))
    yr.backward(g)
    # dx is bf16: up to 9 summed dy values -> one-ulp ~0.06 at |dx|~6
    assert (xb.grad.float() - xf.grad).abs().max().item() < 0.08


# ------------------------------------------------- fused dropout epilogue
def test_fused_gemm_dropout_statistics_and_grads():
    """act=3 GEMM epilogue: kept fraction ~= 1-p, kept values = relu/(1-p),
    and backward is the y>0 mask scaled by 1/(1-p) (no mask storage)."""
    from adanet_amd.ops.linear import HipLinear
    torch.manual_seed(33)
    B, D, H, p = 512, 256, 512, 0.3
    lin = HipLinear(D, H, activation="relu", dropout=p).to(DEV)
    lin = lin.to(torch.bfloat16)
    from adanet_amd.ops.linear import restore_fp32_params
    restore_fp32_params(lin)
    x = torch.randn(B, D, device=DEV).to(torch.bfloat16).requires_grad_(True)
    lin.train()
    y = lin(x)
    # reference pre-dropout activation
    with torch.no_grad():
        ref = torch.relu(x.float() @ lin.weight.float().t() +
                         lin.bias.float())[:, :H]
    kept = (y.float() > 0)
    pos = ref > 1e-3
    drop_rate = 1.0 - kept[pos].float().mean().item()
    assert abs(drop_rate - p) < 0.03, drop_rate
    # kept positives match ref/(1-p)
    sel = kept & pos
    ratio = (y.float()[sel] / ref[sel])
    assert (ratio - 1.0 / (1.0 - p)).abs().max().item() < 0.05
    # backward: dx through the scaled mask
    g = torch.randn_like(y)
    y.backward(g)
    with torch.no_grad():
        dz = g.float() * kept.float() / (1.0 - p)
        dx_ref = dz @ lin.weight.float()
    assert (x.grad.float() - dx_ref).abs().max().item() < 0.15


def test_fused_dropout_fresh_mask_per_step_and_eval_off():
    from adanet_amd.ops.linear import HipLinear, restore_fp32_params
    torch.manual_seed(34)
    lin = HipLinear(64, 128, activation="relu", dropout=0.5).to(DEV)
    lin = lin.to(torch.bfloat16)
    restore_fp32_params(lin)
    x = torch.randn(256, 64, device=DEV).to(torch.bfloat16)
    lin.train()
    y1 = lin(x)
    y2 = lin(x)
    assert not torch.equal(y1, y2), "mask must differ across steps"
    lin.eval()
    y3 = lin(x)
    ref = torch.relu(x.float() @ lin.weight.float().t() + lin.bias.float())
    assert (y3.float() - ref).abs().max().item() < 0.1


# ------------------------------------------------------- batched im2col
@pytest.mark.parametrize("K,stride,pad,cin", [(3, 1, 1, 7), (3, 2, 1, 16),
                                              (1, 2, 0, 9), (5, 1, 2, 4)])
def test_im2col_col2im_vs_unfold(K, stride, pad, cin):
    ext = _ext()
    torch.manual_seed(41)
    B, H, W = 5, 13, 11
    x = torch.randn(B, cin, H, W, device=DEV).to(torch.bfloat16)
    oh = (H + 2 * pad - K) // stride + 1
    ow = (W + 2 * pad - K) // stride + 1
    ckk = cin * K * K
    ckk_pad = (ckk + 31) // 32 * 32
    out = torch.empty((B, ckk_pad, oh, ow), device=DEV, dtype=torch.bfloat16)
    ext.im2col_bf16(x, out, K, stride, pad)
    ref = torch.nn.functional.unfold(x.float(), K, padding=pad,
                                     stride=stride)
    got = out.float().reshape(B, ckk_pad, -1)
    assert torch.equal(got[:, :ckk], ref.to(torch.bfloat16).float())
    assert (got[:, ckk:] == 0).all()
    # col2im == unfold's adjoint (fold)
    du = torch.randn(B, ckk_pad, oh, ow, device=DEV).to(torch.bfloat16)
    dx = torch.empty_like(x)
    ext.col2im_bf16(du, dx, K, stride, pad)
    ref_dx = torch.nn.functional.fold(
        du.float().reshape(B, ckk_pad, -1)[:, :ckk], (H, W), K,
        padding=pad, stride=stride)
    assert (dx.float() - ref_dx).abs().max().item() < 0.15


def test_conv_nxn_fwd_bwd_vs_torch():
    from adanet_amd.ops.conv import HipConvNxN
    torch.manual_seed(42)
    conv = HipConvNxN(16, 32, 3, stride=1, padding=1, bias=True).to(DEV)
    conv.weight.data = conv.weight.data.to(torch.bfloat16)
    x = torch.randn(4, 16, 16, 16, device=DEV)
    xb = x.to(torch.bfloat16).requires_grad_(True)
    y = conv(xb)
    ref = torch.nn.functional.conv2d(
        x, conv.weight.float(), conv.bias.float(), 1, 1)
    assert (y.float() - ref).abs().max().item() < 0.2
    g = torch.randn_like(y)
    y.backward(g)
    xf = x.clone().requires_grad_(True)
    wf = conv.weight.detach().float().requires_grad_(True)
    torch.nn.functional.conv2d(xf, wf, conv.bias.detach().float(), 1,
                               1).backward(g.float())
    assert (xb.grad.float() - xf.grad).abs().max().item() < 0.2
    assert (conv.weight.grad.float() - wf.grad).abs().max().item() / (
        wf.grad.abs().max().item() + 1e-3) < 0.05
