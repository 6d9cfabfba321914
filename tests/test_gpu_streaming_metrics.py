"""Streaming eval-metric kernels (csrc/eval_metrics.hip) against the fp64 CPU
reference of ops/metrics.py on the same bf16 / fp32 logits."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32_EPS = 2.0 ** -23


def _ops():
    from adanet_amd.ops import metrics as metric_ops
    return metric_ops


def _strided(values, ld):
    """`values` [B, C] as a narrow view of a [B, ld] device buffer."""
    B, C = values.shape
    buf = torch.full((B, ld), 77.0, dtype=values.dtype, device=DEV)
    buf[:, :C] = values.to(DEV)
    return buf[:, :C]


# ----------------------------------------------------------------------
# multiclass
# ----------------------------------------------------------------------

def _multiclass_cases():
    # (B, C, row stride, k, eps)
    cases = [(1, 2, 2, 1, 0.0),
             (3, 10, 16, 5, 0.1),    # narrow view, fewer rows than waves
             (5, 64, 64, 5, 0.0),
             (7, 65, 72, 5, 0.0),    # one class past a full wave
             (4, 3, 3, 5, 0.0),      # k >= C
             (130, 1000, 1000, 5, 0.0)]
    return cases + ["second_row"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("ties", [False, True], ids=["normal", "ties"])
@pytest.mark.parametrize("case", _multiclass_cases(), ids=str)
def test_multiclass_kernel_matches_reference(case, ties, dtype):
    from adanet_amd.ops.xent import softmax_xent
    ops = _ops()
    if case == "second_row":
        # more rows than the grid has waves: some wave takes a second row
        case = (4 * ops.max_blocks() + 3, 5, 8, 2, 0.1)
    B, C, ld, k, eps = case
    g = torch.Generator().manual_seed(B * 131 + C)
    if ties:
        vals = torch.randint(-2, 3, (B, C), generator=g).float()
    else:
        vals = torch.randn(B, C, generator=g)
    vals = vals.to(torch.bfloat16)      # fp32 runs see the same values
    labels = torch.randint(0, C, (B,), generator=g)
    labels[0], labels[-1] = 0, C - 1
    logits = _strided(vals.to(dtype), ld)
    assert logits.stride(0) == ld

    want = ops.new_state(ops.multiclass_state_size(C, True))
    ops.multiclass_update(want, vals.to(dtype), labels, k=k,
                          label_smoothing=eps, per_class=True)
    got = ops.new_state(ops.multiclass_state_size(C, True), DEV)
    ops.multiclass_update(got, logits, labels.to(DEV), k=k,
                          label_smoothing=eps, per_class=True)
    got = got.cpu()

    # E: the largest per-row error of the existing loss kernel on this input
    v = vals.double()
    rows64 = torch.logsumexp(v, 1) - (1 - eps) * v.gather(
        1, labels.view(-1, 1))[:, 0] - (eps / C) * v.sum(1)
    rows_kernel = softmax_xent(vals.to(DEV).contiguous(), labels.to(DEV),
                               label_smoothing=eps, reduction="none")
    E = float((rows_kernel.double().cpu() - rows64).abs().max())
    mean64 = float(want[1]) / B
    bound = E if E > 0 else FP32_EPS * abs(mean64)
    dev = abs(float(got[1]) / B - mean64)
    print("multiclass %s ties=%s %s: |mean - mean64| = %.3e (E = %.3e)"
          % (case, ties, dtype, dev, E))

    assert got[0].item() == B
    counts_got, counts_want = got.clone(), want.clone()
    counts_got[1] = counts_want[1] = 0
    assert torch.equal(counts_got, counts_want)
    if k >= C:
        assert got[3].item() == B
    assert dev <= bound
    assert dev <= 0.02


def test_multiclass_nan_row_and_bad_label_make_loss_nan():
    ops = _ops()
    vals = torch.randn(9, 6, generator=torch.Generator().manual_seed(1))
    labels = torch.arange(9) % 6
    nan_row = vals.clone()
    nan_row[4, 3] = float("nan")
    state = ops.new_state(4, DEV)
    ops.multiclass_update(state, nan_row.to(DEV), labels.to(DEV))
    assert torch.isnan(state[1]).item() and state[0].item() == 9
    bad = labels.clone()
    bad[2] = 6      # out of range: nothing is read or counted for that row
    state = ops.new_state(ops.multiclass_state_size(6, True), DEV)
    ops.multiclass_update(state, vals.to(DEV), bad.to(DEV), per_class=True)
    assert torch.isnan(state[1]).item()
    assert state[4:10].sum().item() == 8


# ----------------------------------------------------------------------
# binary
# ----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [8, 200])
@pytest.mark.parametrize("B", [1, 255, 257, 4099])
def test_binary_kernel_matches_reference(B, T, dtype):
    from adanet_amd.head import BinaryClassHead
    ops = _ops()
    g = torch.Generator().manual_seed(B * 7 + T)
    x = (torch.randn(B, generator=g) * 3).clamp(-16, 16).to(torch.bfloat16)
    x[B // 2] = 0.0
    x = x.to(dtype)
    y = torch.randint(0, 2, (B,), generator=g)
    size = ops.binary_state_size(T)

    # loss and accuracy: every row
    want = ops.binary_update(ops.new_state(size), x, y, num_thresholds=T)
    got = ops.binary_update(ops.new_state(size, DEV), x.to(DEV).view(B, 1),
                            y.to(DEV), num_thresholds=T).cpu()
    dev = abs(float(got[1]) - float(want[1])) / B
    print("binary B=%d T=%d %s: |mean - mean64| = %.3e" % (B, T, dtype, dev))
    assert got[0].item() == B
    assert got[2].item() == want[2].item()
    assert dev <= 1e-4

    # histogram: without the rows whose fp64 p*T lies within 1e-3 of an
    # interior bin edge, where a last-ulp sigmoid difference may move the
    # bin. x == 0 stays: its fp32 sigmoid is exactly 0.5 on any device.
    pt = torch.sigmoid(x.double()) * T
    edge = pt.round()
    near = ((pt - edge).abs() < 1e-3) & (edge >= 1) & (edge <= T - 1)
    keep = ~near | (x == 0)
    assert float((~keep).sum()) / B <= 0.01
    xk, yk = x[keep], y[keep]
    head = BinaryClassHead()
    ref = head.streaming_metrics(num_thresholds=T)
    ref.update(xk, yk)
    dut = head.streaming_metrics(device=DEV, num_thresholds=T)
    dut.update(xk.to(DEV), yk.to(DEV))
    assert torch.equal(dut.state.cpu()[3:], ref.state[3:])
    assert dut.state[2].item() == ref.state[2].item()
    r_ref, r_dut = ref.result(), dut.result()
    for key in ("auc", "precision", "recall"):
        assert r_dut[key] == pytest.approx(r_ref[key], rel=1e-12, abs=1e-12,
                                           nan_ok=True)


def test_binary_strided_logits():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(300, 1, generator=g) * 3).to(torch.bfloat16)
    y = torch.randint(0, 2, (300,), generator=g)
    want = ops.binary_update(ops.new_state(3 + 16), x, y, num_thresholds=8)
    got = ops.binary_update(ops.new_state(3 + 16, DEV), _strided(x, 8),
                            y.to(DEV), num_thresholds=8).cpu()
    assert got[2].item() == want[2].item()
    assert got[3:].sum().item() == 300
    assert abs(float(got[1] - want[1])) / 300 <= 1e-4


# ----------------------------------------------------------------------
# regression
# ----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,D", [(1, 1), (257, 3), (4099, 1)])
def test_regression_kernel_matches_reference(B, D, dtype):
    ops = _ops()
    g = torch.Generator().manual_seed(B + D)
    x = torch.randn(B, D, generator=g).to(dtype)
    y = torch.randn(B, D, generator=g)
    want = ops.regression_update(ops.new_state(3), x, y)
    got = ops.regression_update(ops.new_state(3, DEV), _strided(x, D + 5),
                                y.to(DEV)).cpu()
    assert got[0].item() == B * D
    for slot in (1, 2):
        rel = abs(float(got[slot] - want[slot])) / float(want[slot])
        print("regression (%d, %d) %s slot %d: rel = %.3e"
              % (B, D, dtype, slot, rel))
        assert rel <= 1e-6


# ----------------------------------------------------------------------
# determinism, split invariance, reset, merge
# ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _common_case(kind):
    from adanet_amd.head import (BinaryClassHead, MultiClassHead,
                                 RegressionHead)
    g = torch.Generator().manual_seed(17)
    B = 1100       # more than one block in every kernel
    if kind == "multiclass":
        return (MultiClassHead(37, label_smoothing=0.1),
                dict(k=3, per_class=True),
                torch.randn(B, 37, generator=g).to(torch.bfloat16).to(DEV),
                torch.randint(0, 37, (B,), generator=g).to(DEV), [1])
    if kind == "binary":
        return (BinaryClassHead(), dict(num_thresholds=50),
                (torch.randn(B, 1, generator=g) * 3).to(torch.bfloat16)
                .to(DEV), torch.randint(0, 2, (B,), generator=g).to(DEV), [1])
    return (RegressionHead(3), {},
            torch.randn(B, 3, generator=g).to(DEV),
            torch.randn(B, 3, generator=g).to(DEV), [1, 2])


def _run(head, options, logits, labels, sizes):
    state = head.streaming_metrics(device=DEV, **options)
    off = 0
    for n in sizes:
        state.update(logits[off:off + n], labels[off:off + n])
        off += n
    assert off == logits.shape[0]
    return state


def _assert_close_states(a, b, float_slots):
    a, b = a.cpu().clone(), b.cpu().clone()
    for i in float_slots:
        assert a[i].item() == pytest.approx(b[i].item(), rel=1e-12)
        a[i] = b[i] = 0
    assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["multiclass", "binary", "regression"])
def test_determinism_split_reset_merge(kind):
    head, options, logits, labels, float_slots = _common_case(kind)
    B = logits.shape[0]
    sizes = [5, 1, 600, B - 606]
    one = _run(head, options, logits, labels, sizes)
    two = _run(head, options, logits, labels, sizes)
    assert torch.equal(one.state, two.state)      # bit-deterministic

    whole = _run(head, options, logits, labels, [B])
    _assert_close_states(one.state, whole.state, float_slots)

    first = _run(head, options, logits[:B // 2], labels[:B // 2], [B // 2])
    second = _run(head, options, logits[B // 2:], labels[B // 2:],
                  [B - B // 2])
    first.merge_(second)
    _assert_close_states(first.state, whole.state, float_slots)

    whole.reset()
    assert torch.equal(whole.state, torch.zeros_like(whole.state))
    assert whole.state.device.type == "cuda"


def test_multihead_state_on_narrow_views():
    from adanet_amd.head import (BinaryClassHead, MultiClassHead, MultiHead,
                                 RegressionHead)
    head = MultiHead({"bin": BinaryClassHead(), "cls": MultiClassHead(5),
                      "reg": RegressionHead(2)})
    g = torch.Generator().manual_seed(9)
    B = 70
    logits = torch.randn(B, 8, generator=g).to(torch.bfloat16)
    labels = {"bin": torch.randint(0, 2, (B,), generator=g),
              "cls": torch.randint(0, 5, (B,), generator=g),
              "reg": torch.randn(B, 2, generator=g)}
    ref = head.streaming_metrics()
    ref.update(logits, labels)
    dut = head.streaming_metrics(device=DEV)
    dut.update(logits.to(DEV), {k: v.to(DEV) for k, v in labels.items()})
    want, got = ref.result(), dut.result()
    assert set(got) == set(want)
    for key, v in want.items():
        tol = 1e-4 if "loss" in key or "error" in key else 1e-12
        assert got[key] == pytest.approx(v, abs=tol, rel=tol), key


# ----------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------

def test_evaluate_streaming_agrees_with_default_on_equal_batches(tmp_path):
    import adanet_amd
    from adanet_amd.head import MultiClassHead
    from adanet_amd.models import simple_dnn

    torch.manual_seed(0)
    N, D, C = 512, 16, 4
    X = torch.randn(N, D)
    Y = (X @ torch.randn(D, C)).argmax(dim=1)

    def train_fn():
        def gen():
            g = torch.Generator().manual_seed(7)
            while True:
                idx = torch.randint(0, N, (64,), generator=g)
                yield X[idx], Y[idx]
        return gen()

    def eval_fn():
        return iter([(X[i:i + 64], Y[i:i + 64]) for i in range(0, N, 64)])

    est = adanet_amd.Estimator(
        head=MultiClassHead(C),
        subnetwork_generator=simple_dnn.Generator(layer_size=32),
        max_iteration_steps=6, model_dir=str(tmp_path / "model"),
        config=adanet_amd.RunConfig(tf_random_seed=42))
    est.train(train_fn, max_steps=6)
    plain = est.evaluate(eval_fn)
    streamed = est.evaluate(eval_fn, streaming=True)
    print("engine: accuracy %.6f / %.6f, average_loss %.6f / %.6f"
          % (plain["accuracy"], streamed["accuracy"], plain["average_loss"],
             streamed["average_loss"]))
    # equal batches: the batch mean is the global mean
    assert abs(streamed["accuracy"] - plain["accuracy"]) <= 1e-6
    assert abs(streamed["average_loss"] - plain["average_loss"]) <= 0.02
    assert streamed["loss"] == streamed["average_loss"]
    assert 0.0 <= streamed["top_k_accuracy"] <= 1.0
    assert streamed["global_step"] == plain["global_step"]
