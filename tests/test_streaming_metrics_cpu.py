"""Streaming eval metrics on CPU: the fp64 references of ops/metrics.py
against per-row loops, the head states, and the opt-in engine wiring."""

import math

import pytest
import torch

import adanet_amd
from adanet_amd.core.eval_metrics import AUCAccumulator
from adanet_amd.core.evaluator import Objective
from adanet_amd.head import (BinaryClassHead, Head, MultiClassHead,
                             MultiHead, RegressionHead)
from adanet_amd.models import simple_dnn
from adanet_amd.ops import metrics as metric_ops


# ----------------------------------------------------------------------
# independent per-row loops (python floats are fp64)
# ----------------------------------------------------------------------

def _loop_multiclass(logits, labels, k, eps):
    B, C = logits.shape
    out = {"n": B, "loss": 0.0, "c1": 0, "ck": 0,
           "label": [0] * C, "correct": [0] * C}
    for b in range(B):
        row = [float(v) for v in logits[b]]
        y = int(labels[b])
        if any(math.isnan(v) for v in row):
            out["loss"] = float("nan")
            continue
        m = max(row)
        lse = m + math.log(sum(math.exp(v - m) for v in row))
        out["loss"] += lse - (1.0 - eps) * row[y] - (eps / C) * sum(row)
        rank = sum(1 for c, v in enumerate(row)
                   if v > row[y] or (v == row[y] and c < y))
        out["label"][y] += 1
        if rank == 0:
            out["c1"] += 1
            out["correct"][y] += 1
        if rank < k:
            out["ck"] += 1
    return out


def _loop_binary(logits, labels, T):
    out = {"loss": 0.0, "correct": 0, "hist": [[0] * T, [0] * T]}
    p32 = torch.sigmoid(logits.float())
    for i in range(logits.shape[0]):
        x, y = float(logits[i]), int(labels[i] != 0)
        out["loss"] += max(x, 0.0) - x * y + math.log1p(math.exp(-abs(x)))
        out["correct"] += int((x > 0) == bool(y))
        p = min(max(float(p32[i]), 0.0), 1.0)
        b = min(int(float(torch.tensor(p, dtype=torch.float32) * T)), T - 1)
        out["hist"][0 if y else 1][b] += 1
    return out


def _tie_case(B, C, seed):
    """Tie-heavy integer logits; the first rows put the label on the first
    and on the last of the classes tied for the row maximum."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randint(-2, 3, (B, C), generator=g).float()
    labels = torch.randint(0, C, (B,), generator=g)
    logits[0, 0] = logits[0, C - 1] = 2.0
    logits[1, 0] = logits[1, C - 1] = 2.0
    labels[0], labels[1] = 0, C - 1
    return logits, labels


@pytest.mark.parametrize("B,C,k,eps", [(33, 7, 3, 0.0), (16, 5, 5, 0.1),
                                       (9, 3, 8, 0.0), (1, 2, 1, 0.1)])
@pytest.mark.parametrize("ties", [False, True])
def test_multiclass_reference_matches_row_loop(B, C, k, eps, ties):
    if ties and B >= 2:
        logits, labels = _tie_case(B, C, seed=B)
    else:
        g = torch.Generator().manual_seed(B)
        logits = torch.randn(B, C, generator=g)
        labels = torch.randint(0, C, (B,), generator=g)
    want = _loop_multiclass(logits, labels, k, eps)
    state = metric_ops.new_state(metric_ops.multiclass_state_size(C, True))
    metric_ops.multiclass_update(state, logits, labels, k=k,
                                 label_smoothing=eps, per_class=True)
    assert state[0].item() == B
    assert state[1].item() == pytest.approx(want["loss"], rel=1e-12)
    assert state[2].item() == want["c1"]
    assert state[3].item() == want["ck"]
    assert state[4:4 + C].tolist() == want["label"]
    assert state[4 + C:].tolist() == want["correct"]
    if k >= C:
        assert want["ck"] == B  # every finite row is top-k correct


def test_multiclass_tie_rule_is_first_index_argmax():
    logits, labels = _tie_case(64, 6, seed=3)
    state = metric_ops.new_state(4)
    metric_ops.multiclass_update(state, logits, labels, k=2)
    assert state[2].item() == int((logits.argmax(dim=1) == labels).sum())
    # label on the first tied class is correct, on the last it is not
    one = metric_ops.new_state(4)
    metric_ops.multiclass_update(one, logits[:2], labels[:2], k=1)
    assert one[2].item() == 1


def test_multiclass_nan_row_makes_loss_nan():
    logits = torch.randn(6, 4, generator=torch.Generator().manual_seed(0))
    logits[3, 2] = float("nan")
    labels = torch.tensor([0, 1, 2, 3, 0, 1])
    state = metric_ops.new_state(4)
    metric_ops.multiclass_update(state, logits, labels)
    assert math.isnan(state[1].item())
    assert state[0].item() == 6
    head_state = MultiClassHead(4).streaming_metrics()
    head_state.update(logits, labels)
    assert math.isnan(head_state.result()["average_loss"])


def test_multiclass_rejects_bad_input():
    state = metric_ops.new_state(4)
    with pytest.raises(ValueError):
        metric_ops.multiclass_update(state, torch.zeros(2, 3),
                                     torch.tensor([0, 3]))
    with pytest.raises(ValueError):
        metric_ops.multiclass_update(metric_ops.new_state(5),
                                     torch.zeros(2, 3), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        metric_ops.multiclass_update(state, torch.zeros(2, 3),
                                     torch.tensor([0, 1]), k=0)


@pytest.mark.parametrize("B,T", [(1, 8), (77, 8), (300, 200)])
def test_binary_reference_matches_row_loop(B, T):
    g = torch.Generator().manual_seed(B)
    logits = (torch.randn(B, generator=g) * 3).to(torch.bfloat16)
    logits[0] = 0.0
    labels = torch.randint(0, 2, (B,), generator=g)
    want = _loop_binary(logits, labels, T)
    state = metric_ops.new_state(metric_ops.binary_state_size(T))
    metric_ops.binary_update(state, logits.view(B, 1), labels,
                             num_thresholds=T)
    assert state[0].item() == B
    assert state[1].item() == pytest.approx(want["loss"], rel=1e-12)
    assert state[2].item() == want["correct"]
    assert state[3:].view(2, T).tolist() == want["hist"]
    # x == 0 is "predicted negative": correct iff the label is 0
    zero = metric_ops.new_state(metric_ops.binary_state_size(T))
    metric_ops.binary_update(zero, torch.zeros(2), torch.tensor([0, 1]),
                             num_thresholds=T)
    assert zero[2].item() == 1


def test_regression_reference_matches_loop():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(13, 3, generator=g)
    labels = torch.randn(13, 3, generator=g)
    sq = sum((float(a) - float(b)) ** 2
             for a, b in zip(logits.reshape(-1), labels.reshape(-1)))
    ab = sum(abs(float(a) - float(b))
             for a, b in zip(logits.reshape(-1), labels.reshape(-1)))
    state = metric_ops.new_state(3)
    metric_ops.regression_update(state, logits, labels)
    assert state[0].item() == 39
    assert state[1].item() == pytest.approx(sq, rel=1e-12)
    assert state[2].item() == pytest.approx(ab, rel=1e-12)
    res_state = RegressionHead(3).streaming_metrics()
    res_state.update(logits, labels)
    res = res_state.result()
    assert res["average_loss"] == pytest.approx(sq / 39, rel=1e-12)
    assert res["mean_absolute_error"] == pytest.approx(ab / 39, rel=1e-12)
    assert res["root_mean_squared_error"] == pytest.approx(
        math.sqrt(sq / 39), rel=1e-12)


# ----------------------------------------------------------------------
# split invariance, reset, merge
# ----------------------------------------------------------------------

def _feed(state, logits, labels, sizes):
    off = 0
    for n in sizes:
        state.update(logits[off:off + n], labels[off:off + n])
        off += n
    assert off == logits.shape[0]


def _assert_states_match(a, b, n_float):
    """Slots listed in n_float are sums (1e-12 relative), the rest counts
    (exactly equal)."""
    a, b = a.clone(), b.clone()
    for i in n_float:
        assert a[i].item() == pytest.approx(b[i].item(), rel=1e-12)
        a[i] = b[i] = 0
    assert torch.equal(a, b)


def _head_cases():
    g = torch.Generator().manual_seed(21)
    B = 40
    yield (MultiClassHead(6, label_smoothing=0.1), dict(k=2, per_class=True),
           torch.randn(B, 6, generator=g),
           torch.randint(0, 6, (B,), generator=g), [1])
    yield (BinaryClassHead(), dict(num_thresholds=16),
           torch.randn(B, 1, generator=g) * 3,
           torch.randint(0, 2, (B,), generator=g), [1])
    yield (RegressionHead(2), {}, torch.randn(B, 2, generator=g),
           torch.randn(B, 2, generator=g), [1, 2])


@pytest.mark.parametrize("case", list(_head_cases()),
                         ids=["multiclass", "binary", "regression"])
def test_split_invariance_reset_and_merge(case):
    head, options, logits, labels, float_slots = case
    B = logits.shape[0]
    whole = head.streaming_metrics(**options)
    whole.update(logits, labels)
    ragged = head.streaming_metrics(**options)
    _feed(ragged, logits, labels, [5, 1, B - 6])
    _assert_states_match(ragged.state, whole.state, float_slots)
    for k, v in whole.result().items():
        assert ragged.result()[k] == pytest.approx(v, rel=1e-12)

    first = head.streaming_metrics(**options)
    second = head.streaming_metrics(**options)
    first.update(logits[:B // 2], labels[:B // 2])
    second.update(logits[B // 2:], labels[B // 2:])
    assert first.merge_(second) is first
    _assert_states_match(first.state, whole.state, float_slots)

    whole.reset()
    assert torch.equal(whole.state, torch.zeros_like(whole.state))
    assert all(math.isnan(v) for v in whole.result().values())


def test_mean_per_class_accuracy_skips_unseen_classes():
    head = MultiClassHead(4)
    logits = torch.tensor([[5., 0, 0, 0], [0., 5, 0, 0], [5., 0, 0, 0],
                           [0., 0, 5, 0]])
    labels = torch.tensor([0, 0, 0, 2])       # classes 1 and 3 never labelled
    state = head.streaming_metrics(per_class=True, k=2)
    state.update(logits, labels)
    res = state.result()
    assert res["accuracy"] == 0.75
    assert res["mean_per_class_accuracy"] == pytest.approx((2 / 3 + 1) / 2)
    assert "mean_per_class_accuracy" not in \
        head.streaming_metrics().result()


# ----------------------------------------------------------------------
# heads
# ----------------------------------------------------------------------

class _LossAndMetricsOnlyHead(Head):
    """A custom head that knows nothing of streaming states."""

    @property
    def logits_dimension(self):
        return 2

    def loss(self, logits, labels):
        return ((logits.float().sum(dim=1) - labels.float()) ** 2).mean()

    def predictions(self, logits):
        return {"predictions": logits}

    def metrics(self, logits, labels):
        return {"average_loss": float(self.loss(logits, labels)),
                "batch_size": float(logits.shape[0])}


def test_base_head_fallback_keeps_example_weighted_means():
    head = _LossAndMetricsOnlyHead()
    g = torch.Generator().manual_seed(2)
    logits, labels = torch.randn(11, 2, generator=g), torch.randn(
        11, generator=g)
    state = head.streaming_metrics()
    _feed(state, logits, labels, [8, 3])
    res = state.result()
    assert res["average_loss"] == pytest.approx(
        float(head.loss(logits, labels)), rel=1e-6)
    assert res["batch_size"] == pytest.approx((8 * 8 + 3 * 3) / 11)
    other = head.streaming_metrics()
    other.update(logits[:4], labels[:4])
    state.merge_(other)
    assert state.state["n"] == 15
    state.reset()
    assert state.result() == {}
    with pytest.raises(TypeError):
        head.streaming_metrics(k=3)


def test_multihead_keys_and_summed_average_loss():
    head = MultiHead({"cls": MultiClassHead(3), "reg": RegressionHead(2),
                      "bin": BinaryClassHead()})
    g = torch.Generator().manual_seed(4)
    B = 19
    logits = torch.randn(B, head.logits_dimension, generator=g)
    labels = {"cls": torch.randint(0, 3, (B,), generator=g),
              "reg": torch.randn(B, 2, generator=g),
              "bin": torch.randint(0, 2, (B,), generator=g)}
    state = head.streaming_metrics(cls={"k": 2}, bin={"num_thresholds": 8})
    off = 0
    for n in (7, 12):
        state.update(logits[off:off + n],
                     {k: v[off:off + n] for k, v in labels.items()})
        off += n
    res = state.result()
    assert set(res) == {
        "average_loss",
        "bin/accuracy", "bin/average_loss", "bin/auc", "bin/precision",
        "bin/recall",
        "cls/accuracy", "cls/average_loss", "cls/top_k_accuracy",
        "reg/average_loss", "reg/mean_absolute_error",
        "reg/root_mean_squared_error"}
    assert res["average_loss"] == pytest.approx(
        res["bin/average_loss"] + res["cls/average_loss"]
        + res["reg/average_loss"], rel=1e-12)
    # sub-heads read the same split of the logits as loss() does
    assert res["average_loss"] == pytest.approx(
        float(head.loss(logits, labels)), rel=1e-5)
    assert len(state.state) == 3
    with pytest.raises(TypeError):
        head.streaming_metrics(nope={})


# ----------------------------------------------------------------------
# engine wiring
# ----------------------------------------------------------------------

def _binary_problem(n=512, d=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g)
    w = torch.randn(d, generator=g)
    Y = ((X @ w + 0.5 * torch.randn(n, generator=g)) > 0).long()
    return X, Y


def _batches(X, Y, size):
    return lambda: iter([(X[i:i + size], Y[i:i + size])
                         for i in range(0, X.shape[0], size)])


def _trained_binary_estimator(model_dir, X, Y, **kwargs):
    def train_fn():
        def gen():
            g = torch.Generator().manual_seed(7)
            while True:
                idx = torch.randint(0, X.shape[0], (64,), generator=g)
                yield X[idx], Y[idx]
        return gen()

    est = adanet_amd.Estimator(
        head=BinaryClassHead(),
        subnetwork_generator=simple_dnn.Generator(layer_size=8),
        max_iteration_steps=5, model_dir=model_dir,
        config=adanet_amd.RunConfig(tf_random_seed=42), **kwargs)
    est.train(train_fn, max_steps=5)
    return est


def _whole_set_logits(est, X):
    ensemble, _ = est._load_frozen_best(None)
    with torch.no_grad():
        return ensemble(X)


def test_label_sorted_binary_eval_streaming_vs_default(model_dir):
    X, Y = _binary_problem()
    order = torch.argsort(Y, descending=True, stable=True)  # positives first
    X, Y = X[order], Y[order]
    n_pos = int(Y.sum())
    assert n_pos >= 64 and X.shape[0] - n_pos >= 64  # single-class batches
    est = _trained_binary_estimator(model_dir, X, Y)
    input_fn = _batches(X, Y, 64)

    res = est.evaluate(input_fn, streaming=True)
    logits = _whole_set_logits(est, X)
    whole = AUCAccumulator()
    whole.update(torch.sigmoid(logits.float()).reshape(-1), Y)
    want = whole.value()
    assert math.isfinite(res["auc"])
    for key in ("auc", "precision", "recall"):
        assert res[key] == pytest.approx(want[key], rel=1e-12, abs=1e-12)
    # ... and on exactly the same histogram
    state = est._head.streaming_metrics()
    for f, l in input_fn():
        with torch.no_grad():
            state.update(est._load_frozen_best(None)[0](f), l)
    assert torch.equal(state.state[3:].view(2, 200).long(),
                       whole._hist.long())
    # the batch-mean default cannot give an AUC here
    assert math.isnan(est.evaluate(input_fn)["auc"])


def test_ragged_last_batch_is_example_weighted(model_dir):
    X, Y = _binary_problem(n=200)
    est = _trained_binary_estimator(model_dir, X, Y)
    res = est.evaluate(_batches(X, Y, 64), streaming=True)  # 64,64,64,8
    logits = _whole_set_logits(est, X)
    head = BinaryClassHead()
    assert res["average_loss"] == pytest.approx(
        float(head.loss(logits, Y)), rel=1e-6)
    assert res["loss"] == res["average_loss"]
    acc = float(((logits.reshape(-1) > 0).long() == Y).double().mean())
    assert res["accuracy"] == pytest.approx(acc, rel=1e-12)
    assert res["global_step"] == 5
    assert res["architecture/adanet/ensembles"]
    assert "best_ensemble_index_0" in res
    with pytest.raises(ValueError):
        est.evaluate(_batches(X, Y, 64), streaming_options={"x": 1})


def test_evaluate_default_path_is_unchanged(model_dir,
                                            synthetic_classification):
    X, Y, input_fn = synthetic_classification
    est = adanet_amd.Estimator(
        head=MultiClassHead(4),
        subnetwork_generator=simple_dnn.Generator(layer_size=8),
        max_iteration_steps=5, model_dir=model_dir,
        config=adanet_amd.RunConfig(tf_random_seed=42))
    est.train(input_fn, max_steps=5)
    eval_fn = _batches(X[:200], Y[:200], 64)   # ragged last batch
    got = est.evaluate(eval_fn)

    # the default loop, inlined: equal weight per batch
    ensemble, arch = est._load_frozen_best(None)
    head = est._head
    sums, loss_sum, count = {}, 0.0, 0
    for features, labels in eval_fn():
        with torch.no_grad():
            logits = ensemble(features)
            loss_sum += float(head.loss(logits, labels))
            for k, v in head.metrics(logits, labels).items():
                sums[k] = sums.get(k, 0.0) + float(v)
        count += 1
    want = {k: v / count for k, v in sums.items()}
    want["loss"] = loss_sum / count
    want["global_step"] = 5
    want["architecture/adanet/ensembles"] = arch.serialize(
        est.iteration_number, est.global_step)
    want["best_ensemble_index_0"] = est._replay_indices[0]
    assert got == want
    # streaming adds top-k and weights by example
    streamed = est.evaluate(eval_fn, streaming=True,
                            streaming_options={"k": 2, "per_class": True})
    assert set(streamed) - set(got) == {"top_k_accuracy",
                                        "mean_per_class_accuracy"}
    logits = _whole_set_logits(est, X[:200])
    assert streamed["accuracy"] == pytest.approx(
        float((logits.argmax(dim=1) == Y[:200]).double().mean()), rel=1e-12)
    assert streamed["top_k_accuracy"] >= streamed["accuracy"]


def test_user_metric_fn_keeps_batch_mean(model_dir):
    X, Y = _binary_problem(n=200)

    def metric_fn(predictions, features, labels):
        return {"rows": float(features.shape[0])}

    est = _trained_binary_estimator(model_dir, X, Y, metric_fn=metric_fn)
    res = est.evaluate(_batches(X, Y, 64), streaming=True)
    assert res["rows"] == pytest.approx((64 * 3 + 8) / 4)


def _binary_iteration(tmp_path, X):
    """Two single-subnetwork candidates over a binary head."""
    from adanet_amd.core.architecture import _Architecture
    from adanet_amd.core.iteration import (_EnsembleSpec, _Iteration,
                                           _SubnetworkSpec, _TrainManager)
    from adanet_amd.ensemble.weighted import ComplexityRegularizedEnsembler
    from adanet_amd.ops.optim import FusedSGD
    from adanet_amd.subnetwork import Subnetwork

    class _Module(torch.nn.Module):
        def __init__(self, d):
            super().__init__()
            self.lin = torch.nn.Linear(d, 1)
            self.last_layer_dim = d

        def forward(self, x):
            return x, self.lin(x)

    class _Builder(adanet_amd.subnetwork.Builder):
        def __init__(self, name):
            self._name = name

        @property
        def name(self):
            return self._name

        def build_subnetwork(self, features, logits_dimension, training,
                             previous_ensemble=None):
            return Subnetwork(module=_Module(features.shape[1]),
                              complexity=1.0, name=self._name)

    torch.manual_seed(0)
    ensembler = ComplexityRegularizedEnsembler()
    sub_specs, ens_specs = [], []
    for i in range(2):
        b = _Builder("b%d" % i)
        sub = b.build_subnetwork(X[:8], 1, True)
        sub_specs.append(_SubnetworkSpec(
            name="t0_b%d" % i, builder=b, subnetwork=sub,
            optimizer=FusedSGD(sub.module.parameters(), lr=0.1)))
        ens = ensembler.build_ensemble([sub], None, X[:8], None, 1, True,
                                       None)
        ens_specs.append(_EnsembleSpec(
            name="t0_b%d_grow" % i, candidate=None, ensemble=ens,
            ensembler_name=ensembler.name,
            architecture=_Architecture("b%d" % i, ensembler.name),
            optimizer=None, members=(("new", "b%d" % i),)))
    return _Iteration(
        number=0, head=BinaryClassHead(), subnetwork_specs=sub_specs,
        ensemble_specs=ens_specs, frozen_subnetworks={},
        train_manager=_TrainManager(str(tmp_path), 0), max_iteration_steps=5,
        adanet_loss_decay=0.5, device=torch.device("cpu"), placement=None,
        use_streams=False, use_graphs=False)


def test_evaluator_streaming_selects_on_whole_set_auc(tmp_path):
    X, Y = _binary_problem(n=256, seed=3)
    order = torch.argsort(Y, descending=True, stable=True)
    X, Y = X[order], Y[order]                  # single-class batches
    it = _binary_iteration(tmp_path, X)
    ev = adanet_amd.Evaluator(input_fn=_batches(X, Y, 32),
                              metric_name="auc",
                              objective=Objective.MAXIMIZE,
                              streaming=True)
    assert ev.streaming and not adanet_amd.Evaluator(input_fn=None).streaming
    ident = lambda f, l: (f, l)
    vals = it.evaluate_candidates(iter(ev.input_fn()), ev.steps, ident,
                                  metric_name=ev.metric_name,
                                  streaming=ev.streaming)
    want = []
    for spec in it.ensemble_specs:
        with torch.no_grad():
            _, logits = it.subnetwork_specs[
                it.ensemble_specs.index(spec)].subnetwork(X)
            last = X
            logits = spec.ensemble.logits_from([logits], [last])
        acc = AUCAccumulator()
        acc.update(torch.sigmoid(logits.float()).reshape(-1), Y)
        want.append(acc.value()["auc"])
    assert all(math.isfinite(v) for v in vals)
    assert vals == pytest.approx(want, rel=1e-12)
    assert [s.eval_loss for s in it.ensemble_specs] == vals
    # the batch-mean path has no AUC on single-class batches
    plain = it.evaluate_candidates(iter(ev.input_fn()), ev.steps, ident,
                                   metric_name="auc")
    assert all(math.isnan(v) for v in plain)
    with pytest.raises(ValueError, match="not produced by the head"):
        it.evaluate_candidates(iter(ev.input_fn()), ev.steps, ident,
                               metric_name="no_such_metric", streaming=True)
    # adanet_loss ignores the flag
    a = it.evaluate_candidates(iter(ev.input_fn()), 2, ident)
    b = it.evaluate_candidates(iter(ev.input_fn()), 2, ident, streaming=True)
    assert a == b


def test_estimator_passes_evaluator_streaming_flag(model_dir):
    X, Y = _binary_problem(n=256, seed=1)
    ev = adanet_amd.Evaluator(input_fn=_batches(X, Y, 64),
                              metric_name="auc",
                              objective=Objective.MAXIMIZE,
                              streaming=True)
    est = _trained_binary_estimator(model_dir, X, Y, evaluator=ev)
    assert est.iteration_number == 1
    res = est.train_and_evaluate(lambda: iter([]), _batches(X, Y, 64),
                                 max_steps=5, streaming=True)
    assert math.isfinite(res["auc"])
