"""Device-resident image pipeline on the GPU (csrc/augment.hip): the two
kernels against the CPU references of ops/augment.py — exact integers for the
draw, torch.equal on the bf16 batch for the apply — the DeviceImageLoader on
cuda:0 against the same loader on the CPU, and one training run fed by it."""

import itertools
import math

import pytest
import torch

import adanet_amd
from adanet_amd.data import DeviceImageLoader
from adanet_amd.head import MultiClassHead
from adanet_amd.hooks import TrainHook
from adanet_amd.models import improve_nas
from adanet_amd.models.cifar import FakeImageProvider
from adanet_amd.ops import augment as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def explicit_params(n, h, w, pad):
    """Every combination of oy, ox in {0, pad, 2*pad}, both flips and cutout
    centres (0, 0), (h-1, w-1) and the middle; indices cycle through the
    dataset with the last one first and one repeated."""
    centres = [(0, 0), (h - 1, w - 1), (h // 2, w // 2)]
    rows = []
    for k, (oy, ox, flip, (cy, cx)) in enumerate(itertools.product(
            (0, pad, 2 * pad), (0, pad, 2 * pad), (0, 1), centres)):
        index = n - 1 if k % 5 in (0, 1) else k % n
        rows.append([index, oy, ox, flip, cy, cx])
    return torch.tensor(rows, dtype=torch.int32)


def _batches(params, b):
    """The grid in batches of exactly ``b`` rows (the last one wraps)."""
    n = params.shape[0]
    for lo in range(0, n, b):
        yield params[torch.arange(lo, lo + b) % n]


def _data(kind, n, c, h, w):
    g = torch.Generator().manual_seed(n * 1000 + h)
    if kind == "uint8":
        return torch.randint(0, 256, (n, c, h, w), generator=g,
                             dtype=torch.uint8)
    return torch.randn(n, c, h, w, generator=g) * 3 + 0.25


def _affine(c):
    scale = torch.tensor([2.0 / 255.0, 0.37, 1.5][:c])
    shift = torch.tensor([-1.0, 0.11, -0.4][:c])
    return scale, shift


# (source dtype, N, C, H, W, B, pad): the 8-wide vector variant, the scalar
# one (W % 8 != 0), and the float source.
CASES = [
    ("uint8", 5, 3, 32, 32, 7, 4),
    ("uint8", 3, 1, 10, 12, 4, 2),
    ("float32", 4, 3, 16, 16, 5, 4),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%dx%dx%d" % c[:5])
def test_apply_matches_cpu_reference(case):
    kind, n, c, h, w, b, pad = case
    data = _data(kind, n, c, h, w)
    scale, shift = _affine(c)
    d_data, d_scale, d_shift = (t.to(DEV) for t in (data, scale, shift))
    grid = explicit_params(n, h, w, pad)
    for cutout_pad in (0, 8, h):
        for params in _batches(grid, b):
            want = A.augment_apply(data, params, scale, shift, pad,
                                   cutout_pad)
            got = A.augment_apply(d_data, params.to(DEV), d_scale, d_shift,
                                  pad, cutout_pad)
            assert got.dtype == torch.bfloat16 and got.shape == (b, c, h, w)
            assert got.data_ptr() % 16 == 0
            assert torch.equal(got.cpu(), want), (cutout_pad, params)
        if cutout_pad >= max(h, w):  # the hole covers any image
            assert bool((got == 0).all())


def test_apply_misaligned_out_takes_scalar_variant():
    """W % 8 == 0 but ``out`` starts 2 bytes off a 16-byte boundary."""
    kind, n, c, h, w, b, pad = CASES[0]
    data = _data(kind, n, c, h, w)
    scale, shift = _affine(c)
    params = next(_batches(explicit_params(n, h, w, pad)[11:], b))
    want = A.augment_apply(data, params, scale, shift, pad, 8)
    numel = b * c * h * w
    buf = torch.full((numel + 16,), 7.0, device=DEV, dtype=torch.bfloat16)
    out = buf[1:1 + numel].view(b, c, h, w)
    assert out.is_contiguous() and out.data_ptr() % 16 == 2
    res = A.augment_apply(data.to(DEV), params.to(DEV), scale.to(DEV),
                          shift.to(DEV), pad, 8, out=out)
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), want)
    # nothing written on either side of the slice
    assert float(buf[0]) == 7.0 and bool((buf[1 + numel:] == 7.0).all())


@pytest.mark.parametrize("case", CASES[:2], ids=["vector", "scalar"])
def test_apply_clamps_out_of_range_indices(case):
    kind, n, c, h, w, b, pad = case
    data = _data(kind, n, c, h, w).to(DEV)
    scale, shift = (t.to(DEV) for t in _affine(c))
    row = [0, 1, 2 * pad, 1, h // 2, w // 2]
    params = torch.tensor([[-1] + row[1:], [n] + row[1:], row,
                           [n - 1] + row[1:], [2 ** 31 - 1] + row[1:],
                           [-2 ** 31] + row[1:]], dtype=torch.int32)
    got = A.augment_apply(data, params.to(DEV), scale, shift, pad, 2)
    want = A.augment_apply(data.cpu(), params, scale.cpu(), shift.cpu(), pad,
                           2)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got[0], got[2]) and torch.equal(got[1], got[3])
    assert torch.equal(got[4], got[3]) and torch.equal(got[5], got[2])
    assert not torch.equal(got[0], got[1])


def test_apply_rejects_what_it_cannot_index():
    data = _data("uint8", 2, 3, 8, 8).to(DEV)
    scale, shift = (t.to(DEV) for t in _affine(3))
    params = torch.zeros(2, 6, dtype=torch.int32, device=DEV)
    ext = A._extension.require()
    out = torch.empty(2, 3, 8, 8, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):  # fp16 source
        ext.augment_apply(data.half(), params, scale, shift, out, 1, 1)
    with pytest.raises(RuntimeError):  # strided source
        ext.augment_apply(data.transpose(2, 3), params, scale, shift, out, 1,
                          1)
    with pytest.raises(RuntimeError):  # params [B, 5]
        ext.augment_apply(data, params[:, :5].contiguous(), scale, shift,
                          out, 1, 1)
    with pytest.raises(RuntimeError):  # negative pad
        ext.augment_apply(data, params, scale, shift, out, -1, 1)
    with pytest.raises(RuntimeError):  # scale of the wrong length
        ext.augment_apply(data, params, scale[:2].contiguous(), shift, out,
                          1, 1)


_LABELS = (torch.arange(50000) * 7919) % 10


@pytest.mark.parametrize("b,n", [(300, 50000), (1, 1)])
@pytest.mark.parametrize("step,rank,world", [(0, 0, 1), (2 ** 33, 0, 1),
                                             (3, 1, 2)])
def test_draw_matches_cpu_reference(b, n, step, rank, world):
    labels = _LABELS[:n].contiguous()
    want = A.draw_params(77, step, b, n, 32, 32, 4, labels, rank=rank,
                         world=world)
    got = A.draw_params(77, step, b, n, 32, 32, 4, labels.to(DEV), rank=rank,
                        world=world, device=DEV)
    assert got[0].dtype == torch.int32 and got[0].shape == (b, 6)
    assert got[1].dtype == torch.int64 and got[1].shape == (b,)
    assert torch.equal(got[0].cpu(), want[0])
    assert torch.equal(got[1].cpu(), want[1])


def test_draw_without_augmentation_and_large_seed():
    labels = _LABELS[:1000].contiguous()
    args = (2 ** 64 - 3, 5, 70, 1000, 24, 40, 3)
    want = A.draw_params(*args, labels, augment=False)
    got = A.draw_params(*args, labels.to(DEV), augment=False)
    assert torch.equal(got[0].cpu(), want[0])
    assert torch.equal(got[1].cpu(), want[1])
    assert bool((got[0][:, 1:3] == 3).all()) and bool((got[0][:, 3] == 0).all())


def _loaders(**kw):
    g = torch.Generator().manual_seed(21)
    data = torch.randint(0, 256, (40, 3, 32, 32), generator=g,
                         dtype=torch.uint8)
    labels = torch.arange(40) % 10
    args = dict(batch_size=8, seed=5)
    args.update(kw)
    return (DeviceImageLoader(data, labels, device="cpu", **args),
            DeviceImageLoader(data, labels, device=DEV, **args))


@pytest.mark.parametrize("kw", [{}, {"augment": False, "normalize": "none"},
                                {"start_step": 4, "shard": (1, 2)}],
                         ids=["default", "plain", "resumed-shard"])
def test_loader_on_gpu_equals_loader_on_cpu(kw):
    cpu, gpu = _loaders(**kw)
    assert gpu.images.is_cuda and gpu.images.dtype == torch.uint8
    for (xc, yc), (xg, yg) in zip(itertools.islice(cpu(), 3),
                                  itertools.islice(gpu(), 3)):
        assert xg.is_cuda and xg.dtype == torch.bfloat16
        assert yg.is_cuda and yg.dtype == torch.int64
        assert not hasattr(xg, "adanet_cache_key")
        assert torch.equal(xg.cpu(), xc) and torch.equal(yg.cpu(), yc)


def test_loader_evaluation_on_gpu():
    g = torch.Generator().manual_seed(22)
    data = torch.randn(10, 3, 8, 8, generator=g)
    labels = torch.arange(10) % 3
    loader = DeviceImageLoader(data, labels, 4, DEV, training=False)
    batches = list(loader())
    assert [x.shape[0] for x, _ in batches] == [4, 4, 2]
    assert torch.equal(torch.cat([x for x, _ in batches]).cpu(),
                       data.to(torch.bfloat16))
    assert torch.equal(torch.cat([y for _, y in batches]).cpu(), labels)
    assert [x.adanet_cache_key for x, _ in batches] == [
        ("image-eval", id(loader), i) for i in range(3)]


class _LastLoss(TrainHook):

    def begin(self, estimator=None, iteration=None):
        self.iteration = iteration

    def end(self, estimator=None):
        self.losses = [s.last_loss for s in self.iteration.subnetwork_specs]


def _train_once(model_dir):
    hp = improve_nas.Hparams(num_cells=3, num_conv_filters=8, train_steps=8,
                             drop_path_keep=1.0)
    provider = FakeImageProvider(n_examples=64, batch_size=16, seed=3)
    input_fn = provider.get_device_input_fn(DEV)
    est = adanet_amd.Estimator(
        head=MultiClassHead(10, label_smoothing=hp.label_smoothing),
        subnetwork_generator=improve_nas.DynamicGenerator(hp, seed=0),
        max_iteration_steps=8,
        force_grow=True,
        model_dir=model_dir,
        config=adanet_amd.RunConfig(tf_random_seed=1),
    )
    hook = _LastLoss()
    est.train(input_fn, max_steps=8, hooks=[hook])
    return est, hook.losses


def test_training_run_fed_by_the_device_pipeline(tmp_path, monkeypatch):
    # Streams off as in the NAS benchmark: with candidate streams the NASNet
    # space is not run-to-run deterministic (TODO_ROUND3.md #12).
    monkeypatch.setenv("ADANET_NO_STREAMS", "1")
    # 8 and 18 filters are no multiple of 32, so the pointwise convs take
    # the library-conv fallback (ops/conv.py), whose default algorithms are
    # not run-to-run deterministic: the 3x18 candidate's loss moves in the
    # fourth digit between two runs fed by the unchanged host input_fn too.
    # Ask the library for its deterministic algorithms, as a user who wants
    # a reproducible run at these channel counts has to.
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    est, losses = _train_once(str(tmp_path / "a"))
    assert est.iteration_number == 1 and est.global_step == 8
    assert losses and all(math.isfinite(v) for v in losses)
    _, again = _train_once(str(tmp_path / "b"))
    assert again == losses  # bit for bit: float equality on the fp32 losses
