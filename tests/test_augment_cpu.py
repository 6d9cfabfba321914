"""Device-resident image pipeline, CPU side: the counter RNG, the pure-torch
references of ops/augment.py (which the GPU tests use as their oracle), the
DeviceImageLoader on ``device="cpu"`` and the providers' device input_fn."""

import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adanet_amd.data import DeviceImageLoader
from adanet_amd.models import cifar
from adanet_amd.ops import augment as A

PAD = 4


def test_hash_rng_known_answers():
    assert A.hash_rng(0, 0) == 3793791032
    assert A.hash_rng(1234, 5) == 2965353119
    assert A.hash_rng(7, 2 ** 33 + 3) == 3119215489


# --------------------------------------------------------------- draw_params

B, N, H, W = 300, 50000, 32, 32
_LABELS = (torch.arange(N) * 7919) % 10


def _draw(step, rank=0, world=1, seed=11, n=N, b=B):
    labels = _LABELS[:n].contiguous()
    return A.draw_params(seed, step, b, n, H, W, PAD, labels, rank=rank,
                         world=world, device="cpu")


@pytest.fixture(scope="module")
def step0():
    return _draw(0)


def test_draw_fields_in_range_and_labels_gathered(step0):
    params, y = step0
    assert params.shape == (B, 6) and params.dtype == torch.int32
    assert y.shape == (B,) and y.dtype == torch.int64
    lo = params.min(dim=0).values
    hi = params.max(dim=0).values
    assert bool((lo >= 0).all())
    for col, bound in enumerate([N, 2 * PAD + 1, 2 * PAD + 1, 2, H, W]):
        assert int(hi[col]) < bound
    # 300 draws of each field: both ends of the small ranges turn up
    assert int(hi[1]) == 2 * PAD and int(lo[1]) == 0
    assert set(params[:, 3].tolist()) == {0, 1}
    assert torch.equal(y, _LABELS[params[:, 0].long()])


def test_draw_is_a_pure_function(step0):
    again = _draw(0)
    assert torch.equal(step0[0], again[0]) and torch.equal(step0[1], again[1])


def test_draw_differs_between_steps(step0):
    assert not torch.equal(step0[0], _draw(1)[0])


@pytest.mark.parametrize("s", [0, 3])
def test_draw_shards_interleave_the_single_stream(s):
    for rank in (0, 1):
        sharded = _draw(s, rank=rank, world=2)
        single = _draw(2 * s + rank)
        assert torch.equal(sharded[0], single[0])
        assert torch.equal(sharded[1], single[1])


def test_draw_counter_is_64_bit(step0):
    far = _draw(2 ** 33)
    assert not torch.equal(far[0], step0[0])
    # a counter truncated to 32 bits would make 2^33 * B collide with step 0
    assert int(far[0][:, 0].max()) < N and int(far[0].min()) >= 0


def test_draw_single_example():
    params, y = _draw(5, n=1, b=17)
    assert bool((params[:, 0] == 0).all())
    assert torch.equal(y, _LABELS[:1].expand(17))


def test_draw_without_augmentation_centres_and_never_flips():
    labels = _LABELS
    on = A.draw_params(3, 2, 40, N, H, W, PAD, labels)
    off = A.draw_params(3, 2, 40, N, H, W, PAD, labels, augment=False)
    assert torch.equal(on[0][:, 0], off[0][:, 0])  # same indices
    assert bool((off[0][:, 1:3] == PAD).all())
    assert bool((off[0][:, 3] == 0).all())


# ------------------------------------------------------------- augment_apply

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


def compose(data, params, scale, shift, pad, cutout_pad):
    """The pipeline spelled out per sample with F.pad + slicing, torch.flip
    and slice assignment: crop, flip, cutout, as models/cifar.py orders
    them, on the normalised fp32 image."""
    n, c, h, w = data.shape
    out = []
    for index, oy, ox, flip, cy, cx in params.tolist():
        img = data[index].float() * scale.view(c, 1, 1)
        img = img + shift.view(c, 1, 1)
        img = F.pad(img, (pad, pad, pad, pad))[:, oy:oy + h, ox:ox + w]
        if flip:
            img = torch.flip(img, dims=[2])
        img = img.clone()
        if cutout_pad > 0:
            img[:, max(0, cy - cutout_pad):min(h, cy + cutout_pad),
                max(0, cx - cutout_pad):min(w, cx + cutout_pad)] = 0
        out.append(img)
    return torch.stack(out).to(torch.bfloat16)


def _bytes(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.uint8)


_UNIT = (torch.full((3,), 2.0 / 255.0), torch.full((3,), -1.0))


@pytest.mark.parametrize("cutout_pad", [0, 8, 32])
def test_apply_matches_composition_uint8(cutout_pad):
    data = _bytes(5, 3, 32, 32, 1)
    params = explicit_params(5, 32, 32, PAD)
    assert params.shape[0] == 54
    got = A.augment_apply(data, params, *_UNIT, PAD, cutout_pad)
    assert got.dtype == torch.bfloat16 and got.shape == (54, 3, 32, 32)
    assert torch.equal(got, compose(data, params, *_UNIT, PAD, cutout_pad))
    if cutout_pad == 32:  # a hole of +-H around any centre blanks the image
        assert bool((got == 0).all())


@pytest.mark.parametrize("cutout_pad", [0, 3])
def test_apply_matches_composition_float_odd_shape(cutout_pad):
    g = torch.Generator().manual_seed(2)
    data = torch.randn(3, 2, 10, 12, generator=g)
    scale = torch.tensor([0.5, 1.75])
    shift = torch.tensor([0.125, -3.0])
    params = explicit_params(3, 10, 12, 2)
    got = A.augment_apply(data, params, scale, shift, 2, cutout_pad)
    assert torch.equal(got, compose(data, params, scale, shift, 2,
                                    cutout_pad))


def test_apply_clamps_the_index():
    data = _bytes(4, 3, 8, 8, 3)
    params = torch.tensor([[-1, 1, 2, 1, 3, 3], [4, 1, 2, 1, 3, 3],
                           [0, 1, 2, 1, 3, 3], [3, 1, 2, 1, 3, 3]],
                          dtype=torch.int32)
    got = A.augment_apply(data, params, *_UNIT, 2, 2)
    assert torch.equal(got[0], got[2]) and torch.equal(got[1], got[3])
    assert not torch.equal(got[0], got[1])


def test_apply_equals_the_host_functions():
    """Scale 1/255, shift 0 on bytes is today's host path: x / 255, then
    random_crop, random_flip, cutout of models/cifar.py, then the bf16 cast.
    The parameters are recovered by replaying the host generator. (x * fl(1 /
    255) and x / 255 differ in the last fp32 bit for 126 of the 256 byte
    values and in no bf16 bit for any of them.)"""
    data = _bytes(6, 3, 32, 32, 4)
    b = 24
    index = torch.arange(b) % 6
    g = torch.Generator().manual_seed(9)
    oy = torch.randint(0, 2 * PAD + 1, (b,), generator=g)
    ox = torch.randint(0, 2 * PAD + 1, (b,), generator=g)
    flip = torch.rand(b, generator=g) < 0.5
    cy = torch.randint(0, 32, (b,), generator=g)
    cx = torch.randint(0, 32, (b,), generator=g)
    params = torch.stack([index, oy, ox, flip.long(), cy, cx],
                         dim=1).to(torch.int32)

    g = torch.Generator().manual_seed(9)
    host = data[index].float() / 255.0
    host = cifar.random_crop(host, PAD, generator=g)
    host = cifar.random_flip(host, generator=g)
    host = cifar.cutout(host, 8, generator=g)

    got = A.augment_apply(data, params, torch.full((3,), 1.0 / 255.0),
                          torch.zeros(3), PAD, 8)
    assert torch.equal(got, host.to(torch.bfloat16))


def test_apply_unit_range_and_exact_zero_padding():
    data = _bytes(5, 3, 32, 32, 5)
    # 2/255 * x - 1 is never 0 for an integer x (its root is 127.5; 127 and
    # 128 give -+0.0039), so every exact 0 is a padded or a cut pixel.
    params = explicit_params(5, 32, 32, PAD)
    got = A.augment_apply(data, params, *_UNIT, PAD, 8).float()
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    want_zero = compose(torch.full_like(data, 255), params, *_UNIT, PAD,
                        8) == 0
    assert bool(want_zero.any()) and not bool(want_zero.all())
    assert torch.equal(got == 0, want_zero)


# --------------------------------------------------------- DeviceImageLoader

def _take(loader, k):
    return list(itertools.islice(loader(), k))


def _loader(**kw):
    data = _bytes(40, 3, 32, 32, 6)
    labels = torch.arange(40) % 10
    args = dict(batch_size=8, device="cpu", seed=5)
    args.update(kw)
    return DeviceImageLoader(data, labels, **args)


def test_loader_training_batches():
    loader = _loader()
    assert loader.images.dtype == torch.uint8
    batches = _take(loader, 3)
    for x, y in batches:
        assert x.shape == (8, 3, 32, 32) and x.dtype == torch.bfloat16
        assert y.shape == (8,) and y.dtype == torch.int64
        assert not hasattr(x, "adanet_cache_key")
        assert float(x.float().abs().max()) <= 1.0
    assert not torch.equal(batches[0][0], batches[1][0])
    # equal loaders agree bit for bit; so does a second iterator of one
    for other in (_take(_loader(), 3), _take(loader, 3)):
        for (x0, y0), (x1, y1) in zip(batches, other):
            assert torch.equal(x0, x1) and torch.equal(y0, y1)
    assert not torch.equal(_take(_loader(seed=6), 1)[0][0], batches[0][0])


def test_loader_start_step_resumes_the_stream():
    batches = _take(_loader(), 3)
    x, y = _take(_loader(start_step=2), 1)[0]
    assert torch.equal(x, batches[2][0]) and torch.equal(y, batches[2][1])


def test_loader_shards_draw_different_batches():
    a = _take(_loader(shard=(0, 2)), 1)[0]
    b = _take(_loader(shard=(1, 2)), 1)[0]
    single = _take(_loader(), 2)
    assert torch.equal(a[0], single[0][0]) and torch.equal(b[0], single[1][0])


def test_loader_without_augmentation_yields_the_images():
    loader = _loader(augment=False, normalize="none")
    x, y = _take(loader, 1)[0]
    params, _ = A.draw_params(5, 0, 8, 40, 32, 32, PAD, loader.labels)
    index = params[:, 0].long()
    assert torch.equal(x, (loader.images[index].float() * torch.tensor(
        1.0 / 255.0)).to(torch.bfloat16))
    assert torch.equal(y, loader.labels[index])


def test_loader_evaluation_visits_everything_once_in_order():
    g = torch.Generator().manual_seed(7)
    data = torch.randn(10, 3, 8, 8, generator=g)
    labels = torch.arange(10) % 3
    loader = DeviceImageLoader(data, labels, 4, "cpu", training=False)
    batches = list(loader())
    assert [x.shape[0] for x, _ in batches] == [4, 4, 2]
    assert len(loader) == 3
    # float data under "unit" is passed through: the bf16 cast alone
    assert torch.equal(torch.cat([x for x, _ in batches]),
                       data.to(torch.bfloat16))
    assert torch.equal(torch.cat([y for _, y in batches]), labels)
    keys = [x.adanet_cache_key for x, _ in batches]
    assert keys == [("image-eval", id(loader), i) for i in range(3)]


def test_loader_normalize_mean_std():
    data = _bytes(4, 3, 8, 8, 8)
    mean, std = (0.5, 0.25, 0.125), (0.5, 2.0, 0.25)
    loader = DeviceImageLoader(data, torch.zeros(4, dtype=torch.long), 4,
                               "cpu", training=False, normalize=(mean, std))
    x, _ = next(loader())
    m = torch.tensor(mean).view(1, 3, 1, 1)
    s = torch.tensor(std).view(1, 3, 1, 1)
    want = (data.float() / 255.0 - m) / s
    # one bf16 ulp: the loader folds (x/255 - m)/s into a single x*a + b
    assert float((x.float() - want).abs().max()) <= 2.0 ** -8 * float(
        want.abs().max())
    with pytest.raises(ValueError):
        DeviceImageLoader(data, torch.zeros(4, dtype=torch.long), 4, "cpu",
                          normalize="whiten")


# ----------------------------------------------------------------- providers

def test_cifar10_provider_device_input_fn_keeps_bytes(tmp_path):
    rng = np.random.RandomState(0)
    records = rng.randint(0, 256, size=(3, 3073)).astype(np.uint8)
    records[:, 0] = [3, 9, 0]
    for name in ["data_batch_%d.bin" % i for i in range(1, 6)]:
        records.tofile(str(tmp_path / name))
    provider = cifar.Cifar10Provider(data_dir=str(tmp_path), batch_size=4,
                                     seed=2)
    loader = provider.get_device_input_fn("cpu")
    assert isinstance(loader, DeviceImageLoader)
    assert loader.images.dtype == torch.uint8
    assert loader.images.shape == (15, 3, 32, 32)
    assert torch.equal(loader.images[:3], torch.from_numpy(
        records[:, 1:].reshape(3, 3, 32, 32)))
    assert loader.labels.tolist() == [3, 9, 0] * 5
    x, y = next(loader())
    assert x.shape == (4, 3, 32, 32) and x.dtype == torch.bfloat16
    assert y.dtype == torch.int64 and set(y.tolist()) <= {3, 9, 0}
    assert float(x.float().min()) >= -1.0 and float(x.float().max()) <= 1.0
    # the host path still sees the same data as floats in [0, 1]
    hx, hy = provider._data(True)
    assert hx.dtype == torch.float32
    assert torch.equal(hx, loader.images.float() / 255.0)
    assert torch.equal(hy, loader.labels)


def test_cifar10_provider_uint8_npz_stays_uint8(tmp_path):
    rng = np.random.RandomState(1)
    x = rng.randint(0, 256, size=(6, 32, 32, 3)).astype(np.uint8)  # NHWC
    y = np.arange(6).reshape(6, 1)
    np.savez(str(tmp_path / "cifar10.npz"), x_train=x, y_train=y, x_test=x,
             y_test=y)
    provider = cifar.Cifar10Provider(data_dir=str(tmp_path), batch_size=4)
    loader = provider.get_device_input_fn("cpu", partition="test",
                                          training=False)
    assert loader.images.dtype == torch.uint8
    assert torch.equal(loader.images, torch.from_numpy(x).permute(0, 3, 1, 2))
    hx, _ = provider._data(False)
    assert torch.equal(hx, loader.images.float() / 255.0)
    assert [b[0].shape[0] for b in loader()] == [4, 2]


def test_fake_provider_passes_floats_through():
    provider = cifar.FakeImageProvider(n_examples=16, batch_size=4, seed=3)
    loader = provider.get_device_input_fn("cpu")
    assert loader.images.dtype == torch.float32
    assert torch.equal(loader.images, provider._X)
    x, y = next(loader())
    assert x.shape == (4, 3, 32, 32) and x.dtype == torch.bfloat16
