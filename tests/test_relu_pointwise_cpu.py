"""relu_conv1x1 off the GPU: the composition, differentiable."""

import torch
import torch.nn.functional as F


def test_cpu_fallback():
    from adanet_amd.ops.conv import relu_conv1x1, relu_conv1x1_supported
    torch.manual_seed(0)
    x = torch.randn(2, 32, 4, 4, dtype=torch.float64)
    w = torch.randn(32, 32, dtype=torch.float64)
    assert not relu_conv1x1_supported(x, w)
    grads = []
    for fn in (relu_conv1x1, lambda x, w: F.conv2d(
            F.relu(x), w.reshape(32, 32, 1, 1))):
        xi, wi = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = fn(xi, wi)
        y.square().sum().backward()
        grads.append((y.detach(), xi.grad, wi.grad))
    assert all(torch.equal(a, b) for a, b in zip(*grads))
