"""relu_depthwise_conv2d off the GPU: the composition, differentiable."""

import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("C,H,W,KS,stride", [(3, 7, 10, 3, 2), (2, 8, 8, 5, 1)])
def test_cpu_fallback(C, H, W, KS, stride):
    from adanet_amd.ops.conv import (relu_depthwise_conv2d,
                                     relu_depthwise_supported)
    torch.manual_seed(C + H + KS)
    x = torch.randn(2, C, H, W, dtype=torch.float64)
    w = torch.randn(C, 1, KS, KS, dtype=torch.float64)
    assert not relu_depthwise_supported(x, w, stride, KS // 2)
    grads = []
    for fn in (relu_depthwise_conv2d, lambda x, w, s, p: F.conv2d(
            F.relu(x), w, None, s, p, groups=C)):
        xi, wi = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = fn(xi, wi, stride, KS // 2)
        y.square().sum().backward()
        grads.append((y.detach(), xi.grad, wi.grad))
    assert all(torch.equal(a, b) for a, b in zip(*grads))
