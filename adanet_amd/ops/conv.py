"""Native pointwise (1x1) convolution on the batched transposed-staging GEMM.

K9: the NASNet space's FLOPs are dominated by the 1x1 pointwise convs inside
separable convs and the ReLU-Conv-BN adaptors (reference
research/improve_nas/trainer/nasnet_utils.py:182 _stacked_separable_conv,
nasnet.py ReluConvBN usage). On MI355X a pointwise conv IS a batched GEMM:

    y_b[Co, HW] = W[Co, Ci] @ x_b[Ci, HW]          (forward: trans_b staging)
    dX_b        = W^T @ dz_b                       (tt staging)
    dW          = sum_b dz_b @ x_b^T               (split-K over k = b*HW + hw)

so csrc/gemm_tn.hip's gemm_tr_batched (grid.z = image) runs it on MFMA with
zero im2col and zero transpose copies for fwd/dX, and csrc/gemm.hip's
conv1x1_dw reads dz and x for dW where they lie in [B, C, HW] (needs
HW % 8 == 0 and B*HW % 32 == 0; other shapes, and ADANET_CONV_DW_DIRECT=0,
make two channel-major permute copies and call gemm_nt_bf16 — bit-identical
where that GEMM splits K). gemm_tr_batched needs Ci % 32 == 0 and
Co % 32 == 0. Every other channel count (the search space's own 10, 20, 30,
42, ... filters) runs csrc/conv1x1_ragged.hip for forward and dX: the same
accumulation order with the K tail zeroed in LDS and ragged output rows
masked, no padded copies, bit-identical to the aligned path on zero-padded
operands; its dW is conv1x1_dw, whose kernel masks both output axes. So the
pointwise convs are native and run-to-run bit-identical at any channel
count. What remains for torch's conv (MIOpen): HW % 8 != 0, non-bf16 or CPU
tensors, ADANET_NATIVE_CONV=0, and ragged counts under ADANET_CONV_RAGGED=0.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from adanet_amd.ops import _extension


def _native_enabled() -> bool:
    import os
    return os.environ.get("ADANET_NATIVE_CONV", "1") != "0"


def _ragged_enabled() -> bool:
    import os
    return os.environ.get("ADANET_CONV_RAGGED", "1") != "0"


def _on_grid(co: int, ci: int) -> bool:
    """Both channel counts on the 32 grid: gemm_tr_batched's contract."""
    return ci % 32 == 0 and co % 32 == 0


def _ragged_ok(batch: int, hw: int, co: int, ci: int) -> bool:
    """The host-side class of csrc/conv1x1_ragged.hip for activations
    [batch, C, hw] and a [co, ci] weight (pointer alignment apart), with
    ADANET_CONV_RAGGED not 0. The one place that mirrors the file's limits."""
    return _ragged_enabled() and hw > 0 and hw % 8 == 0 \
        and 1 <= batch <= 65535 and 1 <= min(co, ci) \
        and max(co, ci) <= 65536


def _conv1x1_native(x: torch.Tensor, co: int, ci: int) -> bool:
    """Whether `_Conv1x1Fn` takes x [B, Ci, H, W] with a [Co, Ci] weight:
    on the 32 grid through gemm_tr_batched, off it through
    csrc/conv1x1_ragged.hip (ADANET_CONV_RAGGED=0 turns that off)."""
    if not x.is_cuda or x.dtype != torch.bfloat16 or not _native_enabled():
        return False
    hw = x.shape[2] * x.shape[3]
    if hw % 8 != 0 or not x.is_contiguous():
        return False
    if _on_grid(co, ci):
        return True
    return _ragged_ok(x.shape[0], hw, co, ci) and x.data_ptr() % 16 == 0


def _dw_direct_enabled() -> bool:
    import os
    return os.environ.get("ADANET_CONV_DW_DIRECT", "1") != "0"


def _weight_grad(dy3: torch.Tensor, x3: torch.Tensor) -> torch.Tensor:
    """dW[Co, Ci] = sum_b dy3[b] @ x3[b]^T for contiguous bf16 [B, C, HW]."""
    ext = _extension.require()
    B, Co, HW = dy3.shape
    Ci = x3.shape[1]
    dw = torch.empty((Co, Ci), device=dy3.device, dtype=torch.bfloat16)
    if _dw_direct_enabled() and HW % 8 == 0 and (B * HW) % 32 == 0:
        ext.conv1x1_dw(dy3, x3, dw)
    else:
        # Copy path: channel-major [C, B*HW] operands, one permute copy each.
        dz_flat = dy3.permute(1, 0, 2).reshape(Co, B * HW).contiguous()
        x_flat = x3.permute(1, 0, 2).reshape(Ci, B * HW).contiguous()
        ext.gemm_nt_bf16(dz_flat, x_flat, dw, None, 0)
    return dw


def conv1x1_weight_grad(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Weight gradient of a 1x1 conv: dy [B, Co, H, W], x [B, Ci, H, W]
    -> dW [Co, Ci] = sum over b, h, w of dy[b, :, h, w] x[b, :, h, w]^T.

    bf16 GPU tensors run on the MFMA kernels; CPU tensors use an einsum.
    """
    if dy.dim() != 4 or x.dim() != 4 or dy.shape[0] != x.shape[0] \
            or dy.shape[2:] != x.shape[2:]:
        raise ValueError("conv1x1_weight_grad: dy [B,Co,H,W] and x "
                         "[B,Ci,H,W] must agree on B, H, W")
    if not dy.is_cuda:
        return torch.einsum("bohw,bihw->oi", dy, x)
    if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16:
        raise TypeError("conv1x1_weight_grad: GPU tensors must be bf16")
    B, Co, H, W = dy.shape
    return _weight_grad(dy.contiguous().reshape(B, Co, H * W),
                        x.contiguous().reshape(B, x.shape[1], H * W))


class _Conv1x1Fn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias):
        # x [B, Ci, H, W] contiguous; weight [Co, Ci] bf16; bias fp32 [Co].
        ext = _extension.require()
        B, Ci, H, W = x.shape
        Co = weight.shape[0]
        x3 = x.reshape(B, Ci, H * W)
        y = torch.empty((B, Co, H * W), device=x.device, dtype=torch.bfloat16)
        # bias is per-OUTPUT-CHANNEL = per GEMM ROW; the GEMM epilogue's bias
        # is per-column, so add the bias afterwards (broadcast add).
        if _on_grid(Co, Ci):
            ext.gemm_tr_batched(weight, x3, y, None, 0, 0, 1)
        else:
            ext.conv1x1_ragged_fwd(x3, weight, y)
        if bias is not None:
            y = y + bias.to(torch.bfloat16).reshape(1, Co, 1)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y.reshape(B, Co, H, W)

    @staticmethod
    def backward(ctx, dy):
        ext = _extension.require()
        x, weight = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co = weight.shape[0]
        dy3 = dy.contiguous().reshape(B, Co, H * W)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((B, Ci, H * W), device=x.device,
                             dtype=torch.bfloat16)
            # dX_b = W^T @ dz_b: both operands K(=Co)-major -> tt staging.
            if _on_grid(Co, Ci):
                ext.gemm_tr_batched(weight, dy3, dx, None, 0, 1, 1)
            else:
                if dy3.data_ptr() % 16:
                    dy3 = dy3.clone()
                ext.conv1x1_ragged_dx(dy3, weight, dx)
            dx = dx.reshape(B, Ci, H, W)
        if ctx.needs_input_grad[1]:
            # dW[Co, Ci] = dz_all[Co, B*HW] @ x_all[Ci, B*HW]^T, read from
            # the [B, C, HW] layout directly when the shape allows it.
            dw = _weight_grad(dy3, x.reshape(B, Ci, H * W))
        if ctx.has_bias:
            db = dy3.sum(dim=(0, 2)).float()
        return dx, dw, db


class HipConv1x1(nn.Module):
    """1x1 Conv2d on the batched MFMA GEMM with torch (MIOpen) fallback.

    Drop-in for ``nn.Conv2d(c_in, c_out, 1, bias=...)`` (stride 1). The
    weight keeps Conv2d's [Co, Ci, 1, 1] layout so state dicts interop.
    Any channel counts are native for contiguous bf16 GPU input with
    H*W % 8 == 0: multiples of 32 on gemm_tr_batched, the others on
    csrc/conv1x1_ragged.hip (ADANET_CONV_RAGGED=0 sends those to torch).
    """

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True,
                 device=None, dtype=None):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        ref = nn.Conv2d(in_channels, out_channels, 1, bias=bias)
        self.weight = nn.Parameter(ref.weight.detach().to(device=device,
                                                          dtype=dtype))
        if bias:
            self.bias = nn.Parameter(ref.bias.detach().float().to(device))
        else:
            self.register_parameter("bias", None)

    def forward(self, x):
        w2 = self.weight.reshape(self.out_channels, self.in_channels)
        if _conv1x1_native(x, self.out_channels, self.in_channels) \
                and w2.dtype == torch.bfloat16 and w2.is_contiguous():
            return _Conv1x1Fn.apply(x, w2, self.bias)
        return torch.nn.functional.conv2d(
            x, self.weight.to(x.dtype),
            self.bias.to(x.dtype) if self.bias is not None else None)

    def extra_repr(self):
        return "in=%d, out=%d (native when H*W%%8==0)" % (
            self.in_channels, self.out_channels)


def conv1x1(x: torch.Tensor, weight: torch.Tensor,
            bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Functional 1x1 conv: weight [Co, Ci] (or [Co, Ci, 1, 1])."""
    if weight.dim() == 4:
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    co, ci = weight.shape
    if _conv1x1_native(x, co, ci) and weight.dtype == torch.bfloat16 \
            and weight.is_contiguous():
        return _Conv1x1Fn.apply(x, weight, bias)
    return torch.nn.functional.conv2d(
        x, weight.reshape(co, ci, 1, 1).to(x.dtype),
        bias.to(x.dtype) if bias is not None else None)


class _DepthwiseFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        ext = _extension.require()
        B, C, H, W = x.shape
        KS = weight.shape[-1]
        OH = (H + 2 * pad - KS) // stride + 1
        OW = (W + 2 * pad - KS) // stride + 1
        y = torch.empty((B, C, OH, OW), device=x.device, dtype=torch.bfloat16)
        ext.depthwise_fwd(x, weight, y, stride, pad)
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.pad = stride, pad
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _extension.require()
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ext.depthwise_bwd_dx(dy, weight, dx, ctx.stride, ctx.pad)
        if ctx.needs_input_grad[1]:
            dwf = torch.empty(weight.numel(), device=x.device,
                              dtype=torch.float32)
            ext.depthwise_bwd_dw(x, dy, dwf, ctx.stride, ctx.pad)
            dw = dwf.reshape(weight.shape).to(weight.dtype)
        return dx, dw, None, None


class HipDepthwiseConv2d(nn.Module):
    """Depthwise KxK conv on the native kernel (any channel count),
    drop-in for ``nn.Conv2d(C, C, K, stride, padding, groups=C, bias=False)``.
    Falls back to grouped conv2d (MIOpen) off-GPU or for non-bf16 input.
    """

    def __init__(self, channels: int, kernel_size: int, stride: int = 1,
                 padding: int = 0):
        super().__init__()
        self.channels = channels
        self.kernel_size = kernel_size
        self.stride = stride
        self.padding = padding
        ref = nn.Conv2d(channels, channels, kernel_size, stride=stride,
                        padding=padding, groups=channels, bias=False)
        self.weight = nn.Parameter(ref.weight.detach())  # [C,1,K,K]

    def forward(self, x):
        return depthwise_conv2d(x, self.weight, self.stride, self.padding)

    def extra_repr(self):
        return "C=%d, k=%d, s=%d, p=%d (native bf16 path)" % (
            self.channels, self.kernel_size, self.stride, self.padding)


def depthwise_conv2d(x: torch.Tensor, weight: torch.Tensor, stride: int = 1,
                     padding: int = 0) -> torch.Tensor:
    """Functional depthwise conv, weight [C, 1, K, K]: the native kernel for
    contiguous bf16 GPU tensors, grouped conv2d otherwise."""
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous()
            and weight.dtype == torch.bfloat16 and _native_enabled()):
        return _DepthwiseFn.apply(x, weight.contiguous(), stride, padding)
    return torch.nn.functional.conv2d(
        x, weight.to(x.dtype), None, stride, padding, groups=weight.shape[0])


def _fused_relu_dw_enabled() -> bool:
    import os
    return os.environ.get("ADANET_FUSED_RELU_DW", "1") != "0"


def _relu_dw_pays(h: int, w: int, k: int) -> bool:
    """The part of the kernels' class where both fused directions measured
    no slower than the chain (BENCHMARKS.md, "Fused ReLU -> depthwise"): at
    most 2304 tap products per input plane, that is 16x16 with 3x3 taps and
    8x8 with 3x3 or 5x5. Above it the one-launch backward loses to the
    separate dW and dX kernels (32x32 5x5: 183 us against 150), so those
    shapes keep the chain."""
    return h * w * k * k <= 2304


def relu_depthwise_supported(x: torch.Tensor, weight: torch.Tensor,
                             stride: int = 1, padding: int = 0) -> bool:
    """Whether `relu_depthwise_conv2d` runs these arguments on the fused
    kernels (csrc/relu_depthwise.hip) rather than on relu then
    `depthwise_conv2d`: the kernels must take them and must have measured
    no slower than the chain at that size (`_relu_dw_pays`)."""
    if x.dim() != 4 or weight.dim() != 4 or not _native_enabled() \
            or not _fused_relu_dw_enabled() \
            or not (x.is_cuda and x.dtype == torch.bfloat16
                    and x.is_contiguous() and x.data_ptr() % 16 == 0) \
            or not (weight.is_cuda and weight.dtype == torch.bfloat16) \
            or weight.shape[0] != x.shape[1] or weight.shape[1] != 1 \
            or weight.shape[2] != weight.shape[3] or x.numel() == 0:
        return False
    _, c, h, w = x.shape
    k = weight.shape[-1]
    return _relu_dw_pays(h, w, k) and _extension.require(
    ).relu_depthwise_supported(c, h, w, k, stride, padding)


class _ReluDepthwiseFn(torch.autograd.Function):
    """relu -> depthwise KxK on csrc/relu_depthwise.hip: one launch forward,
    one launch plus the slot sum for dX and dW together. Saves x and the
    weight only; relu(x) never exists in memory."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        B, C, H, W = x.shape
        KS = weight.shape[-1]
        y = torch.empty((B, C, (H + 2 * pad - KS) // stride + 1,
                         (W + 2 * pad - KS) // stride + 1), device=x.device,
                        dtype=torch.bfloat16)
        _extension.require().relu_depthwise_fwd(x, weight, y, stride, pad)
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.pad = stride, pad
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dwf = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
        if ctx.needs_input_grad[1]:
            dwf = torch.empty(weight.numel(), device=x.device,
                              dtype=torch.float32)
        _extension.require().relu_depthwise_bwd(
            x, dy.contiguous(), weight, dx, dwf, ctx.stride, ctx.pad)
        if dwf is not None:
            dw = dwf.reshape(weight.shape).to(weight.dtype)
        return dx, dw, None, None


def _relu_dw_strip_enabled() -> bool:
    import os
    return os.environ.get("ADANET_RELU_DW_STRIP", "1") != "0"


def _relu_dw_strip_pays(h: int, w: int, k: int, stride: int) -> bool:
    """The size classes where the strip forward and the strip backward (dX
    plus the dW-only launch and its reduce) both measured no slower than the
    chain (BENCHMARKS.md, "Strip-tiled ReLU -> depthwise"): planes of 256 to
    1024 pixels, where every measured K and stride won both ways (32x32 with
    3x3 and 5x5 at stride 1 and 5x5 at stride 2, 16x16 with 5x5 and 7x7 at
    stride 1 and 7x7 at stride 2: forward 2.4 to 4.9 times faster, backward
    1.14 to 2.2 times). Larger planes of the kernels' class were not
    measured and keep the chain, as do the sizes that the one-launch
    kernels take first (`_relu_dw_pays`)."""
    return 256 <= h * w <= 1024 and not _relu_dw_pays(h, w, k)


def _relu_dw_strip_dw_enabled() -> bool:
    import os
    return os.environ.get("ADANET_RELU_DW_STRIP_DW", "1") != "0"


def _relu_dw_strip_dw_pays(h: int, w: int, k: int, stride: int) -> bool:
    """The size classes where `relu_depthwise_strip_bwd_dw` measured below
    `relu_depthwise_bwd`'s dW-only launch and reduce by more than both
    interquartile ranges (BENCHMARKS.md, "Strip-tiled dW"; us per call at
    batch 256, old / new, every range at most 0.27): 32x32 with 5x5
    113.6 / 57.3, 3x3 56.4 / 39.0, 5x5 at stride 2 44.6 / 34.8; 16x16 with
    5x5 62.9 / 35.8, 3x3 32.0 / 23.1, 7x7 110.6 / 48.2, 7x7 at stride 2
    46.2 / 34.7; 8x8 with 5x5 45.7 / 28.2. That is every measured K and
    stride on planes of 64 to 1024 pixels; larger planes of the kernel's
    class were not measured and keep the old kernel."""
    return 64 <= h * w <= 1024


def relu_depthwise_strip_supported(x: torch.Tensor, weight: torch.Tensor,
                                   stride: int = 1, padding: int = 0) -> bool:
    """Whether `relu_depthwise_conv2d` runs these arguments on the
    strip-tiled kernels (csrc/relu_depthwise_strip.hip): 16-byte aligned
    contiguous bf16 GPU tensors of the kernels' class (K in {3, 5, 7},
    stride 1 or 2, padding K // 2, W % 8 == 0, H*W <= 4096; stride 2: H even
    and W % 16 == 0) at a size where they measured no slower than the chain
    (`_relu_dw_strip_pays`), with ADANET_RELU_DW_STRIP not 0."""
    if x.dim() != 4 or weight.dim() != 4 or not _native_enabled() \
            or not _fused_relu_dw_enabled() or not _relu_dw_strip_enabled() \
            or not _bf16_dense(x) or not _bf16_dense(weight) \
            or weight.shape[0] != x.shape[1] or weight.shape[1] != 1 \
            or weight.shape[2] != weight.shape[3] or x.numel() == 0:
        return False
    _, c, h, w = x.shape
    k = weight.shape[-1]
    return _relu_dw_strip_pays(h, w, k, stride) and _extension.require(
    ).relu_depthwise_strip_supported(c, h, w, k, stride, padding)


class _ReluDepthwiseStripFn(torch.autograd.Function):
    """relu -> depthwise KxK on csrc/relu_depthwise_strip.hip: one launch
    forward, one for the masked dX, and one plus the slot sum for dW: the
    strip-tiled one where it measured faster (`_relu_dw_strip_dw_pays`, with
    ADANET_RELU_DW_STRIP_DW not 0), else relu_depthwise_bwd's dW-only
    instance; the two give the same bits. Saves x and the weight only."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        B, C, H, W = x.shape
        KS = weight.shape[-1]
        y = torch.empty((B, C, (H + 2 * pad - KS) // stride + 1,
                         (W + 2 * pad - KS) // stride + 1), device=x.device,
                        dtype=torch.bfloat16)
        _extension.require().relu_depthwise_strip_fwd(x, weight, y, stride,
                                                      pad)
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.pad = stride, pad
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _extension.require()
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.data_ptr() % 16:
            dy = dy.clone()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ext.relu_depthwise_strip_bwd_dx(x, dy, weight, dx, ctx.stride,
                                            ctx.pad)
        if ctx.needs_input_grad[1]:
            dwf = torch.empty(weight.numel(), device=x.device,
                              dtype=torch.float32)
            if _relu_dw_strip_dw_enabled() and _relu_dw_strip_dw_pays(
                    x.shape[2], x.shape[3], weight.shape[-1], ctx.stride):
                ext.relu_depthwise_strip_bwd_dw(x, dy, dwf, ctx.stride,
                                                ctx.pad)
            else:
                ext.relu_depthwise_bwd(x, dy, weight, None, dwf, ctx.stride,
                                       ctx.pad)
            dw = dwf.reshape(weight.shape).to(weight.dtype)
        return dx, dw, None, None


def relu_depthwise_conv2d(x: torch.Tensor, weight: torch.Tensor,
                          stride: int = 1, padding: int = 0) -> torch.Tensor:
    """depthwise_conv2d(relu(x), weight, stride, padding), weight
    [C, 1, K, K]. Differentiable. Contiguous bf16 GPU tensors with K in
    {3, 5, 7} and stride 1 or 2 run fused kernels at the sizes where those
    measured no slower: the one-launch kernels where H*W*K*K <= 2304
    (`relu_depthwise_supported`), the strip-tiled kernels on larger planes
    (`relu_depthwise_strip_supported`). Their results equal the
    composition's bit for bit and they keep no relu(x) for backward.
    Everything else runs the composition: CPU tensors, other dtypes and
    shapes, ADANET_NATIVE_CONV=0 and ADANET_FUSED_RELU_DW=0;
    ADANET_RELU_DW_STRIP=0 turns off the strip-tiled branch alone, and
    ADANET_RELU_DW_STRIP_DW=0 only its strip-tiled weight gradient, which
    then comes from the one-launch kernel's dW-only instance with the same
    bits.
    ReLU is v > 0 ? v : +0; NaN inputs are outside the bit-for-bit contract.
    """
    if relu_depthwise_supported(x, weight, stride, padding):
        return _ReluDepthwiseFn.apply(x, weight.contiguous(), stride, padding)
    if relu_depthwise_strip_supported(x, weight, stride, padding):
        return _ReluDepthwiseStripFn.apply(x, weight, stride, padding)
    return depthwise_conv2d(F.relu(x), weight, stride, padding)


def _fused_sepconv_enabled() -> bool:
    import os
    return os.environ.get("ADANET_FUSED_SEPCONV", "1") != "0"


def _bf16_dense(t: torch.Tensor) -> bool:
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()
            and t.data_ptr() % 16 == 0)


def _fused_relu_pw_enabled() -> bool:
    import os
    return os.environ.get("ADANET_FUSED_RELU_PW", "1") != "0"


def _relu_pw_pays(ci: int, co: int, hw: int) -> bool:
    """The part of the kernels' class where both fused directions measured
    no slower than the chain (BENCHMARKS.md, "Fused ReLU -> pointwise"):
    planes of at least 256 pixels (16x16 and 32x32, Ci 96 to 320), and
    smaller planes up to Ci = 96 (8x8, 96 -> 32). On 8x8 planes with
    Ci = 640 a block walks 20 chunks with one 64-pixel tile's worth of loads
    in flight, and one direction lost to the chain by more than the spread
    (640 -> 128 forward 35.1 us against 27.3, 640 -> 64 backward 52.7
    against 46.2), so those shapes keep the chain."""
    return hw >= 256 or ci <= 96


def relu_conv1x1_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Whether `relu_conv1x1` runs these arguments on the fused kernels
    (csrc/relu_pointwise.hip) rather than on relu then `conv1x1`: the
    kernels must take them and must have measured no slower than the chain
    at that size (`_relu_pw_pays`)."""
    if x.dim() != 4 or weight.dim() not in (2, 4) or not _native_enabled() \
            or not _fused_relu_pw_enabled() or not _bf16_dense(x) \
            or not _bf16_dense(weight) or x.numel() == 0 \
            or x.shape[0] > 65535 \
            or weight.numel() != weight.shape[0] * x.shape[1]:
        return False
    _, ci, h, w = x.shape
    co = weight.shape[0]
    return _relu_pw_pays(ci, co, h * w) and _extension.require(
    ).relu_pointwise_supported(ci, co, h, w)


class _ReluConv1x1Fn(torch.autograd.Function):
    """relu -> 1x1 conv on csrc/relu_pointwise.hip: one launch forward, one
    for the masked dX, and conv1x1_dw's kernel with the clamp on its x
    fragments for dW. Saves x and the weight only; relu(x) never exists in
    memory."""

    @staticmethod
    def forward(ctx, x, weight):
        B, _, H, W = x.shape
        y = torch.empty((B, weight.shape[0], H, W), device=x.device,
                        dtype=torch.bfloat16)
        _extension.require().relu_pointwise_fwd(x, weight, y)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _extension.require()
        x, weight = ctx.saved_tensors
        B, Ci, H, W = x.shape
        dy = dy.contiguous()
        if dy.data_ptr() % 16:
            dy = dy.clone()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ext.relu_pointwise_bwd_dx(dy, x, weight, dx)
        if ctx.needs_input_grad[1]:
            dy3 = dy.reshape(B, weight.shape[0], H * W)
            if _dw_direct_enabled() and (B * H * W) % 32 == 0:
                dw = torch.empty((weight.shape[0], Ci), device=x.device,
                                 dtype=torch.bfloat16)
                ext.relu_conv1x1_dw(dy3, x.reshape(B, Ci, H * W), dw)
            else:
                # the chain's copy path permutes its operands anyway
                dw = _weight_grad(dy3, F.relu(x).reshape(B, Ci, H * W))
            dw = dw.reshape(weight.shape)
        return dx, dw


def relu_conv1x1(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """conv1x1(relu(x), weight), weight [Co, Ci] or [Co, Ci, 1, 1], no
    bias. Differentiable. Contiguous, 16-byte aligned bf16 GPU tensors with
    Ci % 32 == 0, Co % 32 == 0, Co <= 128 and H*W % 8 == 0, at the sizes
    where they measured no slower (`relu_conv1x1_supported`), run the fused
    kernels, whose y, dx and dW equal the composition's bit for bit and
    which keep no relu(x) for backward. Everything else runs the
    composition: CPU tensors, other dtypes and shapes, ADANET_NATIVE_CONV=0
    and ADANET_FUSED_RELU_PW=0. ReLU is v > 0 ? v : +0; NaN inputs are
    outside the bit-for-bit contract.
    """
    if relu_conv1x1_supported(x, weight):
        return _ReluConv1x1Fn.apply(x, weight)
    return conv1x1(F.relu(x), weight)


def sepconv_infer_supported(x: torch.Tensor,
                            dw_weight: Optional[torch.Tensor],
                            pw_weight: torch.Tensor, stride: int = 1,
                            padding: int = 0) -> bool:
    """Whether `sepconv_bn_infer` runs these arguments on the fused kernel
    (csrc/sepconv_infer.hip) rather than on the four-launch chain."""
    if x.dim() != 4 or not _bf16_dense(x) or not _bf16_dense(pw_weight) \
            or not _native_enabled() or pw_weight.dim() not in (2, 4) \
            or pw_weight.numel() != pw_weight.shape[0] * x.shape[1]:
        return False
    k = 1
    if dw_weight is not None:
        if not _bf16_dense(dw_weight) or dw_weight.dim() != 4 \
                or dw_weight.shape[0] != x.shape[1] \
                or dw_weight.shape[1] != 1 \
                or dw_weight.shape[2] != dw_weight.shape[3]:
            return False
        k = dw_weight.shape[-1]
        if k == 1:      # a 1x1 depthwise scales channels: not the K=1 form
            return False
    elif stride != 1 or padding != 0:
        return False
    _, ci, h, w = x.shape
    return x.shape[0] <= 65535 and _extension.require(
    ).sepconv_infer_supported(ci, pw_weight.shape[0], h, w, k, stride,
                              padding)


def sepconv_bn_infer(x: torch.Tensor, dw_weight: Optional[torch.Tensor],
                     pw_weight: torch.Tensor, bn: Optional[nn.Module] = None,
                     stride: int = 1, padding: int = 0) -> torch.Tensor:
    """Inference-only ReLU -> depthwise KxK -> pointwise 1x1 -> BatchNorm
    (running statistics) of one separable-conv half-stack.

    x [B, Ci, H, W]; dw_weight [Ci, 1, K, K] or None for no depthwise stage
    (ReLU-Conv-BN); pw_weight [Co, Ci] or [Co, Ci, 1, 1]; bn a
    `HipBatchNorm2d` or None. bf16 GPU tensors of a supported shape
    (`sepconv_infer_supported`) take one fused launch that rounds where the
    chain of four kernels rounds; everything else, CPU tensors included,
    runs that chain. There is no backward: tensors that require grad are
    refused while grad mode is on.
    """
    if torch.is_grad_enabled():
        params = [x, dw_weight, pw_weight]
        if bn is not None:
            params += [bn.weight, bn.bias]
        if any(t is not None and t.requires_grad for t in params):
            raise RuntimeError(
                "sepconv_bn_infer has no backward: call it under "
                "torch.no_grad() or with tensors that do not require grad")
    if _fused_sepconv_enabled() and sepconv_infer_supported(
            x, dw_weight, pw_weight, stride, padding):
        ext = _extension.require()
        B, _, H, W = x.shape
        co = pw_weight.shape[0]
        k = 1 if dw_weight is None else dw_weight.shape[-1]
        oh = (H + 2 * padding - k) // stride + 1
        ow = (W + 2 * padding - k) // stride + 1
        y = torch.empty((B, co, oh, ow), device=x.device,
                        dtype=torch.bfloat16)
        mean = rstd = gamma = beta = None
        if bn is not None:
            mean = bn.running_mean.float()
            rstd = (bn.running_var.float() + bn.eps).rsqrt()
            if bn.weight is not None:
                gamma = bn.weight.detach().float()
                beta = bn.bias.detach().float()
        ext.sepconv_infer(x, dw_weight, pw_weight, mean, rstd, gamma, beta,
                          y, stride, padding)
        return y
    y = F.relu(x)
    if dw_weight is not None:
        y = depthwise_conv2d(y, dw_weight, stride, padding)
    y = conv1x1(y, pw_weight)
    return bn.infer(y) if bn is not None else y


class _Im2colFn(torch.autograd.Function):
    """Batched im2col (one launch for the whole batch, zero-padded K dim)
    with the exact col2im adjoint for backward (csrc/im2col.hip)."""

    @staticmethod
    def forward(ctx, x, K, stride, pad, ckk_pad, oh, ow):
        ext = _extension.require()
        B = x.shape[0]
        out = torch.empty((B, ckk_pad, oh, ow), device=x.device,
                          dtype=x.dtype)
        ext.im2col_bf16(x, out, K, stride, pad)
        ctx.meta = (x.shape, K, stride, pad)
        return out

    @staticmethod
    def backward(ctx, du):
        ext = _extension.require()
        shape, K, stride, pad = ctx.meta
        dx = torch.empty(shape, device=du.device, dtype=du.dtype)
        ext.col2im_bf16(du.contiguous(), dx, K, stride, pad)
        return dx, None, None, None, None, None, None


class HipConvNxN(nn.Module):
    """Dense KxK conv as unfold + the batched MFMA GEMM (K9 tail).

    MIOpen falls back to a naive weight-gradient kernel for these NCHW
    bf16 shapes (6.9 ms/call — 35% of the NASNet step,
    profiles/conv_bench_r01.txt); expressing the conv as im2col (one
    torch.unfold copy, a few MB) + gemm_tr_batched keeps fwd/bwd on the
    MFMA path. The im2col K dim (Ci*K*K) is zero-padded to 32 inside the
    padded weight, so ANY in-channel count works. Co % 32 == 0 runs
    gemm_tr_batched; any other Co runs csrc/conv1x1_ragged.hip when the
    output plane has OH*OW % 8 == 0 (else, and with ADANET_CONV_RAGGED=0,
    torch fallback). Drop-in for
    ``nn.Conv2d(ci, co, K, stride, padding, bias=...)``.
    """

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int,
                 stride: int = 1, padding: int = 0, bias: bool = True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.stride = stride
        self.padding = padding
        ref = nn.Conv2d(in_channels, out_channels, kernel_size,
                        stride=stride, padding=padding, bias=bias)
        self.weight = nn.Parameter(ref.weight.detach())  # [Co, Ci, K, K]
        if bias:
            self.bias = nn.Parameter(ref.bias.detach().float())
        else:
            self.register_parameter("bias", None)

    def forward(self, x):
        return conv_nxn(x, self.weight, self.bias, self.stride, self.padding)

    def extra_repr(self):
        return "in=%d, out=%d, k=%d, s=%d (im2col+MFMA)" % (
            self.in_channels, self.out_channels, self.kernel_size,
            self.stride)


def conv_nxn(x: torch.Tensor, weight: torch.Tensor,
             bias: Optional[torch.Tensor] = None, stride: int = 1,
             padding: int = 0) -> torch.Tensor:
    """Functional `HipConvNxN`: weight [Co, Ci, K, K], bias fp32 [Co]."""
    co, ci, K, _ = weight.shape
    ckk = ci * K * K
    ckk_pad = (ckk + 31) // 32 * 32
    oh = (x.shape[2] + 2 * padding - K) // stride + 1
    ow = (x.shape[3] + 2 * padding - K) // stride + 1
    # Co off the 32 grid runs csrc/conv1x1_ragged.hip, which wants whole
    # 16 B vectors per output row
    if (x.is_cuda and x.dtype == torch.bfloat16 and _native_enabled()
            and weight.dtype == torch.bfloat16
            and (co % 32 == 0
                 or _ragged_ok(x.shape[0], oh * ow, co, ckk_pad))):
        # batched im2col with the 32-alignment zero-pad folded in
        # (torch's F.unfold is one im2col launch PER IMAGE).
        u = _Im2colFn.apply(x.contiguous(), K, stride, padding, ckk_pad,
                            oh, ow)
        w2 = weight.reshape(co, ckk)
        if ckk_pad != ckk:
            w2 = torch.nn.functional.pad(w2, (0, ckk_pad - ckk))
        return _Conv1x1Fn.apply(u, w2.contiguous(), bias)
    return torch.nn.functional.conv2d(
        x, weight.to(x.dtype),
        bias.to(x.dtype) if bias is not None else None, stride, padding)


def _fused_factred_enabled() -> bool:
    import os
    return os.environ.get("ADANET_FUSED_FACTRED", "1") != "0"


def _factred_weights(w1: torch.Tensor, w2: torch.Tensor):
    """Both halves as Conv2d-layout [Co/2, Ci, 1, 1] views."""
    return tuple(w if w.dim() == 4 else w.reshape(w.shape[0], w.shape[1], 1, 1)
                 for w in (w1, w2))


def _factred_chain(x, w1, w2):
    """The unfused composition: relu, the one-pixel shift by pad and slice,
    two stride-2 1x1 convs, channel concat."""
    w1, w2 = _factred_weights(w1, w2)
    r = F.relu(x)
    a = conv_nxn(r, w1, None, 2, 0)
    b = conv_nxn(F.pad(r, (0, 1, 0, 1))[:, :, 1:, 1:], w2, None, 2, 0)
    return torch.cat([a, b], dim=1)


def factorized_reduction_supported(x: torch.Tensor, w1: torch.Tensor,
                                   w2: torch.Tensor) -> bool:
    """Whether `factorized_reduction` runs these arguments on the fused
    kernels (csrc/factred.hip) rather than on the unfused composition."""
    if x.dim() != 4 or not _native_enabled() or x.shape[0] > 65535 \
            or not all(_bf16_dense(t) for t in (x, w1, w2)) \
            or w1.shape != w2.shape or w1.dim() not in (2, 4) \
            or w1.numel() != w1.shape[0] * x.shape[1]:
        return False
    _, ci, h, w = x.shape
    return _extension.require().factred_supported(ci, 2 * w1.shape[0], h, w)


def _factred_out(x, w1):
    B, _, H, W = x.shape
    return torch.empty((B, 2 * w1.shape[0], (H - 1) // 2 + 1,
                        (W - 1) // 2 + 1), device=x.device,
                       dtype=torch.bfloat16)


class _FactRedFn(torch.autograd.Function):
    """relu -> two offset stride-2 1x1 convs -> concat on csrc/factred.hip:
    one launch forward, one for dX, one split-K launch plus the slot sum
    for both weight gradients. Saves x and the weights only."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        y = _factred_out(x, w1)
        _extension.require().factred_fwd(x, w1, w2, None, None, None, None, y)
        ctx.save_for_backward(x, w1, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _extension.require()
        x, w1, w2 = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw1 = dw2 = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ext.factred_bwd_dx(dy, x, w1, w2, dx)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            B, ci, H, W = x.shape
            ch = w1.shape[0]
            slots = ext.factred_dw_slots(B, ci, H, W, 0)
            wsp = torch.empty((slots, 2 * ch, ci), device=x.device,
                              dtype=torch.float32)
            dw = torch.empty((2 * ch, ci), device=x.device,
                             dtype=torch.bfloat16)
            ext.factred_bwd_dw(x, dy, dw, wsp, 0)
            dw1, dw2 = dw[:ch].reshape(w1.shape), dw[ch:].reshape(w2.shape)
        return dx, dw1, dw2


def factorized_reduction(x: torch.Tensor, w1: torch.Tensor,
                         w2: torch.Tensor) -> torch.Tensor:
    """ReLU, then two stride-2 1x1 convs over the even and the odd pixel
    lattice, concatenated: y[:, :Co/2, oh, ow] = w1 @ relu(x)[:, :, 2oh, 2ow]
    and y[:, Co/2:, oh, ow] = w2 @ relu(x)[:, :, 2oh+1, 2ow+1] (zero where
    that pixel lies outside). The part of NASNet's factorized reduction in
    front of its BatchNorm.

    x [B, Ci, H, W]; w1, w2 [Co/2, Ci] or [Co/2, Ci, 1, 1]. Returns
    [B, Co, (H-1)//2+1, (W-1)//2+1]. Differentiable. bf16 GPU tensors of a
    supported shape (`factorized_reduction_supported`) run three fused
    kernels that round where the composition rounds; everything else, CPU
    tensors and ADANET_NATIVE_CONV=0 included, runs the composition.
    """
    if factorized_reduction_supported(x, w1, w2):
        return _FactRedFn.apply(x, w1, w2)
    return _factred_chain(x, w1, w2)


def factorized_reduction_bn_infer(x: torch.Tensor, w1: torch.Tensor,
                                  w2: torch.Tensor,
                                  bn: Optional[nn.Module] = None
                                  ) -> torch.Tensor:
    """Inference-only `factorized_reduction` followed by BatchNorm on the
    running statistics of `bn` (a `HipBatchNorm2d`, or None): one launch
    where supported, otherwise the composition and `bn.infer`. There is no
    backward: tensors that require grad are refused while grad mode is on.
    """
    if torch.is_grad_enabled():
        params = [x, w1, w2]
        if bn is not None:
            params += [bn.weight, bn.bias]
        if any(t is not None and t.requires_grad for t in params):
            raise RuntimeError(
                "factorized_reduction_bn_infer has no backward: call it "
                "under torch.no_grad() or with tensors that do not require "
                "grad")
    if _fused_factred_enabled() and factorized_reduction_supported(x, w1, w2):
        y = _factred_out(x, w1)
        mean = rstd = gamma = beta = None
        if bn is not None:
            mean = bn.running_mean.float()
            rstd = (bn.running_var.float() + bn.eps).rsqrt()
            if bn.weight is not None:
                gamma = bn.weight.detach().float()
                beta = bn.bias.detach().float()
        _extension.require().factred_fwd(x, w1, w2, mean, rstd, gamma, beta,
                                         y)
        return y
    y = _factred_chain(x, w1, w2)
    return bn.infer(y) if bn is not None else y


class _Pool3Fn(torch.autograd.Function):
    """3x3 pooling on the native kernel (csrc/pool.hip): avg is
    count_include_pad=False, max saves the window argmax for an exact
    deterministic gather backward."""

    @staticmethod
    def forward(ctx, x, stride, is_max):
        ext = _extension.require()
        x = x.contiguous()
        N, C, H, W = x.shape
        OH = (H + 2 - 3) // stride + 1
        OW = (W + 2 - 3) // stride + 1
        y = torch.empty((N, C, OH, OW), device=x.device, dtype=x.dtype)
        argmax = None
        if is_max:
            argmax = torch.empty((N, C, OH, OW), device=x.device,
                                 dtype=torch.uint8)
        ext.pool3_fwd(x, y, argmax, stride, int(is_max))
        ctx.save_for_backward(argmax) if argmax is not None else \
            ctx.save_for_backward()
        ctx.meta = (x.shape, stride, is_max)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _extension.require()
        shape, stride, is_max = ctx.meta
        argmax = ctx.saved_tensors[0] if ctx.saved_tensors else None
        dy = dy.contiguous()
        dx = torch.empty(shape, device=dy.device, dtype=dy.dtype)
        ext.pool3_bwd(dy, argmax, dx, stride, int(is_max))
        return dx, None, None


class HipPool2d(nn.Module):
    """3x3 avg/max pool, stride 1 or 2, pad 1 — native CDNA4 kernels on
    GPU (the last MIOpen ops on the NASNet cell hot path, K9 remainder);
    torch pooling on CPU."""

    def __init__(self, kind: str, stride: int):
        super().__init__()
        assert kind in ("avg", "max")
        self.kind = kind
        self.stride = stride

    def forward(self, x):
        if x.is_cuda:
            return _Pool3Fn.apply(x.to(torch.bfloat16), self.stride,
                                  self.kind == "max")
        if self.kind == "avg":
            return F.avg_pool2d(x, 3, self.stride, 1,
                                count_include_pad=False)
        return F.max_pool2d(x, 3, self.stride, 1)

    def extra_repr(self):
        return "%s3x3 s%d" % (self.kind, self.stride)
