"""Fused NASNet cell combine: drop-path scale, left+right add, channel concat.

A NASNet-A cell ends every block with ``drop_path(left) + drop_path(right)``
and concatenates the block outputs channel-wise. Unfused that is, per block,
two broadcast multiplies, one add and a share of ``torch.cat`` — 16 launches
and nine passes over each block's activation per normal cell, with strided
multiplies in backward. ``cell_combine`` does a whole group of blocks in one
launch of csrc/combine.hip (read left, read right, write the concat slot) and
one launch in backward, bit-identical to the unfused composition: the kernel
rounds to bf16 exactly where torch materialises a bf16 tensor.

The native path needs CUDA, bf16, contiguous inputs and
``ADANET_FUSED_COMBINE`` (default ``"1"``) not ``"0"``; anything else — CPU,
fp32, strided inputs, the toggle — takes the plain torch composition, which
therefore stays the numerics oracle.
"""

from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch

from adanet_amd.ops import _extension

_MAX_PAIRS = 8  # pointer slots in the kernel-argument struct


def _fused_enabled() -> bool:
    return os.environ.get("ADANET_FUSED_COMBINE", "1") != "0"


def _native_ok(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()


def _compose(lefts, rights, scales_l, scales_r) -> torch.Tensor:
    """The unfused composition, exactly as the cell spelled it out."""
    outs = []
    for i, (left, right) in enumerate(zip(lefts, rights)):
        if scales_l is not None:
            left = left * scales_l[i]
            right = right * scales_r[i]
        outs.append(left + right)
    return torch.cat(outs, dim=1)


class _CellCombineFn(torch.autograd.Function):
    """args = lefts (n), rights (n), then scales_l (n) + scales_r (n) when
    ``scaled``. Saves only the scales: backward never needs activations."""

    @staticmethod
    def forward(ctx, n, scaled, *args):
        ext = _extension.require()
        lefts, rights = list(args[:n]), list(args[n:2 * n])
        sl = list(args[2 * n:3 * n]) if scaled else []
        sr = list(args[3 * n:4 * n]) if scaled else []
        B, F, H, W = lefts[0].shape
        out = torch.empty((B, n * F, H, W), device=lefts[0].device,
                          dtype=torch.bfloat16)
        if out.numel():
            for i0 in range(0, n, _MAX_PAIRS):
                i1 = min(n, i0 + _MAX_PAIRS)
                ext.cell_combine_fwd(lefts[i0:i1], rights[i0:i1], sl[i0:i1],
                                     sr[i0:i1], out, i0)
        ctx.n, ctx.scaled, ctx.F = n, scaled, F
        ctx.save_for_backward(*sl, *sr)
        return out

    @staticmethod
    def backward(ctx, dy):
        n, F = ctx.n, ctx.F
        if not ctx.scaled:
            # What autograd does for add + cat: hand out channel slices of
            # dy, no kernel (a copy would make keep == 1 training slower).
            grads = [dy.narrow(1, i * F, F) if ctx.needs_input_grad[2 + i]
                     else None for i in range(n)]
            grads += [dy.narrow(1, i * F, F)
                      if ctx.needs_input_grad[2 + n + i] else None
                      for i in range(n)]
            return (None, None, *grads)
        ext = _extension.require()
        sl, sr = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        B, _, H, W = dy.shape
        # The kernel takes any batch stride (dy is often a channel slice of
        # an enclosing concat's gradient); each sample must be dense.
        if not (dy.dtype == torch.bfloat16 and dy.numel()
                and dy[0].is_contiguous()
                and (B == 1 or dy.stride(0) >= n * F * H * W)):
            dy = dy.to(torch.bfloat16).contiguous()

        def fresh(k):
            if not ctx.needs_input_grad[2 + k]:
                return None
            return torch.empty((B, F, H, W), device=dy.device,
                               dtype=torch.bfloat16)

        dl = [fresh(i) for i in range(n)]
        dr = [fresh(n + i) for i in range(n)]
        if dy.numel():
            for i0 in range(0, n, _MAX_PAIRS):
                i1 = min(n, i0 + _MAX_PAIRS)
                ext.cell_combine_bwd(dy, list(sl[i0:i1]), list(sr[i0:i1]),
                                     dl[i0:i1], dr[i0:i1], i0)
        return (None, None, *dl, *dr, *([None] * (2 * n)))


def cell_combine(lefts: Sequence[torch.Tensor],
                 rights: Sequence[torch.Tensor],
                 scales_l: Optional[Sequence[torch.Tensor]] = None,
                 scales_r: Optional[Sequence[torch.Tensor]] = None
                 ) -> torch.Tensor:
    """``cat([l*sl + r*sr for each block], dim=1)`` -> ``[B, n*F, H, W]``.

    ``lefts[i]`` / ``rights[i]`` are the two branch outputs of block ``i``,
    all ``[B, F, H, W]``; the same tensor may appear more than once.
    ``scales_l[i]`` / ``scales_r[i]`` are the per-sample drop-path scales
    (``B`` elements, ``0`` or ``1/keep``, e.g. ``[B,1,1,1]``); pass both
    lists or neither (eval, ``keep >= 1``). Never synchronises with the
    host.
    """
    lefts, rights = list(lefts), list(rights)
    n = len(lefts)
    if n == 0 or len(rights) != n:
        raise ValueError("cell_combine: lefts and rights must be non-empty "
                         "lists of equal length (got %d and %d)"
                         % (n, len(rights)))
    if (scales_l is None) != (scales_r is None):
        raise ValueError("cell_combine: pass scales_l and scales_r together "
                         "or neither")
    scaled = scales_l is not None
    if scaled:
        scales_l, scales_r = list(scales_l), list(scales_r)
        if len(scales_l) != n or len(scales_r) != n:
            raise ValueError("cell_combine: one scale per block and side "
                             "(%d blocks, got %d and %d)"
                             % (n, len(scales_l), len(scales_r)))
    shape = lefts[0].shape
    native = (_fused_enabled() and len(shape) == 4
              and all(_native_ok(t) and t.shape == shape
                      for t in lefts + rights))
    if native and scaled:
        native = all(_native_ok(s) and s.numel() == shape[0]
                     and not s.requires_grad for s in scales_l + scales_r)
    if not native:
        return _compose(lefts, rights, scales_l, scales_r)
    extra: List[torch.Tensor] = scales_l + scales_r if scaled else []
    return _CellCombineFn.apply(n, scaled, *lefts, *rights, *extra)
