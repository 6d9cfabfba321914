"""Device-side batch construction: parameter draw + fused augmentation.

``draw_params`` draws, per batch slot, ``(index, oy, ox, flip, cy, cx)`` from
the project's stateless counter RNG (``hash_rng`` in csrc/common.h) and
gathers the labels; ``augment_apply`` turns a device-resident uint8 or fp32
dataset plus those parameters into a bf16 batch: gather, pad-crop, flip,
cutout, per-channel ``x * scale + shift`` and the bf16 cast in one pass
(csrc/augment.hip).

On CUDA tensors both run the HIP kernels through ``_extension.require()``;
there is no eager fallback. On CPU tensors they run the pure-torch/Python
reference below, which is both the GPU-less implementation and the numerics
oracle: the integers are equal and the bf16 images bit-identical.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from adanet_amd.ops import _extension

_M64 = (1 << 64) - 1
FIELDS = 6  # index, oy, ox, flip, cy, cx


def hash_rng(seed: int, idx: int) -> int:
    """``hash_rng`` of csrc/common.h in exact (masked) 64-bit integers."""
    z = (seed + 0x9e3779b97f4a7c15 * ((idx + 1) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M64
    return z >> 32


def _check_draw(step, B, N, H, W, pad, rank, world):
    if not (1 <= N < 2 ** 31):
        raise ValueError("draw_params: need 1 <= N < 2^31 (got %r)" % (N,))
    if B < 0 or H < 1 or W < 1 or pad < 0:
        raise ValueError("draw_params: need B >= 0, H, W >= 1 and pad >= 0")
    if step < 0 or world < 1 or not (0 <= rank < world):
        raise ValueError("draw_params: need step >= 0 and 0 <= rank < world")


def _draw_reference(seed, step, B, N, H, W, pad, rank, world, augment):
    rows = []
    for b in range(B):
        ctr = ((step * world + rank) * B + b) & _M64
        r = [hash_rng(seed, (ctr * 8 + k) & _M64) for k in range(FIELDS)]
        oy = (r[1] * (2 * pad + 1)) >> 32
        ox = (r[2] * (2 * pad + 1)) >> 32
        flip = r[3] >> 31
        if not augment:
            oy, ox, flip = pad, pad, 0
        rows.append([(r[0] * N) >> 32, oy, ox, flip,
                     (r[4] * H) >> 32, (r[5] * W) >> 32])
    return torch.tensor(rows, dtype=torch.int32).reshape(B, FIELDS)


def draw_params(seed: int, step: int, B: int, N: int, H: int, W: int,
                pad: int, labels: torch.Tensor, rank: int = 0,
                world: int = 1, device=None, augment: bool = True
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Parameters of batch ``step`` -> (``params`` int32 ``[B, 6]``,
    ``labels[index]`` int64 ``[B]``), both on ``device`` (default: where
    ``labels`` lives).

    With ``ctr = (step * world + rank) * B + b`` and ``r_k = hash_rng(seed,
    ctr * 8 + k)`` in wrapping 64-bit arithmetic: ``index = r0 * N >> 32``,
    ``oy``/``ox`` ``= r1``/``r2`` ``* (2 * pad + 1) >> 32``, ``flip = r3 >>
    31``, ``cy = r4 * H >> 32``, ``cx = r5 * W >> 32``. A pure function of its
    arguments: rank ``r`` of ``world`` at step ``s`` draws what a single
    process draws at step ``s * world + r``. ``augment=False`` still draws the
    indices but centres the crop (``oy = ox = pad``) and never flips.
    """
    seed = int(seed) & _M64
    step, B, N, H, W, pad = (int(v) for v in (step, B, N, H, W, pad))
    rank, world = int(rank), int(world)
    _check_draw(step, B, N, H, W, pad, rank, world)
    device = labels.device if device is None else torch.device(device)
    if labels.device != device:
        raise ValueError("draw_params: labels live on %s, not on %s"
                         % (labels.device, device))
    if labels.dtype != torch.int64 or labels.dim() != 1 \
            or labels.shape[0] != N:
        raise ValueError("draw_params: labels must be int64 of shape [N]")
    if device.type == "cuda":
        ext = _extension.require()
        params = torch.empty((B, FIELDS), device=device, dtype=torch.int32)
        out = torch.empty((B,), device=device, dtype=torch.int64)
        ext.augment_draw(labels.contiguous(), params, out, seed, step, rank,
                         world, N, pad, H, W, bool(augment))
        return params, out
    params = _draw_reference(seed, step, B, N, H, W, pad, rank, world,
                             bool(augment))
    return params, labels[params[:, 0].long()]


def _apply_reference(data, params, scale, shift, pad, cutout_pad):
    N, C, H, W = data.shape
    p = params.long()
    index = p[:, 0].clamp(0, N - 1)
    oy, ox, flip, cy, cx = (p[:, k].view(-1, 1) for k in range(1, FIELDS))
    y = torch.arange(H).view(1, H)
    x = torch.arange(W).view(1, W)
    sy = y + oy - pad                                    # [B, H]
    sx = torch.where(flip != 0, W - 1 - x, x) + ox - pad  # [B, W]
    keep = ((sy >= 0) & (sy < H)).unsqueeze(2) & \
        ((sx >= 0) & (sx < W)).unsqueeze(1)               # [B, H, W]
    if cutout_pad > 0:
        cut_y = (y >= (cy - cutout_pad).clamp(min=0)) & \
            (y < (cy + cutout_pad).clamp(max=H))
        cut_x = (x >= (cx - cutout_pad).clamp(min=0)) & \
            (x < (cx + cutout_pad).clamp(max=W))
        keep = keep & ~(cut_y.unsqueeze(2) & cut_x.unsqueeze(1))
    # fp32, multiply then add as two roundings (what the kernel does)
    val = data[index].float() * scale.view(1, C, 1, 1)
    val = val + shift.view(1, C, 1, 1)
    B = p.shape[0]
    rows = sy.clamp(0, H - 1).view(B, 1, H, 1).expand(B, C, H, W)
    cols = sx.clamp(0, W - 1).view(B, 1, 1, W).expand(B, C, H, W)
    val = val.gather(2, rows).gather(3, cols)
    val = torch.where(keep.unsqueeze(1), val, torch.zeros((), dtype=val.dtype))
    return val.to(torch.bfloat16)


def augment_apply(data: torch.Tensor, params: torch.Tensor,
                  scale: torch.Tensor, shift: torch.Tensor, pad: int,
                  cutout_pad: int, out: Optional[torch.Tensor] = None
                  ) -> torch.Tensor:
    """bf16 ``[B, C, H, W]`` batch from the resident ``data`` ``[N, C, H, W]``
    (uint8 or float32) and ``params`` (int32 ``[B, 6]``, see ``draw_params``).

    Crop, then flip, then cutout. For ``out[b, c, y, x]``: ``xs = W-1-x`` if
    flipped else ``x``; the source pixel is ``(y + oy - pad, xs + ox - pad)``
    of image ``index``; the pixel is cut when ``cutout_pad > 0`` and ``(y,
    x)`` lies in ``[max(0, cy-cutout_pad), min(H, cy+cutout_pad))`` x the
    same around ``cx``. A cut pixel or one whose source falls outside the
    image is exactly 0; any other is ``bf16(float(src) * scale[c] +
    shift[c])``. ``index`` is clamped to ``[0, N-1]``. ``out``, when given,
    is a contiguous bf16 tensor to fill (any alignment).
    """
    pad, cutout_pad = int(pad), int(cutout_pad)
    if data.dim() != 4 or data.dtype not in (torch.uint8, torch.float32):
        raise ValueError("augment_apply: data must be uint8 or float32 "
                         "[N, C, H, W] (got %s %s)"
                         % (data.dtype, tuple(data.shape)))
    N, C, H, W = data.shape
    if params.dim() != 2 or params.shape[1] != FIELDS \
            or params.dtype != torch.int32:
        raise ValueError("augment_apply: params must be int32 [B, 6]")
    if not (1 <= N < 2 ** 31):
        raise ValueError("augment_apply: need 1 <= N < 2^31")
    if pad < 0 or cutout_pad < 0:
        raise ValueError("augment_apply: pad and cutout_pad must be >= 0")
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.shape != (C,):
            raise ValueError("augment_apply: scale and shift must be "
                             "float32 of shape [C]")
    B = params.shape[0]
    if out is not None and (out.shape != (B, C, H, W)
                            or out.dtype != torch.bfloat16
                            or not out.is_contiguous()
                            or out.device != data.device):
        raise ValueError("augment_apply: out must be contiguous bf16 "
                         "[B, C, H, W] on the data's device")
    if data.is_cuda:
        ext = _extension.require()
        if out is None:
            out = torch.empty((B, C, H, W), device=data.device,
                              dtype=torch.bfloat16)
        ext.augment_apply(data.contiguous(), params.contiguous(),
                          scale.contiguous(), shift.contiguous(), out, pad,
                          cutout_pad)
        return out
    res = _apply_reference(data, params, scale, shift, pad, cutout_pad)
    if out is None:
        return res
    out.copy_(res)
    return out
