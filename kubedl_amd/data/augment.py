"""The image input's resample rule on torch ops: the CPU path and the numerics
reference of ``csrc/augment.hip`` (the pattern of ``predict_margin`` and the
engine's torch backend).

For an output of ``OH x OW``, a box ``(y0, x0, h, w)`` and output column ``ox``
(with flip, ``ox := OW-1-ox`` first):

    d  = 2*OW
    n  = clamp((2*ox+1)*w - OW, 0, (w-1)*d)
    xl = n // d
    wx = ((n % d)*256 + OW) // d          # 0..256
    xr = min(xl+1, w-1)

Rows alike with ``OH, h`` (never flipped).  Per channel, with ``a, b`` the stored
bytes at ``(y0+yl, x0+xl)``, ``(y0+yl, x0+xr)``:

    top = a*(256-wx) + b*wx;  bot likewise on row y0+yh
    q   = (top*(256-wy) + bot*wy + 32768) >> 16          # 0..255

and ``x[b, c, oy, ox] = bf16(fma(float(q), A[c], B[c]))`` with
``A = fp32(1/std)``, ``B = fp32(-mean/std)`` computed in fp64.  The reference
evaluates ``q*A + B`` in fp64 -- exact for 8-bit ``q`` and fp32 ``A, B`` of
comparable magnitude -- and rounds once to fp32, as the fma does.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch


def norm_coeffs(mean: Sequence[float], std: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """``A = fp32(1/std)``, ``B = fp32(-mean/std)`` from fp64 (mean, std in 0..255 units)."""
    m = np.asarray(mean, np.float64)
    s = np.asarray(std, np.float64)
    if m.shape != (3,) or s.shape != (3,) or not (s > 0).all():
        raise ValueError(f"norm_coeffs: three means and three positive stds, got {mean!r}, {std!r}")
    return (1.0 / s).astype(np.float32), (-m / s).astype(np.float32)


def axis_table(out: int, start: torch.Tensor, length: torch.Tensor, flip: torch.Tensor | None = None):
    """(lo, hi, weight) int64 [B, out]: stored indices ``start + lo``, ``start + hi``
    and the 0..256 weight of ``hi`` for each output index."""
    o = torch.arange(out, dtype=torch.int64, device=start.device)[None, :].expand(start.numel(), out)
    if flip is not None:
        o = torch.where(flip[:, None] != 0, out - 1 - o, o)
    ln = length[:, None]
    d = 2 * out
    n = torch.minimum(((2 * o + 1) * ln - out).clamp_min(0), (ln - 1) * d)
    lo = n // d
    wgt = ((n % d) * 256 + out) // d
    hi = torch.minimum(lo + 1, ln - 1)
    return start[:, None] + lo, start[:, None] + hi, wgt


def resample_q(images_u8: torch.Tensor, plan_rows: torch.Tensor, OH: int, OW: int) -> torch.Tensor:
    """The integer bilinear samples ``q`` int64 [B, OH, OW, 3] of ``plan_rows`` int [B, 8]."""
    p = plan_rows.to(device=images_u8.device, dtype=torch.int64)
    src, y0, x0, h, w, flip = (p[:, i] for i in range(6))
    yl, yh, wy = axis_table(OH, y0, h)
    xl, xr, wx = axis_table(OW, x0, w, flip)
    s = src[:, None, None]

    def tap(ys, xs):
        return images_u8[s, ys[:, :, None], xs[:, None, :]].to(torch.int64)  # [B, OH, OW, 3]
    wxe, wye = wx[:, None, :, None], wy[:, :, None, None]
    top = tap(yl, xl) * (256 - wxe) + tap(yl, xr) * wxe
    bot = tap(yh, xl) * (256 - wxe) + tap(yh, xr) * wxe
    return (top * (256 - wye) + bot * wye + 32768) >> 16


def normalize_q(q: torch.Tensor, mean, std) -> torch.Tensor:
    """``bf16(fp32(q*A + B))`` over the last (channel) dimension, the product and sum in fp64."""
    A, B = norm_coeffs(mean, std)
    A = torch.from_numpy(A).to(q.device).double()
    B = torch.from_numpy(B).to(q.device).double()
    return (q.double() * A + B).float().bfloat16()


def augment_reference(images_u8: torch.Tensor, labels: torch.Tensor, plan_rows, OH: int, OW: int, mean, std):
    """``(x bf16 [B, 3, OH, OW] channels_last, y int64 [B])`` of ``plan_rows``
    (int [B, 8]: src, y0, x0, h, w, flip, 0, 0) over ``images_u8`` uint8 [n, H, W, 3]."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.size(3) != 3:
        raise ValueError(f"augment_reference: images uint8 [n, H, W, 3], got {images_u8.dtype} "
                         f"{tuple(images_u8.shape)}")
    plan_rows = torch.as_tensor(plan_rows)
    x = normalize_q(resample_q(images_u8, plan_rows, OH, OW), mean, std)  # [B, OH, OW, 3]
    src = plan_rows[:, 0].to(device=labels.device, dtype=torch.int64)
    return x.permute(0, 3, 1, 2), labels[src].to(torch.int64)


def augment_batch(images_u8, labels, plan, row0: int, B: int, OH: int, OW: int, A, Bc, x, y) -> None:
    """The HIP path: one launch of ``kdl::augment_batch`` on the current stream."""
    from kubedl_amd.ops import _ext
    _ext.load().augment_batch(images_u8, labels, plan, int(row0), int(B), int(OH), int(OW),
                              [float(v) for v in A], [float(v) for v in Bc], x, y)
