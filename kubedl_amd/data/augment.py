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

Mixup and CutMix (``augment_mix_reference``, the kernel ``augment_mix_batch``)
-------------------------------------------------------------------------------
Output image ``i`` is paired with image ``j = B-1-i`` of the same per-rank batch
(for odd ``B`` the middle image pairs with itself).  A step has one ``kind`` in
{0 none, 1 mixup, 2 cutmix}, one ``lam`` and, for CutMix, one box; they are drawn
on the host (``data/plan.py``: ``InputPlan.mix_draw``), a pure function of
(seed, step, rank).

Mixup acts on the integer samples ``q`` above, before the normalisation (which is
affine, so this is the mix of the normalised images):

    lam16 = clamp(round(lam * 65536), 0, 65536)
    m     = lam16 * q_i + (65536 - lam16) * q_j          # <= 255 * 65536 < 2^24
    x     = bf16(fma(float(m), A16[c], B[c])),   A16 = A * 2^-16 (an exact scaling)

``float(m)`` is exact.  The reference evaluates ``m * A16 + B`` in fp64 and rounds
once to fp32: ``m`` is an integer below 2^24 and ``A16`` has 24 significant bits,
so the product is exact in fp64 and spans at most 48 bits above ``ulp(A16)`` -- for
every std <= 255 (``A >= 2^-8``) that lowest bit is 2^-47 or above, and for the
ImageNet statistics the value stays below 2^3.  ``B`` is, as above, of comparable
magnitude (``|B| <= 255 A``, its own lowest bit at or above the product's), so the
sum has one carry bit more, 49 of fp64's 53: the fp64 value is exact, and its
single rounding is the fma's.  With ``lam16 = 65536``,
``m * A16 = q_i * A`` exactly, so the result is bit-equal to the unmixed image.

CutMix: one box ``(cy0, cx0, ch, cw)`` in output coordinates, centre uniform over
the output, sides ``round(OH sqrt(1 - lam))`` and ``round(OW sqrt(1 - lam))``,
clipped to the image (``plan.cutmix_box``).  Inside the box, pixel ``(oy, ox)`` of
output ``i`` is the augmented pixel ``(oy, ox)`` of image ``j`` (its own crop and
flip); outside it is image ``i``'s own: a pure select, every value bit-equal to a
value of the two unmixed images.

Labels: ``y_a = labels[src_i]``, ``y_b = labels[src_j]`` and one fp32 ``lam_label``
per step: Mixup ``lam16 / 65536`` (exact), CutMix the clipped box's weight
``fp32(1 - ch*cw / (OH*OW))`` from fp64, kind none 1.  The loss of an image is
``lam_label * CE(y_a) + (1 - lam_label) * CE(y_b)`` (csrc/head.hip, with label
smoothing composed per term).
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


def mix_lam_label(kind: int, lam16: int, box, OH: int, OW: int) -> float:
    """The step's label weight as an fp32 value: Mixup ``lam16 / 65536``, CutMix
    ``fp32(1 - ch*cw / (OH*OW))`` of the clipped box, kind none 1."""
    if kind == 1:
        return float(np.float32(lam16 / 65536.0))
    if kind == 2:
        return float(np.float32(1.0 - (int(box[2]) * int(box[3])) / float(OH * OW)))
    return 1.0


def check_mix(kind: int, lam16: int, box, OH: int, OW: int) -> None:
    cy0, cx0, ch, cw = (int(v) for v in box)
    if kind not in (0, 1, 2) or not 0 <= lam16 <= 65536:
        raise ValueError(f"mix: kind 0, 1 or 2 and lam16 in [0, 65536], got kind {kind}, lam16 {lam16}")
    if min(cy0, cx0, ch, cw) < 0 or cy0 + ch > OH or cx0 + cw > OW:
        raise ValueError(f"mix: box {(cy0, cx0, ch, cw)} outside the {OH}x{OW} output")


def augment_mix_reference(images_u8: torch.Tensor, labels: torch.Tensor, plan_rows, OH: int, OW: int, mean, std,
                          kind: int, lam16: int = 65536, box=(0, 0, 0, 0)):
    """``(x, y_a, y_b, lam_label)`` of the module docstring's Mixup / CutMix rule: ``x``
    bf16 [B, 3, OH, OW] channels_last with image ``i`` mixed with image ``B-1-i``,
    ``y_a = labels[src_i]``, ``y_b = labels[src_{B-1-i}]``, ``lam_label`` a float."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.size(3) != 3:
        raise ValueError(f"augment_mix_reference: images uint8 [n, H, W, 3], got {images_u8.dtype} "
                         f"{tuple(images_u8.shape)}")
    check_mix(kind, lam16, box, OH, OW)
    plan_rows = torch.as_tensor(plan_rows)
    q = resample_q(images_u8, plan_rows, OH, OW)  # [B, OH, OW, 3]
    qj = q.flip(0)
    if kind == 2:
        cy0, cx0, ch, cw = (int(v) for v in box)
        inside = torch.zeros(OH, OW, dtype=torch.bool, device=q.device)
        inside[cy0:cy0 + ch, cx0:cx0 + cw] = True
        l = torch.where(inside, 0, 65536)[None, :, :, None]
    else:
        l = lam16 if kind == 1 else 65536
    m = l * q + (65536 - l) * qj
    A, Bc = norm_coeffs(mean, std)
    A16 = torch.from_numpy(np.ldexp(A, -16)).to(q.device).double()
    x = (m.double() * A16 + torch.from_numpy(Bc).to(q.device).double()).float().bfloat16()
    src = plan_rows[:, 0].to(device=labels.device, dtype=torch.int64)
    y = labels[src].to(torch.int64)
    return x.permute(0, 3, 1, 2), y, y.flip(0), mix_lam_label(kind, lam16, box, OH, OW)


def augment_mix_batch(images_u8, labels, plan, row0: int, B: int, OH: int, OW: int, A, Bc, kind: int, lam16: int,
                      box, x, y_a, y_b) -> None:
    """The HIP path: one launch of ``kdl::augment_mix_batch`` on the current stream."""
    from kubedl_amd.ops import _ext
    _ext.load().augment_mix_batch(images_u8, labels, plan, int(row0), int(B), int(OH), int(OW),
                                  [float(v) for v in A], [float(v) for v in Bc], int(kind), int(lam16),
                                  [int(v) for v in box], x, y_a, y_b)


def augment_batch(images_u8, labels, plan, row0: int, B: int, OH: int, OW: int, A, Bc, x, y) -> None:
    """The HIP path: one launch of ``kdl::augment_batch`` on the current stream."""
    from kubedl_amd.ops import _ext
    _ext.load().augment_batch(images_u8, labels, plan, int(row0), int(B), int(OH), int(OW),
                              [float(v) for v in A], [float(v) for v in Bc], x, y)
