"""Learning rate as a pure function of the step index (host only).

The trainer sets ``opt.lr = lr_at(step, ...)`` before each optimizer launch; the fused
optimizers take the rate as a kernel argument, so a schedule costs no device write or
sync, and a restarted job resumes on the right rate with nothing in the checkpoint.
"""
from __future__ import annotations

import math

KINDS = ("constant", "poly", "cosine")


def lr_at(step: int, *, peak: float, kind: str = "constant", warmup_steps: int = 0, total_steps: int = 0,
          end_lr: float = 0.0, power: float = 2.0) -> float:
    """Rate of 0-based step ``step``.

    Steps ``0 .. warmup_steps - 1`` warm up linearly: ``peak * (step + 1) / warmup_steps``, so step 0 has
    ``peak / warmup_steps`` and the last warm-up step has ``peak``.  The decay then runs over the remaining
    ``total_steps - warmup_steps`` steps with ``f = (step - warmup_steps) / (total_steps - warmup_steps)``
    (0 at the first decay step, clamped to 1 from ``total_steps`` on):

    * ``constant``: ``peak``;
    * ``poly``:     ``end_lr + (peak - end_lr) * (1 - f) ** power`` (power 2: the MLPerf LARS recipe);
    * ``cosine``:   ``end_lr + (peak - end_lr) * (1 + cos(pi * f)) / 2``.
    """
    if kind not in KINDS:
        raise ValueError(f"lr schedule kind {kind!r}: one of {KINDS}")
    if step < warmup_steps:
        return peak * (step + 1) / warmup_steps
    if kind == "constant":
        return peak
    span = total_steps - warmup_steps
    f = min((step - warmup_steps) / span, 1.0) if span > 0 else 1.0
    if kind == "poly":
        return end_lr + (peak - end_lr) * (1.0 - f) ** power
    return end_lr + (peak - end_lr) * 0.5 * (1.0 + math.cos(math.pi * f))
