"""Streaming AUC for the XDLJob data plane (csrc/ctr_eval.hip).

The metric click-through models are judged by, in the form this data plane
needs: sync-free (``update`` enqueues one kernel, like the training step),
mergeable across workers (the state is an integer histogram: an int64 SUM
all-reduce) and bit-reproducible (integer sums do not depend on arrival
order).  A sort-based AUC is none of the three.

Bucket key of an fp32 logit: ``-0.0`` becomes ``+0.0``; with ``b`` the 32-bit
pattern, ``m = ~b`` if the sign bit is set, else ``b | 0x80000000``;
``key = m >> 16`` in [0, 65535] -- a non-decreasing function of the logit
(1.0 -> 49024).  NaN logits count in ``invalid`` and nowhere else.  A row is
positive when ``y > 0.5``.

State: ``hist`` int64 [2, 65536] (row 0 negatives, row 1 positives),
``invalid`` int64 [1].  Statistic: ``U2 = sum_b neg[b] * (2 * sum_{c>b} pos[c]
+ pos[b])``, ``auc = U2 / (2 P N)`` -- the exact tie-aware Mann-Whitney AUC of
the bucketed scores.  Against the exact AUC of the fp32 logits
``|dU2| <= sum_b pos[b] * neg[b]``: only pairs sharing a bucket can differ,
each by at most 1 in U2 units.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.distributed as dist

from kubedl_amd.ops import _ext

BUCKETS = 65536


def bucket_keys(logit: torch.Tensor) -> torch.Tensor:
    """int64 bucket key of every fp32 logit (NaN rows get a key too: mask them)."""
    x = logit.float()
    x = torch.where(x == 0, torch.zeros_like(x), x)  # -0 ties with +0
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    m = torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)
    return m >> 16


def auc_from_counts(u2: int, p: int, n: int) -> float:
    if p == 0 or n == 0:
        return float("nan")
    return u2 / (2 * p * n)  # Python ints: the correctly rounded float64 quotient


class StreamingAUC:
    """``update`` rows as they are scored, ``merge`` across workers, ``compute``."""

    def __init__(self, device, use_kernel: Optional[bool] = None):
        """``use_kernel``: None = the HIP kernel on a GPU (a missing extension is
        an error there), the torch composition on CPU; False forces the torch
        composition (the benchmark's baseline; the same integers)."""
        self.device = torch.device(device)
        if use_kernel is None:
            use_kernel = self.device.type == "cuda"
            if use_kernel and not _ext.available():
                _ext.require_on_gpu("StreamingAUC")
                use_kernel = False
        self.use_kernel = bool(use_kernel)
        self.hist = torch.zeros(2, BUCKETS, dtype=torch.int64, device=self.device)
        self.invalid = torch.zeros(1, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------ update
    def update(self, logit: torch.Tensor, y: torch.Tensor) -> None:
        """Add rows (logit [n], y [n]); no host synchronisation on the kernel path."""
        logit = logit.detach().reshape(-1)
        y = y.detach().reshape(-1)
        if logit.numel() != y.numel():
            raise ValueError(f"StreamingAUC.update: {logit.numel()} logits, {y.numel()} labels")
        if logit.dtype != torch.float32:
            logit = logit.float()
        if y.dtype != torch.float32:
            y = y.float()
        logit, y = logit.contiguous(), y.contiguous()
        if self.use_kernel:
            _ext.load().auc_accumulate(logit, y, self.hist, self.invalid)
            return
        self._update_torch(logit, y)

    def _update_torch(self, logit: torch.Tensor, y: torch.Tensor) -> None:
        if logit.numel() == 0:
            return
        valid = logit == logit
        key = bucket_keys(logit) + (y > 0.5).to(torch.int64) * BUCKETS
        # NaN rows land in one extra bin past the histogram
        idx = torch.where(valid, key, torch.full_like(key, 2 * BUCKETS))
        counts = torch.bincount(idx, minlength=2 * BUCKETS + 1)
        self.hist += counts[: 2 * BUCKETS].view(2, BUCKETS)
        self.invalid += counts[2 * BUCKETS:]

    # ------------------------------------------------------------ merge / compute
    def merge(self, group=None) -> None:
        """Sum the state over the ranks of ``group`` (gloo or RCCL): afterwards every
        rank holds the statistics of all rows."""
        if not (dist.is_available() and dist.is_initialized()):
            return
        dist.all_reduce(self.hist, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.invalid, op=dist.ReduceOp.SUM, group=group)

    def counts(self):
        """(U2, P, N) as Python ints (synchronises)."""
        if self.use_kernel:
            u2, p, n = (int(v) for v in _ext.load().auc_finalize(self.hist).tolist())
        else:
            neg, pos = self.hist[0], self.hist[1]
            p, n = int(pos.sum()), int(neg.sum())
            u2 = None
        if p >= 1 << 31 or n >= 1 << 31:
            raise OverflowError(f"StreamingAUC.compute: {p} positives / {n} negatives: U2 needs both < 2^31 "
                                "to fit 64 bits; merge fewer rows per state")
        if u2 is None:
            above = torch.flip(torch.cumsum(torch.flip(pos, (0,)), 0), (0,)) - pos  # positives in higher buckets
            u2 = int((neg * (2 * above + pos)).sum())
        return u2, p, n

    def compute(self) -> Dict[str, object]:
        u2, p, n = self.counts()
        return {"auc": auc_from_counts(u2, p, n), "pos": p, "neg": n, "invalid": int(self.invalid.item())}

    # ------------------------------------------------------------ state
    def reset(self) -> None:
        self.hist.zero_()
        self.invalid.zero_()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"hist": self.hist.clone(), "invalid": self.invalid.clone()}

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        hist, invalid = state["hist"], state["invalid"]
        if tuple(hist.shape) != (2, BUCKETS) or hist.dtype != torch.int64 or invalid.numel() != 1:
            raise ValueError("StreamingAUC.load_state_dict: hist int64 [2, 65536] and invalid int64 [1]")
        self.hist.copy_(hist)
        self.invalid.copy_(invalid.reshape(1).to(torch.int64))
