"""Order and augmentation parameters of the image input, decided on the host.

Everything random about the input is drawn here, once per epoch, into an int32
table ``[rows, 8]`` with the columns ``src, y0, x0, h, w, flip, 0, 0``; the
kernel (csrc/augment.hip) and the CPU path (data/augment.py) are pure functions
of that table.

Ownership: image ``i`` of the set belongs to rank ``i % world``; ``src`` is the
index within the rank's owned partition (global index ``rank + src * world``).

Train order: ``steps_per_epoch = (N // world) // batch`` -- the smallest owned
count over the ranks, drop-last -- is a function of ``N``, ``world`` and
``batch`` alone, so every rank computes the same value without a collective.
Epoch ``e`` of rank ``r`` uses ``numpy.random.Generator(PCG64([seed, e, r]))``:
first the permutation of the owned images, then the boxes, then the flips.
Step ``s`` reads epoch ``s // steps_per_epoch``, rows
``(s % steps_per_epoch) * batch ...``.

Determinism and resume: the batch of step ``s`` is a pure function of
``(seed, s, rank, world, batch)`` (and the set's size).  A rank restarted under
the ExitCode policy that resumes at ``done`` optimizer steps therefore reads
exactly the batches the uninterrupted job would have read, with no input state
in the checkpoint.

Train boxes follow torchvision's ``RandomResizedCrop`` rule: area scale uniform
in (0.08, 1), aspect ratio log-uniform in (3/4, 4/3), up to 10 tries, else the
central crop at the clamped ratio; drawn vectorised.  ``flip`` is
Bernoulli(0.5).  The eval plan is the natural order, no flip, the central
``round(0.875 H) x round(0.875 W)`` box (256 stored, 224 out: an exact copy),
``n_own // batch`` full batches, the remainder dropped (``eval_dropped``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

SCALE = (0.08, 1.0)
RATIO = (3.0 / 4.0, 4.0 / 3.0)
TRIES = 10
EVAL_CROP = 0.875


def owned_count(N: int, world: int, rank: int) -> int:
    """Images ``i`` of ``range(N)`` with ``i % world == rank``."""
    return (N - rank + world - 1) // world if rank < N else 0


def steps_per_epoch(N: int, world: int, batch: int) -> int:
    """Drop-last steps of a training epoch: the minimum over ranks of ``n_own // batch``."""
    return (N // world) // batch


@dataclass
class EpochPlan:
    rows: np.ndarray  # int32 [rows, 8]: src, y0, x0, h, w, flip, 0, 0
    n_own: int
    height: int
    width: int

    def validate(self) -> "EpochPlan":
        """Raise ``ValueError`` unless every row is safe to hand to the kernel."""
        r = self.rows
        if not isinstance(r, np.ndarray) or r.dtype != np.int32 or r.ndim != 2 or r.shape[1] != 8:
            raise ValueError(f"plan: int32 [rows, 8] expected, got {getattr(r, 'dtype', None)} "
                             f"{getattr(r, 'shape', None)}")
        src, y0, x0, h, w, flip = (r[:, i].astype(np.int64) for i in range(6))

        def check(ok, what):
            if not ok.all():
                i = int(np.flatnonzero(~ok)[0])
                raise ValueError(f"plan row {i} {r[i, :6].tolist()}: {what}")
        check((src >= 0) & (src < self.n_own), f"src outside [0, {self.n_own})")
        check((h >= 1) & (w >= 1), "empty box (h, w >= 1)")
        check((y0 >= 0) & (x0 >= 0) & (y0 + h <= self.height) & (x0 + w <= self.width),
              f"box outside the {self.height}x{self.width} image")
        check((flip == 0) | (flip == 1), "flip not 0 or 1")
        return self


def fallback_box(H: int, W: int):
    """torchvision's fallback: the central crop at the ratio clamped to RATIO."""
    in_ratio = W / H
    if in_ratio < RATIO[0]:
        w = W
        h = min(H, int(round(w / RATIO[0])))
    elif in_ratio > RATIO[1]:
        h = H
        w = min(W, int(round(h * RATIO[1])))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def random_boxes(rng: np.random.Generator, n: int, H: int, W: int) -> np.ndarray:
    """``n`` RandomResizedCrop boxes (y0, x0, h, w) of an ``H x W`` image, int64 [n, 4]."""
    area = float(H * W)
    scale = rng.uniform(SCALE[0], SCALE[1], size=(n, TRIES))
    ratio = np.exp(rng.uniform(math.log(RATIO[0]), math.log(RATIO[1]), size=(n, TRIES)))
    uy = rng.random(n)
    ux = rng.random(n)
    w = np.rint(np.sqrt(area * scale * ratio)).astype(np.int64)
    h = np.rint(np.sqrt(area * scale / ratio)).astype(np.int64)
    ok = (w >= 1) & (w <= W) & (h >= 1) & (h <= H)
    first = np.argmax(ok, axis=1)  # first try that fits (0 when none does)
    any_ok = ok.any(axis=1)
    rows = np.arange(n)
    h, w = h[rows, first], w[rows, first]
    y0 = np.minimum((uy * (H - h + 1)).astype(np.int64), H - h)
    x0 = np.minimum((ux * (W - w + 1)).astype(np.int64), W - w)
    fy, fx, fh, fw = fallback_box(H, W)
    out = np.stack([np.where(any_ok, y0, fy), np.where(any_ok, x0, fx), np.where(any_ok, h, fh),
                    np.where(any_ok, w, fw)], axis=1)
    return out


def eval_box(H: int, W: int):
    h = min(H, max(1, int(round(EVAL_CROP * H))))
    w = min(W, max(1, int(round(EVAL_CROP * W))))
    return (H - h) // 2, (W - w) // 2, h, w


class InputPlan:
    """The plans of one rank over one set: ``epoch(e)`` is the validated table of
    epoch ``e``, ``locate(step)`` says where a step's batch lies in it."""

    def __init__(self, count: int, height: int, width: int, world: int, rank: int, batch: int, seed: int = 0,
                 train: bool = True):
        if not (0 <= rank < world) or batch < 1:
            raise ValueError(f"InputPlan: rank {rank} of world {world}, batch {batch}")
        self.count, self.height, self.width = int(count), int(height), int(width)
        self.world, self.rank, self.batch, self.seed, self.train = int(world), int(rank), int(batch), int(seed), train
        self.n_own = owned_count(self.count, self.world, self.rank)
        if train:
            self.steps_per_epoch = steps_per_epoch(self.count, self.world, self.batch)
            self.dropped = self.n_own - self.steps_per_epoch * self.batch
        else:
            self.steps_per_epoch = self.n_own // self.batch
            self.dropped = self.n_own - self.steps_per_epoch * self.batch

    def global_index(self, src) -> np.ndarray:
        """Set-wide image indices of owned indices ``src``."""
        return self.rank + np.asarray(src, dtype=np.int64) * self.world

    def locate(self, step: int):
        """(epoch, first row) of step ``step``'s batch."""
        if self.steps_per_epoch < 1:
            raise ValueError(f"InputPlan: no full batch of {self.batch} in {self.n_own} owned images "
                             f"({self.count} images over {self.world} ranks)")
        return step // self.steps_per_epoch, (step % self.steps_per_epoch) * self.batch

    def epoch(self, e: int) -> EpochPlan:
        nrows = self.steps_per_epoch * self.batch
        rows = np.zeros((nrows, 8), np.int32)
        if self.train:
            rng = np.random.Generator(np.random.PCG64([self.seed, int(e), self.rank]))
            rows[:, 0] = rng.permutation(self.n_own)[:nrows]
            rows[:, 1:5] = random_boxes(rng, nrows, self.height, self.width)
            rows[:, 5] = rng.random(nrows) < 0.5
        else:
            rows[:, 0] = np.arange(nrows)
            rows[:, 1:5] = eval_box(self.height, self.width)
        return EpochPlan(rows, self.n_own, self.height, self.width).validate()

    def batch_rows(self, step: int) -> np.ndarray:
        """The ``[batch, 8]`` rows of step ``step`` (a fresh epoch table each call:
        for tests and the per-batch path; ``ShardInput`` caches the epoch)."""
        e, r0 = self.locate(step)
        return self.epoch(e).rows[r0:r0 + self.batch]
