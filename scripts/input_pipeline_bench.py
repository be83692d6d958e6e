"""Time the image input kernel (csrc/augment.hip augment_batch) alone.

    python scripts/input_pipeline_bench.py [--out profiles/input_pipeline.txt]

B = 256, stored 256x256 uint8, out 224x224 bf16, 4096 resident images (805 MB,
random bytes), one launch per batch:
  train  a RandomResizedCrop + flip plan (data/plan.py, seed 0, epoch 0, first batch)
  eval   the central 224x224 box: the exact-copy case
Each figure is the median of 20 runs after warm-up; a run is ``inner``
back-to-back launches between two device events, divided by ``inner``.  Bytes
moved: the bf16 output plus the stored bytes inside the batch's boxes (every
byte of a box counted once; a box wider than the output skips some of them, so
this is the most the launch needs to read).  The floor is those bytes at the
copy rate README.md quotes.  The script first checks the train batch against
``augment_reference`` on 4 of its images.  Needs a GPU: no fallback.

Then the pair-mix launch (``augment_mix_batch``: Mixup, CutMix) against
``augment_batch`` on the same train plan, the three alternating run by run in
one process, after a check against ``augment_mix_reference`` on two pairs.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from kubedl_amd.data.augment import (augment_batch, augment_mix_batch, augment_mix_reference,  # noqa: E402
                                     augment_reference, norm_coeffs)
from kubedl_amd.data.plan import InputPlan  # noqa: E402
from kubedl_amd.data.shards import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402

COPY_RATE = 4.72e12  # B/s, the measured copy rate README.md quotes


def time_us(fn, inner: int = 10, runs: int = 20, warmup: int = 3):
    for _ in range(warmup * inner):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(out), min(out), max(out)


def time_alternating_us(fns: dict, inner: int = 10, runs: int = 20, warmup: int = 3):
    """``time_us`` for several launches in turn, run by run, so that all of them see the same
    stretch of the machine: {name: (median, min, max)}."""
    for fn in fns.values():
        for _ in range(warmup * inner):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def mix_section(images, labels, B, O, A, Bc, x, y, lines) -> None:
    """augment_mix_batch (Mixup, CutMix) against augment_batch on the same train plan, alternating;
    the three launches move the same bytes.  Checked first against augment_mix_reference on the
    images of two pairs."""
    dev, N, S = images.device, images.shape[0], images.shape[1]
    rows = InputPlan(N, S, S, 1, 0, B, seed=0, train=True).epoch(0).rows
    d_rows = torch.from_numpy(rows).to(dev)
    yb = torch.empty_like(y)
    mixes = {"mixup": (1, 19661, (0, 0, 0, 0)), "cutmix": (2, 65536, (37, 60, 120, 131))}
    k = [0, 1, B - 2, B - 1]  # two whole pairs
    sub = rows[k].copy()
    sub_img = images[torch.from_numpy(sub[:, 0].astype(np.int64)).to(dev)].cpu()
    sub[:, 0] = np.arange(len(k))
    for name, (kind, lam16, box) in mixes.items():
        augment_mix_batch(images, labels, d_rows, 0, B, O, O, A, Bc, kind, lam16, box, x, y, yb)
        xr = augment_mix_reference(sub_img, torch.zeros(len(k), dtype=torch.int64), torch.from_numpy(sub), O, O,
                                   IMAGENET_MEAN, IMAGENET_STD, kind, lam16, box)[0]
        assert torch.equal(x[k].permute(0, 2, 3, 1).contiguous().cpu().view(torch.int16),
                           xr.permute(0, 2, 3, 1).contiguous().view(torch.int16)), \
            f"{name}: kernel differs from augment_mix_reference"
    fns = {"plain": lambda: augment_batch(images, labels, d_rows, 0, B, O, O, A, Bc, x, y)}
    for name, (kind, lam16, box) in mixes.items():
        fns[name] = (lambda kind=kind, lam16=lam16, box=box:
                     augment_mix_batch(images, labels, d_rows, 0, B, O, O, A, Bc, kind, lam16, box, x, y, yb))
    res = time_alternating_us(fns)
    lines.append("augment_mix_batch against augment_batch, train plan, alternating run by run (same bytes moved)")
    for name, (med, lo, hi) in res.items():
        lines.append(f"{name:6s} {med:8.1f} us [{lo:.1f} .. {hi:.1f}]  {med / res['plain'][0]:.2f}x of plain")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    N, B, S, O = a.images, a.batch, 256, 224
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (N, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    labels = torch.randint(0, 1000, (N,), generator=g, device=dev)
    A, Bc = norm_coeffs(IMAGENET_MEAN, IMAGENET_STD)
    x = torch.empty(B, O, O, 3, dtype=torch.bfloat16, device=dev).permute(0, 3, 1, 2)
    y = torch.empty(B, dtype=torch.int64, device=dev)
    lines = [f"augment_batch alone: B={B}, stored {S}x{S} uint8 ({N} resident images), out {O}x{O} bf16, "
             f"{torch.cuda.get_device_name(dev)}",
             "median of 20 runs of 10 back-to-back launches (device events), us per launch [min .. max]"]
    for name, train in (("train", True), ("eval", False)):
        rows = InputPlan(N, S, S, 1, 0, B, seed=0, train=train).epoch(0).rows
        d_rows = torch.from_numpy(rows).to(dev)
        augment_batch(images, labels, d_rows, 0, B, O, O, A, Bc, x, y)
        k = [0, 1, B // 2, B - 1]
        sub = rows[k].copy()
        sub_img = images[torch.from_numpy(sub[:, 0].astype(np.int64)).to(dev)].cpu()
        sub[:, 0] = np.arange(len(k))
        xr, _ = augment_reference(sub_img, torch.zeros(len(k), dtype=torch.int64), torch.from_numpy(sub), O, O,
                                  IMAGENET_MEAN, IMAGENET_STD)
        assert torch.equal(x[k].permute(0, 2, 3, 1).contiguous().cpu().view(torch.int16),
                           xr.permute(0, 2, 3, 1).contiguous().view(torch.int16)), \
            f"{name}: kernel differs from augment_reference"
        med, lo, hi = time_us(lambda: augment_batch(images, labels, d_rows, 0, B, O, O, A, Bc, x, y))
        wr = B * O * O * 3 * 2
        rd = int((rows[:B, 3].astype(np.int64) * rows[:B, 4] * 3).sum())
        floor = (wr + rd) / COPY_RATE * 1e6
        lines.append(f"{name:5s} {med:8.1f} us [{lo:.1f} .. {hi:.1f}]  writes {wr / 1e6:.1f} MB + box reads "
                     f"{rd / 1e6:.1f} MB = {(wr + rd) / 1e6:.1f} MB  floor at 4.72 TB/s {floor:.1f} us  "
                     f"ratio {med / floor:.2f}x  ({(wr + rd) / med / 1e6:.2f} TB/s)")
    mix_section(images, labels, B, O, A, Bc, x, y, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
