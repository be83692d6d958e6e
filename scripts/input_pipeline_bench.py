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
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from kubedl_amd.data.augment import augment_batch, augment_reference, norm_coeffs  # noqa: E402
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
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
