"""Time StreamingAUC.update (csrc/ctr_eval.hip auc_accumulate) against two baselines.

    python scripts/ctr_auc_bench.py [--out profiles/ctr_auc_bench.txt]

At N = 4096 and N = 4,194,304 rows (logits randn * 2, 30 % positives):
  kernel    StreamingAUC.update on the HIP kernel
  fallback  the torch composition of the same integers (view-as-int32 keys +
            bincount), run on the GPU
  sort      an exact tie-aware AUC by torch.sort (average ranks), all on the
            device, no host read
Each figure is the median of 20 runs after warm-up; a run is ``inner``
back-to-back calls between two device events, divided by ``inner`` (a single
4096-row call is shorter than the events resolve).  The script first checks
that kernel and fallback hold the same histogram.  Needs a GPU: no fallback.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from kubedl_amd.ops.auc import StreamingAUC  # noqa: E402

COPY_RATE = 4.72e12  # B/s, the measured copy rate README.md quotes


def sort_auc_u2(logit: torch.Tensor, y: torch.Tensor):
    """(U2, P, N) of the exact tie-aware AUC on the device: 2 x average rank of every row."""
    n = logit.numel()
    v, order = torch.sort(logit)
    pos = y[order] > 0.5
    idx = torch.arange(n, device=logit.device)
    edge = v[1:] != v[:-1]
    t = torch.ones(1, dtype=torch.bool, device=logit.device)
    first = torch.cummax(torch.where(torch.cat([t, edge]), idx, torch.zeros_like(idx)), 0).values
    last_at = torch.where(torch.cat([edge, t]), idx, torch.full_like(idx, n - 1))
    last = torch.flip(torch.cummin(torch.flip(last_at, (0,)), 0).values, (0,))
    p = pos.sum()
    u2 = torch.where(pos, first + last + 2, torch.zeros_like(idx)).sum() - p * (p + 1)
    return u2, p, n - p


def time_ms(fn, inner: int, runs: int = 20, warmup: int = 3):
    for _ in range(warmup):
        for _ in range(inner):
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
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out), min(out), max(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ctr_auc_bench needs a GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(dev)}; median (min-max) of 20 runs, ms per call")
    for n, inner in ((4096, 50), (4_194_304, 4)):
        g = torch.Generator(device=dev).manual_seed(n)
        logit = torch.randn(n, generator=g, device=dev) * 2
        y = (torch.rand(n, generator=g, device=dev) < 0.3).float()
        kern, fall = StreamingAUC(dev), StreamingAUC(dev, use_kernel=False)
        kern.update(logit, y)
        fall.update(logit, y)
        same = bool(torch.equal(kern.hist, fall.hist)) and bool(torch.equal(kern.invalid, fall.invalid))
        u2, p, q = (int(v) for v in sort_auc_u2(logit, y))
        ku2, kp, kq = kern.counts()
        bound = int((kern.hist[0] * kern.hist[1]).sum())
        say(f"N={n}: kernel == fallback histogram: {same}; auc bucketed {ku2 / (2 * kp * kq):.9f} exact "
            f"{u2 / (2 * p * q):.9f}; |dU2| {abs(ku2 - u2)} <= bound {bound}: {abs(ku2 - u2) <= bound}")
        if not same or (kp, kq) != (p, q) or abs(ku2 - u2) > bound:
            say("MISMATCH")
            return 1
        res = {"kernel": time_ms(lambda: kern.update(logit, y), inner),
               "fallback": time_ms(lambda: fall.update(logit, y), inner),
               "sort": time_ms(lambda: sort_auc_u2(logit, y), inner)}
        floor_ms = n * 8 / COPY_RATE * 1e3
        for name, (med, lo, hi) in res.items():
            say(f"N={n} {name:8s} {med:9.4f} ms ({lo:.4f}-{hi:.4f})  {n / med / 1e6:9.2f} G rows/s"
                f"  x{med / res['kernel'][0]:.2f} of kernel")
        say(f"N={n} byte floor {floor_ms:.5f} ms ({n * 8 / 1e6:.2f} MB read per call at {COPY_RATE / 1e12:.2f} TB/s);"
            f" kernel at {res['kernel'][0] / floor_ms:.1f}x the floor")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
