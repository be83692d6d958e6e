"""Evaluation rate of ResNet-50 on one GPU, against the two alternatives.

Times, alternating within one process, ``--repeats`` times each (median reported):

* ``eval``     ``ResNetTrainer.evaluate`` over ``--batches`` held-out batches (the inference forward with
               BatchNorm folded into the conv epilogues + the evaluation head);
* ``train_fwd`` the engine's training ``forward()`` over as many batches (batch statistics, every activation
               kept): the inference forward does strictly less work, so it must not be slower;
* ``autograd`` the autograd module in ``eval()`` under ``no_grad`` (MIOpen convs): the only way to evaluate
               before.

Each timed region is preceded by ``--warmup`` batches of the same kind and bracketed by device synchronisations.
Also prints the bytes one inference forward must move (every activation written once and read once, plus the
weights and the input) and the share of the measured copy rate (``--copy-tbs``) the measured time corresponds to.

    python scripts/eval_rate.py --batch 256 > profiles/eval_rate_b256.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def infer_bytes(model, batch: int, image: int) -> dict:
    """HBM bytes of one inference forward computed from the shapes: the input read once, every activation
    (bf16) written once and read once, every weight (bf16) and coefficient table (fp32) read once."""
    act = 0
    h = (image - 1) // 2 + 1
    act += batch * h * h * 64        # stem conv output
    h = (h - 1) // 2 + 1
    act += batch * h * h * 64        # pooled stem output
    for blk in model.layers:
        s = blk.conv2.stride[0]
        w, out = blk.conv1.out_channels, blk.conv3.out_channels
        act += batch * h * h * w     # a1
        h = (h - 1) // s + 1
        act += batch * h * h * w     # a2
        if blk.down_conv is not None:
            act += batch * h * h * out  # the identity branch
        act += batch * h * h * out   # block output
    weights = sum(p.numel() for n, p in model.named_parameters() if p.dim() > 1) * 2
    coefs = sum(2 * b.numel() for n, b in model.named_buffers() if n.endswith("running_mean")) * 4
    inp = batch * 3 * image * image * 2
    return {"activation_bytes": 2 * 2 * act, "weight_bytes": weights, "coef_bytes": coefs, "input_bytes": inp,
            "total_bytes": 2 * 2 * act + weights + coefs + inp}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--copy-tbs", type=float, default=4.72, help="measured device copy rate, TB/s (README)")
    a = ap.parse_args()
    from kubedl_amd.parallel.dist import DistInfo
    from kubedl_amd.workers.resnet50 import ResNetTrainer
    dev = torch.device("cuda", 0)
    tr = ResNetTrainer(DistInfo(0, 1, 0, dev, "nccl"), batch=a.batch, image=a.image, bn_backend="hip")
    tr.step()
    distinct = tr.eval_batches(5)
    run = [distinct[i % 5] for i in range(a.batches)]
    warm = [distinct[i % 5] for i in range(a.warmup)]

    def on_stream(fn, items):
        caller = torch.cuda.current_stream(dev)
        tr.stream.wait_stream(caller)
        with torch.cuda.stream(tr.stream):
            fn(items)
        caller.wait_stream(tr.stream)

    def train_fwd(items):
        for x, _ in items:
            tr.engine.forward(x)
        tr.engine._saved = None

    ref = tr.model

    @torch.no_grad()
    def autograd(items):
        ref.eval()
        for x, _ in items:
            ref(x)
        ref.train()

    kinds = {"eval": lambda items: tr.evaluate(items), "train_fwd": lambda items: on_stream(train_fwd, items),
             "autograd": lambda items: on_stream(autograd, items)}
    times = {k: [] for k in kinds}
    for rep in range(a.repeats):
        for k, fn in kinds.items():
            fn(warm)
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            fn(run)
            torch.cuda.synchronize(dev)
            times[k].append(time.perf_counter() - t)
            print(json.dumps({"kind": k, "repeat": rep, "seconds": times[k][-1],
                              "images_per_sec": a.batches * a.batch / times[k][-1]}), flush=True)
    by = infer_bytes(tr.model, a.batch, a.image)
    med = {k: statistics.median(v) for k, v in times.items()}
    per_fwd = med["eval"] / a.batches
    out = {"batch": a.batch, "image": a.image, "batches": a.batches, "repeats": a.repeats,
           **{f"{k}_images_per_sec": a.batches * a.batch / med[k] for k in kinds},
           **{f"{k}_ms_per_batch": med[k] / a.batches * 1e3 for k in kinds}, **by,
           "eval_tb_per_s": by["total_bytes"] / per_fwd / 1e12,
           "share_of_copy_rate": by["total_bytes"] / per_fwd / 1e12 / a.copy_tbs}
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
