"""Time of ``FusedLARS.step()`` against ``FusedSGD.step()`` on the ResNet-50 parameter space, one GPU.

Both optimizers own the same ``FlatParamSpace`` (bf16 parameters and gradients, fp32 master); a sample is
``--inner`` consecutive steps between two device events, the two kinds alternate, the median of ``--repeats``
samples is reported with its range.  The byte floor is computed from the space: SGD streams 20 bytes per
element (bf16 grad + fp32 master + fp32 momentum in, fp32 master + fp32 momentum + bf16 param out), LARS 26
(its norm pass reads the bf16 grad and the fp32 master once more), so the floor of the ratio is 1.3.

    python scripts/lars_rate.py > profiles/lars_rate.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copy-tbs", type=float, default=4.72, help="measured device copy rate, TB/s (README)")
    a = ap.parse_args()
    from kubedl_amd.models.resnet import resnet50
    from kubedl_amd.ops import _ext
    from kubedl_amd.ops.optim import FlatParamSpace, FusedLARS, FusedSGD
    _ext.load()
    dev = torch.device("cuda", 0)
    with torch.device(dev):
        model = resnet50(1000)
    for p in model.parameters():
        p.data = p.data.to(torch.bfloat16)
    sp = FlatParamSpace(model, dtype=torch.bfloat16, device=dev)
    sp.grad.copy_(torch.randn(sp.numel, device=dev) * 1e-2)
    sp.mark_packed()
    opts = {"sgd": FusedSGD(sp, lr=1e-3, momentum=0.9, weight_decay=5e-5),
            "lars": FusedLARS(sp, lr=1e-3, momentum=0.9, weight_decay=5e-5)}
    for o in opts.values():
        for _ in range(a.warmup):
            o.step()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in opts}
    for rep in range(a.repeats):
        for k, o in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                o.step()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
            print(json.dumps({"kind": k, "repeat": rep, "ms_per_step": ms[k][-1]}), flush=True)
    elems = int((sp.chunks_cpu[:, 1] & 0xffffffff).sum())  # what the kernels stream: the slots, padded to 8
    per = {"sgd": 20, "lars": 26}
    out = {"elements": elems, "chunks": int(sp.chunks_cpu.shape[0]), "chunk": sp.chunk, "repeats": a.repeats,
           "inner": a.inner, "floor_ratio": per["lars"] / per["sgd"]}
    for k in opts:
        med = statistics.median(ms[k])
        out.update({f"{k}_ms": med, f"{k}_ms_min": min(ms[k]), f"{k}_ms_max": max(ms[k]), f"{k}_bytes": per[k] * elems,
                    f"{k}_tb_per_s": per[k] * elems / (med * 1e-3) / 1e12,
                    f"{k}_share_of_copy_rate": per[k] * elems / (med * 1e-3) / 1e12 / a.copy_tbs})
    out["lars_over_sgd"] = out["lars_ms"] / out["sgd_ms"]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
