"""The quantile objectives on one GPU: the leaf renewal of csrc/gbdt_quantile.hip (count + step launches of
all passes after a grown tree), the base-margin select over all rows, its all-keys-equal case, ``torch.sort``
of as many fp32 keys (the core of any vendor-op route), and boosting rounds/s of ``reg:quantileerror`` beside
``reg:squarederror`` on the same X.

Rows are the worker's synthetic regression rows.  Every timed call has a device synchronisation on each side
and is preceded by ``--warmup`` calls of the same kind; the median, minimum and maximum of ``--repeats``
calls are printed.

    python scripts/gbdt_quantile_bench.py > profiles/gbdt_quantile_bench.txt
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gbdt_rank_bench import line, rounds_per_s, timed  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--alpha", type=float, default=0.9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    from kubedl_amd.models.gbdt import GBDTParams, HistGBDT
    from kubedl_amd.ops import _ext
    from kubedl_amd.workers.xgboost_dist import load_data
    ext = _ext.load()
    X, y = load_data(SimpleNamespace(dataset="synthetic", rows=a.rows, features=a.features, objective_hint="reg"), 0, 1)
    X, y = X.cuda(), y.cuda().float().contiguous()
    print(f"# {a.rows} x {a.features}, depth {a.depth}, alpha {a.alpha}, {torch.cuda.get_device_name(0)}; warm-up "
          f"{a.warmup}, every call synchronised on both sides", flush=True)
    # one grown tree of the objective, then its leaf renewal alone, again and again (the same result each time)
    m = HistGBDT(GBDTParams(objective="reg:quantileerror", quantile_alpha=a.alpha, max_depth=a.depth), "cuda")
    m.fit_cuts(X)
    gr = m._device_grower(m.quantise(X).contiguous())
    lo, hi = torch.tensor([[0], [a.rows]], dtype=torch.int32, device="cuda")
    pred = torch.full((a.rows, 1), float(ext.gbdt_segment_quantile(y, lo, hi, a.alpha)), device="cuda")
    g, h = m._grad_hess(pred, y)
    gr.grow_local(g[:, 0].contiguous(), h[:, 0].contiguous())
    line(f"leaf renewal of one depth-{a.depth} tree (leaf plan + 4 x (count + step))",
         timed(lambda: gr.renew_leaves(y, pred, 0, a.alpha), a.warmup, a.repeats))
    print(f"# (leaf nodes of that tree, by its feature array: {int((gr.tree()[0] < 0).sum())} of "
          f"{gr.tree()[0].numel()} heap slots hold no split; value range after renewal "
          f"{float(gr.tree()[3].min()):.4f}..{float(gr.tree()[3].max()):.4f})", flush=True)
    sel = line("base-margin select over all rows (plan + 4 x (count + step), its workspaces allocated per call)",
               timed(lambda: ext.gbdt_segment_quantile(y, lo, hi, a.alpha), a.warmup, a.repeats))
    same = torch.full_like(y, 1.5)
    line("the same with all keys equal", timed(lambda: ext.gbdt_segment_quantile(same, lo, hi, a.alpha), a.warmup,
                                               a.repeats))
    srt = line("torch.sort of the same fp32 keys", timed(lambda: torch.sort(y), a.warmup, a.repeats))
    ref = torch.sort(y).values[max(math.ceil(a.alpha * a.rows) - 1, 0)]
    got = ext.gbdt_segment_quantile(y, lo, hi, a.alpha)[0]
    print(f"# select == sorted[ceil(alpha n) - 1]: {bool(got == ref)}; torch.sort / select = {srt / sel:.2f}", flush=True)
    for _ in range(2):  # alternating
        rounds_per_s("reg:quantileerror", X, y, a.rounds, a.depth)
        rounds_per_s("reg:squarederror", X, y, a.rounds, a.depth)
        rounds_per_s("binary:logistic", X, (y > 0).long(), a.rounds, a.depth)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
