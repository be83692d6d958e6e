"""The learning-to-rank gradient on one GPU: the pair kernels of csrc/gbdt_rank.hip against the torch path
of the same call (``HistGBDT._rank_grad_hess_torch`` on device tensors), and boosting rounds/s of
``rank:ndcg`` beside ``binary:logistic`` on the same X.

Rows are the worker's synthetic rows in query groups of about ``--group-size`` (its ``load_groups``), the
scores a noisy copy of the target, so positions are not trivial.  Every timed call has a device
synchronisation on each side and is preceded by ``--warmup`` calls of the same kind; the median, minimum and
maximum of ``--repeats`` calls are printed.  The torch path pads groups of similar size to [c, L] and forms
the pairs in [c, i, L] blocks of at most 2^22 elements (its temporaries would not fit otherwise): it is
chunked by construction, and timed on the first ``--torch-groups`` groups only and scaled by rows.

    python scripts/gbdt_rank_bench.py > profiles/gbdt_rank_bench.txt
    python scripts/gbdt_rank_bench.py --rounds-only     # binary:logistic rounds/s alone (A/B runs of two builds)
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, warmup: int, repeats: int):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def line(name: str, ms) -> float:
    med = statistics.median(ms)
    print(f"{name}: median {med:.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  n {len(ms)}", flush=True)
    return med


def rounds_per_s(objective: str, X, y, rounds: int, depth: int, **fit_kw):
    from kubedl_amd.models.gbdt import GBDTParams, HistGBDT
    out = []
    for _ in range(3):  # the first fit pays for code loading
        m = HistGBDT(GBDTParams(objective=objective, n_estimators=rounds, max_depth=depth), "cuda")
        m.fit(X, y, **fit_kw)
        out.append(rounds / m.stats["boost_s"])
    print(f"{objective}: {rounds} rounds, depth {depth}: rounds/s of three fits (boosting rounds alone): "
          f"{out[0]:.0f} (first, loads code) {out[1]:.0f} {out[2]:.0f}", flush=True)
    return out[1:]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--group-size", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--torch-groups", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds-only", action="store_true")
    a = ap.parse_args()
    from kubedl_amd.models.gbdt import GBDTParams, HistGBDT
    from kubedl_amd.workers.xgboost_dist import load_data
    args = SimpleNamespace(dataset="synthetic", rows=a.rows, features=a.features, group_size=a.group_size,
                           objective_hint="binary")
    X, yb = load_data(args, 0, 1)
    X = X.cuda()
    print(f"# {a.rows} x {a.features}, {torch.cuda.get_device_name(0)}; warm-up {a.warmup}, every call synchronised "
          f"on both sides", flush=True)
    if a.rounds_only:
        rounds_per_s("binary:logistic", X, yb, a.rounds, a.depth)
        return 0
    from kubedl_amd.workers.xgboost_dist import load_groups
    args.objective_hint = "rank"
    _, y = load_data(args, 0, 1)
    sizes = load_groups(args, 0)
    print(f"# {sizes.numel()} groups of {int(sizes.min())}..{int(sizes.max())} rows (mean {float(sizes.float().mean()):.1f}), "
          f"{int((sizes.long() ** 2).sum()) / 1e6:.0f} M ordered pairs", flush=True)
    g = torch.Generator().manual_seed(7)
    score = (y.float() * 0.5 + torch.randn(a.rows, generator=g)).cuda().view(-1, 1).contiguous()
    for obj in ("rank:ndcg", "rank:pairwise"):
        m = HistGBDT(GBDTParams(objective=obj), "cuda")
        assert m.use_hip
        rk = m._rank_setup(y.cuda(), sizes)
        k_ms = line(f"{obj} gradient, kernels ({rk['plan_wave'].shape[0]} wave slots, {rk['plan_block'].shape[0]} "
                    f"block items)", timed(lambda: m._grad_hess(score, y, rk), a.warmup, a.repeats))
        q = min(a.torch_groups, sizes.numel())
        n = int(sizes[:q].sum())
        rs = m._rank_setup(y[:n].cuda(), sizes[:q], plan=False)
        ss = score[:n, 0].contiguous()
        t_ms = line(f"{obj} gradient, torch path on the GPU, first {q} groups ({n} rows)",
                    timed(lambda: m._rank_grad_hess_torch(ss, rs), 1, 5))
        gk, hk = m._grad_hess(score, y, rk)
        gt, ht, _ = m._rank_grad_hess_torch(ss, rs)
        print(f"{obj}: torch path scaled to {a.rows} rows: {t_ms * a.rows / n:.1f} ms = {t_ms * a.rows / n / k_ms:.0f}x the "
              f"kernels; max |kernel - torch| g {float((gk[:n, 0] - gt).abs().max()):.3e} h "
              f"{float((hk[:n, 0] - ht).abs().max()):.3e} (max |g| {float(gt.abs().max()):.3e})", flush=True)
    mv = HistGBDT(GBDTParams(objective="rank:ndcg", eval_at=10), "cuda")
    rv = mv._rank_setup(y.cuda(), sizes, plan=False)
    sv = score.view(-1)
    line("ndcg@10 of all groups (DCG kernel + fp64 division and sum on [Q])", timed(lambda: mv._ndcg_sum(sv, rv), a.warmup,
                                                                                 a.repeats))
    for _ in range(2):  # alternating
        rounds_per_s("rank:ndcg", X, y, a.rounds, a.depth, group=sizes)
        rounds_per_s("binary:logistic", X, yb, a.rounds, a.depth)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
