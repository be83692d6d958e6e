"""``HistGBDT.predict_contribs`` on one GPU: the contribution kernel (csrc/gbdt_shap.hip) against the torch
path of the same call, the cover pass, and ``predict`` beside them.

The model is fitted here (binary:logistic on the worker's synthetic rows), the background is the first
``--background`` rows.  Every timed call has a device synchronisation on each side and is preceded by
``--warmup`` calls of the same kind; the median, minimum and maximum of ``--repeats`` calls are printed.
The torch path is timed on the first ``--torch-rows`` rows only (it needs seconds per 64k rows) and scaled.
Bytes: X read once and the output written once, computed from the shapes; the path table stays in L2.

    python scripts/gbdt_contribs_bench.py > profiles/gbdt_contribs_bench.txt
    python scripts/gbdt_contribs_bench.py --predict-only     # predict's time alone (A/B runs of two builds)
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

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


def line(name: str, ms, rows: int) -> float:
    med = statistics.median(ms)
    print(f"{name}: median {med:.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}  n {len(ms)}  "
          f"{rows / med / 1e3:.1f} M rows/s", flush=True)
    return med


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--background", type=int, default=65536)
    ap.add_argument("--torch-rows", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--copy-tbs", type=float, default=4.72, help="measured device copy rate, TB/s (README)")
    ap.add_argument("--predict-ms", type=float, default=0.81, help="predict on this workload, ms (README)")
    ap.add_argument("--predict-only", action="store_true")
    a = ap.parse_args()
    from kubedl_amd.models.gbdt import GBDTParams, HistGBDT
    from kubedl_amd.ops import _ext
    g = torch.Generator().manual_seed(1234)
    X = torch.randn(a.rows, a.features, generator=g)
    logit = X[:, 0] * 1.5 - X[:, 1] ** 2 + X[:, 2] * X[:, 3] + 0.5 * torch.sin(3 * X[:, 4 % a.features])
    y = (logit + 0.3 * torch.randn(a.rows, generator=g) > 0).long()
    m = HistGBDT(GBDTParams(objective="binary:logistic", n_estimators=a.rounds, max_depth=a.depth), "cuda")
    assert m.use_hip
    X = X.cuda()
    m.fit(X, y)
    print(f"# {a.rows} x {a.features}, {len(m.trees)} rounds, depth {a.depth}, binary:logistic, "
          f"{torch.cuda.get_device_name(0)}; warm-up {a.warmup}, every call synchronised on both sides", flush=True)
    p_ms = line("predict (output_margin=True)", timed(lambda: m.predict(X, output_margin=True), a.warmup, 20), a.rows)
    if a.predict_only:
        return 0
    B = X[:a.background].contiguous()
    line(f"set_background ({a.background} rows: cover kernel + zeroed counts)", timed(lambda: m.set_background(B),
                                                                                      a.warmup, a.repeats), a.background)
    nodes, off, _ = m._forest()
    counts = torch.zeros(nodes.shape[0], dtype=torch.int64, device="cuda")
    ext = _ext.load()
    line("cover kernel alone", timed(lambda: ext.gbdt_cover(B, nodes, off, 0, off.numel() - 1, counts), a.warmup,
                                     a.repeats), a.background)
    m.set_background(B)
    t = time.perf_counter()
    table = m._path_table(len(m.trees))
    pad = table["pad"]
    print(f"path table: {pad['feat'].shape[0]} paths, longest {pad['feat'].shape[1]} elements, "
          f"{table['slots'].shape[0] * 16 / 1024:.0f} KiB in {table['chunk_off'].numel() - 1} chunks, built on the host in "
          f"{time.perf_counter() - t:.2f} s (once per model and background)", flush=True)
    c_ms = line("predict_contribs (contribution kernel + output allocation)", timed(lambda: m.predict_contribs(X),
                                                                                    a.warmup, a.repeats), a.rows)
    out = torch.empty(a.rows, 1, a.features + 1, device="cuda")
    k_ms = line("contribution kernel alone (onto a resident output)", timed(
        lambda: ext.gbdt_contribs(X, table["slots"], table["chunk_off"], table["class_chunk"], table["bias"], 1, out),
        a.warmup, a.repeats), a.rows)
    moved = a.rows * (a.features + a.features + 1) * 4
    floor = moved / (a.copy_tbs * 1e12) * 1e3
    print(f"bytes moved: {moved / 1e6:.0f} MB (X read, contributions written) = {moved / k_ms / 1e9:.3f} TB/s, copy floor "
          f"{floor:.3f} ms at {a.copy_tbs} TB/s: the kernel takes {k_ms / floor:.0f}x the floor; {k_ms / a.predict_ms:.0f}x "
          f"predict's {a.predict_ms} ms ({k_ms / p_ms:.0f}x the {p_ms:.3f} ms measured above)", flush=True)
    Xs = X[:a.torch_rows].contiguous()
    t_ms = line(f"torch path, first {a.torch_rows} rows", timed(lambda: m._contribs_torch(Xs, table), 1, 3), a.torch_rows)
    ref = m._contribs_torch(Xs, table)
    got = m.predict_contribs(Xs)
    gap = (m.predict_contribs(X).double().sum(-1) - m.predict(X, output_margin=True).double()).abs().max()
    print(f"torch path scaled to {a.rows} rows: {t_ms * a.rows / a.torch_rows:.0f} ms, {t_ms * a.rows / a.torch_rows / c_ms:.0f}x "
          f"predict_contribs; max |kernel - torch path| {float((got - ref).abs().max()):.3e}, max |sum - margin| "
          f"{float(gap):.3e}", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
