"""``HistGBDT.predict_interactions`` on one GPU: the interaction kernel (csrc/gbdt_interactions.hip) against the
torch path of the same call on the GPU and against ``predict_contribs`` on the same model.

The model is fitted here (binary:logistic on the worker's synthetic rows), the background is the first
``--background`` rows.  The result of all rows holds ``rows * (features + 1)^2`` floats (6.7 GB at the defaults),
so one timed call walks the rows in blocks of ``--block-rows`` onto one resident output block; every timed call
has a device synchronisation on each side and is preceded by ``--warmup`` calls of the same kind; the median,
minimum and maximum of ``--repeats`` calls are printed.  The torch path is timed on the first ``--torch-rows``
rows only and scaled.  Bytes: X read once per conditioning feature and the output written once, from the shapes.

    python scripts/gbdt_interactions_bench.py > profiles/gbdt_interactions_bench.txt
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
          f"{rows / med / 1e3:.2f} M rows/s", flush=True)
    return med


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--background", type=int, default=65536)
    ap.add_argument("--block-rows", type=int, default=262144)
    ap.add_argument("--torch-rows", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
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
          f"{torch.cuda.get_device_name(0)}; blocks of {a.block_rows} rows; warm-up {a.warmup}, every call "
          "synchronised on both sides", flush=True)
    m.set_background(X[:a.background].contiguous())
    ext, F1 = _ext.load(), a.features + 1
    t = time.perf_counter()
    table = m._path_table(len(m.trees))
    pairs = m._pair_table(len(m.trees), a.features)
    lists = int((pairs["feat_chunk"].diff() > 0).sum())
    print(f"tables: {table['pad']['feat'].shape[0]} paths, longest {table['pad']['feat'].shape[1]} elements; path table "
          f"{table['slots'].shape[0] * 16 / 1024:.0f} KiB, per-feature table {pairs['slots'].shape[0] * 16 / 1024:.0f} KiB "
          f"in {pairs['chunk_off'].numel() - 1} chunks of {lists} lists, built on the host in "
          f"{time.perf_counter() - t:.2f} s (once per model and background); rows per block "
          f"{ext.gbdt_interactions_rows_per_block(a.features)}", flush=True)
    c_ms = line("predict_contribs (all rows, one call)", timed(lambda: m.predict_contribs(X), a.warmup, a.repeats), a.rows)
    blocks = [X[r0:r0 + a.block_rows] for r0 in range(0, a.rows, a.block_rows)]

    def public_call():
        for b in blocks:
            m.predict_interactions(b)
    i_ms = line("predict_interactions (all rows in blocks, output allocated per block)",
                timed(public_call, a.warmup, a.repeats), a.rows)
    out = torch.empty(a.block_rows, 1, F1, F1, device="cuda")

    def kernel_only():
        for b in blocks:
            ext.gbdt_interactions(b, pairs["slots"], pairs["chunk_off"], pairs["feat_chunk"], table["bias"], 1,
                                  out[:b.shape[0]])
    k_ms = line("interaction kernel alone (all rows in blocks, onto one resident block)",
                timed(kernel_only, a.warmup, a.repeats), a.rows)
    moved = a.rows * (a.features * lists + F1 * F1) * 4
    print(f"bytes moved: {moved / 1e9:.2f} GB (X read by {lists} conditioning features, {F1} x {F1} floats written per "
          f"row) = {moved / k_ms / 1e9:.3f} TB/s; the kernel takes {k_ms / c_ms:.1f}x predict_contribs; output of all "
          f"rows {a.rows * F1 * F1 * 4 / 1e9:.2f} GB", flush=True)
    Xs = X[:a.torch_rows].contiguous()
    t_ms = line(f"torch path on the GPU, first {a.torch_rows} rows", timed(lambda: m._interactions_torch(Xs, table), 1, 3),
                a.torch_rows)
    ref, got = m._interactions_torch(Xs, table), m.predict_interactions(Xs)
    gap = (got.double().sum((-1, -2)) - m.predict(Xs, output_margin=True).double()).abs().max()
    print(f"torch path scaled to {a.rows} rows: {t_ms * a.rows / a.torch_rows:.0f} ms, "
          f"{t_ms * a.rows / a.torch_rows / i_ms:.0f}x predict_interactions; max |kernel - torch path| "
          f"{float((got - ref).abs().max()):.3e}, max |sum over both axes - margin| {float(gap):.3e}", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
