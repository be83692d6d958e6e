"""``HistGBDT.predict_contribs(perturbation="interventional")`` on one GPU: the mask-histogram kernel, the host
compaction and the explain kernel (csrc/gbdt_iv.hip) against the torch path of the same call and against
path-dependent ``predict_contribs`` in the same process.

The model is fitted here (binary:logistic on the worker's synthetic rows), the background is the first
``--background`` rows.  Every timed call has a device synchronisation on each side and is preceded by
``--warmup`` calls of the same kind; the median, minimum and maximum of ``--repeats`` calls are printed.
The torch path evaluates every (row, background row, path): it is timed once on the first ``--torch-rows``
rows and scaled by rows.

    python scripts/gbdt_contribs_iv_bench.py > profiles/gbdt_contribs_iv_bench.txt
    python scripts/gbdt_contribs_iv_bench.py --path-dependent-only   # A/B runs of two builds (KDL_C_PATH)
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
    ap.add_argument("--torch-rows", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--path-dependent-only", action="store_true")
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
    print(f"# {a.rows} x {a.features}, {len(m.trees)} rounds, depth {a.depth}, binary:logistic, background "
          f"{a.background} rows, {torch.cuda.get_device_name(0)}; warm-up {a.warmup}, every call synchronised on "
          f"both sides", flush=True)
    B = X[:a.background].contiguous()
    m.set_background(B, interventional=not a.path_dependent_only)
    m._path_table(len(m.trees))
    pd_ms = line("predict_contribs path-dependent (same process)", timed(lambda: m.predict_contribs(X), a.warmup,
                                                                         a.repeats), a.rows)
    if a.path_dependent_only:
        return 0
    ext = _ext.load()
    t = time.perf_counter()
    iv = m._iv_table(len(m.trees))
    print(f"first _iv_table call {time.perf_counter() - t:.3f} s: mask table + histogram kernel {iv['hist_seconds'] * 1e3:.1f} ms"
          f" (first launch), host compaction {iv['compact_seconds'] * 1e3:.1f} ms (once per model, background and "
          f"n_rounds)", flush=True)
    print(f"explain table: {iv['paths']} paths as {iv['table_paths']} table paths, {iv['hist'].numel()} counters, "
          f"{iv['records']} records = {iv['records'] / max(iv['paths'], 1):.1f} per path, "
          f"{iv['slots'].shape[0] * 16 / 1024:.0f} KiB in {iv['chunk_off'].numel() - 1} chunks; mask table "
          f"{iv['masks'][0].shape[0] * 16 / 1024:.0f} KiB in {iv['masks'][1].numel() - 1} chunks", flush=True)
    scratch = torch.zeros_like(iv["hist"])
    line(f"mask-histogram kernel alone ({a.background} rows)", timed(
        lambda: ext.gbdt_path_masks(B, *iv["masks"], scratch), a.warmup, a.repeats), a.background)
    c_ms = line("predict_contribs interventional (explain kernel + output allocation)", timed(
        lambda: m.predict_contribs(X, perturbation="interventional"), a.warmup, a.repeats), a.rows)
    out = torch.empty(a.rows, 1, a.features + 1, device="cuda")
    k_ms = line("explain kernel alone (onto a resident output)", timed(
        lambda: ext.gbdt_contribs_iv(X, iv["slots"], iv["chunk_off"], iv["class_chunk"], iv["bias"], 1, out),
        a.warmup, a.repeats), a.rows)
    print(f"interventional / path-dependent predict_contribs: {c_ms / pd_ms:.2f}x; (row, record) terms per call: "
          f"{a.rows * iv['records'] / 1e9:.1f} G = {a.rows * iv['records'] / k_ms / 1e6:.0f} G terms/s", flush=True)
    Xs = X[:a.torch_rows].contiguous()
    table = m._path_table(len(m.trees))
    m._contribs_iv_torch(Xs[:1], table, B[:64], 64)  # code loading
    torch.cuda.synchronize()
    t = time.perf_counter()
    ref = m._contribs_iv_torch(Xs, table, B, a.background)
    torch.cuda.synchronize()
    t_ms = (time.perf_counter() - t) * 1e3
    got = m.predict_contribs(Xs, perturbation="interventional")
    gap = (m.predict_contribs(X, perturbation="interventional").double().sum(-1)
           - m.predict(X, output_margin=True).double()).abs().max()
    print(f"torch path on the GPU, first {a.torch_rows} rows, one call: {t_ms:.0f} ms; scaled to {a.rows} rows: "
          f"{t_ms * a.rows / a.torch_rows / 1e3:.0f} s, {t_ms * a.rows / a.torch_rows / c_ms:.0f}x predict_contribs "
          f"interventional; max |kernel - torch path| {float((got - ref).abs().max()):.3e}, max |sum - margin| "
          f"{float(gap):.3e}", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
