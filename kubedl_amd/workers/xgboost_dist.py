"""XGBoostJob worker: distributed histogram GBDT on MI355X (one GPU per rank).

Accepts the reference example's arguments
(``example/xgboost/xgboostjob_v1alpha1_iris_train.yaml``):
``--job_type=Train --xgboost_parameter=objective:multi:softprob,num_class:3
--n_estimators=10 --learning_rate=0.1 --model_path=... --model_storage_type=oss``.

Rendezvous uses the env the XGBoost controller injects (``MASTER_ADDR``,
``MASTER_PORT``, ``WORLD_SIZE``); because the reference gives master-0 and
worker-0 the same ``RANK`` (a rabit-ism, ``controllers/xgboost/pod.go:112-143``)
the process-group rank comes from ``KDL_RANK`` when present.

Data: ``--dataset iris`` (scikit-learn's bundled copy; every rank takes a
row shard) or ``--dataset synthetic`` (``--rows`` x ``--features`` float
rows per rank with a nonlinear target, HIGGS-like shape).

``--job_type=Train`` (the default) fits a model, prints one JSON line with the
training metric and rounds/s, and rank 0 writes the model to ``--model_path``
(``HistGBDT.save``: ``<path>.json``).  ``--eval_fraction=f`` holds out every
``round(1/f)``-th row of the rank's shard as a validation set (its metric per
round is ``evals_result``); ``--early_stopping_rounds=n`` (or
``early_stopping_rounds:n`` in ``--xgboost_parameter``) stops once that metric
has not improved for ``n`` rounds and reports ``best_iteration`` / ``best_score``.

``--job_type=Predict`` loads the model a Train job wrote (same ``--model_path``
rule: an absolute path with ``--model_storage_type=local`` is used as given,
anything else lives in the pod sandbox) on every rank, predicts the rank's row
shard, writes the predictions to ``<model file>.pred.rank<R>.npy`` and rank 0
prints one JSON line with the metric against the labels and the prediction
rate (the second of two ``predict`` calls, synchronised on both sides; the
first pays for code loading and forest packing).  A missing model file is an
error (exit code 2), never a retrain.  ``examples/xgboost/`` has a Train and a
Predict job spec that share a model path.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

from kubedl_amd.models.gbdt import GBDTParams, HistGBDT
from kubedl_amd.parallel import dist as kdist
from kubedl_amd.workers import common


def load_data(args, rank: int, world: int):
    if args.dataset == "iris":
        try:
            from sklearn.datasets import load_iris
            X, y = load_iris(return_X_y=True)
            X = torch.tensor(X, dtype=torch.float32)
            y = torch.tensor(y)
        except Exception:  # no sklearn: iris-shaped synthetic
            g = torch.Generator().manual_seed(0)
            y = torch.arange(150) % 3
            X = torch.randn(150, 4, generator=g) + y[:, None].float()
        return X[rank::world].contiguous(), y[rank::world].contiguous()
    g = torch.Generator().manual_seed(1234 + rank)
    X = torch.randn(args.rows, args.features, generator=g)
    logit = X[:, 0] * 1.5 - X[:, 1] ** 2 + X[:, 2] * X[:, 3] + 0.5 * torch.sin(3 * X[:, 4 % args.features])
    if args.objective_hint == "binary":
        y = (logit + 0.3 * torch.randn(args.rows, generator=g) > 0).long()
    else:
        y = logit + 0.1 * torch.randn(args.rows, generator=g)
    return X, y


def model_file(args) -> str:
    """Where ``--model_path`` lives on this node (the writer's and the reader's rule)."""
    path = args.model_path
    if args.model_storage_type != "local" or not os.path.isabs(path):
        # no object store on the node: keep the model in the pod sandbox
        path = os.path.join(os.environ.get("KDL_SANDBOX", "."), "model", path.strip("/"))
    return path + ".json"


def run_predict(args, info) -> int:
    import numpy as np
    if not args.model_path:
        print("xgboost_dist: --job_type=Predict needs --model_path", file=sys.stderr, flush=True)
        return 2
    path = model_file(args)
    if not os.path.isfile(path):
        print(f"xgboost_dist: --job_type=Predict: no model file at {path} (run a Train job with the same "
              "--model_path first)", file=sys.stderr, flush=True)
        return 2
    model = HistGBDT.load(path, info.device)
    if args.dataset is None:
        args.dataset = "iris" if model.p.objective.startswith("multi:") else "synthetic"
        if args.dataset == "synthetic" and model.cuts is not None:
            args.features = int(model.cuts.shape[0])
    if not model.p.objective.startswith(("multi:", "binary:")):
        args.objective_hint = "reg"
    X, y = load_data(args, info.rank, info.world_size)
    X = X.to(info.device)

    def sync():
        if info.device.type == "cuda":
            torch.cuda.synchronize(info.device)
    model.predict(X, output_margin=True)  # code loading + forest packing
    sync()
    t0 = time.perf_counter()
    margin = model.predict(X, output_margin=True)
    sync()
    dt = kdist.all_reduce_max(time.perf_counter() - t0, info)
    pred = model.transform_margin(margin)
    out_path = f"{path}.pred.rank{info.rank}.npy"
    np.save(out_path, pred.cpu().numpy())
    common.report_progress(1, final=True)
    met = model.metric(margin, y.to(info.device))
    if info.rank == 0:
        print(json.dumps({"job_type": "Predict", "rank": info.rank, "world_size": info.world_size,
                          "objective": model.p.objective, "rounds": len(model.trees), "rows": int(X.shape[0]),
                          "features": int(X.shape[1]), "predict_seconds": dt,
                          "predict_rows_per_sec": X.shape[0] / dt if dt > 0 else 0.0, "model": path,
                          "predictions": out_path, "device": str(info.device), "hip_kernels": model.use_hip, **met}),
              flush=True)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--job_type", default="Train")
    ap.add_argument("--xgboost_parameter", default="")
    ap.add_argument("--n_estimators", type=int, default=10)
    ap.add_argument("--learning_rate", type=float, default=0.3)
    ap.add_argument("--max_depth", type=int, default=6)
    ap.add_argument("--max_bin", type=int, default=256)
    ap.add_argument("--model_path", default="")
    ap.add_argument("--model_storage_type", default="local")
    ap.add_argument("--oss_param", default="")
    ap.add_argument("--dataset", default=None, choices=[None, "iris", "synthetic"])
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--objective_hint", default="binary", choices=["binary", "reg"])
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--eval_fraction", type=float, default=0.0)
    ap.add_argument("--early_stopping_rounds", type=int, default=0)
    args, _unknown = ap.parse_known_args(argv)
    if os.environ.get("KDL_RANK"):
        os.environ["RANK"] = os.environ["KDL_RANK"]
    info = kdist.init_from_env("cpu" if args.cpu else None)
    common.signal_ready({"rank": info.rank})
    job_type = args.job_type.strip().lower()
    if job_type not in ("train", "predict"):
        print(f"xgboost_dist: unknown --job_type {args.job_type!r} (Train or Predict)", file=sys.stderr, flush=True)
        kdist.shutdown(info)
        return 2
    if job_type == "predict":
        rc = run_predict(args, info)
        kdist.shutdown(info)
        return rc
    if args.dataset is None:
        args.dataset = "iris" if "num_class:3" in args.xgboost_parameter else "synthetic"
    default_obj = "binary:logistic" if args.objective_hint == "binary" else "reg:squarederror"
    params = GBDTParams.parse(args.xgboost_parameter or f"objective:{default_obj}",
                              n_estimators=args.n_estimators, learning_rate=args.learning_rate,
                              max_depth=args.max_depth, max_bin=args.max_bin)
    if args.dataset == "iris" and params.max_bin > 64:
        params.max_bin = 64
    if args.early_stopping_rounds > 0:
        params.early_stopping_rounds = args.early_stopping_rounds
    X, y = load_data(args, info.rank, info.world_size)
    fit_kw = {}
    if args.eval_fraction > 0:
        # every round(1 / fraction)-th row of the shard is held out
        step = max(int(round(1.0 / args.eval_fraction)), 2)
        held = torch.zeros(X.shape[0], dtype=torch.bool)
        held[step - 1::step] = True
        fit_kw = {"eval_set": (X[held].contiguous(), y[held].contiguous()),
                  "early_stopping_rounds": params.early_stopping_rounds}
        X, y = X[~held].contiguous(), y[~held].contiguous()
    model = HistGBDT(params, info.device)
    t0 = time.perf_counter()
    pred = model.fit(X, y, callback=lambda it, _p: common.report_progress(
        it + 1, final=it + 1 == params.n_estimators), **fit_kw)
    if info.device.type == "cuda":
        torch.cuda.synchronize()
    dt = kdist.all_reduce_max(time.perf_counter() - t0, info)
    met = model.metric(pred, y.to(info.device))
    rounds = len(model.trees)  # < n_estimators after an early stop
    if fit_kw:
        common.report_progress(rounds, final=True)
    out = {"job_type": "Train", "rank": info.rank, "world_size": info.world_size, "objective": params.objective,
           "rounds": rounds, "rows_per_rank": int(X.shape[0]), "features": int(X.shape[1]),
           "seconds": dt, "fit_rounds_per_sec": rounds / dt if dt > 0 else 0.0,
           # boosting rounds alone (setup = H2D copy + cuts + quantisation, reported apart)
           "rounds_per_sec": (rounds / model.stats["boost_s"]
                              if model.stats.get("boost_s", 0) > 0 else 0.0),
           "device": str(info.device), "hip_kernels": model.use_hip, **met, **model.stats}
    if fit_kw:
        out.update({"eval_rows": int(fit_kw["eval_set"][0].shape[0]), "eval_metric": model.eval_metric,
                    "eval_last": model.evals_result[-1] if model.evals_result else None,
                    "best_iteration": model.best_iteration, "best_score": model.best_score})
    if info.rank == 0:
        print(json.dumps(out), flush=True)
        if args.model_path:
            model.save(model_file(args))
    kdist.shutdown(info)
    return 0


if __name__ == "__main__":
    from kubedl_amd.parallel.dist import run_rank
    sys.exit(run_rank(main))
