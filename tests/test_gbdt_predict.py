"""GBDT batch prediction: the forest inference kernel (csrc/gbdt_predict.hip)
against ``HistGBDT.predict_margin`` bit for bit, ``predict`` / ``save`` /
``load``, ``fit`` with a validation set and early stopping, and the worker's
Train -> Predict pair.

The kernel tests build forests synthetically (seeded random trees, no
training); the reference is ``predict_margin`` of a CPU model holding the same
``Tree`` objects.  One lane owns a row's accumulators and adds the leaves in
tree order, as the reference does, so the comparison is ``torch.equal``.
"""
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from kubedl_amd.models.gbdt import GBDTParams, HistGBDT, Tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 12  # predict_margin walks max_depth + 1 levels: deeper than every synthetic tree


# ------------------------------------------------------------------ synthetic forests
def _rand_tree(g, F, depth, p_stop=0.0, p_inf=0.1):
    """A tree in the grower's append order: level by level, every split node's
    children allocated as an adjacent pair.  ``p_stop``: chance that a node above
    ``depth`` is a leaf anyway (unbalanced trees); ``p_inf``: chance of a +inf
    threshold."""
    t = Tree()
    level = [t.add()]
    for d in range(depth + 1):
        nxt = []
        for nid in level:
            t.value[nid] = float(torch.randn((), generator=g))
            if d == depth or float(torch.rand((), generator=g)) < p_stop:
                continue
            t.feature[nid] = int(torch.randint(0, F, (), generator=g))
            thr = float(torch.randn((), generator=g))
            t.threshold[nid] = math.inf if float(torch.rand((), generator=g)) < p_inf else thr
            l, r = t.add(), t.add()
            t.left[nid], t.right[nid] = l, r
            nxt += [l, r]
        level = nxt
    return t


def _rows(g, N, F):
    """Random rows with NaN, +inf and -inf sprinkled over every column."""
    X = torch.randn(N, F, generator=g)
    u = torch.rand(N, F, generator=g)
    X[u < 0.04] = float("nan")
    X[(u >= 0.04) & (u < 0.07)] = math.inf
    X[(u >= 0.07) & (u < 0.10)] = -math.inf
    return X


def _model(K, device, rounds):
    p = (GBDTParams(objective="multi:softprob", num_class=K, max_depth=DEPTH) if K > 1
         else GBDTParams(objective="reg:squarederror", max_depth=DEPTH))
    m = HistGBDT(p, device)
    m.trees = rounds
    return m


def _forest(g, F, K, shapes):
    """``shapes``: per round a (depth, p_stop) pair; K trees of that shape per round."""
    return [[_rand_tree(g, F, d, ps) for _ in range(K)] for d, ps in shapes]


def _chunk_plus_one():
    """Rounds of full depth-6 trees (127 nodes): as many as fill the kernel's LDS
    chunk, plus one."""
    from kubedl_amd.ops import _ext
    return _ext.load().gbdt_predict_chunk_nodes() // 127 + 1


# (N, F, K, rounds as (depth, p_stop)); None = filled in at run time (needs the extension)
KERNEL_CASES = {
    "one_row_one_leaf": (1, 1, 1, [(0, 0.0)]),
    "single_leaf_forest": (63, 5, 3, [(0, 0.0)] * 3),
    "depth1": (64, 5, 3, [(1, 0.0)] * 2),
    "chunk_boundary": (65, 28, 1, None),
    "unbalanced_multiclass": (257, 28, 3, [(8, 0.3)] * 5),
    "depth10_heap_and_small": (1007, 28, 1, [(6, 0.2), (10, 0.0), (3, 0.0), (10, 0.0), (7, 0.3)]),
    "one_feature": (1007, 1, 1, [(4, 0.2)] * 3),
    "large_f_128_rows": (257, 200, 3, [(7, 0.3)] * 2),
    "large_f_64_rows": (130, 400, 1, [(7, 0.3)] * 3),
    "no_staging": (65, 700, 1, [(7, 0.3), (10, 0.0)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_gpu_forest_kernel_equals_predict_margin(case):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    N, F, K, shapes = KERNEL_CASES[case]
    if shapes is None:
        shapes = [(6, 0.0)] * _chunk_plus_one()
    # the cases are meant to cover every launch variant
    want_rows = {"large_f_128_rows": 128, "large_f_64_rows": 64, "no_staging": 0}.get(case, 256)
    assert ext.gbdt_predict_rows_per_block(F, K) == want_rows
    g = torch.Generator().manual_seed(len(case) * 1000 + N)
    rounds = _forest(g, F, K, shapes)
    if case == "chunk_boundary":
        assert all(len(t.value) == 127 for r in rounds for t in r)
    if case == "depth10_heap_and_small":
        assert len(rounds[1][0].value) == 2047 > ext.gbdt_predict_chunk_nodes()
    X = _rows(g, N, F)
    ref = _model(K, "cpu", rounds).predict_margin(X)
    got = _model(K, "cuda", rounds).predict(X, output_margin=True)
    assert got.shape == ref.shape and torch.equal(got.cpu(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N,F,K,r0,r1", [(1007, 5, 3, 1, 4), (65, 28, 1, 3, 7)])
def test_gpu_forest_kernel_tree_range_onto_nonzero_margin(N, F, K, r0, r1):
    """Trees [r0 * K, r1 * K) added onto the margin of rounds [0, r0) give the margin
    of rounds [0, r1)."""
    from kubedl_amd.ops import _ext
    g = torch.Generator().manual_seed(7 + N)
    rounds = _forest(g, F, K, [(0, 0.0), (5, 0.3), (6, 0.0), (9, 0.4), (1, 0.0), (6, 0.0), (6, 0.0), (4, 0.2)])
    X = _rows(g, N, F)
    start = _model(K, "cpu", rounds[:r0]).predict_margin(X)
    ref = _model(K, "cpu", rounds[:r1]).predict_margin(X)
    assert float(start.abs().min()) > 0  # a non-zero margin to add onto
    m = _model(K, "cuda", rounds)
    nodes, off, _ = m._forest()
    margin = start.cuda()
    _ext.load().gbdt_predict(X.cuda(), nodes, off, r0 * K, r1 * K, margin)
    assert torch.equal(margin.cpu(), ref)
    # n_rounds is the same range from tree 0
    assert torch.equal(m.predict(X, output_margin=True, n_rounds=r1).cpu(), ref)


def _multiclass_data(n=4000, f=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, f, generator=g)
    s = X[:, 0] - X[:, 1] * X[:, 2] + 0.2 * torch.randn(n, generator=g)
    return X, (s > 0.5).long() + (s > -0.5).long()


def _binary_data(n=4000, f=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, f, generator=g)
    return X, ((X[:, 0] - X[:, 1] * X[:, 2] + 0.2 * torch.randn(n, generator=g)) > 0).long()


@pytest.mark.gpu
def test_gpu_device_heap_packer_equals_host_packer():
    """A tree grown by GbdtGrower, as heap_packed() -> gbdt_heap_nodes on the device,
    predicts what the same tree predicts as a host Tree through the host packer."""
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    X, y = _binary_data(3000, 8, seed=5)
    m = HistGBDT(GBDTParams(objective="binary:logistic", max_depth=5, max_bin=64), "cuda")
    Xd = X.cuda()
    m.fit_cuts(Xd)
    grower = m._device_grower(m.quantise(Xd).contiguous())
    assert grower is not None
    g, h = m._grad_hess(m._base(len(X)), y.cuda())
    packed = m._grow_device(grower, g[:, 0].contiguous(), h[:, 0].contiguous())
    heap = packed.shape[1]
    assert heap == 2 ** 6 - 1 and int((packed[0] >= 0).sum()) > 0  # the tree has splits
    nodes = torch.empty(heap, 4, dtype=torch.int32, device="cuda")
    ext.gbdt_heap_nodes(packed, nodes)
    off = torch.tensor([0, heap], dtype=torch.int32, device="cuda")
    Xq = _rows(torch.Generator().manual_seed(1), 1007, 8).cuda()
    dev = m._base(len(Xq))
    ext.gbdt_predict(Xq, nodes, off, 0, 1, dev)
    m.trees = [[HistGBDT._heap_tree(packed.cpu().tolist())]]
    host = m.predict(Xq, output_margin=True)
    assert torch.equal(dev, host)
    assert torch.equal(host, m.predict_margin(Xq))


@pytest.mark.gpu
@pytest.mark.parametrize("objective", ["binary:logistic", "multi:softprob"])
def test_gpu_model_predict_equals_reference_and_fit(objective):
    multi = objective.startswith("multi:")
    X, y = _multiclass_data() if multi else _binary_data()
    m = HistGBDT(GBDTParams(objective=objective, num_class=3 if multi else 1, n_estimators=5, max_depth=4), "cuda")
    assert m.use_hip
    pred = m.fit(X, y)
    margin = m.predict(X, output_margin=True)
    assert torch.equal(margin, m.predict_margin(X))
    torch.testing.assert_close(margin, pred, atol=1e-4, rtol=1e-4)  # tests/test_gbdt.py's bound for this
    out = m.predict(X)
    if multi:
        assert out.shape == (len(X), 3)
        torch.testing.assert_close(out, torch.softmax(margin, 1))
    else:
        assert out.shape == (len(X),)
        torch.testing.assert_close(out, torch.sigmoid(margin[:, 0]))
    # the packed forest is cached, and rebuilt when the trees change
    nodes = m._forest()[0]
    assert m._forest()[0] is nodes
    m.trees = m.trees[:3]
    assert m._forest()[0] is not nodes
    assert torch.equal(m.predict(X, output_margin=True), m.predict_margin(X))


@pytest.mark.gpu
@pytest.mark.parametrize("objective", ["binary:logistic", "multi:softprob", "reg:squarederror"])
def test_gpu_fit_eval_set_matches_predict_per_round(objective):
    multi = objective.startswith("multi:")
    X, y = _multiclass_data(5000) if multi else _binary_data(5000)
    if objective.startswith("reg:"):
        y = X[:, 0] - X[:, 1] * X[:, 2]
    Xt, yt, Xv, yv = X[:4000], y[:4000], X[4000:], y[4000:]
    m = HistGBDT(GBDTParams(objective=objective, num_class=3 if multi else 1, n_estimators=5, max_depth=4), "cuda")
    m.fit(Xt, yt, eval_set=(Xv, yv))
    assert len(m.evals_result) == 5 and m.best_iteration is None
    name = {"binary:logistic": "logloss", "multi:softprob": "mlogloss", "reg:squarederror": "rmse"}[objective]
    assert m.eval_metric == name
    for i, v in enumerate(m.evals_result):
        ref = m.metric(m.predict(Xv, output_margin=True, n_rounds=i + 1), yv.cuda())[name]
        print(f"round {i}: evals_result {v!r} metric {ref!r} rel {abs(v - ref) / abs(ref):.3e}")
        assert abs(v - ref) <= 1e-5 * abs(ref)
    assert m.evals_result[-1] < m.evals_result[0]


# ------------------------------------------------------------------ CPU
def test_params_parse_early_stopping_rounds():
    p = GBDTParams.parse("objective:binary:logistic,early_stopping_rounds:7,no_such_key:1")
    assert p.early_stopping_rounds == 7 and p.objective == "binary:logistic"
    assert GBDTParams.parse("").early_stopping_rounds == 0


def test_cpu_predict_equals_predict_margin_and_transforms():
    X, y = _multiclass_data(600, 5)
    m = HistGBDT(GBDTParams(objective="multi:softprob", num_class=3, n_estimators=3, max_depth=3, max_bin=32), "cpu")
    m.fit(X, y)
    margin = m.predict(X, output_margin=True)
    assert torch.equal(margin, m.predict_margin(X))
    assert torch.equal(m.predict(X), torch.softmax(margin, 1))
    two = HistGBDT(m.p, "cpu")
    two.cuts, two.trees = m.cuts, m.trees[:2]
    assert torch.equal(m.predict(X, output_margin=True, n_rounds=2), two.predict_margin(X))
    with pytest.raises(ValueError):
        m.predict(X[:, :4])
    with pytest.raises(ValueError):
        m.predict(X, n_rounds=4)


def test_pack_forest_renumbers_non_adjacent_children():
    """A tree whose children are not an adjacent pair is renumbered as a whole; one
    that already satisfies the invariant is packed as it is."""
    t = Tree()
    for _ in range(5):
        t.add()
    # root 0 -> (3, 1); 3 -> (2, 4): children neither adjacent nor in (left, left + 1) order
    t.feature[0], t.threshold[0], t.left[0], t.right[0] = 1, 0.5, 3, 1
    t.feature[3], t.threshold[3], t.left[3], t.right[3] = 0, -0.25, 2, 4
    t.value = [0.0, 1.0, 2.0, 0.0, 4.0]
    feat, thr, left, val = HistGBDT._pack_tree(t)
    assert feat.tolist() == [1, 0, -1, -1, -1] and left.tolist() == [1, 3, -1, -1, -1]
    assert thr.tolist()[:2] == [0.5, -0.25] and val.tolist() == [0.0, 0.0, 1.0, 2.0, 4.0]
    g = torch.Generator().manual_seed(3)
    ok = _rand_tree(g, 4, 5, 0.3)
    feat, _, left, _ = HistGBDT._pack_tree(ok)
    assert feat.tolist() == ok.feature and left.tolist() == ok.left
    bad = _rand_tree(g, 4, 2)
    bad.left[0] = 99
    with pytest.raises(ValueError):
        HistGBDT._pack_tree(bad)


def test_save_load_predict_bit_for_bit(tmp_path):
    X, y = _binary_data(800, 6, seed=2)
    m = HistGBDT(GBDTParams(objective="binary:logistic", n_estimators=4, max_depth=4, max_bin=16), "cpu")
    m.fit(X, y)
    # a +inf threshold (the grower writes one for a split at the last bin): put one in by hand
    t = m.trees[0][0]
    node = next(i for i, f in enumerate(t.feature) if f >= 0)
    t.threshold[node] = math.inf
    path = str(tmp_path / "sub" / "model.json")
    m.save(path)
    doc = json.load(open(path))
    assert {"params", "cuts", "trees"} <= set(doc) <= {"params", "cuts", "trees", "version"}
    m2 = HistGBDT.load(path, device="cpu")
    assert m2.trees[0][0].threshold[node] == math.inf
    assert m2.p == m.p and torch.equal(m2.cuts, m.cuts)
    Xq = _rows(torch.Generator().manual_seed(9), 500, 6)
    assert torch.equal(m2.predict(Xq), m.predict(Xq))
    assert torch.equal(m2.predict(Xq, output_margin=True), m.predict_margin(Xq))


def test_load_rejects_out_of_range_feature(tmp_path):
    X, y = _binary_data(400, 4, seed=4)
    m = HistGBDT(GBDTParams(objective="binary:logistic", n_estimators=2, max_depth=2, max_bin=16), "cpu")
    m.fit(X, y)
    path = str(tmp_path / "model.json")
    m.save(path)
    doc = json.load(open(path))
    doc["trees"][1][0]["feature"][0] = 4  # cuts has rows 0..3
    json.dump(doc, open(path, "w"))
    with pytest.raises(ValueError, match=r"round 1 tree 0 splits on feature 4.*4 features"):
        HistGBDT.load(path, device="cpu")


def _contrary(n=1200, f=6, seed=3):
    """Training data and a validation set whose labels are the complement of what
    the training data implies: its loss rises from the first round."""
    X, y = _binary_data(n, f, seed)
    return X[:900], y[:900], X[900:], 1 - y[900:]


def test_early_stopping_on_rising_validation_loss():
    Xt, yt, Xv, yv = _contrary()
    m = HistGBDT(GBDTParams(objective="binary:logistic", n_estimators=20, max_depth=3, max_bin=32), "cpu")
    m.fit(Xt, yt, eval_set=(Xv, yv), early_stopping_rounds=3)
    assert len(m.trees) == 4 and len(m.evals_result) == 4  # stopped after round index 3
    assert m.best_iteration == 0 and m.best_score == m.evals_result[0]
    assert all(a < b for a, b in zip(m.evals_result, m.evals_result[1:]))
    one = HistGBDT(m.p, "cpu")
    one.cuts, one.trees = m.cuts, m.trees[:1]
    assert torch.equal(m.predict(Xv, output_margin=True), one.predict_margin(Xv))  # one round by default
    assert torch.equal(m.predict(Xv, output_margin=True, n_rounds=4), m.predict_margin(Xv))
    for i, v in enumerate(m.evals_result):
        ref = m.metric(m.predict(Xv, output_margin=True, n_rounds=i + 1), yv)["logloss"]
        assert abs(v - ref) <= 1e-5 * abs(ref)


def test_fit_without_eval_set_leaves_eval_state_alone():
    X, y = _binary_data(500, 4)
    m = HistGBDT(GBDTParams(objective="binary:logistic", n_estimators=2, max_depth=2, max_bin=16), "cpu")
    m.fit(X, y)
    assert m.evals_result == [] and m.best_iteration is None and m.best_score is None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


ES_PARAMS = dict(objective="binary:logistic", n_estimators=12, max_depth=3, max_bin=32)


def _dist_eval_worker(rank, world, port, data, out):
    import torch.distributed as dist
    torch.set_num_threads(1)
    Xt, yt, Xv, yv = data
    m = HistGBDT(GBDTParams(**ES_PARAMS), "cpu")
    # the single process's cuts, bit for bit: fitted on the full data before the process group
    # exists (inside it fit_cuts gathers every rank's sample, here the full data twice over,
    # whose quantiles interpolate differently)
    m.fit_cuts(Xt, sample=len(Xt))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m.fit(Xt[rank::world], yt[rank::world], eval_set=(Xv[rank::world], yv[rank::world]), early_stopping_rounds=3)
    out[rank] = (list(m.evals_result), len(m.trees), m.best_iteration, m.best_score)
    dist.destroy_process_group()


def test_distributed_eval_set_agrees_across_ranks_and_with_single_process():
    data = _contrary()
    Xt, yt, Xv, yv = data
    single = HistGBDT(GBDTParams(**ES_PARAMS), "cpu")
    single.fit_cuts(Xt, sample=len(Xt))
    single.fit(Xt, yt, eval_set=(Xv, yv), early_stopping_rounds=3)
    mgr = mp.Manager()
    out = mgr.dict()
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dist_eval_worker, args=(r, 2, port, data, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert out[0] == out[1], "ranks disagree on the validation metric or the stopping round"
    evals, ntrees, best_it, _ = out[0]
    assert ntrees == len(single.trees) == 4 and best_it == single.best_iteration == 0
    assert len(evals) == len(single.evals_result)
    for a, b in zip(evals, single.evals_result):
        print(f"two ranks {a!r} single {b!r} rel {abs(a - b) / abs(b):.3e}")
        assert abs(a - b) <= 1e-5 * abs(b)


def _worker(args, env_extra=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "KDL_RANK", "KDL_SANDBOX", "KDL_PROGRESS_FILE", "KDL_READY_FILE"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "-m", "kubedl_amd.workers.xgboost_dist", "--cpu", "--dataset", "iris"] + args,
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)


def _json_line(stdout):
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("{")][-1])


def test_worker_train_then_predict(tmp_path):
    import numpy as np
    model = str(tmp_path / "models" / "iris")
    common = ["--xgboost_parameter=objective:multi:softprob,num_class:3", f"--model_path={model}",
              "--model_storage_type=local"]
    r = _worker(["--job_type=Train", "--n_estimators=5", "--learning_rate=0.3"] + common)
    assert r.returncode == 0, r.stderr
    train = _json_line(r.stdout)
    assert train["job_type"] == "Train" and os.path.isfile(model + ".json")
    r = _worker(["--job_type=predict"] + common)  # case-insensitive
    assert r.returncode == 0, r.stderr
    pred = _json_line(r.stdout)
    assert pred["job_type"] == "Predict" and pred["rows"] == 150
    assert pred["accuracy"] == train["accuracy"] and pred["predict_seconds"] > 0 and pred["predict_rows_per_sec"] > 0
    out = np.load(model + ".json.pred.rank0.npy")
    assert out.shape == (150, 3) and out.dtype == np.float32 and np.allclose(out.sum(1), 1.0, atol=1e-5)


def test_worker_predict_without_model_fails(tmp_path):
    model = str(tmp_path / "nothing" / "here")
    r = _worker(["--job_type=Predict", f"--model_path={model}", "--model_storage_type=local"])
    assert r.returncode != 0
    assert "no model file" in r.stderr and model in r.stderr
    assert not os.path.exists(model + ".json")  # it did not train one


def test_worker_train_with_eval_fraction_and_early_stopping(tmp_path):
    r = _worker(["--job_type=Train", "--n_estimators=8", "--learning_rate=0.3", "--eval_fraction=0.2",
                 "--xgboost_parameter=objective:multi:softprob,num_class:3,early_stopping_rounds:4"])
    assert r.returncode == 0, r.stderr
    out = _json_line(r.stdout)
    assert out["eval_rows"] == 30 and out["rows_per_rank"] == 120 and out["eval_metric"] == "mlogloss"
    assert out["eval_last"] > 0 and 0 <= out["best_iteration"] < out["rounds"] <= 8
    assert out["best_score"] <= out["eval_last"]


def test_example_train_then_predict_jobs_succeed(tmp_path, monkeypatch):
    """examples/xgboost: the Train spec, then the Predict spec on the model it wrote,
    through ``Manager.apply`` to Succeeded (the style of tests/test_examples_e2e.py)."""
    from kubedl_amd.api import codec
    from kubedl_amd.api import common as c
    from kubedl_amd.engine.manager import Manager, ManagerOptions
    model = str(tmp_path / "models" / "iris-gbdt")
    monkeypatch.setenv("KDL_ZYGOTE", "0")
    m = Manager(ManagerOptions(home=str(tmp_path / "home"), gpus=0)).start()
    try:
        for name in ("iris_train.yaml", "iris_predict.yaml"):
            (obj,) = codec.load_file(os.path.join(ROOT, "examples", "xgboost", name))
            for spec in obj["spec"]["xgbReplicaSpecs"].values():
                ctr = spec["template"]["spec"]["containers"][0]
                ctr["args"] = [f"--model_path={model}" if a.startswith("--model_path=") else a for a in ctr["args"]]
            job = m.apply(obj)
            md = job["metadata"]
            done = m.wait_for_condition("XGBoostJob", md["namespace"], md["name"], ["Succeeded", "Failed"],
                                        timeout=240)
            assert c.last_condition_type(done["status"]) == "Succeeded", done["status"]
            if name == "iris_train.yaml":
                assert os.path.isfile(model + ".json")
        assert os.path.isfile(model + ".json.pred.rank0.npy") and os.path.isfile(model + ".json.pred.rank1.npy")
    finally:
        m.stop()
