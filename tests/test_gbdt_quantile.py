"""reg:absoluteerror / reg:quantileerror: the segmented quantile select (csrc/gbdt_quantile.hip and
its torch path) and the adaptive leaves against ``np.sort`` -- sorted(keys)[max(ceil(alpha n) - 1, 0)],
the product in fp64 -- compared for exact float equality (-0.0 == 0.0 counts as equal)."""
import json
import multiprocessing as mp
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubedl_amd.models.gbdt import GBDTParams, HistGBDT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 2048  # positions per chunk of the count kernel (asserted against the extension below)
ALPHAS = [0.0, 0.1, 0.25, 0.5, 0.9, 1.0]  # 0.25 n is an integer for the sizes C and 4 C
LAYOUTS = {  # segment sizes in position order
    "tiny": [1, 2, 3],
    "chunk_edges": [C - 1, C, C + 1],
    "one_segment_many_chunks": [4 * C],
    "one_odd_segment": [2 * C + 17],
    "1024_with_empty": [0 if i % 3 == 0 else (i * 7) % 13 + 1 for i in range(1023)] + [C + 5],
}
SPECIALS = [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, -1.0, 3.5, -2.25]
KEYS = {  # n, generator -> fp32 keys
    "all_equal": lambda n, g: np.full(n, 1.5, np.float32),
    "lowest_digit": lambda n, g: (0x3F800000 + g.integers(0, 256, n)).astype(np.uint32).view(np.float32),
    # the top byte varies, bit 23 stays clear: finite values of both signs
    "highest_digit": lambda n, g: ((g.integers(0, 256, n) << 24) | 0x00400000).astype(np.uint32).view(np.float32),
    "specials": lambda n, g: np.asarray(SPECIALS, np.float32)[g.integers(0, len(SPECIALS), n)],
    "ties": lambda n, g: np.round(g.standard_normal(n) * 1.5).astype(np.float32),
    "normal": lambda n, g: g.standard_normal(n).astype(np.float32),
}
GUARD = np.float32(-3e38)  # between the segments: a key that no segment may count


def _case(layout, keys):
    """keys with a guard position before, between and after the segments; lo, hi."""
    sizes = np.asarray(LAYOUTS[layout], np.int64)
    lo = np.cumsum(sizes + 1) - sizes
    hi = lo + sizes
    g = np.random.default_rng(5)
    k = np.full(int(hi[-1]) + 1, GUARD, np.float32)
    for a, b in zip(lo, hi):
        k[a:b] = KEYS[keys](b - a, g)
    return k, lo.astype(np.int32), hi.astype(np.int32)


def _ref(k, lo, hi, alpha):
    out = np.zeros(len(lo), np.float32)
    for s, (a, b) in enumerate(zip(lo, hi)):
        if b > a:
            out[s] = np.sort(k[a:b])[max(int(np.ceil(alpha * int(b - a))) - 1, 0)]
    return out


def _check_leaves(m, X, y, margin):
    """Every leaf of every tree = fp32(lr) * quantile of the fp32 residuals of its rows against the margin
    before the tree; the accumulated margin equals ``margin`` (fit's) and ``predict``'s."""
    Xn, yn = X.numpy().astype(np.float32), y.numpy().astype(np.float32)
    lr, a = np.float32(m.p.learning_rate), m._alpha()
    cur = np.full(len(yn), np.float32(m.p.base_score), np.float32)
    assert m.p.base_score == float(_ref(yn, [0], [len(yn)], a)[0])
    for (t,) in m.trees:
        node = np.zeros(len(yn), np.int64)
        feat, thr = np.asarray(t.feature), np.asarray(t.threshold, np.float32)
        left, right, val = np.asarray(t.left), np.asarray(t.right), np.asarray(t.value, np.float32)
        for _ in range(m.p.max_depth):
            f = feat[node]
            nxt = np.where(Xn[np.arange(len(yn)), np.maximum(f, 0)] <= thr[node], left[node], right[node])
            node = np.where(f < 0, node, nxt)
        res = yn - cur
        for leaf in np.unique(node):
            r = np.sort(res[node == leaf])
            assert val[leaf] == lr * r[max(int(np.ceil(a * len(r))) - 1, 0)], (leaf, len(r))
        cur = cur + val[node]
    assert np.array_equal(cur, margin.cpu().numpy()[:, 0])
    assert torch.equal(m.predict(X, output_margin=True, n_rounds=len(m.trees)).cpu(), margin.cpu())


def _early_leaf_data(n=400, seed=2):
    """A third of the rows lie far above the rest, told apart by feature 0 alone.  The root splits them off;
    one side's gradients then all agree in every round (alpha 0.5: the far rows', alpha 0.9: the others'), so no
    split of it has a positive gain and it stays one leaf at depth 1."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 4, generator=g)
    low = torch.arange(n) % 3 == 0
    X[:, 0] = torch.where(low, -3.0 - torch.rand(n, generator=g), X[:, 0].abs())
    y = torch.where(low, 100.0 + torch.randn(n, generator=g), X[:, 1] * 2 + torch.sin(3 * X[:, 2]) + X[:, 0])
    return X, y


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("keys", list(KEYS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_torch_select_equals_sort(layout, keys):
    k, lo, hi = _case(layout, keys)
    seg = np.full(len(k), -1, np.int64)
    for s, (a, b) in enumerate(zip(lo, hi)):
        seg[a:b] = s
    kt, st = torch.from_numpy(k[seg >= 0]), torch.from_numpy(seg[seg >= 0])
    for alpha in ALPHAS:
        assert np.array_equal(HistGBDT._select_torch(kt, st, len(lo), alpha).numpy(), _ref(k, lo, hi, alpha))


@pytest.mark.parametrize("alpha", [0.1, 0.9])
def test_cpu_fit_covers_alpha_stops_at_the_minimum_and_round_trips(alpha, tmp_path):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(2500, 5, generator=g)
    y = X[:, 0] * 1.5 - X[:, 1] ** 2 + (0.5 + X[:, 2].abs()) * torch.randn(2500, generator=g)
    Xv, yv, X, y = X[2000:], y[2000:], X[:2000], y[:2000]
    m = HistGBDT(GBDTParams(objective="reg:quantileerror", quantile_alpha=alpha, n_estimators=40, max_depth=3,
                            learning_rate=0.3, base_score=123.0), "cpu")
    margin = m.fit(X, y, eval_set=(Xv, yv), early_stopping_rounds=3)
    _check_leaves(m, X, y, margin)
    assert abs(float((y < margin[:, 0]).float().mean()) - alpha) <= 0.1
    d = y.double().numpy() - margin[:, 0].double().numpy()
    assert abs(m.metric(margin, y)["quantile"] - np.maximum(alpha * d, (alpha - 1) * d).mean()) <= 1e-12
    assert m.eval_metric == "quantile"
    assert m.best_score == min(m.evals_result) and m.best_iteration == int(np.argmin(m.evals_result))
    m.save(str(tmp_path / "q.json"))
    back = HistGBDT.load(str(tmp_path / "q.json"), "cpu")
    assert back.p.quantile_alpha == alpha and back.p.base_score == m.p.base_score != 123.0
    assert torch.equal(back.predict(Xv, n_rounds=len(m.trees)), m.predict(Xv, n_rounds=len(m.trees)))


def test_cpu_absolute_error_leaves_metric_and_refusals():
    X, y = _early_leaf_data()
    m = HistGBDT(GBDTParams(objective="reg:absoluteerror", n_estimators=3, max_depth=3, quantile_alpha=0.9), "cpu")
    margin = m.fit(X, y)
    assert m._alpha() == 0.5
    _check_leaves(m, X, y, margin)
    assert abs(m.metric(margin, y)["mae"] - np.abs(y.double().numpy() - margin[:, 0].double().numpy()).mean()) <= 1e-12
    for bad in (0.0, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="quantile_alpha"):
            HistGBDT(GBDTParams(objective="reg:quantileerror", quantile_alpha=bad), "cpu").fit(X, y)
    y_nan = y.clone()
    y_nan[7] = float("nan")
    with pytest.raises(ValueError, match="NaN label"):
        HistGBDT(GBDTParams(objective="reg:quantileerror"), "cpu").fit(X, y_nan)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fit_values(cuts, Xs, ys):
    m = HistGBDT(GBDTParams(objective="reg:absoluteerror", n_estimators=3, max_depth=3, max_bin=32), "cpu")
    m.cuts = cuts  # given, so that both runs quantise identically
    m.fit(Xs, ys)
    return m.p.base_score, [(t.feature, t.split_bin, t.value) for (t,) in m.trees]


def _dist_worker(rank, world, port, cuts, X, y, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    out[rank] = _fit_values(cuts, X[rank::world], y[rank::world])
    dist.destroy_process_group()


def test_two_gloo_ranks_give_the_leaves_of_one_rank():
    """g = +-0.5 and h = 1 sum exactly in fp32, so the ranks' all-reduced histograms, the trees and the
    (integer-counted) quantiles are those of one process on all rows."""
    X, y = _early_leaf_data(600, seed=4)
    one = HistGBDT(GBDTParams(max_bin=32), "cpu")
    one.fit_cuts(X, sample=len(X))
    out, port = mp.Manager().dict(), _free_port()
    procs = [mp.get_context("spawn").Process(target=_dist_worker, args=(r, 2, port, one.cuts, X, y, out))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert out[0] == out[1] == _fit_values(one.cuts, X, y)


def test_worker_runs_the_example_train_jobs(tmp_path):
    from kubedl_amd.api import codec
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "KDL_RANK", "KDL_SANDBOX", "KDL_PROGRESS_FILE", "KDL_READY_FILE"):
        env.pop(k, None)
    share = []
    for obj in codec.load_file(os.path.join(ROOT, "examples", "xgboost", "quantile_train.yaml")):
        args = obj["spec"]["xgbReplicaSpecs"]["Master"]["template"]["spec"]["containers"][0]["args"]
        small = ["--cpu", "--rows=3000", "--n_estimators=8", f"--model_path={tmp_path / 'q'}"]
        r = subprocess.run([sys.executable, "-m", "kubedl_amd.workers.xgboost_dist"] + args + small, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert out["objective"] == "reg:quantileerror" and out["eval_metric"] == "quantile" and out["quantile"] > 0
        share.append(HistGBDT.load(str(tmp_path / "q") + ".json", "cpu").p.quantile_alpha)
    assert share == [0.1, 0.9]


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("keys", list(KEYS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_select_equals_sort(layout, keys):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    assert ext.gbdt_quantile_chunk_rows() == C
    k, lo, hi = _case(layout, keys)
    kd, lod, hid = torch.from_numpy(k).cuda(), torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    for alpha in ALPHAS:
        got = ext.gbdt_segment_quantile(kd, lod, hid, alpha)
        assert np.array_equal(got.cpu().numpy(), _ref(k, lo, hi, alpha)), alpha
        again = ext.gbdt_segment_quantile(kd, lod, hid, alpha)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    assert np.array_equal(kd.cpu().numpy().view(np.int32), k.view(np.int32))  # the keys are only read


@pytest.mark.gpu
def test_gpu_select_refusals():
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    k, b = torch.zeros(8, device="cuda"), torch.tensor([0, 8], dtype=torch.int32, device="cuda")
    lo, hi = b[:1], b[1:]
    assert float(ext.gbdt_segment_quantile(k, lo, hi, 0.5)) == 0.0
    for args in [(k.double(), lo, hi, 0.5), (k.cpu(), lo, hi, 0.5), (k.view(2, 4), lo, hi, 0.5), (k[::2], lo, hi, 0.5),
                 (k, lo.long(), hi, 0.5), (k, lo.cpu(), hi, 0.5), (k, lo, b, 0.5),
                 (k, lo[:0], hi[:0], 0.5), (k, torch.zeros(1025, dtype=torch.int32, device="cuda"),
                                            torch.zeros(1025, dtype=torch.int32, device="cuda"), 0.5),
                 (k, lo, hi, -0.01), (k, lo, hi, 1.01), (k, lo, hi, float("nan"))]:
        with pytest.raises(RuntimeError, match="gbdt_segment_quantile"):
            ext.gbdt_segment_quantile(*args)


@pytest.mark.gpu
@pytest.mark.parametrize("obj,alpha", [("reg:absoluteerror", 0.5), ("reg:quantileerror", 0.9)])
def test_gpu_fit_renews_every_leaf(obj, alpha):
    X, y = _early_leaf_data()
    m = HistGBDT(GBDTParams(objective=obj, quantile_alpha=alpha, n_estimators=3, max_depth=3), "cuda")
    margin = m.fit(X, y)
    assert m.stats["hist_builds"] > 0  # the device grower grew the trees
    for (t,) in m.trees:  # a leaf at depth 1 beside leaves at depth 3
        assert min(t.feature[1], t.feature[2]) < 0 and max(t.feature[1], t.feature[2]) >= 0 and max(t.feature[3:7]) >= 0
    _check_leaves(m, X, y, margin)


@pytest.mark.gpu
def test_gpu_per_pass_renewal_equals_the_one_call():
    """The count / step methods that several ranks interleave with their all-reduce, on one rank."""
    X, y = (t.cuda() for t in _early_leaf_data())
    m = HistGBDT(GBDTParams(objective="reg:quantileerror", quantile_alpha=0.9, max_depth=3), "cuda")
    m.fit_cuts(X)
    gr = m._device_grower(m.quantise(X).contiguous())
    pred = torch.zeros(len(y), 1, device="cuda")
    g, h = m._grad_hess(pred, y)
    gr.grow_local(g[:, 0].contiguous(), h[:, 0].contiguous())
    feat, val = gr.tree()[0], gr.tree()[3]
    gr.renew_leaves(y, pred, 0, 0.9)
    one = val.clone()
    val.fill_(7.0)
    for p in range(4):
        table = gr.leaf_count(p, y, pred, 0)
        assert table.dtype == torch.int64 and tuple(table.shape) == (8, 256)
        assert p > 0 or int(table.sum()) == len(y)
        gr.leaf_step(p, 0.9)
        assert int(table.abs().sum()) == 0  # the step leaves the table clean
    written = val != 7.0
    assert int(written.sum()) == int((feat >= 0).sum()) + 1 and torch.equal(val[written], one[written])


@pytest.mark.gpu
def test_gpu_grad_hess_code_3():
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    g = torch.Generator().manual_seed(1)
    pred, y = torch.randn(1000, 1, generator=g).cuda(), torch.randn(1000, generator=g).cuda()
    pred[:10, 0] = y[:10]  # pred == y takes the lower branch
    for alpha in (0.5, 0.9):
        gq, hq = ext.gbdt_grad_hess(pred, y, 3, alpha) if alpha != 0.5 else ext.gbdt_grad_hess(pred, y, 3)
        a = np.float32(alpha)
        assert np.array_equal(gq.cpu().numpy()[:, 0], np.where((pred[:, 0] > y).cpu().numpy(), np.float32(1) - a, -a))
        assert bool((hq == 1).all())
    for code in (0, 1):  # the default argument leaves the other codes alone
        for u, v in zip(ext.gbdt_grad_hess(pred, y, code), ext.gbdt_grad_hess(pred, y, code, 0.9)):
            assert torch.equal(u, v)
    g0, _ = ext.gbdt_grad_hess(pred, y, 0)
    assert torch.equal(g0, pred - y[:, None])
    p3, y3 = pred.expand(-1, 3).contiguous(), (y > 0).float() * 2
    for u, v in zip(ext.gbdt_grad_hess(p3, y3, 2), ext.gbdt_grad_hess(p3, y3, 2, 0.1)):
        assert torch.equal(u, v)
