"""GBDT feature contributions: ``HistGBDT.set_background`` (the cover pass) and
``HistGBDT.predict_contribs`` (csrc/gbdt_shap.hip; on CPU the torch path).

The reference is the definition, by brute force in fp64 numpy: ``E_t(x, S)`` as a
recursion over the nodes of the ``Tree`` (vectorised over rows, kept per leaf) for
every subset ``S`` of the features the forest splits on, and the Shapley sum over
those subsets.  It shares no path logic with the code under test; features the
forest never splits on are null players (exactly 0).

Tolerance: ``|got - ref| <= C * 2^-24 * A`` per element, ``A[n, k, f]`` the sum over
(tree, leaf) of the absolute value of the leaf's term, from the reference.  ``C``
counts the fp32 roundings on the kernel's longest chain (csrc/gbdt_shap.hip,
path_term) for a path of ``m`` elements and ``Q = ceil(m / 2) <= 5`` nodes:

* a factor ``o t + z (1 - t)``: z is rounded once when stored, the constants t and
  1 - t once each, then one product and one sum (the fmaf rounds once, counted as
  two): the factor carries at most 4 roundings, every part being >= 0;
* the product of the m - 1 other factors: 4 (m - 1) + (m - 2) products;
* times the weight (a rounded constant, one product) and summed over the nodes
  (Q - 1 sums of terms >= 0): 2 + (Q - 1);
* times ``o - z`` (``1 - z`` is stored rounded from fp64, ``-z`` likewise: 1) and
  times v (exact): 1 + 2 products;

so a term carries at most ``5 m + Q - 2 <= 5 m + 3`` roundings relative to itself, and
its sum into one accumulator adds one rounding of a partial sum <= A per addition, at
most one per leaf ``L_k`` of the class: ``C = 5 u + 3 + L_k`` with ``u >= m`` the number
of features the forest splits on.  The bias column is one rounding of an fp64 sum.
The CPU path works in fp64 and rounds its result once: ``C = 2`` there.  The check
against the margin adds the margin's own count, one addition per tree and the base.
"""
import functools
import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubedl_amd.models.gbdt import GBDTParams, HistGBDT, Tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def _tree(g, feats, depth, p_stop):
    """A random tree in the grower's append order over the features ``feats``; one
    threshold in ten is +inf."""
    t = Tree()
    level = [t.add()]
    for d in range(depth + 1):
        nxt = []
        for nid in level:
            t.value[nid] = float(torch.randn((), generator=g))
            if d == depth or float(torch.rand((), generator=g)) < p_stop:
                continue
            t.feature[nid] = feats[int(torch.randint(0, len(feats), (), generator=g))]
            thr = float(torch.randn((), generator=g))
            t.threshold[nid] = math.inf if float(torch.rand((), generator=g)) < 0.1 else thr
            t.left[nid], t.right[nid] = t.add(), t.add()
            nxt += [t.left[nid], t.right[nid]]
        level = nxt
    return t


def _rows(g, N, F):
    X = torch.randn(N, F, generator=g)
    u = torch.rand(N, F, generator=g)
    X[u < 0.04] = float("nan")
    X[(u >= 0.04) & (u < 0.07)] = math.inf
    X[(u >= 0.07) & (u < 0.10)] = -math.inf
    return X


def _model(K, device, rounds):
    p = (GBDTParams(objective="multi:softprob", num_class=K, max_depth=12) if K > 1
         else GBDTParams(objective="reg:squarederror", max_depth=12))
    m = HistGBDT(p, device)
    m.trees = rounds
    return m


# ------------------------------------------------------------------ brute force
def _cover(t, B):
    c = np.zeros(len(t.value))
    todo = [(0, np.arange(len(B)))]
    while todo:
        i, rows = todo.pop()
        c[i] = len(rows)
        if t.feature[i] >= 0:
            go = B[rows, t.feature[i]] <= t.threshold[i]
            todo += [(t.left[i], rows[go]), (t.right[i], rows[~go])]
    return c


def _leaves(t, c, X, S, i=0):
    """[N, leaves under node i]: E(x, S) at node i, kept apart per leaf."""
    f = t.feature[i]
    if f < 0:
        return np.full((len(X), 1), t.value[i])
    L, R = _leaves(t, c, X, S, t.left[i]), _leaves(t, c, X, S, t.right[i])
    if f in S:
        go = (X[:, f] <= t.threshold[i])[:, None]  # NaN goes right
        return np.concatenate([np.where(go, L, 0.0), np.where(go, 0.0, R)], 1)
    wl, wr = (c[t.left[i]] / c[i], c[t.right[i]] / c[i]) if c[i] else (0.0, 0.0)
    return np.concatenate([wl * L, wr * R], 1)


def _brute_force(rounds, K, X, B, base):
    """phi and A, both [N, K, F + 1] fp64."""
    N, F = X.shape
    used = sorted({f for r in rounds for t in r for f in t.feature if f >= 0})
    assert len(used) <= 6
    covers = [[_cover(t, B) for t in r] for r in rounds]
    subsets = [frozenset(s) for n in range(len(used) + 1) for s in itertools.combinations(used, n)]
    phi, A = np.zeros((N, K, F + 1)), np.zeros((N, K, F + 1))
    for k in range(K):
        E = {S: np.concatenate([_leaves(r[k], c[k], X, S) for r, c in zip(rounds, covers)], 1) for S in subsets}
        for f in used:
            term = 0.0
            for S in subsets:
                if f not in S:
                    w = math.factorial(len(S)) * math.factorial(len(used) - 1 - len(S)) / math.factorial(len(used))
                    term = term + w * (E[S | {f}] - E[S])
            phi[:, k, f], A[:, k, f] = term.sum(1), np.abs(term).sum(1)
        phi[:, k, F] = E[frozenset()].sum(1) + base
        A[:, k, F] = np.abs(E[frozenset()]).sum(1) + abs(base)
    return phi, A


# name: (N, F, K, rounds as (depth, p_stop), features drawn from, background rows (0: X itself), rows per block)
CASES = {
    "single_leaf": (1, 1, 1, [(0, 0.0)], [0], 8, 256),
    "depth1_multiclass": (65, 5, 3, [(1, 0.0)] * 2, [0, 1, 2, 3, 4], 0, 256),
    "merged_paths": (257, 6, 1, [(8, 0.3)] * 3, [0, 2, 5], 0, 256),
    "depth10_full": (33, 6, 1, [(10, 0.0)], [0, 1, 2, 3, 4, 5], 257, 256),
    "small_disjoint_background": (65, 5, 1, [(5, 0.0)] * 2, [0, 1, 2, 3, 4], 8, 256),
    "f100_128_rows": (257, 100, 1, [(4, 0.2)] * 2, [3, 41, 57, 99], 0, 128),
    "f200_64_rows": (130, 200, 1, [(4, 0.2)] * 2, [3, 57, 101, 150, 199], 0, 64),
    "f400_no_staging_multiclass": (65, 400, 3, [(3, 0.2)] * 2, [0, 199, 399], 0, 0),
    "f700_no_staging": (257, 700, 1, [(4, 0.2)] * 2, [5, 350, 699], 0, 0),
}
CPU_CASES = ["single_leaf", "depth1_multiclass", "merged_paths", "small_disjoint_background"]


@functools.lru_cache(maxsize=None)
def _case(name):
    N, F, K, shapes, feats, nb, _ = CASES[name]
    g = torch.Generator().manual_seed(len(name) * 1000 + N)
    rounds = [[_tree(g, feats, d, ps) for _ in range(K)] for d, ps in shapes]
    X = _rows(g, N, F)
    B = _rows(g, nb, F) if nb else X
    base = float(_model(K, "cpu", rounds)._base(1)[0, 0])
    phi, A = _brute_force(rounds, K, X.double().numpy(), B.double().numpy(), base)
    leaves = [sum(sum(f < 0 for f in r[k].feature) for r in rounds) for k in range(K)]
    used = len({f for r in rounds for t in r for f in t.feature if f >= 0})
    return rounds, X, B, phi, A, np.asarray(leaves, dtype=np.float64)[None, :, None], used


def _check(got, margin, phi, A, C, trees_per_class):
    got, margin = got.double().cpu().numpy(), margin.double().cpu().numpy()
    err = np.abs(got - phi)
    gap = np.abs(got.sum(-1) - margin)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("worst |got - ref| / (C eps A):", np.nanmax(np.where(A > 0, err / (C * EPS * A), err * np.inf)),
              " worst |sum - margin| / bound:", np.nanmax(gap / ((C.max(-1) + trees_per_class + 1) * EPS * A.sum(-1))))
    assert (err <= C * EPS * A).all()
    assert (gap <= (C.max(-1) + trees_per_class + 1) * EPS * A.sum(-1)).all()


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", CPU_CASES)
def test_cpu_contribs_equal_brute_force_and_sum_to_margin(case):
    rounds, X, B, phi, A, _, _ = _case(case)
    K = CASES[case][2]
    m = _model(K, "cpu", rounds)
    assert m.set_background(B).dtype == torch.int64
    got = m.predict_contribs(X)
    assert got.shape == phi.shape and got.dtype == torch.float32
    _check(got, m.predict_margin(X), phi, A, np.full(phi.shape, 2.0), len(rounds))


def test_cpu_contribs_refusals():
    rounds, X, B, _, _, _, _ = _case("depth1_multiclass")
    m = _model(3, "cpu", rounds)
    with pytest.raises(ValueError, match="background"):
        m.predict_contribs(X)
    with pytest.raises(ValueError, match="empty"):
        m.set_background(X[:0])
    m.set_background(B)
    with pytest.raises(ValueError, match="features"):
        m.predict_contribs(X[:, :4])
    m.predict_contribs(X)
    m.trees = m.trees[:1]  # other trees: the covers no longer apply
    with pytest.raises(ValueError, match="background"):
        m.predict_contribs(X)


def test_worker_pred_contribs_file(tmp_path):
    from kubedl_amd.workers import xgboost_dist
    model = str(tmp_path / "models" / "iris")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "KDL_RANK", "KDL_SANDBOX", "KDL_PROGRESS_FILE", "KDL_READY_FILE"):
        env.pop(k, None)
    common = [sys.executable, "-m", "kubedl_amd.workers.xgboost_dist", "--cpu", "--dataset", "iris",
              "--xgboost_parameter=objective:multi:softprob,num_class:3", f"--model_path={model}",
              "--model_storage_type=local"]
    for extra in (["--job_type=Train", "--n_estimators=2"], ["--job_type=Predict", "--pred_contribs"]):
        r = subprocess.run(common + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["contribs_seconds"] > 0 and out["contribs"] == model + ".json.contribs.rank0.npy"
    got = np.load(out["contribs"])
    assert got.shape == (150, 3, 5) and got.dtype == np.float32
    X, _ = xgboost_dist.load_data(type("A", (), {"dataset": "iris"}), 0, 1)
    m = HistGBDT.load(model + ".json", "cpu")
    m.set_background(X)
    assert np.array_equal(got, m.predict_contribs(X).numpy())
    gap = float((torch.from_numpy(got).double().sum(-1) - m.predict_margin(X).double()).abs().max())
    assert abs(out["contribs_max_abs_sum_minus_margin"] - gap) <= 1e-12  # fp64 sums of five terms of order 1


# ------------------------------------------------------------------ GPU
# (N, F, K, rounds as (depth, p_stop)); None: one more full depth-6 tree than predict's LDS chunk holds
COVER_CASES = {
    "one_row": (1, 5, 1, [(3, 0.2)] * 2),
    "chunk_boundary": (257, 28, 1, None),
    "depth10_counts_in_global": (257, 6, 1, [(4, 0.2), (10, 0.0), (3, 0.0)]),
    "multiclass": (257, 5, 3, [(5, 0.3)] * 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(COVER_CASES))
def test_gpu_cover_equals_cpu_traversal(case):
    from kubedl_amd.ops import _ext
    N, F, K, shapes = COVER_CASES[case]
    if shapes is None:
        shapes = [(6, 0.0)] * (_ext.load().gbdt_predict_chunk_nodes() // 127 + 1)
    g = torch.Generator().manual_seed(len(case) * 1000 + N)
    rounds = [[_tree(g, list(range(F)), d, ps) for _ in range(K)] for d, ps in shapes]
    X = _rows(g, N, F)
    ref = _model(K, "cpu", rounds).set_background(X)
    got = _model(K, "cuda", rounds).set_background(X)
    assert got.dtype == torch.int64 and got.is_cuda and int(ref.sum()) > N * len(shapes) * K
    assert torch.equal(got.cpu(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_contribs_kernel_equals_brute_force_and_sums_to_margin(case):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    N, F, K, shapes, _, _, want_rows = CASES[case]
    assert ext.gbdt_contribs_rows_per_block(F) == want_rows  # the cases are meant to cover every launch
    rounds, X, B, phi, A, leaves, used = _case(case)
    m = _model(K, "cuda", rounds)
    m.set_background(B)
    got = m.predict_contribs(X)
    assert got.shape == phi.shape and got.dtype == torch.float32 and got.is_cuda
    if case == "depth10_full":
        assert m._path_table(1)["slots"].shape[0] > 8 * ext.gbdt_contribs_chunk_slots()
    C = np.broadcast_to(5.0 * used + 3.0 + leaves, phi.shape)
    _check(got, m.predict(X, output_margin=True), phi, A, C, len(rounds))
    assert torch.equal(got, m.predict_contribs(X))  # a fixed order of additions: reproducible
