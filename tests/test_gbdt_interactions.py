"""GBDT SHAP interaction values: ``HistGBDT.predict_interactions`` (csrc/gbdt_interactions.hip;
on CPU ``_interactions_torch``).

Reference: the definition by brute force in fp64 numpy -- ``E_t(x, S)`` as a recursion over the nodes
of the ``Tree`` (kept per leaf) for every subset ``S`` of the split features, the Shapley interaction
index as the weighted sum of ``grad_ij(S)``, the Shapley value likewise, diagonal and bias as defined
in kubedl_amd/models/gbdt.py.  Kept on the split features and the bias only: every other entry is a
null player's, exactly 0.  The random forests split on at most 7 features; the depth-10 chain needs
10 for its m = 10 path and is one tree of 11 leaves.

Tolerance: ``|got - ref| <= C * 2^-24 * A`` per entry, ``A`` the fp64 sum over (tree, leaf) of the
absolute path terms feeding the entry: ``|off_ij|`` off the diagonal, ``|c_i| + sum_j |off_ij|`` on it
(``c_i`` the leaf's contribution term), ``sum |E(empty)| + |base|`` at the bias.  ``C`` counts the fp32
roundings of pair_term for a path of m elements, Q = ceil(m / 2) <= 5 nodes:
* a factor ``o t + z (1 - t)``: z, t, 1 - t rounded once each, a product and a sum: 4, all parts >= 0;
* ``W_ij``: m - 2 factors, m - 2 products joining them and the weight (a rounded constant: + 1),
  Q - 1 sums of terms >= 0: ``5 m + Q - 10``; ``W_i``, one factor more: ``5 m + Q - 5``;
* an off-diagonal term: ``o - z`` of i and of j (stored rounded from fp64: 1 each) and the products
  ``v d_i``, ``* d_j``, ``* W_ij`` (0.5 is exact): ``5 m + Q - 5 <= 5 m``; a contribution term: ``d_i``
  and two products: ``5 m + Q - 2 <= 5 m + 3``;
* the diagonal's m - 1 subtractions each round a partial sum below the leaf's
  ``|c_i| + sum_j |off_ij|``: m - 1 more; every addition into an accumulator rounds a partial sum
  <= A, at most one per leaf ``L_k`` of the class.
With ``u >= m`` split features: ``C = 5 u + L_k`` off the diagonal, ``5 u + 3 + (u - 1) + L_k`` on it; the
bias is one rounding of an fp64 sum.  The CPU path is fp64 rounded once: half an fp32 ulp of at most
A, ``2^-24 A``, plus ``2^-40 A`` for the fp64 work on both sides (fewer than 2^12 roundings of 2^-53).
A sum over entries is checked against the sum of their bounds plus the other side's own bound:
``predict_contribs``' ``(5 u + 3 + L_k) 2^-24 sum |c_i|`` (tests/test_gbdt_contribs.py), the margin's
one addition per tree and the base, ``(T + 1) 2^-24`` of the sum of all A.
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
CPU_C = 1.0 + 2.0 ** -16  # 2^-24 A + 2^-40 A


def _tree(g, feats, depth, p_stop):
    """A random tree in the grower's append order over ``feats``; p_stop < 0: a chain that splits
    on feats[d] at depth d and goes on to the right."""
    t = Tree()
    level = [t.add()]
    for d in range(depth + 1):
        nxt = []
        for nid in level:
            t.value[nid] = float(torch.randn((), generator=g))
            if d == depth or (nid != level[-1] if p_stop < 0 else float(torch.rand((), generator=g)) < p_stop):
                continue  # a leaf (a chain: every left child)
            t.feature[nid] = feats[d] if p_stop < 0 else feats[int(torch.randint(0, len(feats), (), generator=g))]
            t.threshold[nid] = float(torch.randn((), generator=g)) * 0.5
            t.left[nid], t.right[nid] = t.add(), t.add()
            nxt += [t.left[nid], t.right[nid]]
        level = nxt
    return t


def _model(K, device, rounds):
    p = (GBDTParams(objective="multi:softprob", num_class=K, max_depth=12) if K > 1
         else GBDTParams(objective="reg:squarederror", max_depth=12))
    m = HistGBDT(p, device)
    m.trees = rounds
    return m


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


def _brute_force(rounds, K, X, B, base, used):
    """Phi, A [N, K, u + 1, u + 1] and sum |c_i| [N, K, u + 1] over ``used`` + the bias, fp64."""
    N, u, fac = len(X), len(used), math.factorial
    covers = [[_cover(t, B) for t in r] for r in rounds]
    subsets = [frozenset(s) for n in range(u + 1) for s in itertools.combinations(used, n)]
    phi, A, Ac = np.zeros((N, K, u + 1, u + 1)), np.zeros((N, K, u + 1, u + 1)), np.zeros((N, K, u + 1))
    for k in range(K):
        E = {S: np.concatenate([_leaves(r[k], c[k], X, S) for r, c in zip(rounds, covers)], 1) for S in subsets}
        absoff = np.zeros((u,) + E[subsets[0]].shape)
        for a, b in itertools.combinations(range(u), 2):
            i, j = used[a], used[b]
            term = 0.0
            for S in subsets:
                if i not in S and j not in S:
                    w = fac(len(S)) * fac(u - 2 - len(S)) / (2 * fac(u - 1))
                    # in this order a leaf whose path lacks i or j gives exactly 0, as in exact arithmetic
                    term = term + w * ((E[S | {i, j}] - E[S | {i}]) - (E[S | {j}] - E[S]))
            phi[:, k, a, b] = phi[:, k, b, a] = term.sum(1)
            A[:, k, a, b] = A[:, k, b, a] = np.abs(term).sum(1)
            absoff[a] += np.abs(term)
            absoff[b] += np.abs(term)
        for a, i in enumerate(used):
            c = sum(fac(len(S)) * fac(u - 1 - len(S)) / fac(u) * (E[S | {i}] - E[S]) for S in subsets if i not in S)
            phi[:, k, a, a] = c.sum(1) - phi[:, k, a, :u].sum(1)
            A[:, k, a, a] = (np.abs(c) + absoff[a]).sum(1)
            Ac[:, k, a] = np.abs(c).sum(1)
        phi[:, k, u, u] = E[frozenset()].sum(1) + base
        A[:, k, u, u] = Ac[:, k, u] = np.abs(E[frozenset()]).sum(1) + abs(base)
    return phi, A, Ac


# name: (F, K, rounds as (features, depth, p_stop), background rows (0: X itself), rows per block); N is R + 1
CASES = {
    "chain_m1_m2": (5, 1, [([1, 3], 2, -1.0)], 0, 256),                 # leaves with m = 1 and m = 2 (W_ij = 1)
    "chain_m10": (12, 1, [(list(range(1, 11)), 10, -1.0)], 0, 256),     # m = 1 .. 10
    "chain_resplit_zero_cover": (5, 1, [([0, 2, 0, 4, 2], 5, -1.0), ([4, 0], 2, -1.0)], 2, 256),  # merged; z = 0
    "multiclass": (6, 3, [([0, 1, 2, 4, 5], 3, 0.2)] * 2, 0, 256),
    "multi_chunk": (28, 1, [([0, 3, 9, 20, 27], 5, 0.0)] * 6, 0, 256),  # a feature's list spans LDS chunks
    "f100_128_rows": (100, 1, [([3, 41, 57, 99], 4, 0.2)] * 2, 0, 128),
    "f200_64_rows": (200, 1, [([3, 57, 101, 150, 199], 4, 0.2)] * 2, 0, 64),
    "f304_no_staging": (304, 1, [([0, 199, 303], 3, 0.0)] * 2, 0, 0),
}
CPU_CASES = ["chain_m1_m2", "chain_resplit_zero_cover", "multiclass"]


@functools.lru_cache(maxsize=None)
def _case(name):
    F, K, shapes, nb, R = CASES[name]
    N = (R or 256) + 1
    g = torch.Generator().manual_seed(len(name) * 1000 + F)
    rounds = [[_tree(g, feats, d, ps) for _ in range(K)] for feats, d, ps in shapes]
    X = torch.randn(N, F, generator=g)
    X[torch.rand(N, F, generator=g) < 0.05] = float("nan")
    B = torch.randn(nb, F, generator=g) if nb else X
    used = sorted({f for r in rounds for t in r for f in t.feature if f >= 0})
    assert len(used) <= (10 if name == "chain_m10" else 7)
    base = float(_model(K, "cpu", rounds)._base(1)[0, 0])
    phi, A, Ac = _brute_force(rounds, K, X.double().numpy(), B.double().numpy(), base, used)
    leaves = np.asarray([sum(sum(f < 0 for f in r[k].feature) for r in rounds) for k in range(K)], dtype=np.float64)
    u = len(used)
    C = np.full((K, u + 1, u + 1), 5.0 * u) + leaves[:, None, None]   # off the diagonal
    C[:, np.arange(u), np.arange(u)] = 6.0 * u + 2.0 + leaves[:, None]
    C[:, u, u] = 1.0
    return rounds, X, B, used, phi, A, Ac, C, leaves


def _check(got, contribs, margin, case, C, Cc, n):
    """``got`` against the reference's first n rows; C, Cc: the rounding counts of ``got`` and ``contribs``."""
    rounds, used, (phi, A, Ac) = _case(case)[0], _case(case)[3], [a[:n] for a in _case(case)[4:7]]
    F, u = got.shape[-1] - 1, len(used)
    got, idx = got.cpu().numpy(), np.asarray(used + [F])
    sub = got[:, :, idx][:, :, :, idx].astype(np.float64)
    assert np.count_nonzero(got) == np.count_nonzero(sub)          # unused features, row F, column F: exactly 0
    assert not sub[:, :, u, :u].any() and not sub[:, :, :u, u].any()
    bound = C * EPS * A
    gap_c = np.abs(sub.sum(-1) - contribs.double().cpu().numpy()[:, :, idx])
    gap_m = np.abs(sub.sum((-1, -2)) - margin.double().cpu().numpy())
    print("worst |got - ref| / bound:", np.nanmax(np.abs(sub - phi)[A > 0] / bound[A > 0]),
          " asymmetry / bound:", np.nanmax((np.abs(sub - sub.swapaxes(-1, -2)))[A > 0] / (2 * bound[A > 0])))
    assert (np.abs(sub - phi) <= bound).all()
    assert (np.abs(sub - sub.swapaxes(-1, -2)) <= 2 * bound).all()
    assert (gap_c <= bound.sum(-1) + Cc * EPS * Ac).all()
    assert (gap_m <= bound.sum((-1, -2)) + (len(rounds) + 1) * EPS * A.sum((-1, -2))).all()


@pytest.mark.parametrize("case", CPU_CASES)
def test_cpu_interactions_equal_brute_force_and_sum_to_contribs_and_margin(case):
    rounds, X, B, used, phi, _, _, C, _ = _case(case)
    m = _model(CASES[case][1], "cpu", rounds)
    m.set_background(B)
    got = m.predict_interactions(X[:65])
    assert got.shape == (65, CASES[case][1], X.shape[1] + 1, X.shape[1] + 1) and got.dtype == torch.float32
    assert torch.equal(got[:, :, -1, -1], m.predict_contribs(X[:65])[:, :, -1])  # the bias, exactly
    _check(got, m.predict_contribs(X[:65]), m.predict_margin(X[:65]), case, np.full(C.shape, CPU_C), CPU_C, 65)


def test_cpu_interactions_n_rounds_default_and_refusals():
    rounds, X, B, _, _, _, _, _, _ = _case("multiclass")
    m = _model(3, "cpu", rounds)
    with pytest.raises(ValueError, match="background"):
        m.predict_interactions(X)
    m.set_background(B)
    with pytest.raises(ValueError, match="features"):
        m.predict_interactions(X[:, :4])
    with pytest.raises(ValueError, match="n_rounds"):
        m.predict_interactions(X, n_rounds=3)
    m.best_iteration = 0  # as after an early stop: the default is the best round's prefix
    got = m.predict_interactions(X[:9])
    assert torch.equal(got, m.predict_interactions(X[:9], n_rounds=1))
    assert not torch.equal(got, m.predict_interactions(X[:9], n_rounds=2))


def test_worker_pred_interactions_file(tmp_path):
    from kubedl_amd.workers import xgboost_dist
    model = str(tmp_path / "models" / "iris")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "KDL_RANK", "KDL_SANDBOX", "KDL_PROGRESS_FILE", "KDL_READY_FILE"):
        env.pop(k, None)
    common = [sys.executable, "-m", "kubedl_amd.workers.xgboost_dist", "--cpu", "--dataset", "iris",
              "--xgboost_parameter=objective:multi:softprob,num_class:3", f"--model_path={model}",
              "--model_storage_type=local"]
    for extra in (["--job_type=Train", "--n_estimators=2"],
                  ["--job_type=Predict", "--pred_interactions", "--interactions_block_rows=64"]):
        r = subprocess.run(common + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["interactions_seconds"] > 0 and out["interactions"] == model + ".json.interactions.rank0.npy"
    got = np.load(out["interactions"])
    assert got.shape == (150, 3, 5, 5) and got.dtype == np.float32
    X, _ = xgboost_dist.load_data(type("A", (), {"dataset": "iris"}), 0, 1)
    m = HistGBDT.load(model + ".json", "cpu")
    m.set_background(X)
    assert np.array_equal(got, m.predict_interactions(X).numpy())  # three row blocks, the same values


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_interactions_kernel_equals_brute_force_and_cpu_path(case):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    F, K, _, _, R = CASES[case]
    assert ext.gbdt_interactions_rows_per_block(F) == R  # the cases are meant to cover every launch
    rounds, X, B, used, _, A, _, C, leaves = _case(case)
    m = _model(K, "cuda", rounds)
    m.set_background(B)
    u, N, F1 = len(used), X.shape[0], F + 1
    Cc = (5.0 * u + 3.0 + leaves)[:, None]
    contribs, margin = m.predict_contribs(X), m.predict(X, output_margin=True)
    for n in (1, N - 1, N):  # one row, a full block, a block and one row
        got = m.predict_interactions(X[:n])
        assert got.shape == (n, K, F1, F1) and got.dtype == torch.float32 and got.is_cuda
        _check(got, contribs[:n], margin[:n], case, C, Cc, n)
    pairs = m._pair_table(len(rounds), F)
    if case == "multi_chunk":
        assert int(pairs["feat_chunk"].diff().max()) > 1
    # the kernel again, into the middle of a larger buffer: nothing outside is written, and the same bits
    buf = torch.full((N * K * F1 * F1 + 2 * 1024,), -7.5, device="cuda")
    out = buf[1024:-1024].view(N, K, F1, F1)
    ext.gbdt_interactions(X.cuda(), pairs["slots"], pairs["chunk_off"], pairs["feat_chunk"],
                          m._path_table(len(rounds))["bias"], K, out)
    assert bool((buf[:1024] == -7.5).all()) and bool((buf[-1024:] == -7.5).all())
    assert torch.equal(out, got)
    if F <= 32:  # the CPU path on the same rows: both bounds together
        mc = _model(K, "cpu", rounds)
        mc.set_background(B)
        idx = np.asarray(used + [F])
        err = np.abs(got.double().cpu().numpy() - mc.predict_interactions(X).double().numpy())
        assert (err[:, :, idx][:, :, :, idx] <= (C + CPU_C) * EPS * A).all()
        assert np.count_nonzero(err) == np.count_nonzero(err[:, :, idx][:, :, :, idx])
