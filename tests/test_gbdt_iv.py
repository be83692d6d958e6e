"""Interventional TreeSHAP: ``HistGBDT.set_background(X, interventional=True)`` and
``HistGBDT.predict_contribs(X, perturbation="interventional")`` (csrc/gbdt_iv.hip: the
mask-histogram and the explain kernel; on CPU ``_contribs_iv_torch``).

The reference is the definition by brute force in fp64 numpy: for every subset ``S`` of
the features the forest splits on (at most 10), ``v(S) = mean_z f_k(h(S))`` by a plain
traversal of the ``Tree`` lists over the hybrid rows, and the Shapley values from the
subset formula.  It shares no path, mask or histogram logic with the code under test.

Tolerance: ``|got - ref| <= C * 2^-24 * A_k`` per entry, ``A_k`` the summed absolute leaf
values of class k's trees (plus the base margin).  ``C`` counts the fp32 roundings of the
explain kernel (csrc/gbdt_iv.hip, path_iv) for one path with ``r`` records: ``w`` is
rounded once when stored (1), the weight table entry once (1), their product (1), one
addition per record into the register accumulator (r; the terms of a path sum to at most
1 in absolute value, so each rounding is relative to at most 1), the product with ``v``
(1) -- ``(4 + r) |v|`` per path -- and one LDS addition per table path of a partial sum of
at most ``A_k``.  ``r <= min(2^u, B)`` with ``u`` the features the forest splits on and
``B`` the background rows; a path is stored as at most two table paths (1,024 records
against 1,002 per chunk), so ``C = 4 + min(2^u, B) + 2 L_k`` with ``L_k`` the leaves of
class k.  The bias column is one rounding of an fp64 sum.  The CPU path works in fp64 and
rounds once: ``C = 2``.  The check against the margin sums ``u + 1`` such entries and adds
the margin's own count, one addition per tree and the base.
"""
import functools
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


def _chain(g, feats):
    """A chain: level d splits on ``feats[d]``, one child is a leaf (sides alternate), the
    other goes on -- leaves with 1 .. len(feats) splits above them; a feature that comes
    twice gives a merged element."""
    t = Tree()
    nid = t.add()
    for d, f in enumerate(feats):
        t.feature[nid], t.threshold[nid] = f, float(torch.randn((), generator=g)) * 0.5
        t.left[nid], t.right[nid] = t.add(), t.add()
        leaf, nid = (t.left[nid], t.right[nid]) if d % 2 else (t.right[nid], t.left[nid])
        t.value[leaf] = float(torch.randn((), generator=g))
    t.value[nid] = float(torch.randn((), generator=g))
    return t


def _rows(g, N, F):
    X = torch.randn(N, F, generator=g)
    u = torch.rand(N, F, generator=g)
    X[u < 0.06] = float("nan")
    X[(u >= 0.06) & (u < 0.09)] = math.inf
    return X


def _model(K, device, rounds):
    p = (GBDTParams(objective="multi:softprob", num_class=K, max_depth=12) if K > 1
         else GBDTParams(objective="reg:squarederror", max_depth=12))
    m = HistGBDT(p, device)
    m.trees = rounds
    return m


def _margin64(trees, X):
    out = np.zeros(len(X))
    rows = np.arange(len(X))
    for t in trees:
        feat, thr, left, right = (np.asarray(a) for a in (t.feature, t.threshold, t.left, t.right))
        node = np.zeros(len(X), dtype=np.int64)
        while (feat[node] >= 0).any():
            f = feat[node]
            nxt = np.where(X[rows, np.maximum(f, 0)] <= thr[node], left[node], right[node])  # NaN goes right
            node = np.where(f >= 0, nxt, node)
        out += np.asarray(t.value)[node]
    return out


def _brute_force(rounds, K, X, Z, base):
    N, F = X.shape
    used = sorted({f for r in rounds for t in r for f in t.feature if f >= 0})
    u = len(used)
    assert u <= 10
    val = np.empty((1 << u, N, K))
    for s in range(1 << u):
        H = np.repeat(Z[None], N, 0)  # [N, B, F]: the features in S from x, the others from z
        cols = [used[i] for i in range(u) if s >> i & 1]
        H[:, :, cols] = X[:, None, cols]
        for k in range(K):
            val[s, :, k] = _margin64([r[k] for r in rounds], H.reshape(-1, F)).reshape(N, -1).mean(1)
    phi = np.zeros((N, K, F + 1))
    for i, f in enumerate(used):
        for s in range(1 << u):
            if not s >> i & 1:
                c = bin(s).count("1")
                w = math.factorial(c) * math.factorial(u - 1 - c) / math.factorial(u)
                phi[:, :, f] += w * (val[s | 1 << i] - val[s])
    phi[:, :, F] = val[0] + base
    return phi, used


# name: (distinct rows of X, F, K, per round the chain's features, background rows (0: all 1,024 side patterns
#        of the ten thresholds), rows per block of the explain kernel)
CASES = {
    "chains_1_to_10": (6, 10, 1, [list(range(10))], 67, 256),
    "merged_nan_k3": (7, 5, 3, [[0, 2, 0, 4, 2, 1], [3, 3, 1]], 33, 256),
    "split_records": (4, 10, 1, [list(range(10))], 0, 256),
    "f100_128_rows": (5, 100, 1, [[3, 57, 99, 57], [41]], 9, 128),
    "f200_64_rows": (5, 200, 1, [[199, 3, 101], [150, 3]], 9, 64),
    "f700_no_staging_k3": (5, 700, 3, [[0, 699, 350, 0]], 9, 0),
}
CPU_CASES = ["chains_1_to_10", "merged_nan_k3", "f100_128_rows"]


@functools.lru_cache(maxsize=None)
def _case(name):
    n, F, K, chains, nb, _ = CASES[name]
    g = torch.Generator().manual_seed(len(name) * 1000 + F)
    rounds = [[_chain(g, feats) for _ in range(K)] for feats in chains]
    X = _rows(g, n, F)
    if nb:
        Z = _rows(g, nb, F)
    else:  # every combination of sides of the chain's ten thresholds: all 1,024 masks of the deepest path
        t = rounds[0][0]
        thr = torch.tensor([t.threshold[i] for i in range(len(t.feature)) if t.feature[i] >= 0])
        Z = thr + ((torch.arange(1024)[:, None] >> torch.arange(10)) & 1).float() * 2 - 1
    base = float(_model(K, "cpu", rounds)._base(1)[0, 0])
    phi, used = _brute_force(rounds, K, X.double().numpy(), Z.double().numpy(), base)
    A = np.asarray([sum(abs(v) for r in rounds for v, f in zip(r[k].value, r[k].feature) if f < 0) + abs(base)
                    for k in range(K)])
    leaves = np.asarray([sum(f < 0 for r in rounds for f in r[k].feature) for k in range(K)], dtype=np.float64)
    return rounds, X, Z, phi, A[None, :, None], leaves[None, :, None], used


def _check(got, margin, phi, A, C, used, trees_per_class):
    got, margin = got.double().cpu().numpy(), margin.double().cpu().numpy()
    err, gap = np.abs(got - phi), np.abs(got.sum(-1) - margin)
    bound = ((len(used) + 1) * C.max(-1) + trees_per_class + 1) * EPS * A[..., 0]
    print("worst |got - ref| / (C eps A):", (err / (C * EPS * A)).max(), " worst |sum - margin| / bound:",
          (gap / bound).max())
    assert (err <= C * EPS * A).all()
    assert (gap <= bound).all()
    unused = [f for f in range(phi.shape[2] - 1) if f not in used]
    assert (got[:, :, unused] == 0).all()  # null players: exactly 0


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", CPU_CASES)
def test_cpu_iv_equals_brute_force_and_sums_to_margin(case):
    rounds, X, Z, phi, A, _, used = _case(case)
    m = _model(CASES[case][2], "cpu", rounds)
    m.set_background(Z, interventional=True)
    got = m.predict_contribs(X, perturbation="interventional")
    assert got.shape == phi.shape and got.dtype == torch.float32
    _check(got, m.predict_margin(X), phi, A, np.full(phi.shape, 2.0), used, len(rounds))
    m.set_background(X[2:3], interventional=True)  # x is the single background row: D = E = 0 on every path
    assert (m.predict_contribs(X[2:3], perturbation="interventional")[:, :, :-1] == 0).all()


def test_cpu_iv_refusals():
    rounds, X, Z, _, _, _, _ = _case("merged_nan_k3")
    m = _model(3, "cpu", rounds)
    with pytest.raises(ValueError, match="background"):
        m.predict_contribs(X, perturbation="interventional")
    m.set_background(Z)  # the covers alone
    with pytest.raises(ValueError, match="interventional=True"):
        m.predict_contribs(X, perturbation="interventional")
    with pytest.raises(ValueError, match="perturbation"):
        m.predict_contribs(X, perturbation="marginal")
    m.set_background(Z, interventional=True)
    m.predict_contribs(X, perturbation="interventional")
    m.trees = m.trees[:1]  # other trees: the background no longer applies
    with pytest.raises(ValueError, match="background"):
        m.predict_contribs(X, perturbation="interventional")


def test_worker_feature_perturbation_file(tmp_path):
    from kubedl_amd.workers import xgboost_dist
    model = str(tmp_path / "models" / "iris")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "KDL_RANK", "KDL_SANDBOX", "KDL_PROGRESS_FILE", "KDL_READY_FILE"):
        env.pop(k, None)
    common = [sys.executable, "-m", "kubedl_amd.workers.xgboost_dist", "--cpu", "--dataset", "iris",
              "--xgboost_parameter=objective:multi:softprob,num_class:3", f"--model_path={model}",
              "--model_storage_type=local"]
    for extra in (["--job_type=Train", "--n_estimators=2"],
                  ["--job_type=Predict", "--pred_contribs", "--feature_perturbation", "interventional"]):
        r = subprocess.run(common + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["feature_perturbation"] == "interventional" and out["contribs"] == model + ".json.contribs.rank0.npy"
    got = np.load(out["contribs"])
    assert got.shape == (150, 3, 5) and got.dtype == np.float32
    X, _ = xgboost_dist.load_data(type("A", (), {"dataset": "iris"}), 0, 1)
    m = HistGBDT.load(model + ".json", "cpu")
    m.set_background(X, interventional=True)
    assert np.array_equal(got, m.predict_contribs(X, perturbation="interventional").numpy())
    assert not np.array_equal(got, m.predict_contribs(X).numpy())


# ------------------------------------------------------------------ GPU
def _hist_ref(rounds, K, Z):
    """The dense histogram from the Tree lists: per class, tree and leaf (left child first), the
    count of every mask; bit l belongs to the l-th distinct feature on the way down."""
    out = []

    def walk(t, i, conds):
        f = t.feature[i]
        if f < 0:
            if conds:
                mask = sum(c.astype(np.int64) << l for l, (_, c) in enumerate(conds))
                out.append(np.bincount(mask, minlength=1 << len(conds)))
            return
        go = Z[:, f] <= t.threshold[i]
        j = next((j for j, (ff, _) in enumerate(conds) if ff == f), None)
        for child, ok in ((t.left[i], go), (t.right[i], ~go)):
            walk(t, child, conds + [(f, ok)] if j is None else conds[:j] + [(f, conds[j][1] & ok)] + conds[j + 1:])
    for k in range(K):
        for r in rounds:
            walk(r[k], 0, [])
    return np.concatenate(out)


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [None, -1, 0, 1])  # B = 1, R - 1, R, R + 1
def test_gpu_mask_histogram_equals_numpy_count(delta):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    F, K = 10, 2
    R = ext.gbdt_path_masks_rows_per_block(F)
    B = 1 if delta is None else R + delta
    g = torch.Generator().manual_seed(77)
    rounds = [[_chain(g, list(range(10))) for _ in range(K)], [_chain(g, [4, 4, 9, 4]) for _ in range(K)]]
    Z = _rows(g, B, F)  # NaN and inf rows included
    m = _model(K, "cuda", rounds)
    m.set_background(Z, interventional=True)
    hist = m._iv_table(2)["hist"]
    assert hist.dtype == torch.int64 and hist.numel() > ext.gbdt_path_masks_chunk_counters()  # spans counter chunks
    assert R == 256 and 1 << 10 <= ext.gbdt_path_masks_chunk_counters()  # an m = 10 path: 1,024 counters
    assert np.array_equal(hist.cpu().numpy(), _hist_ref(rounds, K, Z.double().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_iv_kernel_equals_brute_force_and_cpu_path(case):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    _, F, K, _, _, want_rows = CASES[case]
    R = ext.gbdt_contribs_iv_rows_per_block(F)
    assert R == want_rows  # the cases are meant to cover every launch
    rounds, X, Z, phi, A, leaves, used = _case(case)
    m = _model(K, "cuda", rounds)
    m.set_background(Z, interventional=True)
    iv = m._iv_table(len(rounds))
    if case == "split_records":  # the two deepest paths hold 1,024 records each: two table paths each
        assert iv["records"] > 2048 and iv["table_paths"] == iv["paths"] + 2
    C = 4.0 + min(1 << len(used), Z.shape[0]) + 2.0 * leaves  # [1, K, 1]
    idx = torch.arange((R or 256) + 1) % X.shape[0]  # the distinct rows, tiled over more than one block
    Xt, G, F1 = X[idx].cuda(), 64, F + 1
    for n in (1, R or 256, (R or 256) + 1):
        buf = torch.full((n * K * F1 + 2 * G,), -7.0, device="cuda")
        out = buf[G:G + n * K * F1].view(n, K, F1)
        ext.gbdt_contribs_iv(Xt[:n], iv["slots"], iv["chunk_off"], iv["class_chunk"], iv["bias"], K, out)
        assert (buf[:G] == -7.0).all() and (buf[-G:] == -7.0).all()  # nothing written around the output
        assert torch.equal(out, m.predict_contribs(Xt[:n], perturbation="interventional"))  # bit-reproducible
    _check(out, m.predict(Xt, output_margin=True), phi[idx.numpy()], A, C, used, len(rounds))
    mc = _model(K, "cpu", rounds)
    mc.set_background(Z, interventional=True)
    cpu = mc.predict_contribs(X, perturbation="interventional").double().numpy()
    assert (np.abs(out[:X.shape[0]].double().cpu().numpy() - cpu) <= (C + 2.0) * EPS * A).all()
