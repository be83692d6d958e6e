"""Learning to rank in the GBDT: ``rank:pairwise`` / ``rank:ndcg`` gradients (csrc/gbdt_rank.hip; on
CPU the torch path) and the ``ndcg@k`` metric, against the definition in kubedl_amd/models/gbdt.py's
module docstring.

The reference is that definition as a plain fp64 numpy double loop over the pairs of each group
(the inner loop written as one numpy expression over j, or the 2,500-row case would take a minute);
positions come from a stable argsort of the negated fp32 scores; ``1 - rho`` is ``1 / (1 + exp(-d))``.
It shares no code with the code under test.  Positions (through ``disc = D[pos]``) are compared exactly.

Tolerance, per row: ``|got - ref| <= C * 2^-24 * A_i``, ``A_i = sum_j |term_ij|`` from the reference.
``C`` counts, in roundings of relative size 2^-24 (an operation documented to 1 ulp counts 2), the
kernel's longest chain (csrc/gbdt_rank.hip, pair_term), the h term ``sm * r * w``:

* ``a = expf(-|d|)``: 2 (1 ulp); ``1 + a``: 1; the division: 1 -- r carries 4, ``sm = a * r`` 5;
* ``w``: the integer gain difference converted once (1), ``|D_i - D_j|`` (1), two products (2): 4
  (D and inv_idcg are the shared fp32 values, exact inputs);
* ``sm * r``: 5 + 4 + 1, times w: + 4 + 1 -- 15 (the g term ``rho * w`` carries 10);
* the rounding of ``d = s_hi - s_lo`` moves d by at most ``|d| 2^-24`` and rho, 1 - rho and
  rho (1 - rho) by at most that relative amount: ``R`` = the case's score range bounds ``|d|``;
* one addition per j into a partial sum of at most A_i: ``n_q``.

``C = 15 + R + n_q``.  The CPU path works in fp64 and rounds once: ``C = 2``.

Underflow: the bound above is relative, and fp32 has no relative precision below its smallest normal
number.  A saturated pair (d = 120: rho = 8e-53, which the kernel must return as exactly 0) has terms
that no fp32 result can hold, so each path gets the absolute term its format forces, ``U``: the CPU
path's one rounding to fp32 errs by at most the smallest subnormal, ``U = 2^-149``; in the kernel every
term may pass through a subnormal (or flushed) intermediate, an error of at most 2^-126 times the
remaining factors, and ``w <= |D_i - D_j| / D[n_q - 1] <= log2(n_q + 1) <= 32``: ``U = 32 n_q 2^-126``
(4e-35 for the longest group here; the hessian's own floor is 1e-16).  The check is
``|got - ref| <= C * 2^-24 * A_i + U``.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubedl_amd.models.gbdt import GBDTParams, HistGBDT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
OBJECTIVES = ["rank:pairwise", "rank:ndcg"]


# ------------------------------------------------------------------ the definition, by loops
def _disc_table(n):
    return (1.0 / np.log2(np.arange(n) + 2.0)).astype(np.float32)


def _positions(s):
    pos = np.empty(len(s), dtype=np.int64)
    pos[np.argsort(-s, kind="stable")] = np.arange(len(s))
    return pos


def _ref_grad(s, y, sizes, ndcg):
    """g, h, A_g, A_h (fp64) and disc (fp32) of fp32 scores s, integer labels y."""
    D = _disc_table(max(sizes))
    g, h, ag, ah = (np.zeros(len(s)) for _ in range(4))
    disc = np.zeros(len(s), dtype=np.float32)
    o = 0
    for n in sizes:
        sq, yq = s[o:o + n].astype(np.float64), y[o:o + n]
        G = 2.0 ** yq - 1.0
        Dq = D[_positions(s[o:o + n])]
        disc[o:o + n] = Dq
        idcg = float(np.sum(np.sort(G)[::-1] * D[:n].astype(np.float64)))
        inv = float(np.float32(1.0 / idcg)) if idcg > 0 else 0.0
        Dq = Dq.astype(np.float64)
        for i in range(n):  # the loop over j is a numpy expression over the rows with another label
            j = np.flatnonzero(yq != yq[i])
            hi = yq[i] > yq[j]
            d = np.where(hi, sq[i] - sq[j], sq[j] - sq[i])
            rho, one_minus = 1.0 / (1.0 + np.exp(d)), 1.0 / (1.0 + np.exp(-d))
            w = np.abs(G[i] - G[j]) * np.abs(Dq[i] - Dq[j]) * inv if ndcg else np.ones(len(j))
            g[o + i] = np.sum(np.where(hi, -1.0, 1.0) * rho * w)
            h[o + i] = ah[o + i] = np.sum(rho * one_minus * w)
            ag[o + i] = np.sum(rho * w)
        o += n
    return g, np.maximum(h, float(np.float32(1e-16))), ag, ah, disc


def _ref_ndcg(s, y, sizes, k):
    """ndcg@k per group, and the number of terms added into each DCG."""
    D = _disc_table(max(sizes)).astype(np.float64)
    out, terms, o = [], [], 0
    for n in sizes:
        G = 2.0 ** y[o:o + n] - 1.0
        pos = _positions(s[o:o + n])
        top = n if k == 0 else min(k, n)
        dcg = sum(G[i] * D[pos[i]] for i in range(n) if pos[i] < top)
        idcg = float(np.sum(np.sort(G)[::-1][:top] * D[:top]))
        out.append(dcg / idcg if idcg > 0 else 1.0)
        terms.append(top)
        o += n
    return np.array(out), np.array(terms)


# name: (group sizes, scores: "randn" | "equal" | "five" | "sat", labels: "grades" | "one")
CASES = {
    "cpu_small": ([1, 2, 3, 7], "randn", "grades"),
    "cpu_round0": ([1, 2, 3, 7], "equal", "grades"),
    "cpu_one_label": ([3, 7], "randn", "one"),
    "cpu_zero_group": ([7, 3], "randn", "zero_first"),
    "cpu_saturated": ([2, 7], "sat", "grades"),
    "wave": ([1, 2, 63, 64], "randn", "grades"),
    "first_block_group": ([65, 64, 1], "randn", "grades"),
    "tile_edge": ([256, 257], "randn", "grades"),
    "chunk_edge": ([1023, 1024, 1025], "randn", "grades"),
    "tiles_and_chunks": ([2500], "randn", "grades"),
    "ties_equal": ([300], "equal", "grades"),
    "ties_five": ([300], "five", "grades"),
    "one_label": ([130], "randn", "one"),
    "saturated": ([70], "sat", "grades"),
}
CPU_CASES = [c for c in CASES if c.startswith("cpu_")]
GPU_CASES = [c for c in CASES if not c.startswith("cpu_")]
_inputs = {}


def _case(name):
    """(s fp32, y int64, sizes, score range R) and the reference per objective, computed once."""
    if name not in _inputs:
        sizes, scores, labels = CASES[name]
        N = sum(sizes)
        g = torch.Generator().manual_seed(1000 + len(name) + N)
        s = {"randn": lambda: 2.0 * torch.randn(N, generator=g),
             "equal": lambda: torch.full((N,), 0.25),
             "five": lambda: torch.randint(0, 5, (N,), generator=g).float() * 0.5 - 1.0,
             "sat": lambda: torch.randint(0, 2, (N,), generator=g).float() * 120.0 - 60.0}[scores]()
        y = torch.randint(0, 5, (N,), generator=g)
        if labels == "one":
            y[:] = 3
        elif labels == "zero_first":
            y[:sizes[0]] = 0
        y[0] = 31 if labels == "grades" and N > 64 else y[0]  # the largest gain, once
        s_np, y_np = s.numpy(), y.numpy()
        refs = {obj: _ref_grad(s_np, y_np, sizes, obj == "rank:ndcg") for obj in OBJECTIVES}
        _inputs[name] = (s, y, sizes, float(s.max() - s.min()), refs)
    return _inputs[name]


def _check_grad(name, obj, device, C_of):
    s, y, sizes, R, refs = _case(name)
    g_ref, h_ref, ag, ah, disc_ref = refs[obj]
    m = HistGBDT(GBDTParams(objective=obj), device)
    rk = m._rank_setup(y.to(device), sizes)
    pred = s.to(device).view(-1, 1).contiguous()
    if device == "cpu":
        g, h, disc = m._rank_grad_hess_torch(pred.view(-1), rk)
    else:
        g, h = m._grad_hess(pred, y, rk)
        g2, h2 = m._grad_hess(pred, y, rk)
        assert torch.equal(g, g2) and torch.equal(h, h2)  # no atomics: bit-reproducible
        assert g.shape == (len(s), 1) and g.is_cuda
        disc = rk["disc"]
    if obj == "rank:ndcg":
        assert np.array_equal(disc.cpu().numpy(), disc_ref)  # the positions, exactly
    C, U = np.repeat(np.array([C_of(R, n) for n in sizes]), sizes, axis=0).T
    for got, ref, A in ((g, g_ref, ag), (h, h_ref, ah)):
        err = np.abs(got.double().cpu().numpy().reshape(-1) - ref)
        print(name, obj, "largest error over bound:", float(np.max(err / (C * EPS * A + U))))
        assert np.all(err <= C * EPS * A + U)
    if CASES[name][2] == "one":
        assert not g.any() and bool((h == 1e-16).all())


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("obj", OBJECTIVES)
@pytest.mark.parametrize("name", CPU_CASES)
def test_cpu_gradient_equals_pair_loops(name, obj):
    _check_grad(name, obj, "cpu", lambda R, n: (2.0, 2.0 ** -149))


@pytest.mark.parametrize("k", [0, 1, 3])
def test_cpu_metric_equals_loop_ndcg(k):
    sizes = [2, 7, 3, 1]  # a group shorter than k = 3, and (labels below) one with IDCG = 0
    g = torch.Generator().manual_seed(5)
    s, y = torch.randn(13, generator=g), torch.randint(0, 5, (13,), generator=g)
    y[9:12] = 0
    m = HistGBDT(GBDTParams(objective="rank:ndcg", eval_at=k), "cpu")
    ref, _ = _ref_ndcg(s.numpy(), y.numpy(), sizes, k)
    assert ref[2] == 1.0
    got = m.metric(s.view(-1, 1), y, group=sizes)
    assert list(got) == ["ndcg" if k == 0 else f"ndcg@{k}"]
    assert abs(got[m._ndcg_name()] - ref.mean()) <= 16 * 2.0 ** -53  # fp64 sums of at most 7 terms <= 1


def test_refusals():
    X, y = torch.randn(6, 2), torch.tensor([0, 1, 2, 0, 1, 2])
    rank = HistGBDT(GBDTParams(objective="rank:ndcg", n_estimators=1), "cpu")
    with pytest.raises(ValueError, match="group"):
        rank.fit(X, y)
    with pytest.raises(ValueError, match="group"):
        HistGBDT(GBDTParams(objective="binary:logistic"), "cpu").fit(X, (y > 0).long(), group=[6])
    for bad in ([3, 0, 3], [4, -1, 3], [3, 4]):
        with pytest.raises(ValueError, match="group"):
            rank.fit(X, y, group=bad)
    for bad in (torch.tensor([0, 1, 2, 0, 1, 32]), torch.tensor([0, 1, 2, 0, 1, -1])):
        with pytest.raises(ValueError, match="labels"):
            rank.fit(X, bad, group=[3, 3])
    with pytest.raises(ValueError, match="eval_set"):
        rank.fit(X, y, group=[3, 3], eval_set=(X, y))
    with pytest.raises(ValueError, match="group"):
        rank.metric(torch.zeros(6, 1), y)


def _synthetic(seed, groups, lo, hi):
    """Groups of lo..hi rows whose 0-4 grade is a noisy monotone function of feature 0."""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(lo, hi + 1, (groups,), generator=g)
    N = int(sizes.sum())
    X = torch.randn(N, 4, generator=g)
    y = torch.bucketize(X[:, 0] + 0.3 * torch.randn(N, generator=g), torch.tensor([-1.0, -0.3, 0.3, 1.0]))
    return X, y, sizes


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_cpu_fit_improves_ndcg_stops_at_the_maximum_and_round_trips(obj, tmp_path):
    X, y, sizes = _synthetic(3, 40, 2, 12)
    Xv, yv, sv = _synthetic(4, 30, 2, 12)
    m = HistGBDT(GBDTParams(objective=obj, n_estimators=12, max_depth=2, learning_rate=0.5, eval_at=3), "cpu")
    margin = m.fit(X, y, group=sizes, eval_set=(Xv, yv, sv), early_stopping_rounds=3)
    ev = m.evals_result
    assert m.eval_metric == "ndcg@3" and len(ev) == len(m.trees) and ev[-1] > ev[0]
    assert m.best_score == max(ev) and m.best_iteration == ev.index(max(ev))  # the maximum, first reached
    assert len(ev) == min(12, m.best_iteration + 1 + 3)
    assert torch.equal(m.predict(X, output_margin=True, n_rounds=len(m.trees)), margin)
    assert abs(m.metric(m.predict(Xv, output_margin=True), yv, group=sv)["ndcg@3"] - m.best_score) <= 1e-12
    m.save(str(tmp_path / "rank.json"))
    back = HistGBDT.load(str(tmp_path / "rank.json"), "cpu")
    assert back.p.objective == obj and back.p.eval_at == 3
    assert torch.equal(back.predict(Xv, n_rounds=len(m.trees)), m.predict(Xv, n_rounds=len(m.trees)))


def test_worker_trains_and_predicts_a_ranking_model(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "KDL_RANK", "KDL_SANDBOX", "KDL_PROGRESS_FILE", "KDL_READY_FILE"):
        env.pop(k, None)
    common = [sys.executable, "-m", "kubedl_amd.workers.xgboost_dist", "--cpu", "--dataset", "synthetic",
              "--objective_hint", "rank", "--rows", "2000", "--n_estimators", "5", "--max_depth", "3",
              "--xgboost_parameter=objective:rank:ndcg,eval_at:10", f"--model_path={tmp_path / 'rank'}"]
    outs = []
    for job in ("Train", "Predict"):
        r = subprocess.run(common + [f"--job_type={job}"], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    assert outs[0]["objective"] == "rank:ndcg" and 0.5 < outs[0]["ndcg@10"] <= 1.0
    assert outs[1]["ndcg@10"] == outs[0]["ndcg@10"]  # the same rows, groups and trees


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("obj", OBJECTIVES)
@pytest.mark.parametrize("name", GPU_CASES)
def test_gpu_pair_kernels_equal_pair_loops(name, obj):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    assert (ext.gbdt_rank_wave_max(), ext.gbdt_rank_tile_rows(), ext.gbdt_rank_chunk_rows()) == (64, 256, 1024)
    _check_grad(name, obj, "cuda", lambda R, n: (15.0 + R + n, 32.0 * n * 2.0 ** -126))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 10])
def test_gpu_ndcg_kernel_equals_loop_ndcg(k):
    from kubedl_amd.ops import _ext
    sizes = CASES["first_block_group"][0] + CASES["tile_edge"][0] + [3]
    g = torch.Generator().manual_seed(11)
    N = sum(sizes)
    s, y = torch.randn(N, generator=g).round(decimals=1), torch.randint(0, 5, (N,), generator=g)  # with ties
    y[-3:] = 0
    m = HistGBDT(GBDTParams(objective="rank:ndcg", eval_at=k), "cuda")
    rk = m._rank_setup(y.cuda(), sizes, plan=False)
    dcg = _ext.load().gbdt_rank_ndcg(s.cuda(), rk["y"], rk["ptr"], rk["dtab"], rk["max_group"], k)
    ref, terms = _ref_ndcg(s.numpy(), y.numpy(), sizes, k)
    idcg = rk["idcg_k"].cpu().numpy()
    got = np.where(idcg > 0, dcg.cpu().numpy() / np.where(idcg > 0, idcg, 1.0), 1.0)
    # per added term one product and one sum, the same for the ideal DCG, and the division
    assert np.all(np.abs(got - ref) <= (4 * terms + 1) * 2.0 ** -53 * np.maximum(ref, 1.0))
    assert abs(m.metric(s.view(-1, 1), y, group=sizes)[m._ndcg_name()] - ref.mean()) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_gpu_fit_runs_both_kernel_paths_and_improves_ndcg(obj):
    X, y, sizes = _synthetic(7, 200, 5, 150)
    Xv, yv, sv = _synthetic(8, 60, 5, 150)
    assert int(sizes.min()) <= 64 < int(sizes.max())
    m = HistGBDT(GBDTParams(objective=obj, n_estimators=10, max_depth=4, eval_at=10), "cuda")
    margin = m.fit(X, y, group=sizes, eval_set=(Xv, yv, sv))
    assert len(m.trees) == 10 and m.stats["hist_builds"] > 0 and m.evals_result[-1] > m.evals_result[0]
    assert torch.equal(m.predict(X, output_margin=True), margin)
