"""Distributed histogram gradient-boosted trees (the XGBoostJob data plane).

XGBoost's ``hist`` algorithm, depth-wise, re-designed for one GPU per rank:

* features quantised once to <= 256 bins (uint8 [N, F]) with quantile cuts
  agreed on by all ranks (samples all-gathered, every rank computes the same
  cuts -- the role of XGBoost's distributed sketch);
* per level: gradient/hessian histograms of every active node built by the
  ``gbdt_hist`` HIP kernel (LDS atomics, lane = feature), ALL-REDUCED across
  ranks (RCCL over xGMI; the rabit tree-allreduce of the reference's image),
  best split per (node, feature) by the ``gbdt_split`` kernel (block scan over
  bins + XGBoost gain), rows routed by ``gbdt_route`` and regrouped by a
  stable sort on child id;
* histogram subtraction: below the root only the smaller child of each split
  is built; its sibling is ``parent - child`` (halves the histogram work);
* objectives ``reg:squarederror``, ``binary:logistic``, ``multi:softprob``
  (one tree per class per round, as XGBoost).

On the GPU a tree never leaves the device while it grows: the native
``GbdtGrower`` (csrc/gbdt_grower.cpp over csrc/gbdt.hip) keeps nodes in heap
order, rows grouped per node by a stable in-segment partition, and the split
decisions, child segments and smaller-child choice in device arrays; the host
only enqueues a fixed kernel sequence per level (plus the two all-reduces per
level with several ranks).  The trees' heap arrays are copied to the host once,
at the end of ``fit``.  Quantisation is one kernel (``gbdt_quantise``).

Every rank holds a row shard; all ranks grow identical trees because they
see identical all-reduced histograms.  On CPU (or without the extension)
the same algorithm runs on torch ops -- that path is the numerics reference
for the kernels in tests.

Inference: ``predict`` packs the trees into a node table once and runs the
forest kernel (csrc/gbdt_predict.hip: one lane per row, rows and whole trees
staged in LDS, leaves added in tree order -- bit-identical to
``predict_margin``, the torch traversal, which is also the CPU path).  The
same kernel over a tree range advances the validation margin of
``fit(eval_set=...)`` straight from the grower's heap arrays (early stopping,
``evals_result``).  ``save`` / ``load`` keep a model as JSON.

Feature contributions: ``set_background`` counts the background rows that reach
each node (the covers) and ``predict_contribs`` returns exact path-dependent
TreeSHAP values [N, K, F + 1] (csrc/gbdt_shap.hip: the cover kernel and the
contribution kernel over a host-built table of root-to-leaf paths; on CPU the
same path formula on torch ops in fp64).

Interaction values: ``predict_interactions`` returns fp32 [N, K, F + 1, F + 1] in
XGBoost's ``pred_interactions`` layout (csrc/gbdt_interactions.hip over a
per-feature table of the same paths; on CPU ``_interactions_torch``, fp64 rounded
once).  The definition, shared by both paths and by the tests, in the notation of
csrc/gbdt_shap.hip (a path of class k: leaf value v, m <= 10 merged elements with
feature f_l, zero fraction z_l and o_l in {0, 1} the interval test on the row):

* ``i != j``, both ``< F``: ``Phi[n, k, i, j]`` is the sum, over the paths of class k
  that hold both features, of ``0.5 * v * (o_i - z_i) * (o_j - z_j) * W_ij`` with
  ``W_ij = int_0^1 prod_{l != i, j} (o_l t + z_l (1 - t)) dt`` -- the Shapley
  interaction index of ``S -> E_t(x, S)``; ``s! (m - 2 - s)! / (m - 1)!`` is the Beta
  integral of ``t^s (1 - t)^(m - 2 - s)``.  ``W_ij = 1`` for ``m = 2``; a path with
  ``m = 1`` has no off-diagonal term.
* Diagonal: ``Phi[n, k, i, i] = phi_i - sum_{j != i} Phi[n, k, i, j]`` with ``phi_i``
  the contribution of ``predict_contribs``, per path ``v (o_i - z_i) W_i``.
* Bias: ``Phi[n, k, F, F] = bias[k]`` (the fp64-summed bias of ``predict_contribs``,
  paths with ``m = 0`` included); the rest of row ``F`` and column ``F`` is 0.
* So the matrix is symmetric up to rounding, its last axis sums to
  ``predict_contribs`` and both axes sum to the raw margin.

Every integrand has degree at most ``m - 1``: Gauss-Legendre with ``ceil(m / 2)``
nodes is exact for ``W_i`` and ``W_ij``.

Interventional contributions: ``set_background(X, interventional=True)`` keeps the
background rows and ``predict_contribs(X, perturbation="interventional")`` returns the
interventional (marginal) TreeSHAP values, fp32 [N, K, F + 1] (csrc/gbdt_iv.hip: a
mask-histogram kernel over the background and an explain kernel over the compacted
histogram; on CPU ``_contribs_iv_torch``, fp64 over the background rows themselves,
rounded once).  The definition, shared by both paths and by the tests, in the notation
of csrc/gbdt_shap.hip (a path of class k: leaf value v, m <= 10 merged elements with
feature f_l and o_l(r) in {0, 1} the interval test on row r; NaN fails every left and
passes every right condition; ``full = 2^m - 1``; ``mask(r)`` has bit l = o_l(r)):

* For a row x and a background row z the hybrid row ``h(S)`` takes the features in S
  from x and the others from z.  The path's game ``S -> v * [h(S) reaches the leaf]`` is
  a conjunction.  With ``mx = mask(x)``, ``mz = mask(z)``: if ``(mx | mz) != full`` the
  path contributes nothing; otherwise let ``D = mx & ~mz`` with ``a = popcount(D)`` and
  ``E = mz & ~mx`` with ``b = popcount(E)``: every element in D gets
  ``+v (a-1)! b! / (a+b)!``, every element in E gets ``-v a! (b-1)! / (a+b)!``, elements
  with both bits set are dummies.
* ``phi[n, k, f_l]`` is the mean over the background rows (all ranks') of the sum over
  class k's paths.
* ``phi[n, k, F] = base + mean_z f_k(z)``: per path ``v * count(mask == full) / B``, paths
  with ``m = 0`` add v; summed in fp64 on the host.
* So the last axis sums to ``predict(X, output_margin=True)``, a feature no path of the
  class uses gets exactly 0, and x equal to a background row contributes exactly 0 for
  that z.

For a fixed path and x a background row matters only through ``mz``: the GPU path
reduces the background once to ``hist[path][mask]`` (int64 counts, 2^m per path, merged
over the ranks by an integer all-reduce) and walks each path's distinct masks with
``w = count / B``; its cost per row does not depend on B.

Learning to rank: objectives ``rank:pairwise`` and ``rank:ndcg`` (LambdaMART).  On the
GPU the gradient is the pair kernels of csrc/gbdt_rank.hip over a work plan built
once per ``fit``; on CPU the same definition on torch ops in fp64, rounded once.  The
definition, shared by both paths and by the tests:

* Groups: ``fit(X, y, group=sizes)``, ``sizes`` int [Q], positive, summing to N; the
  rows of a group are contiguous and in the given order (XGBoost's ``set_group``).
  ``group_ptr`` (int32 [Q + 1]) lives on the device.  A group lives on one rank:
  nothing new is all-reduced in training.
* Labels: integer relevance in [0, 31]; gain ``G(y) = 2^y - 1``.
* Position: ``pos_i`` is the 0-based position of row i in its group sorted by score,
  descending, ties to the lower row index (at round 0 every score ties).
* Discount: ``D[p]`` is the fp64 value ``1 / log2(p + 2)`` rounded once to fp32, a
  host-built table as long as the longest group, uploaded once per fit.  Every path
  indexes that fp32 table; no ``log`` runs on the device.
* ``inv_idcg[q]``: the group's ideal DCG (``sum_p G(y sorted descending)[p] * D[p]`` in
  fp64), inverted and rounded to fp32; 0 where the ideal DCG is 0.  Once per fit.
* Pair terms: for every ordered pair ``i != j`` of one group with ``y_i != y_j``, ``hi``
  the row of the larger label and ``lo`` the other, ``d = s_hi - s_lo``,
  ``rho = 1 / (1 + exp(d))``, ``w = 1`` (``rank:pairwise``) or
  ``|G(y_i) - G(y_j)| * |D[pos_i] - D[pos_j]| * inv_idcg[q]`` (``rank:ndcg``):
  ``g_i += (i is hi ? -1 : +1) * rho * w``, ``h_i += rho * (1 - rho) * w``; at the end
  ``h_i = max(h_i, 1e-16)``.  No pair sampling, truncation or score normalisation: a
  pure function of (scores, labels, groups).
* Base margin 0, one tree per round, ``transform_margin`` is the identity.
* Metric: ``ndcg@k`` = the mean over groups of ``DCG@k / IDCG@k`` (``DCG@k = sum over
  pos_i < k of G(y_i) * D[pos_i]`` in fp64; a group whose ``IDCG@k`` is 0 counts as
  1), ``k = GBDTParams.eval_at``, 0 = the whole list; the metric is named ``ndcg`` for
  ``k = 0`` and ``ndcg@k`` otherwise.  Higher is better: early stopping maximises it.

Robust and quantile regression: objectives ``reg:absoluteerror`` (alpha = 0.5) and
``reg:quantileerror`` (``GBDTParams.quantile_alpha``), the pinball loss.  Its gradient is one
of two constants (``g = pred > y ? 1 - alpha : -alpha``, ``h = 1``) and carries no leaf
value, so the tree's structure is grown on (g, h) and every leaf is then renewed
(XGBoost's adaptive leaves): ``value = fp32(learning_rate) * q`` (one fp32 multiply), ``q``
the alpha-quantile of the residuals ``y[r] - margin[r]`` (one fp32 subtraction, the margin
before the tree) of the rows r of all ranks that ended in the leaf.  The alpha-quantile
of n keys is ``sorted(keys)[t]`` with ``t = max(ceil(alpha * n) - 1, 0)``, the product and
the ceil in fp64 -- an element of the input, never an interpolation; keys are ordered
as floats (-0 and +0 tie) and must not be NaN; an empty leaf gets 0.  The base margin is
the same quantile of y over all ranks, stored in ``base_score`` by ``fit``.  On the GPU
the select is csrc/gbdt_quantile.hip (a radix select over 8-bit digits of the ordered
bit pattern: per pass a count kernel, the integer all-reduce of its [leaves, 256] table
when there are several ranks, and a step kernel); on CPU ``_select_torch`` runs the same
passes with ``bincount``.  Metrics: ``mae`` and ``quantile`` (the mean pinball loss
``max(alpha d, (alpha - 1) d)``, ``d = y - pred``); lower is better.
"""
from __future__ import annotations

import json
import math
import os
import time
from dataclasses import dataclass, field
from typing import List, Optional

import torch
import torch.distributed as dist

from kubedl_amd.ops import _ext

RANK_OBJECTIVES = ("rank:pairwise", "rank:ndcg")
QUANTILE_OBJECTIVES = ("reg:absoluteerror", "reg:quantileerror")
QUANTILE_PASSES = 4  # 8-bit digits of the 32-bit key (csrc/gbdt_quantile.hip)
MAX_RANK_LABEL = 31


@dataclass
class GBDTParams:
    objective: str = "reg:squarederror"
    num_class: int = 1
    n_estimators: int = 10
    learning_rate: float = 0.3
    max_depth: int = 6
    max_bin: int = 256
    reg_lambda: float = 1.0
    gamma: float = 0.0
    min_child_weight: float = 1.0
    base_score: float = 0.5
    early_stopping_rounds: int = 0  # 0 = off (fit's ``early_stopping_rounds`` argument overrides it)
    eval_at: int = 0  # ranking objectives: the k of ndcg@k, 0 = the whole list
    quantile_alpha: float = 0.5  # reg:quantileerror: the quantile to fit, in (0, 1)

    @classmethod
    def parse(cls, spec: str, **kw) -> "GBDTParams":
        """``objective:multi:softprob,num_class:3`` (the example's --xgboost_parameter)."""
        p = cls(**kw)
        if not spec:
            return p
        spec = spec.strip().strip('"')
        for part in spec.split(","):
            if ":" not in part:
                continue
            k, v = part.split(":", 1)
            k = k.strip()
            alias = {"eta": "learning_rate", "lambda": "reg_lambda", "num_round": "n_estimators",
                     "min_split_loss": "gamma"}
            k = alias.get(k, k)
            if not hasattr(p, k):
                continue
            cur = getattr(p, k)
            setattr(p, k, type(cur)(v) if not isinstance(cur, str) else v)
        return p


@dataclass
class Tree:
    feature: List[int] = field(default_factory=list)
    split_bin: List[int] = field(default_factory=list)
    threshold: List[float] = field(default_factory=list)
    left: List[int] = field(default_factory=list)
    right: List[int] = field(default_factory=list)
    value: List[float] = field(default_factory=list)

    def add(self) -> int:
        for a in (self.feature, self.split_bin, self.left, self.right):
            a.append(-1)
        self.threshold.append(0.0)
        self.value.append(0.0)
        return len(self.value) - 1


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _allreduce_(t: torch.Tensor) -> torch.Tensor:
    if _world() > 1:
        dist.all_reduce(t)
    return t


class HistGBDT:
    def __init__(self, params: GBDTParams, device=None):
        self.p = params
        self.device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.cuts: Optional[torch.Tensor] = None  # [F, B-1]
        self.trees: List[List[Tree]] = []
        self.use_hip = self.device.type == "cuda"
        if self.use_hip and not _ext.available():
            _ext.require_on_gpu("HistGBDT")
            self.use_hip = False
        self.stats = {"hist_builds": 0, "hist_subtracted": 0}
        # fit(eval_set=...): the validation metric per round; with early stopping the best round
        self.evals_result: List[float] = []
        self.eval_metric: Optional[str] = None
        self.best_iteration: Optional[int] = None
        self.best_score: Optional[float] = None
        self._forest_cache = None  # (key, trees kept alive, nodes, tree_off, max feature): _forest()
        self._cover_cache = None  # (forest key, int64 covers [num_nodes], background F): set_background()
        self._paths_cache = None  # (key, path table): _path_table()
        self._pairs_cache = None  # (the same key, per-feature path table): _pair_table()
        self._iv_bg = None  # (forest key, background rows, rows over all ranks): set_background(interventional=True)
        self._iv_cache = None  # (the path table's key, explain table): _iv_table()

    # ------------------------------------------------------------ quantisation
    def fit_cuts(self, X: torch.Tensor, sample: int = 65536, seed: int = 0) -> None:
        B = self.p.max_bin
        n = X.shape[0]
        # a systematic sample (every n/sample-th row from a seeded offset): the
        # same rows on every device, no host permutation of n ids (torch.randperm
        # of 2M ids was ~0.15 s of the fit's set-up on the CPU)
        k = min(sample, n)
        off = (seed * 7919 + 17) % max(n // k, 1)
        idx = (torch.arange(k, device=X.device, dtype=torch.int64) * n) // k + off
        samp = X[idx.clamp_(max=n - 1)].float()
        if _world() > 1:
            # every rank contributes the same number of rows
            k = torch.tensor([samp.shape[0]], device=X.device)
            dist.all_reduce(k, op=dist.ReduceOp.MIN)
            samp = samp[: int(k.item())].contiguous()
            parts = [torch.empty_like(samp) for _ in range(_world())]
            dist.all_gather(parts, samp)
            samp = torch.cat(parts)
        # torch.quantile's 'linear' rule as a sort + lerp: the same cuts (to fp32
        # rounding), but torch.quantile's first call on a GPU costs ~0.18 s of
        # kernel loading where one sort costs ~8 ms (scripts/quantile_probe.py)
        q = torch.linspace(0, 1, B + 1, device=samp.device, dtype=torch.float64)[1:-1]
        srt, _ = torch.sort(samp.T.contiguous(), dim=1)  # [F, m]
        pos = q * (srt.shape[1] - 1)
        lo, hi = pos.floor().long(), pos.ceil().long()
        w = (pos - lo.double()).float()
        self.cuts = (srt[:, lo] * (1 - w) + srt[:, hi] * w).contiguous()  # [F, B-1]

    def host_cuts(self, X: torch.Tensor, sample: int = 65536, seed: int = 0) -> torch.Tensor:
        """``fit_cuts`` on a host copy of X, bitwise the same cuts: the same
        systematic sample, the same order statistics (``numpy.partition`` puts each
        needed rank exactly where a full sort would), the same float32 lerp.  On a
        fresh GPU process the device version's first calls load torch's sort and
        elementwise code objects (0.1-0.6 s, ``scripts/cuts_probe.py``); this one
        loads nothing and runs beside the host->device copy (``fit``)."""
        import numpy as np
        B = self.p.max_bin
        n = X.shape[0]
        k = min(sample, n)
        off = (seed * 7919 + 17) % max(n // k, 1)
        idx = np.minimum((np.arange(k, dtype=np.int64) * n) // k + off, n - 1)
        samp = np.ascontiguousarray(X.detach().numpy()[idx].astype(np.float32, copy=False))  # [k, F]
        q = torch.linspace(0, 1, B + 1, dtype=torch.float64)[1:-1]
        pos = q * (k - 1)
        lo, hi = pos.floor().long(), pos.ceil().long()
        w = (pos - lo.double()).float()
        kth = np.unique(np.concatenate([lo.numpy(), hi.numpy()]))
        part = np.partition(samp, kth, axis=0)
        a = torch.from_numpy(np.ascontiguousarray(part[lo.numpy()].T))  # [F, B-1]
        b = torch.from_numpy(np.ascontiguousarray(part[hi.numpy()].T))
        return (a * (1 - w) + b * w).contiguous()

    def quantise(self, X: torch.Tensor) -> torch.Tensor:
        if self.use_hip and X.is_cuda:
            return _ext.load().gbdt_quantise(X, self.cuts, self.p.max_bin)
        F = X.shape[1]
        out = torch.empty(X.shape, dtype=torch.uint8, device=X.device)
        for f in range(F):
            out[:, f] = torch.bucketize(X[:, f].contiguous().float(), self.cuts[f].contiguous(), right=False).clamp_(
                max=self.p.max_bin - 1).to(torch.uint8)
        return out

    # ------------------------------------------------------------ objectives
    def _grad_hess(self, pred: torch.Tensor, y: torch.Tensor, rank: Optional[dict] = None):
        obj = self.p.objective
        if obj in RANK_OBJECTIVES:
            if rank is None:
                raise ValueError(f"{obj} needs the query groups: fit(X, y, group=sizes)")
            if self.use_hip and pred.is_cuda:
                # csrc/gbdt_rank.hip: the pair kernels over the fit's plan
                g, h = _ext.load().gbdt_rank_grad_hess(pred.view(-1), rank["y"], rank["plan_wave"], rank["plan_block"],
                                                       rank["dtab"], rank["max_group"], rank["disc"],
                                                       obj == "rank:ndcg")
                return g, h
            g, h, _ = self._rank_grad_hess_torch(pred.view(-1), rank)
            return g.view(-1, 1), h.view(-1, 1)
        quant = obj in QUANTILE_OBJECTIVES
        if self.use_hip and pred.is_cuda:
            # csrc/gbdt.hip grad_hess_kernel: one launch, the torch composition's expressions
            code = 3 if quant else 0 if obj.startswith("reg:") else 1 if obj == "binary:logistic" else 2 if obj.startswith("multi:") else -1
            if code >= 0:
                c = getattr(self, "_yf", None)
                if c is None or c[0] is not y:  # the labels as fp32, converted once per fit
                    c = self._yf = (y, y if (y.dtype == torch.float32 and y.is_contiguous()) else y.float().contiguous())
                if quant:
                    return _ext.load().gbdt_grad_hess(pred.contiguous(), c[1].view(-1), code, self._alpha())
                g, h = _ext.load().gbdt_grad_hess(pred.contiguous(), c[1].view(-1), code)
                return g, h
        if quant:
            a = self._alpha()
            up = pred > y.view_as(pred).float()
            return torch.where(up, 1.0 - a, -a).to(torch.float32), torch.ones_like(pred)
        if obj.startswith("reg:"):
            return pred - y.view_as(pred), torch.ones_like(pred)
        if obj == "binary:logistic":
            pr = torch.sigmoid(pred)
            return pr - y.view_as(pred), (pr * (1 - pr)).clamp_min(1e-16)
        if obj.startswith("multi:"):
            pr = torch.softmax(pred, dim=1)
            yy = torch.nn.functional.one_hot(y.long(), self.p.num_class).to(pr.dtype)
            return pr - yy, (2.0 * pr * (1 - pr)).clamp_min(1e-16)
        raise ValueError(f"unsupported objective {obj}")

    def _base(self, n: int) -> torch.Tensor:
        K = self.p.num_class if self.p.objective.startswith("multi:") else 1
        if self.p.objective == "binary:logistic":
            b = math.log(self.p.base_score / (1 - self.p.base_score))
        elif self.p.objective.startswith("multi:") or self.p.objective in RANK_OBJECTIVES:
            b = 0.0
        else:
            b = self.p.base_score
        return torch.full((n, K), b, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------ quantile objectives
    def _alpha(self) -> float:
        return 0.5 if self.p.objective == "reg:absoluteerror" else float(self.p.quantile_alpha)

    @staticmethod
    def _select_torch(keys: torch.Tensor, seg: torch.Tensor, S: int, alpha: float) -> torch.Tensor:
        """fp32 [S]: the alpha-quantile (module docstring) of the fp32 ``keys`` of every segment,
        ``seg`` [n] holding each key's segment id, counted over all ranks; 0 for an empty
        segment.  The digit passes of csrc/gbdt_quantile.hip on torch ops: the CPU path, which
        serves gloo ranks too."""
        b = keys.contiguous().view(torch.int32).long() & 0xFFFFFFFF
        u = torch.where(b >= 1 << 31, b ^ 0xFFFFFFFF, b | (1 << 31))  # unsigned order = float order
        seg = seg.long()
        prefix = torch.zeros(S, dtype=torch.int64, device=keys.device)
        n_s = t = None
        for p in range(QUANTILE_PASSES):
            shift = 24 - 8 * p
            m = (u >> (shift + 8)) == prefix[seg]  # pass 0: every key (0 == 0)
            hist = _allreduce_(torch.bincount(seg[m] * 256 + ((u[m] >> shift) & 255), minlength=S * 256)).view(S, 256)
            if p == 0:
                n_s = hist.sum(1)
                t = (torch.ceil(alpha * n_s.double()).long() - 1).clamp_(min=0)
            cum = hist.cumsum(1)
            d = (cum <= t[:, None]).sum(1).clamp_(max=255)[:, None]  # the first digit whose count passes t
            t = t - (cum.gather(1, d) - hist.gather(1, d))[:, 0]
            prefix = prefix * 256 + d[:, 0]
        bits = torch.where(prefix >= 1 << 31, prefix ^ (1 << 31), prefix ^ 0xFFFFFFFF)
        q = (bits - ((bits >= 1 << 31).long() << 32)).int().view(torch.float32)
        return torch.where(n_s > 0, q, torch.zeros_like(q))

    def _quantile_of(self, yf: torch.Tensor, alpha: float) -> float:
        """The alpha-quantile of every rank's labels (the base margin)."""
        n = yf.shape[0]
        if self.use_hip and yf.is_cuda and _world() == 1:
            b = torch.tensor([0, n], dtype=torch.int32, device=yf.device)
            return float(_ext.load().gbdt_segment_quantile(yf, b[:1], b[1:], alpha))
        return float(self._select_torch(yf, torch.zeros(n, dtype=torch.int64, device=yf.device), 1, alpha))

    def _renew_leaves_torch(self, tree: "Tree", leaf: torch.Tensor, yf: torch.Tensor, margin: torch.Tensor) -> None:
        """Adaptive leaves on torch ops: every leaf of ``tree`` becomes fp32(lr) * the quantile of
        the residuals of the rows that ``leaf`` (the tree node of each row) puts in it."""
        q = self._select_torch(yf - margin, leaf, len(tree.value), self._alpha())
        vals = (q * torch.tensor(self.p.learning_rate, dtype=torch.float32, device=q.device)).tolist()
        for nid, f in enumerate(tree.feature):
            if f < 0:
                tree.value[nid] = vals[nid]

    # ------------------------------------------------------------ learning to rank
    def _ndcg_name(self) -> str:
        k = int(self.p.eval_at)
        return f"ndcg@{k}" if k > 0 else "ndcg"

    def _rank_setup(self, y: torch.Tensor, group, plan: bool = True) -> dict:
        """Check the groups and labels and build, once per fit (eval set, ``metric`` call),
        what the ranking paths share: ``group_ptr``, the int32 labels, the discount table,
        ``inv_idcg`` and ``IDCG@k`` (module docstring) and, with ``plan`` on the GPU, the
        work plan of csrc/gbdt_rank.hip (its header has the layout) and the ``disc``
        workspace."""
        import numpy as np
        dev = self.device
        sizes = torch.as_tensor(group).detach().cpu().reshape(-1)
        if sizes.dtype.is_floating_point or sizes.dtype == torch.bool:
            raise ValueError("group: integer sizes expected")
        sizes = sizes.numpy().astype(np.int64)
        n, Q = int(y.shape[0]), int(sizes.size)
        if Q and int(sizes.min()) <= 0:
            raise ValueError(f"group: sizes must be positive (smallest: {int(sizes.min())})")
        if int(sizes.sum()) != n:
            raise ValueError(f"group: the sizes sum to {int(sizes.sum())}, there are {n} rows")
        if n >= 2 ** 31:
            raise ValueError("ranking: 2^31 or more rows on one rank")
        yl = y.reshape(-1)
        if yl.shape[0] != n:
            raise ValueError(f"ranking: y must hold one label per row, got {tuple(y.shape)}")
        if n and (yl.dtype.is_floating_point and bool((yl != yl.round()).any())
                  or int(yl.min()) < 0 or int(yl.max()) > MAX_RANK_LABEL):
            raise ValueError(f"ranking: labels must be integers in [0, {MAX_RANK_LABEL}]")
        y32 = yl.to(device=dev, dtype=torch.int32).contiguous()
        ptr = np.zeros(Q + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(sizes)
        L = max(int(sizes.max()) if Q else 1, 1)
        dtab = (1.0 / np.log2(np.arange(L, dtype=np.float64) + 2.0)).astype(np.float32)
        gid = torch.repeat_interleave(torch.arange(Q, device=dev), torch.from_numpy(sizes).to(dev))
        # the ideal order: labels descending inside each group (one device sort); the sums on the host, fp64, in order
        ys = (MAX_RANK_LABEL - torch.sort(gid * 32 + (MAX_RANK_LABEL - y32.long())).values % 32).cpu().numpy()
        pos = np.arange(n, dtype=np.int64) - np.repeat(ptr[:-1], sizes)
        term = (np.ldexp(1.0, ys.astype(np.int32)) - 1.0) * dtab.astype(np.float64)[pos]
        k = int(self.p.eval_at)
        idcg = np.add.reduceat(term, ptr[:-1]) if Q else np.zeros(0)
        idcg_k = np.add.reduceat(np.where(pos < k, term, 0.0), ptr[:-1]) if (Q and k > 0) else idcg
        with np.errstate(divide="ignore"):
            inv = np.where(idcg > 0, 1.0 / idcg, 0.0).astype(np.float32)
        rk = {"Q": Q, "n": n, "sizes": sizes, "ptr_host": ptr, "y": y32, "gid": gid, "max_group": L,
              "ptr": torch.from_numpy(ptr.astype(np.int32)).to(dev), "dtab": torch.from_numpy(dtab).to(dev),
              "inv_idcg": torch.from_numpy(inv).to(dev), "idcg_k": torch.from_numpy(idcg_k).to(dev)}
        if plan and self.use_hip:
            ext = _ext.load()
            wmax, tile = ext.gbdt_rank_wave_max(), ext.gbdt_rank_tile_rows()
            bits = inv.view(np.int32).astype(np.int64)

            def by_size(sel):  # largest first: the waves of a block get groups of similar length
                idx = np.flatnonzero(sel)
                return idx[np.argsort(-sizes[idx], kind="stable")]
            small, big = by_size(sizes <= wmax), by_size(sizes > wmax)
            tiles = (sizes[big] + tile - 1) // tile
            rep = np.repeat(big, tiles)
            i0 = (np.arange(int(tiles.sum()), dtype=np.int64) - np.repeat(np.cumsum(tiles) - tiles, tiles)) * tile
            wave = np.stack([ptr[small], sizes[small], bits[small], small], 1).astype(np.int32)
            block = np.stack([ptr[rep], sizes[rep], bits[rep], i0], 1).astype(np.int32)
            rk["plan_wave"] = torch.from_numpy(wave).to(dev)
            rk["plan_block"] = torch.from_numpy(block).to(dev)
            rk["disc"] = torch.zeros(n, dtype=torch.float32, device=dev)
        return rk

    @staticmethod
    def _rank_positions_torch(score: torch.Tensor, rk: dict) -> torch.Tensor:
        """pos [N] (int64): two stable sorts, by score descending and then by group."""
        o1 = torch.sort(-score, stable=True).indices
        order = o1[torch.sort(rk["gid"][o1], stable=True).indices]  # rows by (group, score descending, index)
        pos = torch.empty_like(order)
        pos[order] = torch.arange(order.numel(), device=score.device) - rk["ptr"].long()[rk["gid"]]
        return pos

    def _rank_grad_hess_torch(self, score: torch.Tensor, rk: dict):
        """The ranking gradient on torch ops (the CPU path): fp64 inside, rounded once.
        Groups of similar size are padded to [c, L] and their pairs formed as [c, i, L]
        blocks of at most 2^22 elements.  Returns g, h, disc (fp32 [N])."""
        ndcg = self.p.objective == "rank:ndcg"
        dev, n = score.device, rk["n"]
        s, y = score.double(), rk["y"].long()
        G = torch.ldexp(torch.ones(n, dtype=torch.float64, device=dev), rk["y"]) - 1.0
        disc = rk["dtab"].double()[self._rank_positions_torch(score, rk)] if ndcg else torch.zeros_like(s)
        inv = rk["inv_idcg"].double()
        g, h = torch.zeros_like(s), torch.zeros_like(s)
        if "chunks" not in rk:  # (groups, padded length), by size
            import numpy as np
            sizes = rk["sizes"]
            order = np.argsort(sizes, kind="stable")
            chunks, a = [], 0
            while a < len(order):
                L = int(sizes[order[a]])
                b = a + 1
                while b < len(order) and (b + 1 - a) * int(sizes[order[b]]) ** 2 <= 1 << 22:
                    L = int(sizes[order[b]])
                    b += 1
                chunks.append((torch.from_numpy(order[a:b]).to(dev), L))
                a = b
            rk["chunks"] = chunks
        ptr, nq_all = rk["ptr"].long(), torch.from_numpy(rk["sizes"]).to(dev)
        for qs, L in rk["chunks"]:
            ar = torch.arange(L, device=dev)
            valid = ar[None, :] < nq_all[qs][:, None]                                    # [c, L]
            idx = torch.where(valid, ptr[qs][:, None] + ar[None, :], torch.zeros_like(ar)[None, :])
            S, Y, Gc, Dc = s[idx], y[idx], G[idx], disc[idx]
            gc, hc = torch.zeros_like(S), torch.zeros_like(S)
            step = max(1, (1 << 22) // (L * len(qs)))
            for a in range(0, L, step):
                i = slice(a, a + step)
                hi = Y[:, i, None] > Y[:, None, :]
                d = torch.where(hi, S[:, i, None] - S[:, None, :], S[:, None, :] - S[:, i, None])
                e = torch.exp(-d.abs())
                r = 1.0 / (1.0 + e)
                sm = e * r  # the smaller of rho and 1 - rho, never formed by subtraction
                rho = torch.where(d > 0, sm, r)
                w = ((Y[:, i, None] != Y[:, None, :]) & valid[:, i, None] & valid[:, None, :]).double()
                if ndcg:
                    w = w * (Gc[:, i, None] - Gc[:, None, :]).abs() * (Dc[:, i, None] - Dc[:, None, :]).abs() \
                        * inv[qs][:, None, None]
                gc[:, i] = (torch.where(hi, -rho, rho) * w).sum(2)
                hc[:, i] = (sm * r * w).sum(2)
            g[idx[valid]], h[idx[valid]] = gc[valid], hc[valid]
        return g.float(), h.float().clamp_min_(1e-16), disc.float()

    def _ndcg_sum(self, score: torch.Tensor, rk: dict) -> torch.Tensor:
        """The sum over this rank's groups of ``DCG@k / IDCG@k`` (1 where IDCG@k is 0), one
        fp64 scalar on the device; the DCG is csrc/gbdt_rank.hip's on the GPU."""
        k, Q = int(self.p.eval_at), rk["Q"]
        if Q == 0:
            return torch.zeros((), dtype=torch.float64, device=self.device)
        if self.use_hip and score.is_cuda:
            dcg = _ext.load().gbdt_rank_ndcg(score, rk["y"], rk["ptr"], rk["dtab"], rk["max_group"], k)
        else:
            pos = self._rank_positions_torch(score, rk)
            term = (torch.ldexp(torch.ones(rk["n"], dtype=torch.float64, device=score.device), rk["y"]) - 1.0) \
                * rk["dtab"].double()[pos]
            if k > 0:
                term = torch.where(pos < k, term, torch.zeros_like(term))
            dcg = torch.zeros(Q, dtype=torch.float64, device=score.device).index_add_(0, rk["gid"], term)
        idcg = rk["idcg_k"]
        return torch.where(idcg > 0, dcg / idcg.clamp_min(1e-300), torch.ones_like(dcg)).sum()

    # ------------------------------------------------------------ kernels (HIP or torch)
    def _hist(self, bins, g, h, rows, seg_cpu, F, B):
        nodes = len(seg_cpu) - 1
        hist = torch.zeros(nodes, F, B, 2, dtype=torch.float32, device=self.device)
        if nodes == 0:
            return hist
        self.stats["hist_builds"] += nodes
        if self.use_hip:
            seg = torch.tensor(seg_cpu, dtype=torch.int32, device=self.device)
            maxr = max(seg_cpu[i + 1] - seg_cpu[i] for i in range(nodes))
            _ext.load().gbdt_hist(bins, g, h, 1, rows, seg, int(maxr), B, hist)
            return hist
        counts = torch.tensor([seg_cpu[i + 1] - seg_cpu[i] for i in range(nodes)], device=self.device)
        node_of = torch.repeat_interleave(torch.arange(nodes, device=self.device), counts)
        rb = bins[rows.long()].long()  # [n, F]
        base = (node_of[:, None] * F + torch.arange(F, device=self.device)[None, :]) * B + rb
        flat = hist.view(-1, 2)
        flat[:, 0].index_add_(0, base.reshape(-1), g[rows.long()].repeat_interleave(F))
        flat[:, 1].index_add_(0, base.reshape(-1), h[rows.long()].repeat_interleave(F))
        return hist

    def _split(self, hist):
        lam, mcw = self.p.reg_lambda, self.p.min_child_weight
        if self.use_hip:
            return _ext.load().gbdt_split(hist.contiguous(), lam, mcw)
        G = hist[..., 0].cumsum(-1)
        H = hist[..., 1].cumsum(-1)
        tg, th = G[..., -1:], H[..., -1:]
        gr, hr = tg - G, th - H
        gain = G * G / (H + lam) + gr * gr / (hr + lam) - tg * tg / (th + lam)
        ok = (H >= mcw) & (hr >= mcw)
        ok[..., -1] = False
        gain = torch.where(ok, gain, torch.full_like(gain, -math.inf))
        best, bin_ = gain.max(-1)
        gl = G.gather(-1, bin_[..., None])[..., 0]
        hl = H.gather(-1, bin_[..., None])[..., 0]
        bin_ = torch.where(torch.isinf(best), torch.full_like(bin_, -1), bin_)
        return best, bin_.int(), gl, hl

    def _route(self, bins, rows, row_node, sfeat, sbin):
        if self.use_hip:
            return _ext.load().gbdt_route(bins, rows, row_node, sfeat, sbin)
        f = sfeat[row_node.long()].long()
        b = bins[rows.long(), f.clamp_min(0)].int()
        return ((f >= 0) & (b > sbin[row_node.long()])).int()

    # ------------------------------------------------------------ one tree
    def _grow(self, bins, g, h, n_local: int) -> (Tree, torch.Tensor):
        """Depth-wise growth.  Per level the host does O(1) device syncs (one
        batched read of the split decisions, one of the child counts): every
        per-node quantity is gathered/scattered with one tensor op per level,
        and each row's node id is carried through the stable sort instead of
        being re-expanded from the segment counts."""
        p = self.p
        F, B = bins.shape[1], p.max_bin
        dev = self.device
        tree = Tree()
        root = tree.add()
        rows = torch.arange(n_local, dtype=torch.int32, device=dev)
        row_node = torch.zeros(n_local, dtype=torch.int32, device=dev)  # level-local node of each row in ``rows``
        seg = [0, n_local]
        level_nodes = [root]
        leaf_of_row = torch.zeros(n_local, dtype=torch.int32, device=dev)
        hist = _allreduce_(self._hist(bins, g, h, rows, seg, F, B))
        ncut = self.cuts.shape[1]
        for depth in range(p.max_depth + 1):
            nodes = len(level_nodes)
            tot = hist[:, 0].sum(1)  # [nodes, 2] (every feature sums to the node total)
            weight = -tot[:, 0] / (tot[:, 1] + p.reg_lambda) * p.learning_rate
            if depth < p.max_depth:
                gain, sbin, gl, hl = self._split(hist)
                best_gain, best_f = gain.max(1)
                do_split = (best_gain > p.gamma) & torch.isfinite(best_gain)
                best_b = sbin.gather(1, best_f[:, None])[:, 0].long()
                thr = self.cuts[best_f, best_b.clamp(0, ncut - 1)]
                thr = torch.where(best_b < ncut, thr, torch.full_like(thr, math.inf))
                # one device->host transfer for every per-node decision of this level
                host = torch.stack([do_split.double(), weight.double(), best_f.double(), best_b.double(),
                                    thr.double()]).tolist()
                ds, weights, bf, bb, th = host[0], host[1], [int(v) for v in host[2]], [int(v) for v in host[3]], \
                    host[4]
                ds = [v > 0.5 for v in ds]
            else:
                ds, weights = [False] * nodes, weight.tolist()
            # leaves of this level: every row of a non-split node ends here
            leaf_id = [-1 if ds[i] else level_nodes[i] for i in range(nodes)]
            if any(v >= 0 for v in leaf_id):
                lid = torch.tensor(leaf_id, dtype=torch.int32, device=dev)[row_node.long()]
                m = lid >= 0
                leaf_of_row[rows[m].long()] = lid[m]
            for i, nid in enumerate(level_nodes):
                if not ds[i]:
                    tree.value[nid] = weights[i]
            if not any(ds):
                break
            sfeat = torch.tensor([bf[i] if ds[i] else -1 for i in range(nodes)], dtype=torch.int32, device=dev)
            sb = torch.tensor([bb[i] if ds[i] else -1 for i in range(nodes)], dtype=torch.int32, device=dev)
            go_right = self._route(bins, rows, row_node, sfeat, sb)
            next_nodes, remap = [], []
            for i, nid in enumerate(level_nodes):
                if ds[i]:
                    l, r = tree.add(), tree.add()
                    tree.feature[nid], tree.split_bin[nid] = bf[i], bb[i]
                    tree.threshold[nid] = th[i]
                    tree.left[nid], tree.right[nid] = l, r
                    remap.append((len(next_nodes), len(next_nodes) + 1))
                    next_nodes += [l, r]
                else:
                    remap.append((-1, -1))
            # new child index per row (-1 = leaf reached); the stable sort keeps rows grouped by child
            child = torch.tensor(remap, dtype=torch.int32, device=dev)[row_node.long(), go_right.long()]
            keep = child >= 0
            child, rows_k = child[keep], rows[keep]
            child, order = torch.sort(child, stable=True)
            rows = rows_k[order].contiguous()
            row_node = child.contiguous()
            ccount = torch.bincount(child, minlength=len(next_nodes))
            # histogram subtraction: build the smaller child (by global count), derive the sibling
            glob = _allreduce_(ccount.clone().float())
            cc = torch.stack([torch.cumsum(ccount, 0).double(), glob.double()]).tolist()
            seg = [0] + [int(v) for v in cc[0]]
            gl_ = cc[1]
            small = [2 * j + (0 if gl_[2 * j] <= gl_[2 * j + 1] else 1) for j in range(len(next_nodes) // 2)]
            sub_seg = [0]
            sub_rows = []
            for c in small:
                sub_rows.append(rows[seg[c]:seg[c + 1]])
                sub_seg.append(sub_seg[-1] + seg[c + 1] - seg[c])
            srows = torch.cat(sub_rows) if sub_rows else rows[:0]
            h_small = _allreduce_(self._hist(bins, g, h, srows.contiguous(), sub_seg, F, B))
            parents = torch.tensor([i for i in range(nodes) if ds[i]], dtype=torch.long, device=dev)
            small_t = torch.tensor(small, dtype=torch.long, device=dev)
            parent_hist = hist
            hist = torch.empty(len(next_nodes), F, B, 2, dtype=torch.float32, device=dev)
            hist[small_t] = h_small
            hist[small_t ^ 1] = parent_hist[parents] - h_small
            self.stats["hist_subtracted"] += len(small)
            level_nodes = next_nodes
        return tree, leaf_of_row

    # ------------------------------------------------------------ device-resident tree
    def _device_grower(self, bins):
        p = self.p
        if not self.use_hip or p.max_depth > 10 or (bins.shape[1] * p.max_bin) % 2:
            return None
        return _ext.load().GbdtGrower(bins, self.cuts, p.max_bin, p.max_depth, p.reg_lambda, p.gamma,
                                      p.learning_rate, p.min_child_weight)

    def _grow_device(self, gr, g, h, renew=None):
        """One tree on the GPU; returns its [4, heap] arrays (feature, split bin,
        threshold, value).  ``renew = (y, margin, k, alpha)``: the quantile objectives'
        leaf renewal after the last level, its count tables all-reduced pass by pass."""
        D = self.p.max_depth
        if _world() == 1:
            gr.grow_local(g, h)
        else:
            _allreduce_(gr.begin_tree(g, h))
            for d in range(D + 1):
                cnt = gr.level_a(d, False)
                if d < D:
                    _allreduce_(cnt)                    # global child counts -> same smaller child on all ranks
                    _allreduce_(gr.level_b(d, True))    # the built children's histograms
                    gr.level_c(d)
        if renew is not None:
            yf, margin, k, alpha = renew
            if _world() == 1:
                gr.renew_leaves(yf, margin, k, alpha)
            else:
                for ps in range(QUANTILE_PASSES):
                    _allreduce_(gr.leaf_count(ps, yf, margin, k))  # global counts -> the same leaves on all ranks
                    gr.leaf_step(ps, alpha)
        return gr.heap_packed()  # [4, heap] in one launch (the leaf values go in by add_leaf)

    @staticmethod
    def _heap_tree(arr) -> Tree:
        feat, tbin, thr, val = arr
        t = Tree()
        t.feature = [int(v) for v in feat]
        t.split_bin = [int(v) for v in tbin]
        t.threshold = [float(v) for v in thr]
        t.value = [float(v) for v in val]
        t.left = [2 * i + 1 if f >= 0 else -1 for i, f in enumerate(t.feature)]
        t.right = [2 * i + 2 if f >= 0 else -1 for i, f in enumerate(t.feature)]
        return t

    # ------------------------------------------------------------ training
    def _sync_time(self) -> float:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def fit(self, X: torch.Tensor, y: torch.Tensor, log_every: int = 0, callback=None, eval_set=None,
            early_stopping_rounds: Optional[int] = None, group=None):
        """``stats['setup_s']``: host->device copy, cut fitting, quantisation and the
        grower's workspaces; ``stats['boost_s']``: the boosting rounds alone (one
        synchronisation at each end, none inside).

        ``eval_set=(Xv, yv)``: a held-out set (this rank's shard of it) whose margin is
        advanced by each round's trees; ``evals_result[i]`` is the objective's metric
        (``eval_metric``: rmse / logloss / mlogloss / mae / quantile) after round ``i``, from loss sums
        all-reduced over the ranks.  Without ``early_stopping_rounds`` the sums stay
        on the device until the end of ``fit`` (one copy); with it one value is read
        per round, training stops once the metric has not improved for that many
        rounds (every rank at the same round), ``best_iteration`` / ``best_score``
        are set, all grown trees are kept and ``predict`` defaults to the best round.

        ``group=sizes`` (the ranking objectives only, and required there): the query
        group sizes of this rank's rows, see the module docstring; ``eval_set`` is then
        ``(Xv, yv, groupv)`` and the metric ``ndcg@k``, which early stopping maximises."""
        ranking = self.p.objective in RANK_OBJECTIVES
        if ranking and group is None:
            raise ValueError(f"{self.p.objective} needs the query groups: fit(X, y, group=sizes)")
        if not ranking and group is not None:
            raise ValueError(f"group is for the ranking objectives, not {self.p.objective}")
        if ranking and X.shape[0] != y.shape[0]:
            raise ValueError(f"fit: {X.shape[0]} rows of X for {y.shape[0]} labels")
        quant = self.p.objective in QUANTILE_OBJECTIVES
        if quant:
            if not 0.0 < self._alpha() < 1.0:
                raise ValueError(f"{self.p.objective}: quantile_alpha must lie in (0, 1), got {self.p.quantile_alpha}")
            if y.numel() != X.shape[0]:
                raise ValueError(f"fit: {X.shape[0]} rows of X for {y.numel()} labels")
            if y.dtype.is_floating_point and bool(torch.isnan(y).any()):
                raise ValueError(f"{self.p.objective}: NaN label")
        t0 = self._sync_time()
        host_cuts = {}
        th = None
        if (self.cuts is None and X.device.type == "cpu" and self.device.type == "cuda" and _world() == 1
                and X.dim() == 2 and X.dtype in (torch.float32, torch.float64)):
            # the cuts from the host copy, beside the host->device copy (numpy and
            # the copy release the GIL)
            import threading

            def run():
                try:
                    host_cuts["c"] = self.host_cuts(X)
                except BaseException as e:  # re-raised below
                    host_cuts["e"] = e
            th = threading.Thread(target=run, name="gbdt-cuts", daemon=True)
            th.start()
        X = X.to(self.device)
        y = y.to(self.device)
        ta = self._sync_time()
        if th is not None:
            th.join()
            if "e" in host_cuts:
                raise host_cuts["e"]
            self.cuts = host_cuts["c"].to(self.device)
        elif self.cuts is None:
            self.fit_cuts(X)
        if self.cuts.device != self.device:  # cuts fitted on a host copy (fit_cuts on a CPU X)
            self.cuts = self.cuts.to(self.device)
        tb = self._sync_time()
        bins = self.quantise(X).contiguous()
        n = X.shape[0]
        yq = None
        if quant:  # the base margin: the labels' quantile over all ranks, kept in the parameters
            yq = y.reshape(-1).float().contiguous()
            self.p.base_score = self._quantile_of(yq, self._alpha())
        pred = self._base(n)
        K = pred.shape[1]
        tc = self._sync_time()
        grower = self._device_grower(bins)
        rank = self._rank_setup(y, group) if ranking else None
        t1 = self._sync_time()
        for k, v in (("setup_h2d_s", ta - t0), ("setup_cuts_s", tb - ta), ("setup_quantise_s", tc - tb),
                     ("setup_grower_s", t1 - tc)):
            self.stats[k] = self.stats.get(k, 0.0) + v
        dev_trees = []
        ev = self._eval_begin(eval_set, early_stopping_rounds, grower) if eval_set is not None else None
        for it in range(self.p.n_estimators):
            g_all, h_all = self._grad_hess(pred, y, rank)
            round_trees = []
            for k in range(K):
                g = g_all[:, k].contiguous()
                h = h_all[:, k].contiguous()
                if grower is not None:
                    renew = (yq, pred, k, self._alpha()) if quant else None
                    round_trees.append(self._grow_device(grower, g, h, renew))
                    grower.add_leaf(pred, k)  # pred[:, k] += the rows' leaf values, one launch
                    continue
                tree, leaf = self._grow(bins, g, h, n)
                if quant:
                    self._renew_leaves_torch(tree, leaf, yq, pred[:, k])
                vals = torch.tensor(tree.value, dtype=torch.float32, device=self.device)
                pred[:, k] += vals[leaf.long()]
                round_trees.append(tree)
            if grower is not None:
                dev_trees.append(round_trees)
            else:
                self.trees.append(round_trees)
            if callback is not None:
                callback(it, pred)
            if ev is not None and self._eval_round(ev, it, round_trees):
                break
        if ev is not None:
            self._eval_end(ev)
        t2 = self._sync_time()
        self.stats["setup_s"] = self.stats.get("setup_s", 0.0) + (t1 - t0)
        self.stats["boost_s"] = self.stats.get("boost_s", 0.0) + (t2 - t1)
        if grower is not None:
            # the only device->host copy of training: every tree's heap arrays at once
            if dev_trees:
                host = torch.stack([torch.stack(r) for r in dev_trees]).cpu()
                self.trees += [[self._heap_tree(host[i, k]) for k in range(K)] for i in range(len(dev_trees))]
            b, s = grower.stats()
            self.stats["hist_builds"] += b
            self.stats["hist_subtracted"] += s
            # the fused route + scan's look-back never timed out (a timeout means
            # its partition was wrong: fail loudly rather than return bad trees)
            faults = grower.scan_faults()
            if faults:
                raise RuntimeError(f"GBDT route+scan: {faults} look-back timeouts (csrc/gbdt.hip route_scan_kernel)")
        return pred

    # ------------------------------------------------------------ validation set (fit(eval_set=...))
    def _num_class(self) -> int:
        return self.p.num_class if self.p.objective.startswith("multi:") else 1

    def _loss_sum(self, margin: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """The sum over rows of ``metric``'s per-row loss (squared error for rmse), one
        fp64 scalar on the device."""
        obj = self.p.objective
        if obj.startswith("multi:"):
            pr = torch.softmax(margin, 1)
            row = -torch.log(pr.gather(1, y.long()[:, None]).clamp_min(1e-15))
        elif obj == "binary:logistic":
            pr = torch.sigmoid(margin[:, 0])
            yy = y.float()
            row = -(yy * torch.log(pr.clamp_min(1e-15)) + (1 - yy) * torch.log((1 - pr).clamp_min(1e-15)))
        elif obj in QUANTILE_OBJECTIVES:  # mae: the absolute error; quantile: the pinball loss
            a, d = self._alpha(), y.reshape(-1).double() - margin[:, 0].double()
            row = d.abs() if obj == "reg:absoluteerror" else torch.maximum(a * d, (a - 1.0) * d)
        else:
            row = (margin[:, 0] - y.float()) ** 2
        return row.sum(dtype=torch.float64)

    def _eval_begin(self, eval_set, early_stopping_rounds, grower) -> dict:
        ranking = self.p.objective in RANK_OBJECTIVES
        if ranking and len(eval_set) != 3:
            raise ValueError(f"{self.p.objective}: eval_set must be (Xv, yv, groupv)")
        Xv, yv = eval_set[:2] if ranking else eval_set
        Xv = Xv.to(self.device).float().contiguous()
        yv = yv.to(self.device)
        if Xv.dim() != 2 or Xv.shape[1] != self.cuts.shape[0] or yv.shape[0] != Xv.shape[0]:
            raise ValueError(f"eval_set: Xv {tuple(Xv.shape)} / yv {tuple(yv.shape)} do not match the "
                             f"{self.cuts.shape[0]} training features")
        K = self._num_class()
        esr = self.p.early_stopping_rounds if early_stopping_rounds is None else early_stopping_rounds
        obj = self.p.objective
        self.eval_metric = "mlogloss" if obj.startswith("multi:") else "logloss" if obj == "binary:logistic" else \
            "mae" if obj == "reg:absoluteerror" else "quantile" if obj == "reg:quantileerror" else "rmse"
        self.evals_result = []
        self.best_iteration = self.best_score = None
        count = float(Xv.shape[0])
        rank = None
        if ranking:  # ndcg@k: a mean over groups, and the one metric here where higher is better
            self.eval_metric = self._ndcg_name()
            rank = self._rank_setup(yv, eval_set[2], plan=False)
            count = float(rank["Q"])
        ev = {"X": Xv, "y": yv, "margin": self._base(Xv.shape[0]), "sums": [], "esr": int(esr or 0),
              "best": -math.inf if ranking else math.inf, "best_it": 0, "rank": rank,
              # the validation rows (ranking: groups) of every rank, reduced once
              "count": _allreduce_(torch.tensor([count], dtype=torch.float64, device=self.device))}
        if ev["esr"] > 0:
            ev["count_host"] = float(ev["count"])  # read once, before the rounds
        if grower is not None:
            heap = (1 << (self.p.max_depth + 1)) - 1
            ev["heap"] = heap
            ev["nodes"] = torch.empty(K * heap, 4, dtype=torch.int32, device=self.device)
            ev["off"] = torch.arange(K + 1, dtype=torch.int32, device=self.device) * heap
        return ev

    def _eval_value(self, loss_sum: float, count: float) -> float:
        m = loss_sum / max(count, 1.0)
        return math.sqrt(m) if self.eval_metric == "rmse" else m

    def _eval_round(self, ev: dict, it: int, round_trees) -> bool:
        """Add this round's trees to the validation margin and record its loss sum;
        True = stop training (early stopping)."""
        if "nodes" in ev:
            # the device grower's heap arrays -> packed nodes -> range kernel: no host copy
            ext, heap = _ext.load(), ev["heap"]
            for k, packed in enumerate(round_trees):
                ext.gbdt_heap_nodes(packed, ev["nodes"][k * heap:(k + 1) * heap])
            if ev["X"].shape[0]:
                ext.gbdt_predict(ev["X"], ev["nodes"], ev["off"], 0, len(round_trees), ev["margin"])
        else:
            self._add_trees_torch(ev["X"], ev["margin"], [round_trees])
        if ev["rank"] is not None:
            s = _allreduce_(self._ndcg_sum(ev["margin"].view(-1), ev["rank"]).view(1))
        else:
            s = _allreduce_(self._loss_sum(ev["margin"], ev["y"]).view(1))
        ev["sums"].append(s)
        if ev["esr"] <= 0:
            return False
        v = self._eval_value(float(s), ev["count_host"])  # the one small read of the round
        if (v > ev["best"]) if ev["rank"] is not None else (v < ev["best"]):
            ev["best"], ev["best_it"] = v, it
            return False
        return it - ev["best_it"] >= ev["esr"]

    def _eval_end(self, ev: dict) -> None:
        if not ev["sums"]:
            return
        host = torch.cat(ev["sums"] + [ev["count"]]).tolist()  # one copy for every round
        self.evals_result = [self._eval_value(v, host[-1]) for v in host[:-1]]
        if ev["esr"] > 0:
            self.best_iteration, self.best_score = ev["best_it"], ev["best"]

    # ------------------------------------------------------------ prediction
    def _add_trees_torch(self, X: torch.Tensor, pred: torch.Tensor, rounds) -> torch.Tensor:
        """pred[:, k] += each round's tree k, in order: the torch traversal (the CPU
        path and the numerics reference of csrc/gbdt_predict.hip)."""
        for round_trees in rounds:
            for k, t in enumerate(round_trees):
                feat = torch.tensor(t.feature, device=self.device)
                thr = torch.tensor(t.threshold, device=self.device, dtype=torch.float32)
                left = torch.tensor(t.left, device=self.device)
                right = torch.tensor(t.right, device=self.device)
                val = torch.tensor(t.value, device=self.device)
                node = torch.zeros(X.shape[0], dtype=torch.long, device=self.device)
                for _ in range(self.p.max_depth + 1):
                    f = feat[node]
                    leafm = f < 0
                    if bool(leafm.all()):
                        break
                    xv = X.gather(1, f.clamp_min(0)[:, None])[:, 0]
                    nxt = torch.where(xv <= thr[node], left[node], right[node])
                    node = torch.where(leafm, node, nxt)
                pred[:, k] += val[node]
        return pred

    def predict_margin(self, X: torch.Tensor) -> torch.Tensor:
        X = X.to(self.device).float()
        return self._add_trees_torch(X, self._base(X.shape[0]), self.trees)

    @staticmethod
    def _pack_tree(t: Tree):
        """One tree as (feature, threshold, left, value) numpy arrays in node-table
        form: the children of a split are the adjacent pair (left, left + 1), both
        after their parent.  Both growers number nodes that way; a tree that does
        not (a loaded file) is renumbered as a whole, breadth first."""
        import numpy as np
        n = len(t.value)
        feat = np.asarray(t.feature, dtype=np.int64)
        left = np.asarray(t.left, dtype=np.int64)
        right = np.asarray(t.right, dtype=np.int64)
        thr = np.asarray(t.threshold, dtype=np.float32)
        val = np.asarray(t.value, dtype=np.float32)
        if n == 0 or not (len(feat) == len(left) == len(right) == len(thr) == n):
            raise ValueError(f"tree with inconsistent node arrays (value {n}, feature {len(feat)}, left {len(left)}, "
                             f"right {len(right)}, threshold {len(thr)})")
        split = feat >= 0
        idx = np.arange(n)
        if ((left[split] < 0) | (left[split] >= n) | (right[split] < 0) | (right[split] >= n)).any():
            raise ValueError("tree with a child index outside its node list")
        if not ((right[split] == left[split] + 1) & (left[split] > idx[split])).all():
            order, seen, q = [0], {0}, 0
            while q < len(order):  # breadth first: children get the next two ids
                i = order[q]
                q += 1
                if feat[i] >= 0:
                    for c in (int(left[i]), int(right[i])):
                        if c in seen:
                            raise ValueError("tree whose nodes are shared or form a cycle")
                        seen.add(c)
                        order.append(c)
            order = np.asarray(order)
            new = np.full(n, -1, dtype=np.int64)
            new[order] = np.arange(len(order))
            feat, thr, val = feat[order], thr[order], val[order]
            left = new[left[order]]
            split = feat >= 0
        left = np.where(split, left, -1)
        return feat.astype(np.int32), thr, left.astype(np.int32), val

    def _forest(self):
        """The packed forest on the device: nodes int32 [n, 4] (GbdtNode of
        csrc/kdl_api.h), tree_off int32 [T + 1], tree ``t`` = round ``t // K``, class
        ``t % K``.  Cached; rebuilt when ``trees`` holds other Tree objects (a Tree
        edited in place is not noticed: assign a new one)."""
        import numpy as np
        K = self._num_class()
        flat = []
        for r in self.trees:
            if len(r) != K:
                raise ValueError(f"a boosting round with {len(r)} trees in a {K}-class model")
            flat += r
        key = (str(self.device), tuple(id(t) for t in flat))
        c = self._forest_cache
        if c is not None and c[0] == key:
            return c[2], c[3], c[4]
        parts = [self._pack_tree(t) for t in flat]
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        if parts:
            off[1:] = np.cumsum([len(p[0]) for p in parts])
        if off[-1] >= 2 ** 31:
            raise ValueError("forest of 2^31 or more nodes")
        nodes = np.empty((int(off[-1]), 4), dtype=np.int32)
        if parts:
            nodes[:, 0] = np.concatenate([p[0] for p in parts])
            nodes[:, 1] = np.concatenate([p[1] for p in parts]).view(np.int32)
            nodes[:, 2] = np.concatenate([p[2] for p in parts])
            nodes[:, 3] = np.concatenate([p[3] for p in parts]).view(np.int32)
        max_feat = int(nodes[:, 0].max()) if len(nodes) else -1
        d_nodes = torch.from_numpy(nodes).to(self.device)
        d_off = torch.from_numpy(off.astype(np.int32)).to(self.device)
        self._forest_cache = (key, flat, d_nodes, d_off, max_feat)
        return d_nodes, d_off, max_feat

    def predict(self, X: torch.Tensor, output_margin: bool = False, n_rounds: Optional[int] = None) -> torch.Tensor:
        """Batch prediction with the first ``n_rounds`` rounds (default: up to the best
        round of an early-stopped fit, else all).  ``output_margin=True`` returns the
        raw margin [N, K] (``predict_margin``'s result, bit for bit); otherwise the
        objective's transform: probabilities [N] (``binary:logistic``, sigmoid),
        [N, K] (``multi:softprob``, softmax) or the value [N] (regression).  On the
        GPU this is the forest kernel of csrc/gbdt_predict.hip, on CPU the torch
        traversal."""
        if X.dim() != 2:
            raise ValueError(f"predict: X must be [N, F], got {tuple(X.shape)}")
        if self.cuts is not None and X.shape[1] != self.cuts.shape[0]:
            raise ValueError(f"predict: X has {X.shape[1]} features, the model was fitted on {self.cuts.shape[0]}")
        total = len(self.trees)
        if n_rounds is None:
            n_rounds = total if self.best_iteration is None else self.best_iteration + 1
        if not 0 <= n_rounds <= total:
            raise ValueError(f"predict: n_rounds {n_rounds} outside the model's {total} rounds")
        X = X.to(self.device).float().contiguous()
        margin = self._base(X.shape[0])
        if self.use_hip and X.is_cuda:
            nodes, off, max_feat = self._forest()
            if max_feat >= X.shape[1]:
                raise ValueError(f"predict: the trees split on feature {max_feat}, X has {X.shape[1]} features")
            _ext.load().gbdt_predict(X, nodes, off, 0, n_rounds * margin.shape[1], margin)
        else:
            self._add_trees_torch(X, margin, self.trees[:n_rounds])
        return margin if output_margin else self.transform_margin(margin)

    def transform_margin(self, margin: torch.Tensor) -> torch.Tensor:
        """The objective's output transform of a raw margin [N, K] (see ``predict``)."""
        if self.p.objective.startswith("multi:"):
            return torch.softmax(margin, 1)
        if self.p.objective == "binary:logistic":
            return torch.sigmoid(margin[:, 0])
        return margin[:, 0]

    # ------------------------------------------------------------ feature contributions
    def set_background(self, X: torch.Tensor, interventional: bool = False) -> torch.Tensor:
        """The covers ``predict_contribs`` weighs unknown features with: per node of
        the packed forest, the number of rows of ``X`` (this rank's shard; summed over
        the ranks of a process group) that reach it under ``predict``'s routing.
        int64 [num_nodes], kept beside the forest cache (not saved with the model) and
        dropped when ``trees`` is replaced.  On the GPU this is the cover kernel of
        csrc/gbdt_shap.hip, on CPU a torch traversal.

        ``interventional=True`` also keeps the rows themselves (on the device) for
        ``predict_contribs(..., perturbation="interventional")``, whose first call per
        ``n_rounds`` reduces them to the per-path mask histogram (csrc/gbdt_iv.hip) --
        with several ranks that first call is collective.  The torch path loops over
        the background rows, so with several ranks it gathers every rank's rows here."""
        if X.dim() != 2:
            raise ValueError(f"set_background: X must be [N, F], got {tuple(X.shape)}")
        if self.cuts is not None and X.shape[1] != self.cuts.shape[0]:
            raise ValueError(f"set_background: X has {X.shape[1]} features, the model was fitted on "
                             f"{self.cuts.shape[0]}")
        X = X.to(self.device).float().contiguous()
        rows = _allreduce_(torch.tensor([X.shape[0]], dtype=torch.int64, device=self.device))
        if int(rows) == 0:
            raise ValueError("set_background: an empty background set")
        nodes, off, max_feat = self._forest()
        if max_feat >= X.shape[1]:
            raise ValueError(f"set_background: the trees split on feature {max_feat}, X has {X.shape[1]} features")
        counts = torch.zeros(nodes.shape[0], dtype=torch.int64, device=self.device)
        if self.use_hip and X.is_cuda:
            _ext.load().gbdt_cover(X, nodes, off, 0, off.numel() - 1, counts)
        else:
            self._cover_torch(X, nodes, off, counts)
        _allreduce_(counts)
        self._cover_cache = (self._forest_cache[0], counts, X.shape[1])
        self._paths_cache = self._pairs_cache = None
        self._iv_bg = self._iv_cache = None
        if interventional:
            if _world() > 1 and not (self.use_hip and X.is_cuda):
                parts = [None] * _world()
                dist.all_gather_object(parts, X.cpu())
                X = torch.cat(parts).to(self.device)
            self._iv_bg = (self._forest_cache[0], X, int(rows))
        return counts

    @staticmethod
    def _cover_torch(X: torch.Tensor, nodes: torch.Tensor, off: torch.Tensor, counts: torch.Tensor) -> None:
        """counts[node] += rows of X reaching the node, on torch ops (the CPU path and
        the reference of csrc/gbdt_shap.hip's cover kernel)."""
        offs = off.tolist()
        for o, e in zip(offs, offs[1:]):
            if e == o:
                continue
            feat, left = nodes[o:e, 0].long(), nodes[o:e, 2].long()
            thr = nodes[o:e, 1].contiguous().view(torch.float32)
            rows = torch.arange(X.shape[0], device=X.device)
            node = torch.zeros_like(rows)
            while rows.numel():
                counts[o:e] += torch.bincount(node, minlength=e - o)
                f = feat[node]
                m = f >= 0
                rows, node, f = rows[m], node[m], f[m]
                node = left[node] + (~(X[rows, f] <= thr[node])).long()

    def _path_table(self, n_rounds: int) -> dict:
        """The first ``n_rounds`` rounds as root-to-leaf paths (csrc/gbdt_shap.hip's
        header has the layout): per path the leaf value and one merged element per
        distinct feature -- ``lo`` (largest right-turn threshold, NaN: none), ``hi``
        (smallest left-turn threshold, with a has-left flag) and the zero fraction
        ``z`` = prod cover[child] / cover[parent] over the feature's splits (0 / 0 := 0),
        in fp64 until the end.  Class-major, cut into chunks of whole paths.  Cached per
        (forest, covers, n_rounds)."""
        import numpy as np
        nodes, off, _ = self._forest()
        c = self._cover_cache
        if c is None or c[0] != self._forest_cache[0]:
            raise ValueError("predict_contribs: no background set for these trees (call set_background(X) first)")
        key = (c[0], id(c[1]), n_rounds)
        if self._paths_cache is not None and self._paths_cache[0] == key:
            return self._paths_cache[1]
        K = self._num_class()
        nd, offs, cover = nodes.cpu().numpy(), off.cpu().tolist(), c[1].cpu().tolist()
        nan = math.nan
        p_v, p_m, p_cls = [], [], []                                  # per path
        e_path, e_j, e_f, e_lo, e_hi, e_hl, e_z = [], [], [], [], [], [], []  # per element
        bias = [0.0] * K
        bias0 = [0.0] * K  # the leaves of single-leaf trees (m = 0): what the interventional bias adds as it is
        for k in range(K):
            for t in range(k, n_rounds * K, K):
                o, e = offs[t], offs[t + 1]
                feat, left = nd[o:e, 0].tolist(), nd[o:e, 2].tolist()
                thr = np.ascontiguousarray(nd[o:e, 1]).view(np.float32).tolist()
                val = np.ascontiguousarray(nd[o:e, 3]).view(np.float32).tolist()
                stack = [(0, ())] if e > o else []
                while stack:
                    i, elems = stack.pop()
                    f = feat[i]
                    if f < 0:
                        z_all = 1.0
                        for j, (ef, lo, hi, hl, z) in enumerate(elems):
                            e_path.append(len(p_v)); e_j.append(j); e_f.append(ef); e_lo.append(lo)
                            e_hi.append(hi); e_hl.append(hl); e_z.append(z)
                            z_all *= z
                        bias[k] += val[i] * z_all
                        if elems:
                            p_v.append(val[i]); p_m.append(len(elems)); p_cls.append(k)
                        else:
                            bias0[k] += val[i]
                        continue
                    th, cp = thr[i], cover[o + i]
                    at = next((j for j, el in enumerate(elems) if el[0] == f), -1)
                    for child, is_left in ((left[i] + 1, False), (left[i], True)):  # the left child is popped first
                        frac = cover[o + child] / cp if cp > 0 else 0.0
                        _, lo, hi, hl, z = elems[at] if at >= 0 else (f, nan, 0.0, False, 1.0)
                        if is_left:  # x <= hi and x <= th; a NaN threshold lets nothing through
                            hi = th if not hl else hi if hi != hi else th if th != th else min(hi, th)
                            hl = True
                        elif th == th:  # !(x <= lo) and !(x <= th); a NaN threshold lets everything through
                            lo = th if lo != lo else max(lo, th)
                        el = (f, lo, hi, hl, z * frac)
                        new = elems[:at] + (el,) + elems[at + 1:] if at >= 0 else elems + (el,)
                        if len(new) > 10:
                            raise ValueError("predict_contribs: a root-to-leaf path splits on more than 10 features")
                        stack.append((child, new))
        m = np.asarray(p_m, dtype=np.int64)
        length = 1 + m + (m + 3) // 4
        start = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
        if start[-1] >= 2 ** 29:
            raise ValueError("predict_contribs: path table of 2^29 or more slots")
        # chunks of whole paths, none across a class boundary
        limit = _ext.load().gbdt_contribs_chunk_slots() if self.use_hip else 512
        chunk_off, class_chunk, cur = [0], [0] * (K + 1), 0
        for p in range(len(m)):
            if p_cls[p] != cur or start[p + 1] - chunk_off[-1] > limit:
                if start[p] > chunk_off[-1]:
                    chunk_off.append(int(start[p]))
                for kk in range(cur + 1, p_cls[p] + 1):
                    class_chunk[kk] = len(chunk_off) - 1
                cur = p_cls[p]
        if start[-1] > chunk_off[-1]:
            chunk_off.append(int(start[-1]))
        for kk in range(cur + 1, K + 1):
            class_chunk[kk] = len(chunk_off) - 1
        ep, ej = np.asarray(e_path, dtype=np.int64), np.asarray(e_j, dtype=np.int64)
        ef, ehl = np.asarray(e_f, dtype=np.int64), np.asarray(e_hl, dtype=bool)
        elo, ehi, ez = (np.asarray(a, dtype=np.float64) for a in (e_lo, e_hi, e_z))
        slots = np.zeros((int(start[-1]), 4), dtype=np.int32)
        fl = slots.view(np.float32)
        head = start[:-1]
        fl[head, 0] = np.asarray(p_v, dtype=np.float32)
        slots[head, 1] = m
        at = head[ep] + 1 + ej
        slots[at, 0] = ef | (ehl.astype(np.int64) << 30)
        fl[at, 1], fl[at, 2], fl[at, 3] = elo, ehi, ez
        fl[head[ep] + 1 + m[ep] + ej // 4, ej % 4] = 1.0 - ez  # rounded from fp64, not formed in fp32
        # the same paths padded to [P, M] for the torch path
        M = int(m.max()) if len(m) else 0
        pad = {"feat": np.zeros((len(m), M), dtype=np.int64), "lo": np.full((len(m), M), nan),
               "hi": np.zeros((len(m), M)), "hl": np.zeros((len(m), M), dtype=bool), "z": np.ones((len(m), M)),
               "valid": np.zeros((len(m), M), dtype=bool)}
        for name, a in (("feat", ef), ("lo", elo), ("hi", ehi), ("hl", ehl), ("z", ez), ("valid", True)):
            pad[name][ep, ej] = a
        pad["v"], pad["cls"] = np.asarray(p_v, dtype=np.float64), np.asarray(p_cls, dtype=np.int64)
        base = float(self._base(1)[0, 0])
        dev = self.device
        table = {"slots": torch.from_numpy(slots).to(dev),
                 "chunk_off": torch.tensor(chunk_off, dtype=torch.int32, device=dev),
                 "class_chunk": torch.tensor(class_chunk, dtype=torch.int32, device=dev),
                 "bias64": [b + base for b in bias], "bias0": [b + base for b in bias0], "pad": pad}
        table["bias"] = torch.tensor(table["bias64"], dtype=torch.float32, device=dev)
        self._paths_cache = (key, table)
        return table

    def _contribs_torch(self, X: torch.Tensor, table: dict) -> torch.Tensor:
        """``predict_contribs`` on torch ops, fp64 inside: the kernel's path formula
        (Gauss-Legendre in t, prefix and suffix products) over padded paths, a block of
        rows and paths at a time.  The CPU path."""
        import numpy as np
        N, F = X.shape
        K = self._num_class()
        dev = X.device
        pad = {k: torch.from_numpy(v).to(dev) for k, v in table["pad"].items()}
        P, M = pad["feat"].shape
        phi = torch.zeros(N, K * (F + 1), dtype=torch.float64, device=dev)
        if P and N:
            Q = (M + 1) // 2  # exact for degree M - 1
            gx, gw = np.polynomial.legendre.leggauss(Q)
            tq = torch.from_numpy((gx + 1) / 2).to(dev)
            wq = torch.from_numpy(gw / 2).to(dev)
            nr = min(N, 65536)
            pc = max(1, (1 << 22) // (nr * M * Q))
            for r0 in range(0, N, nr):
                Xr = X[r0:r0 + nr].double()
                n = Xr.shape[0]
                one = torch.ones(n, 1, 1, Q, dtype=torch.float64, device=dev)
                for p0 in range(0, P, pc):
                    s = slice(p0, p0 + pc)
                    f, z, valid = pad["feat"][s], pad["z"][s], pad["valid"][s]
                    xv = Xr[:, f.reshape(-1)].view(n, -1, M)
                    o = (~(xv <= pad["lo"][s]) & (~pad["hl"][s] | (xv <= pad["hi"][s]))) | ~valid
                    fac = o.double()[..., None] * tq + (z[..., None] * (1 - tq))
                    fac = torch.where(valid[..., None], fac, torch.ones_like(fac))
                    ones = one.expand(n, fac.shape[1], 1, Q)
                    pre = torch.cat([ones, fac[:, :, :-1]], 2).cumprod(2)
                    suf = torch.cat([fac[:, :, 1:], ones], 2).flip(2).cumprod(2).flip(2)
                    W = (pre * suf * wq).sum(-1)
                    d = torch.where(o, 1.0 - z, -z) * valid
                    term = pad["v"][s][:, None] * d * W
                    idx = (pad["cls"][s][:, None] * (F + 1) + f).reshape(-1)
                    phi[r0:r0 + n].index_add_(1, idx, term.reshape(n, -1))
        phi = phi.view(N, K, F + 1)
        phi[:, :, F] = torch.tensor(table["bias64"], dtype=torch.float64, device=dev)
        return phi.float()

    def predict_contribs(self, X: torch.Tensor, n_rounds: Optional[int] = None,
                         perturbation: str = "path_dependent") -> torch.Tensor:
        """Per-feature contributions to the raw margin, fp32 [N, K, F + 1]: exact
        path-dependent TreeSHAP with the covers of ``set_background`` (row counts), the
        Shapley values of ``S -> sum over the class's trees of E_t(x, S)``.  Column ``F``
        is the bias (the expected margin over the background plus the base margin); the
        last axis sums to ``predict(X, output_margin=True)`` up to rounding.
        ``n_rounds`` as in ``predict``.  On the GPU this is the contribution kernel of
        csrc/gbdt_shap.hip, on CPU the same formula on torch ops in fp64.

        ``perturbation="interventional"``: the interventional (marginal) TreeSHAP of the
        module docstring over the rows of ``set_background(X, interventional=True)``; the
        bias is then the mean margin over those rows.  On the GPU the kernels of
        csrc/gbdt_iv.hip over the mask histogram, on CPU ``_contribs_iv_torch``."""
        if perturbation not in ("path_dependent", "interventional"):
            raise ValueError(f"predict_contribs: perturbation {perturbation!r} (path_dependent or interventional)")
        if X.dim() != 2:
            raise ValueError(f"predict_contribs: X must be [N, F], got {tuple(X.shape)}")
        if self.cuts is not None and X.shape[1] != self.cuts.shape[0]:
            raise ValueError(f"predict_contribs: X has {X.shape[1]} features, the model was fitted on "
                             f"{self.cuts.shape[0]}")
        total = len(self.trees)
        if n_rounds is None:
            n_rounds = total if self.best_iteration is None else self.best_iteration + 1
        if not 0 <= n_rounds <= total:
            raise ValueError(f"predict_contribs: n_rounds {n_rounds} outside the model's {total} rounds")
        table = self._path_table(n_rounds)
        if X.shape[1] != self._cover_cache[2]:
            raise ValueError(f"predict_contribs: X has {X.shape[1]} features, the background set had "
                             f"{self._cover_cache[2]}")
        X = X.to(self.device).float().contiguous()
        if perturbation == "interventional":
            bg = self._iv_bg
            if bg is None or bg[0] != self._forest_cache[0]:
                raise ValueError("predict_contribs: perturbation='interventional' needs the background rows of these "
                                 "trees (call set_background(X, interventional=True) first)")
            if self.use_hip and X.is_cuda:
                iv = self._iv_table(n_rounds)
                out = torch.empty(X.shape[0], self._num_class(), X.shape[1] + 1, dtype=torch.float32,
                                  device=self.device)
                _ext.load().gbdt_contribs_iv(X, iv["slots"], iv["chunk_off"], iv["class_chunk"], iv["bias"],
                                             out.shape[1], out)
                return out
            return self._contribs_iv_torch(X, table, bg[1], bg[2])
        if self.use_hip and X.is_cuda:
            out = torch.empty(X.shape[0], self._num_class(), X.shape[1] + 1, dtype=torch.float32, device=self.device)
            _ext.load().gbdt_contribs(X, table["slots"], table["chunk_off"], table["class_chunk"], table["bias"],
                                      out.shape[1], out)
            return out
        return self._contribs_torch(X, table)

    # ------------------------------------------------------------ interventional contributions
    @staticmethod
    def _iv_weights():
        """The Shapley weights of a conjunction game, fp64 [11, 11] each (module docstring):
        ``Wp[a][b] = (a-1)! b! / (a+b)!`` (a >= 1), ``Wn[a][b] = a! (b-1)! / (a+b)!`` (b >= 1),
        0 elsewhere and where ``a + b > 10``."""
        import numpy as np
        fact = [float(math.factorial(i)) for i in range(11)]
        wp, wn = np.zeros((11, 11)), np.zeros((11, 11))
        for a in range(11):
            for b in range(11 - a):
                if a:
                    wp[a, b] = fact[a - 1] * fact[b] / fact[a + b]
                if b:
                    wn[a, b] = fact[a] * fact[b - 1] / fact[a + b]
        return wp, wn

    def _contribs_iv_torch(self, X: torch.Tensor, table: dict, Z: torch.Tensor, B: int) -> torch.Tensor:
        """``predict_contribs(perturbation="interventional")`` on torch ops, fp64 inside and
        rounded once: the module docstring's definition evaluated for every (row, background
        row, path), a block at a time -- the background rows ``Z`` themselves, not their
        mask histogram.  ``B``: the background rows of all ranks.  The CPU path."""
        N, F = X.shape
        K, dev = self._num_class(), X.device
        pad = {k: torch.from_numpy(v).to(dev) for k, v in table["pad"].items()}
        P, M = pad["feat"].shape
        wp, wn = (torch.from_numpy(w).to(dev) for w in self._iv_weights())
        phi = torch.zeros(N, K * (F + 1), dtype=torch.float64, device=dev)
        bias = torch.tensor(table["bias0"], dtype=torch.float64, device=dev)

        def inside(R, s):  # [rows, paths, M]: the interval tests, False at the padding
            xv = R[:, pad["feat"][s].reshape(-1)].view(R.shape[0], -1, M)
            return ~(xv <= pad["lo"][s]) & (~pad["hl"][s] | (xv <= pad["hi"][s])) & pad["valid"][s]
        if P:
            Zd = Z.double()
            nr, nz = max(min(N, 256), 1), min(Zd.shape[0], 64)
            pc = max(1, (1 << 22) // (nr * nz * M))
            for p0 in range(0, P, pc):
                s = slice(p0, p0 + pc)
                valid, v = pad["valid"][s], pad["v"][s]
                idx = (pad["cls"][s][:, None] * (F + 1) + pad["feat"][s]).reshape(-1)
                full = torch.zeros(v.shape[0], dtype=torch.float64, device=dev)  # background rows that reach the leaf
                for z0 in range(0, Zd.shape[0], nz):
                    oz = inside(Zd[z0:z0 + nz], s)
                    full += (oz | ~valid).all(-1).sum(0)
                    for r0 in range(0, N, nr):
                        ox = inside(X[r0:r0 + nr].double(), s)[:, None]  # [n, 1, p, M] against [z, p, M]
                        reach = (ox | oz | ~valid).all(-1)
                        D, E = ox & ~oz, oz & ~ox
                        a, b = D.sum(-1), E.sum(-1)
                        term = (D * wp[a, b][..., None] - E * wn[a, b][..., None]) * reach[..., None]
                        term = term.sum(1) * v[:, None]
                        phi[r0:r0 + ox.shape[0]].index_add_(1, idx, term.reshape(ox.shape[0], -1))
                bias.index_add_(0, pad["cls"][s], v * full / B)
            phi /= B
        phi = phi.view(N, K, F + 1)
        phi[:, :, F] = bias
        return phi.float()

    def _iv_table(self, n_rounds: int) -> dict:
        """The explain table of csrc/gbdt_iv.hip (its header has both layouts) for the first
        ``n_rounds`` rounds: the background rows are reduced by the mask-histogram kernel to
        ``hist[path][mask]`` (int64, all-reduced over the ranks), and the masks with a count
        above 0 are compacted behind each path's elements as records ``{mask, count / B}``.
        A path with more records than a chunk holds becomes several table paths.  ``bias``:
        the base margin plus the mean margin over the background, summed in fp64.  Cached
        beside the path table, under its key."""
        import numpy as np
        table = self._path_table(n_rounds)
        key = self._paths_cache[0]
        if self._iv_cache is not None and self._iv_cache[0] == key:
            return self._iv_cache[1]
        ext, dev, K = _ext.load(), self.device, self._num_class()
        pad, (_, Z, B) = table["pad"], self._iv_bg
        m = pad["valid"].sum(1).astype(np.int64)  # a path's elements are its first m
        P = len(m)
        hoff = np.concatenate([[0], np.cumsum(np.left_shift(1, m))]).astype(np.int64)  # 2^m counters per path
        if hoff[-1] >= 2 ** 31:
            raise ValueError("predict_contribs: mask histogram of 2^31 or more counters")

        def put(slots, head, paths):  # headers { v, m, ., . } and elements of the table paths at ``head``
            mm = m[paths]
            g = np.repeat(np.arange(len(paths)), mm)
            j = np.arange(len(g)) - np.repeat(np.cumsum(mm) - mm, mm)
            at, sp, fl = head[g] + 1 + j, paths[g], slots.view(np.float32)
            fl[head, 0] = pad["v"][paths]
            slots[head, 1] = mm
            slots[at, 0] = pad["feat"][sp, j] | (pad["hl"][sp, j].astype(np.int64) << 30)
            fl[at, 1], fl[at, 2] = pad["lo"][sp, j], pad["hi"][sp, j]
        t0 = self._sync_time()
        # kernel A's table: chunks of whole paths within both the slot and the counter budget
        mstart = np.concatenate([[0], np.cumsum(1 + m)]).astype(np.int64)
        lim_s, lim_c = ext.gbdt_path_masks_chunk_slots(), ext.gbdt_path_masks_chunk_counters()
        chunk_off, cnt_off = [0], [0]
        for p in range(P):
            if mstart[p + 1] - chunk_off[-1] > lim_s or hoff[p + 1] - cnt_off[-1] > lim_c:
                chunk_off.append(int(mstart[p]))
                cnt_off.append(int(hoff[p]))
        if P:
            chunk_off.append(int(mstart[-1]))
            cnt_off.append(int(hoff[-1]))
        mslots = np.zeros((int(mstart[-1]), 4), dtype=np.int32)
        put(mslots, mstart[:-1], np.arange(P))
        mslots[mstart[:-1], 2] = hoff[:-1]
        hist = torch.zeros(int(hoff[-1]), dtype=torch.int64, device=dev)
        masks = (torch.from_numpy(mslots).to(dev), torch.tensor(chunk_off, dtype=torch.int32, device=dev),
                 torch.tensor(cnt_off, dtype=torch.int32, device=dev))
        ext.gbdt_path_masks(Z, *masks, hist)
        _allreduce_(hist)
        t1 = self._sync_time()
        h = hist.cpu().numpy()
        if P and not (np.add.reduceat(h, hoff[:-1]) == B).all():
            raise RuntimeError("predict_contribs: a path's mask counters do not sum to the background rows "
                               "(csrc/gbdt_iv.hip path_masks_kernel)")
        # records: the masks with a count above 0, in (path, mask) order; w rounds once, from fp64
        nz = np.flatnonzero(h)
        rp = np.searchsorted(hoff, nz, side="right") - 1
        r = np.bincount(rp, minlength=P)
        limit = ext.gbdt_contribs_iv_chunk_slots()
        cap = 2 * (limit - 1 - m)  # records one table path can hold
        pieces = np.maximum((r + cap - 1) // cap, 1)
        first = np.cumsum(pieces) - pieces
        pp = np.repeat(np.arange(P), pieces)  # the path of each table path
        pr = np.minimum(cap[pp], r[pp] - (np.arange(len(pp)) - first[pp]) * cap[pp])
        start = np.concatenate([[0], np.cumsum(1 + m[pp] + (pr + 1) // 2)]).astype(np.int64)
        if start[-1] >= 2 ** 29:
            raise ValueError("predict_contribs: interventional explain table of 2^29 or more slots")
        cls = pad["cls"][pp]
        chunk_off, class_chunk, cur = [0], [0] * (K + 1), 0
        for p in range(len(pp)):  # chunks of whole table paths, none across a class boundary
            if cls[p] != cur or start[p + 1] - chunk_off[-1] > limit:
                if start[p] > chunk_off[-1]:
                    chunk_off.append(int(start[p]))
                for kk in range(cur + 1, cls[p] + 1):
                    class_chunk[kk] = len(chunk_off) - 1
                cur = cls[p]
        if start[-1] > chunk_off[-1]:
            chunk_off.append(int(start[-1]))
        for kk in range(cur + 1, K + 1):
            class_chunk[kk] = len(chunk_off) - 1
        slots = np.zeros((int(start[-1]), 4), dtype=np.int32)
        put(slots, start[:-1], pp)
        slots[start[:-1], 2] = pr
        slots[start[:-1], 3] = np.left_shift(1, m[pp]) - 1
        ri = np.arange(len(rp)) - (np.cumsum(r) - r)[rp]  # the record's index in its path
        j = ri % cap[rp]
        at = start[first[rp] + ri // cap[rp]] + 1 + m[rp] + j // 2
        slots[at, (j % 2) * 2] = nz - hoff[rp]
        slots.view(np.float32)[at, (j % 2) * 2 + 1] = h[nz] / B
        # bias: base + paths with m = 0 + v * count(mask == full) / B, in fp64
        bias = np.asarray(table["bias0"], dtype=np.float64)
        if P:
            bias = bias + np.bincount(pad["cls"], weights=pad["v"] * h[hoff[1:] - 1] / B, minlength=K)
        t2 = self._sync_time()
        iv = {"slots": torch.from_numpy(slots).to(dev),
              "chunk_off": torch.tensor(chunk_off, dtype=torch.int32, device=dev),
              "class_chunk": torch.tensor(class_chunk, dtype=torch.int32, device=dev),
              "bias": torch.from_numpy(bias.astype(np.float32)).to(dev), "hist": hist, "masks": masks,
              "paths": P, "table_paths": int(len(pp)), "records": int(len(nz)), "hist_seconds": t1 - t0, "compact_seconds": t2 - t1}
        self._iv_cache = (key, iv)
        return iv

    # ------------------------------------------------------------ interaction values
    def _pair_table(self, n_rounds: int, F: int) -> dict:
        """``_path_table``'s paths regrouped for csrc/gbdt_interactions.hip (its header
        has the layout): per class and per feature a path of the class splits on, the
        paths that hold the feature, in table order, with that feature's element
        rotated to slot 0; the same 16-byte slots.  Every (class, feature) list is cut
        into chunks of whole paths; list ``k * F + i`` owns chunks
        ``[feat_chunk[k * F + i], feat_chunk[k * F + i + 1])``.  Cached beside the path
        table, under its key."""
        import numpy as np
        table = self._path_table(n_rounds)
        key = (self._paths_cache[0], F)
        if self._pairs_cache is not None and self._pairs_cache[0] == key:
            return self._pairs_cache[1]
        pad, K = table["pad"], self._num_class()
        m = pad["valid"].sum(1)
        pp, ee = np.nonzero(pad["valid"])  # one copy of path pp per element ee (a path's elements are its first m)
        gid = pad["cls"][pp] * F + pad["feat"][pp, ee]
        order = np.lexsort((pp, gid))  # by list, then table order
        pp, ee, gid = pp[order], ee[order], gid[order]
        mg = m[pp]
        start = np.concatenate([[0], np.cumsum(1 + mg + (mg + 3) // 4)]).astype(np.int64)
        if start[-1] >= 2 ** 29:  # sum m^2 slots, not sum m: the int32 table's limit comes sooner here
            raise ValueError("predict_interactions: per-feature path table of 2^29 or more slots")
        limit = _ext.load().gbdt_interactions_chunk_slots() if self.use_hip else 512
        chunk_off, feat_chunk, cur = [0], [0] * (K * F + 1), 0
        for g in range(len(pp)):
            if gid[g] != cur or start[g + 1] - chunk_off[-1] > limit:
                if start[g] > chunk_off[-1]:
                    chunk_off.append(int(start[g]))
                for kk in range(cur + 1, int(gid[g]) + 1):
                    feat_chunk[kk] = len(chunk_off) - 1
                cur = int(gid[g])
        if start[-1] > chunk_off[-1]:
            chunk_off.append(int(start[-1]))
        for kk in range(cur + 1, K * F + 1):
            feat_chunk[kk] = len(chunk_off) - 1
        # slot s of copy g: the rotated element first, then the others in their order
        eg = np.repeat(np.arange(len(pp)), mg)
        s = np.arange(len(eg)) - np.repeat(np.cumsum(mg) - mg, mg)
        src = np.where(s == 0, ee[eg], np.where(s <= ee[eg], s - 1, s))
        sp, head = pp[eg], start[:-1]
        slots = np.zeros((int(start[-1]), 4), dtype=np.int32)
        fl = slots.view(np.float32)
        fl[head, 0] = pad["v"][pp]
        slots[head, 1] = mg
        at = head[eg] + 1 + s
        slots[at, 0] = pad["feat"][sp, src] | (pad["hl"][sp, src].astype(np.int64) << 30)
        fl[at, 1], fl[at, 2], fl[at, 3] = pad["lo"][sp, src], pad["hi"][sp, src], pad["z"][sp, src]
        fl[head[eg] + 1 + mg[eg] + s // 4, s % 4] = 1.0 - pad["z"][sp, src]  # rounded from fp64
        dev = self.device
        pairs = {"slots": torch.from_numpy(slots).to(dev),
                 "chunk_off": torch.tensor(chunk_off, dtype=torch.int32, device=dev),
                 "feat_chunk": torch.tensor(feat_chunk, dtype=torch.int32, device=dev)}
        self._pairs_cache = (key, pairs)
        return pairs

    def _interactions_torch(self, X: torch.Tensor, table: dict) -> torch.Tensor:
        """``predict_interactions`` on torch ops, fp64 inside and rounded once at the end:
        the module docstring's formula over ``_path_table``'s padded paths.  For each
        conditioning slot ``a`` the factor of ``a`` is set to 1, so prefix times suffix
        products give ``W_ab`` at ``b != a`` and ``W_a`` at ``b = a``.  The CPU path."""
        import numpy as np
        N, F = X.shape
        K, F1, dev = self._num_class(), F + 1, X.device
        pad = {k: torch.from_numpy(v).to(dev) for k, v in table["pad"].items()}
        P, M = pad["feat"].shape
        out = torch.zeros(N, K, F1, F1, dtype=torch.float32, device=dev)
        if N == 0:
            return out
        Q = max((M + 1) // 2, 1)  # exact for degree M - 1
        gx, gw = np.polynomial.legendre.leggauss(Q)
        tq = torch.from_numpy((gx + 1) / 2).to(dev)
        wq = torch.from_numpy(gw / 2).to(dev)
        bias = torch.tensor(table["bias64"], dtype=torch.float64, device=dev)
        nr = max(1, min(N, (1 << 24) // (K * F1 * F1)))
        pc = max(1, (1 << 22) // (nr * max(M, 1) * Q))
        for r0 in range(0, N, nr):
            Xr = X[r0:r0 + nr].double()
            n = Xr.shape[0]
            phi = torch.zeros(n, K * F1 * F1, dtype=torch.float64, device=dev)
            for p0 in range(0, P, pc):
                s = slice(p0, p0 + pc)
                f, z, valid = pad["feat"][s], pad["z"][s], pad["valid"][s]
                xv = Xr[:, f.reshape(-1)].view(n, -1, M)
                o = (~(xv <= pad["lo"][s]) & (~pad["hl"][s] | (xv <= pad["hi"][s]))) | ~valid
                fac = o.double()[..., None] * tq + (z[..., None] * (1 - tq))
                fac = torch.where(valid[..., None], fac, torch.ones_like(fac))
                ones = torch.ones(n, fac.shape[1], 1, Q, dtype=torch.float64, device=dev)
                d = torch.where(o, 1.0 - z, -z) * valid  # o - z, 0 at the padding
                v = pad["v"][s][None, :, None]
                cell = pad["cls"][s][:, None] * (F1 * F1) + f  # + f_a * F1: the entry's flat index
                for a in range(M):
                    fa = fac.clone()
                    fa[:, :, a] = 1.0
                    pre = torch.cat([ones, fa[:, :, :-1]], 2).cumprod(2)
                    suf = torch.cat([fa[:, :, 1:], ones], 2).flip(2).cumprod(2).flip(2)
                    W = (pre * suf * wq).sum(-1)
                    term = 0.5 * v * d[:, :, a:a + 1] * d * W
                    term[:, :, a] = 0.0
                    term[:, :, a] = v[..., 0] * d[:, :, a] * W[:, :, a] - term.sum(-1)
                    phi.index_add_(1, (cell + f[:, a:a + 1] * F1).reshape(-1), term.reshape(n, -1))
            phi = phi.view(n, K, F1, F1)
            phi[:, :, F, F] = bias
            out[r0:r0 + n] = phi.float()
        return out

    def predict_interactions(self, X: torch.Tensor, n_rounds: Optional[int] = None) -> torch.Tensor:
        """SHAP interaction values of the raw margin, fp32 [N, K, F + 1, F + 1] in XGBoost's
        ``pred_interactions`` layout (the module docstring has the definition): the
        Shapley interaction index off the diagonal, the diagonal so that the last axis
        sums to ``predict_contribs(X)``, the bias at ``[F, F]``.  Needs the covers of
        ``set_background``; ``n_rounds`` as in ``predict``.  On the GPU this is the kernel
        of csrc/gbdt_interactions.hip, on CPU ``_interactions_torch``.  The result holds
        ``N K (F + 1)^2`` floats: call it on row blocks of a large ``X``."""
        if X.dim() != 2:
            raise ValueError(f"predict_interactions: X must be [N, F], got {tuple(X.shape)}")
        if self.cuts is not None and X.shape[1] != self.cuts.shape[0]:
            raise ValueError(f"predict_interactions: X has {X.shape[1]} features, the model was fitted on "
                             f"{self.cuts.shape[0]}")
        total = len(self.trees)
        if n_rounds is None:
            n_rounds = total if self.best_iteration is None else self.best_iteration + 1
        if not 0 <= n_rounds <= total:
            raise ValueError(f"predict_interactions: n_rounds {n_rounds} outside the model's {total} rounds")
        table = self._path_table(n_rounds)
        if X.shape[1] != self._cover_cache[2]:
            raise ValueError(f"predict_interactions: X has {X.shape[1]} features, the background set had "
                             f"{self._cover_cache[2]}")
        X = X.to(self.device).float().contiguous()
        if self.use_hip and X.is_cuda:
            N, F, K = X.shape[0], X.shape[1], self._num_class()
            pairs = self._pair_table(n_rounds, F)
            out = torch.empty(N, K, F + 1, F + 1, dtype=torch.float32, device=self.device)
            _ext.load().gbdt_interactions(X, pairs["slots"], pairs["chunk_off"], pairs["feat_chunk"], table["bias"],
                                          K, out)
            return out
        return self._interactions_torch(X, table)

    # ------------------------------------------------------------ model file
    FORMAT_VERSION = 1

    def save(self, path: str) -> None:
        """The model as JSON: ``params``, ``cuts`` ([F, B-1]) and ``trees`` (per round,
        per class, the Tree arrays), plus ``version``.  Infinite thresholds are
        written as JSON's ``Infinity`` extension, which ``load`` reads back."""
        doc = {"version": self.FORMAT_VERSION, "params": dict(self.p.__dict__),
               "cuts": None if self.cuts is None else self.cuts.cpu().tolist(),
               "trees": [[dict(t.__dict__) for t in r] for r in self.trees]}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(doc, f)

    @classmethod
    def load(cls, path: str, device=None) -> "HistGBDT":
        with open(path) as f:
            doc = json.load(f)
        missing = [k for k in ("params", "cuts", "trees") if k not in doc]
        if missing:
            raise ValueError(f"{path}: not a HistGBDT model file (no {', '.join(missing)})")
        if int(doc.get("version", 1)) > cls.FORMAT_VERSION:
            raise ValueError(f"{path}: model file version {doc['version']} is newer than this code reads "
                             f"({cls.FORMAT_VERSION})")
        known = GBDTParams.__dataclass_fields__
        m = cls(GBDTParams(**{k: v for k, v in doc["params"].items() if k in known}), device)
        if doc["cuts"] is not None:
            m.cuts = torch.tensor(doc["cuts"], dtype=torch.float32, device=m.device)
            if m.cuts.dim() != 2:
                raise ValueError(f"{path}: cuts must be [features, bins - 1]")
        K = m._num_class()
        fields = Tree.__dataclass_fields__
        for ri, r in enumerate(doc["trees"]):
            if len(r) != K:
                raise ValueError(f"{path}: round {ri} has {len(r)} trees, the objective needs {K}")
            trees = []
            for k, d in enumerate(r):
                if set(d) != set(fields):
                    raise ValueError(f"{path}: round {ri} tree {k}: expected the arrays {sorted(fields)}")
                t = Tree(**{name: list(d[name]) for name in fields})
                try:
                    feat = cls._pack_tree(t)[0]
                except ValueError as e:
                    raise ValueError(f"{path}: round {ri} tree {k}: {e}") from None
                if m.cuts is not None and len(feat) and int(feat.max()) >= m.cuts.shape[0]:
                    raise ValueError(f"{path}: round {ri} tree {k} splits on feature {int(feat.max())}, but the "
                                     f"model has only {m.cuts.shape[0]} features (rows of cuts)")
                trees.append(t)
            m.trees.append(trees)
        return m

    def metric(self, pred: torch.Tensor, y: torch.Tensor, group=None) -> dict:
        obj = self.p.objective
        if obj in RANK_OBJECTIVES:
            if group is None:
                raise ValueError(f"{obj}: the metric needs the query groups: metric(pred, y, group=sizes)")
            if pred.shape[0] != y.shape[0]:
                raise ValueError(f"metric: {pred.shape[0]} predictions for {y.shape[0]} labels")
            rk = self._rank_setup(y.to(self.device), group, plan=False)
            score = pred.to(self.device).reshape(pred.shape[0], -1)[:, 0].float().contiguous()
            return {self._ndcg_name(): float(self._ndcg_sum(score, rk)) / rk["Q"] if rk["Q"] else 1.0}
        if obj.startswith("multi:"):
            pr = torch.softmax(pred, 1)
            ll = -torch.log(pr.gather(1, y.long()[:, None]).clamp_min(1e-15)).mean()
            return {"mlogloss": float(ll), "accuracy": float((pr.argmax(1) == y.long()).float().mean())}
        if obj == "binary:logistic":
            pr = torch.sigmoid(pred[:, 0])
            yy = y.float()
            ll = -(yy * torch.log(pr.clamp_min(1e-15)) + (1 - yy) * torch.log((1 - pr).clamp_min(1e-15))).mean()
            return {"logloss": float(ll), "accuracy": float(((pr > 0.5).float() == yy).float().mean())}
        if obj in QUANTILE_OBJECTIVES:
            name = "mae" if obj == "reg:absoluteerror" else "quantile"
            return {name: float(self._loss_sum(pred.reshape(pred.shape[0], -1), y)) / max(pred.shape[0], 1)}
        return {"rmse": float(torch.sqrt(((pred[:, 0] - y.float()) ** 2).mean()))}
