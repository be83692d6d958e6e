"""The device-resident GBDT grower (csrc/gbdt_grower.cpp over csrc/gbdt.hip), level by level, against
exact references.

A tree is verified against the data it was grown from, not against another grower's tree: the walker
steps one tree through the public stepping API (``begin_tree`` / ``level_a`` / ``level_b`` / ``level_c``,
the calls ``HistGBDT._grow_device`` makes for several ranks) and after every call reads the grower's own
tensors through ``debug_state``.  For each node it takes the rows the device says it owns, recomputes the
node's histogram in int64 / fp64, checks that the device's decision is optimal within a derived rounding
margin, and then *follows the device's decision*.  A near-tie therefore costs nothing, while every
structural quantity -- row order, segments, counts, node ids, built / subtracted histograms, leaf adds --
is compared exactly.

* Tier 1 -- exact data: g integer in -4..4, h in {1, 2}, lambda = 1.  The rows per chunk are a power of
  two, so both fixed-point scales 2^30 / (rpb * max) are powers of two: every quantised value, block sum
  and flushed term is an exact integer, and every fp32 atomic add, prefix scan and subtraction is exact in
  any order while 4 N < 2^24 (asserted on the inputs).  Histograms and totals are compared with the int64
  reference at ``atol = 0``.  Decisions: fp64 gains of all (f, b < B - 1) candidates from the exact
  histogram; the device's candidate must reach ``max - m`` with ``m = 2^-20 (t1 + t2 + t3)`` (the three
  gain terms; at most six fp32 roundings of relative size 2^-24, > 2x slack), evaluated at the device's
  candidate and at the best one (each side's fp32 gain is off by less than m / 2, so the larger m covers
  the sum).  Feature 5 is a copy of feature 2 and feature 2 uses even bins only, so exact ties exist at
  every node: among the candidates with the device choice's integer (GL, HL, GR, HR) the device must have
  picked the lowest feature, then the lowest bin.
* Tier 2 -- realistic data (logistic g / h after a few rounds; tiny and skewed hessians).  The same
  walker; histograms per bin against fp64 sums within ``0.5 step count + 1e-6 |ref| + 1e-9`` (step = rpb *
  max / 2^30) for the root and built children and ``bound(parent) + bound(built) + 2^-24 |value|`` for the
  subtracted siblings; decisions on fp64 gains of the device's own ``hist_cur`` with the margin widened
  by the fp32 prefix scan's worst case (``eG = B 2^-24 sum_b |g_b|``).  All structural checks stay exact.
  The worst ``error / bound`` ratio per stage is printed (``pytest -rA``).  A second grower's
  ``grow_local`` is compared bit for bit in Tier 1 only: the order of the fp32 flush atomics is free, so
  with inexact data two runs may round a histogram differently.
* CPU self-checks (no ``gpu`` marker): the reference side accepts every decision of the torch grower
  ``HistGBDT(..., "cpu")._grow`` on the Tier 1 inputs (its fp32 histograms are exact there), the int64
  histogram builder equals a plain fp64 ``index_add_``, and the exactness conditions hold for every
  parametrized Tier 1 case.
"""
import contextlib
import functools
import math
from typing import NamedTuple

import pytest
import torch

from kubedl_amd.models.gbdt import GBDTParams, HistGBDT

gpu = pytest.mark.gpu
CAP = 2 ** 24
U32 = 2.0 ** -24
INF = float("inf")


def _ext():
    from kubedl_amd.ops import _ext
    return _ext.load()


@contextlib.contextmanager
def _dispatch(plan=-1, scan=-1, rows=-2, pack=-1):
    """The grower's dispatch knobs for one walk, back at their defaults afterwards."""
    ext = _ext()
    try:
        ext.GbdtGrower.set_route_plan(plan)
        ext.GbdtGrower.set_route_scan(scan)
        ext.set_gbdt_hist_rows(rows)
        ext.set_gbdt_pack64(pack)
        yield ext
    finally:
        ext.GbdtGrower.set_route_plan(-1)
        ext.GbdtGrower.set_route_scan(-1)
        ext.set_gbdt_hist_rows(-2)
        ext.set_gbdt_pack64(-1)


def _f32(x):
    """The grower keeps lambda / gamma / lr / min_child_weight as fp32."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _rpb(N):
    """GbdtGrower's rows per histogram chunk: the smallest power of two giving <= 512 root chunks, 256..4096."""
    r = 256
    while r < 4096 and r * 512 < N:
        r *= 2
    return r


# ---------------------------------------------------------------- cases and data
class Case(NamedTuple):
    N: int
    F: int
    B: int
    D: int
    mcw: float = 1.0
    gamma: float = 0.0
    zero_g: bool = False
    ncut: int = 0  # columns of the cuts (0: B - 1); fewer make the upper split bins' thresholds inf


LAM, LR1 = 1.0, 0.5
TIER1 = {
    "base": Case(6037, 8, 32, 4),                    # 24 root chunks, six level tiles (ragged), N % 4 != 0
    "f28_b256": Case(6037, 28, 256, 4),              # the workload's feature count (fp = 32)
    "f7_b16": Case(6037, 7, 16, 4, ncut=8),          # F % 4 != 0: the slot kernel; thr = inf from bin 8 up
    "f100_b64": Case(6037, 100, 64, 4),              # two feature tiles
    "deep": Case(20011, 8, 32, 10),                  # 512 parents at the deepest level, most empty
    "root_only": Case(6037, 8, 32, 0),
    "tiny": Case(100, 8, 32, 4),                     # less than one chunk, less than one tile
    "zero_g": Case(6037, 8, 32, 4, zero_g=True),     # gh_max[0] = 0: no split, val = 0
    "leafy": Case(6037, 8, 32, 4, 40.0, 50.0),       # mid-depth leaves beside splitting siblings
}
# the first geometry across the dispatch settings: (route plan, route scan, hist rows, pack64)
DISPATCH = {
    "plan": (1, 0, 4, 1),
    "scan2": (0, 0, 4, 1),
    "fused": (0, 1, 4, 1),
    "slot": (1, 0, 0, 1),
    "rows8": (1, 0, 8, 1),
    "rows4_nopack": (1, 0, 4, 0),
    "rows8_nopack": (0, 0, 8, 0),
}


class Data(NamedTuple):
    bins: torch.Tensor   # uint8 [N, F]
    g: torch.Tensor      # fp32 [N]
    h: torch.Tensor      # fp32 [N]
    cuts: torch.Tensor   # fp32 [F, ncut]
    B: int


def _cuts(F, B):
    return (torch.arange(B - 1, dtype=torch.float32)[None, :] * 0.5
            + 0.125 * torch.arange(F, dtype=torch.float32)[:, None]).contiguous()


@functools.lru_cache(maxsize=None)
def _tier1(name):
    """Exact inputs: integer g in -4..4 (one |g| = 4 at least), h in {1, 2} (one 2 at least).  Feature 2
    carries the strongest signal and uses even bins only (every candidate ties with the empty bin above
    it), feature 5 copies it (every candidate on 2 ties with one on 5), feature 0 uses every fourth bin,
    and feature 3 is constant among the rows at or below the planted root split."""
    c = TIER1[name]
    N, F, B = c.N, c.F, c.B
    gen = torch.Generator().manual_seed(1000 * F + B + N)
    bins = torch.randint(0, B, (N, F), generator=gen, dtype=torch.uint8)
    bins[:, 2] = (bins[:, 2] // 2) * 2
    bins[:, 0] = (bins[:, 0] // 4) * 4
    t0 = (B // 2) // 2 * 2
    low = bins[:, 2] <= t0
    bins[low, 3] = 1
    bins[:, 5] = bins[:, 2]
    s2 = torch.where(bins[:, 2] > t0, 1, -1)
    s0 = torch.where(bins[:, 0] > B // 3, 1, -1)
    s1 = torch.where(bins[:, 1] > (2 * B) // 3, 1, -1)
    s4 = torch.where(bins[:, 4] > B // 2, 1, -1)
    noise = torch.randint(-1, 2, (N,), generator=gen)
    # feature 0 matters above the root split only, feature 4 in one grandchild only: with gamma > 0
    # leaves appear beside splitting siblings
    g = (2 * s2 + s0 * (s2 > 0) + s1 + s4 * ((s2 < 0) & (s1 > 0)) + noise).clamp(-4, 4)
    g[0], g[1] = 4, -4
    if c.zero_g:
        g = torch.zeros_like(g)
    h = torch.randint(1, 3, (N,), generator=gen)
    h[0], h[1] = 2, 1
    cuts = _cuts(F, B)[:, :c.ncut or B - 1].contiguous()
    return Data(bins.contiguous(), g.float().contiguous(), h.float().contiguous(), cuts, B)


def _exactness_conditions(name):
    """The inputs' side of the Tier 1 argument (a condition, not a tolerance)."""
    c, d = TIER1[name], _tier1(name)
    assert 4 * c.N < CAP, name
    assert bool((d.g == d.g.round()).all()) and float(d.g.abs().max()) <= 4
    assert set(d.h.tolist()) <= {1.0, 2.0} and float(d.h.max()) == 2.0
    if not c.zero_g:
        assert float(d.g.abs().max()) == 4.0
    rpb = _rpb(c.N)
    for mx in (float(d.g.abs().max()), float(d.h.max())):
        if mx == 0.0:
            continue  # scale 0: every quantised value is 0
        scale = 2.0 ** 30 / (rpb * mx)
        assert math.frexp(scale)[0] == 0.5, (name, scale)  # a power of two
        assert scale * 1.0 == int(scale) and rpb * mx * scale <= 2 ** 30
    return rpb


# ---------------------------------------------------------------- references
def _level_hist(bins_l, wg, wh, rows, pos, h0, L, B, count=False):
    """[L, F, B, 2] sums of (wg, wh) (int64 or fp64, row-indexed) over the rows that ``pos`` places in
    the level's nodes h0 .. h0 + L; with ``count`` also the rows per bin [L, F, B] (fp64)."""
    F = bins_l.shape[1]
    i = pos - h0
    m = (i >= 0) & (i < L)
    r, i = rows[m], i[m]
    idx = ((i[:, None] * F + torch.arange(F)[None, :]) * B + bins_l[r]).reshape(-1)
    out = torch.zeros(2, L * F * B, dtype=wg.dtype)
    out[0].index_add_(0, idx, wg[r].repeat_interleave(F))
    out[1].index_add_(0, idx, wh[r].repeat_interleave(F))
    hist = out.t().reshape(L, F, B, 2).contiguous()
    if not count:
        return hist
    cnt = torch.zeros(L * F * B, dtype=torch.float64)
    cnt.index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    return hist, cnt.view(L, F, B)


def _ref_partition(bins_l, rows, pos, lo, hi, split, feat, tbin, h0):
    """The plain rule: in each split node's segment the rows with ``bin[row, f] <= b`` first, then the
    others, both in their old order; everything else stays where it is."""
    L = split.numel()
    nr, npos = rows.clone(), pos.clone()
    lon, hin = torch.zeros(2 * L, dtype=torch.long), torch.zeros(2 * L, dtype=torch.long)
    for i in split.nonzero().flatten().tolist():
        a, z = int(lo[i]), int(hi[i])
        if z <= a:
            continue
        seg = rows[a:z]
        left = bins_l[seg, int(feat[h0 + i])] <= int(tbin[h0 + i])
        nl = int(left.sum())
        nr[a:z] = torch.cat([seg[left], seg[~left]])
        npos[a:a + nl] = 2 * (h0 + i) + 1
        npos[a + nl:z] = 2 * (h0 + i) + 2
        lon[2 * i], hin[2 * i], lon[2 * i + 1], hin[2 * i + 1] = a, a + nl, a + nl, z
    return nr, npos, lon, hin


def _ref_leaf(bins_l, feat, tbin, D):
    """Heap id of every row's leaf by walking the tree arrays from the root."""
    node = torch.zeros(bins_l.shape[0], dtype=torch.long)
    rid = torch.arange(bins_l.shape[0])
    for _ in range(D):
        f = feat[node].long()
        nxt = 2 * node + 1 + (bins_l[rid, f.clamp_min(0)] > tbin[node].long()).long()
        node = torch.where(f >= 0, nxt, node)
    return node


def _first_diff(a, b):
    ne = (a != b).flatten().nonzero()
    return int(ne[0]) if ne.numel() else -1


def _same(got, exp, what, owner=None):
    """``torch.equal`` with the first differing position (and the heap node owning it) in the message."""
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)} != {tuple(exp.shape)}"
    if torch.equal(got, exp):
        return
    p = _first_diff(got, exp)
    node = "" if owner is None else f" (heap node {int(owner.flatten()[p])})"
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(p), got.shape))
    raise AssertionError(f"{what}: first difference at {idx}{node}: got {got.flatten()[p].item()}, "
                         f"expected {exp.flatten()[p].item()}")


def _bits(t):
    return t.contiguous().view(torch.int32)


class Ctx:
    """What one walk needs everywhere: the case, its parameters and the running statistics."""

    def __init__(self, name, tier, N, F, B, D, lam, gamma, lr, mcw, cuts):
        self.name, self.tier, self.N, self.F, self.B, self.D = name, tier, N, F, B, D
        self.lam, self.gamma, self.lr, self.mcw = _f32(lam), _f32(gamma), _f32(lr), _f32(mcw)
        self.cuts = cuts
        self.stats = {"split": 0, "tie_nodes": 0, "const_feature_nodes": 0, "leaf_beside_split": 0, "empty": 0,
                      "inf_thr": 0}
        self.ratio = {}

    def worst(self, stage, err, bound):
        r = float((err / bound).max()) if err.numel() else 0.0
        self.ratio[stage] = max(self.ratio.get(stage, 0.0), r)
        return r


def _need(ctx, d, ok, what):
    """``ok`` [L] bool: fail at the first node of level d where it does not hold."""
    if bool(ok.all()):
        return
    i = int((~ok).nonzero()[0])
    raise AssertionError(f"{ctx.name}: level {d}, heap node {(1 << d) - 1 + i}: {what(i) if callable(what) else what}")


def _check_decisions(ctx, d, hist, exists, split, feat, tbin, thr, val, tot, exists_next, val_nodes=None):
    """split_find + decide of level d.  ``hist`` [L, F, B, 2]: the exact int64 histogram (Tier 1) or the
    device's own ``hist_cur`` as fp64 (Tier 2).  ``feat`` / ``tbin`` / ``thr`` / ``val`` are the heap
    arrays, ``split`` / ``tot`` / ``exists`` the level's.  ``val_nodes`` [L] bool limits the leaf-weight
    check (the torch grower stores a value for leaves only)."""
    L, F, B = hist.shape[:3]
    h0, nc, can_split = L - 1, B - 1, d < ctx.D
    lam, gamma, mcw = ctx.lam, ctx.gamma, ctx.mcw
    ex, sp = exists.bool(), split.bool()
    f, b = feat[h0:h0 + L].long(), tbin[h0:h0 + L].long()
    c = hist.cumsum(2)
    GLi, HLi, Gti, Hti = c[:, :, :-1, 0], c[:, :, :-1, 1], c[:, :, -1:, 0], c[:, :, -1:, 1]
    GRi, HRi = Gti - GLi, Hti - HLi
    GL, HL, GR, HR, Gt, Ht = (t.double() for t in (GLi, HLi, GRi, HRi, Gti, Hti))
    t1, t2, t3 = GL * GL / (HL + lam), GR * GR / (HR + lam), (Gt * Gt / (Ht + lam)).expand(L, F, nc)
    gain = t1 + t2 - t3
    m = 2.0 ** -20 * (t1 + t2 + t3)
    valid = (HL >= mcw) & (HR >= mcw)
    if ctx.tier == 1:
        border = torch.zeros_like(valid)
        eG = eH = None
    else:
        ab = hist.abs().sum(2)  # [L, F, 2]
        eG, eH = B * U32 * ab[..., 0:1], B * U32 * ab[..., 1:2]  # the fp32 prefix scan's worst case

        def T(G, H):
            return 2 * G.abs() * eG / (H + lam) + G * G * eH / (H + lam) ** 2
        m = m + 2 * (T(GL, HL) + T(GR, HR) + T(Gt, Ht))
        border = ((HL - mcw).abs() <= eH) | ((HR - mcw).abs() <= eH)
    strict, allowed = valid & ~border, valid | border
    gflat, mflat = gain.reshape(L, -1), m.reshape(L, -1)
    mx, am = gflat.masked_fill(~strict.reshape(L, -1), -INF).max(1)
    m_star = torch.where(torch.isfinite(mx), mflat.gather(1, am[:, None])[:, 0], torch.zeros_like(mx))

    # structure of the decision
    _need(ctx, d, ~sp | ex, "a node that does not exist was split")
    _need(ctx, d, ~sp | torch.tensor(can_split), "a node of the last level was split")
    _need(ctx, d, ~sp | ((f >= 0) & (f < F) & (b >= 0) & (b < nc)), lambda i: f"split on (f, b) = ({f[i]}, {b[i]})")
    _need(ctx, d, sp | ((f == -1) & (b == -1) & (_bits(thr[h0:h0 + L]) == 0)),
          lambda i: f"a leaf with feat {f[i]}, tbin {b[i]}, thr {thr[h0 + i]}")
    _need(ctx, d, ex | (_bits(val[h0:h0 + L]) == 0), lambda i: f"a non-existing node with val {val[h0 + i]}")
    if exists_next is not None:
        _same(exists_next, split.repeat_interleave(2), f"{ctx.name}: level {d}: exists[{d + 1}] vs split")
    ncut = ctx.cuts.shape[1]
    fc, bc = f.clamp_min(0), b.clamp_min(0)
    thr_ref = torch.where(bc < ncut, ctx.cuts[fc, bc.clamp_max(ncut - 1)], torch.full((L,), INF))
    _need(ctx, d, ~sp | (_bits(thr[h0:h0 + L]) == _bits(thr_ref)),
          lambda i: f"thr {thr[h0 + i]} is not cuts[{f[i]}][{b[i]}] = {thr_ref[i]}")

    # optimality of the chosen candidate, and split / no split against gamma
    flat = (fc * nc + bc)[:, None]
    g_dev, m_dev = gflat.gather(1, flat)[:, 0], mflat.gather(1, flat)[:, 0]
    tol = torch.maximum(m_dev, m_star)
    _need(ctx, d, ~sp | allowed.reshape(L, -1).gather(1, flat)[:, 0],
          lambda i: f"({f[i]}, {b[i]}) leaves a child below min_child_weight")
    _need(ctx, d, ~sp | (g_dev >= mx - tol),
          lambda i: f"({f[i]}, {b[i]}) has gain {g_dev[i]:.9g}, the best candidate "
                    f"({am[i] // nc}, {am[i] % nc}) {mx[i]:.9g}, margin {tol[i]:.3g}")
    _need(ctx, d, ~sp | (g_dev >= gamma - m_dev),
          lambda i: f"split with gain {g_dev[i]:.9g} <= gamma {gamma} (margin {m_dev[i]:.3g})")
    _need(ctx, d, sp | ~ex | torch.tensor(not can_split) | (mx <= gamma + m_star),
          lambda i: f"not split although ({am[i] // nc}, {am[i] % nc}) has gain {mx[i]:.9g} > gamma {gamma} "
                    f"(margin {m_star[i]:.3g})")
    if bool(sp.any()):
        ctx.worst("decision", (mx - g_dev)[sp].clamp_min(0), tol[sp].clamp_min(1e-300))

    # totals and leaf weights
    if ctx.tier == 1:
        tot_ref = torch.stack([Gti[:, 0, 0], Hti[:, 0, 0]], 1)
        _same(tot.double(), tot_ref.double(), f"{ctx.name}: level {d}: tot [node, (G, H)]")
        Gn, Hn = tot_ref[:, 0].double(), tot_ref[:, 1].double()
        # the tie rule: lowest feature, then lowest bin, among candidates with the same integer sums
        key = lambda t: t.reshape(L, -1)
        same = key(strict)
        for t in (GLi, HLi, GRi, HRi):
            same = same & (key(t) == key(t).gather(1, flat))
        first = same.int().argmax(1)
        _need(ctx, d, ~sp | (first == flat[:, 0]),
              lambda i: f"tie rule: chose ({f[i]}, {b[i]}) although ({first[i] // nc}, {first[i] % nc}) has the "
                        f"same (GL, HL, GR, HR)")
        ctx.stats["tie_nodes"] += int(((same.sum(1) > 1) & sp).sum())
        one_bin = ((hist[..., 1] != 0).sum(2) == 1).any(1)
        ctx.stats["const_feature_nodes"] += int((one_bin & ex).sum())
    else:
        dev_sum = torch.stack([Gt[:, 0, 0], Ht[:, 0, 0]], 1)
        err = (tot.double() - dev_sum).abs()
        bound = torch.stack([eG[:, 0, 0], eH[:, 0, 0]], 1) + 1e-300
        r = ctx.worst("tot", err, bound)
        assert r <= 1.0, f"{ctx.name}: level {d}: tot off by {r:.3g} x the scan bound"
        Gn, Hn = tot[:, 0].double(), tot[:, 1].double()
    val_ref = -Gn / (Hn + lam) * ctx.lr
    ulp = torch.where(val_ref == 0, torch.zeros_like(val_ref), torch.ldexp(torch.ones_like(val_ref),
                                                                            torch.frexp(val_ref)[1] - 24))
    vmask = ex if val_nodes is None else (ex & val_nodes)
    verr = (val[h0:h0 + L].double() - val_ref).abs()
    _need(ctx, d, ~vmask | (verr <= 4 * ulp),
          lambda i: f"val {val[h0 + i]} vs -G / (H + lambda) lr = {val_ref[i]:.9g} ({verr[i] / ulp[i]:.2f} ulp)")
    if bool((vmask & (ulp > 0)).any()):
        k = vmask & (ulp > 0)
        ctx.worst("val_ulp/4", verr[k], 4 * ulp[k])
    ctx.stats["split"] += int(sp.sum())
    ctx.stats["inf_thr"] += int((sp & torch.isinf(thr_ref)).sum())
    if 0 < d < ctx.D:
        pair_ex = ex.view(-1, 2).all(1)
        ctx.stats["leaf_beside_split"] += int((pair_ex & (sp.view(-1, 2).sum(1) == 1)).sum())


# ---------------------------------------------------------------- the walker (GPU)
def _cpu(t):
    return t.detach().cpu().clone()


def _hist_bound(ref, cnt, step):
    """The quantised build's bound per bin: half a step per row plus the flush's fp32 roundings."""
    return 0.5 * cnt[..., None] * step + 1e-6 * ref.abs() + 1e-9


def _walk(name, tier, data, D, mcw, gamma, lr, pick_in_a, lam=LAM):
    """Grow one tree step by step and check every stage; returns the Ctx (statistics, ratios)."""
    ext = _ext()
    N, F = data.bins.shape
    B = data.B
    ctx = Ctx(name, tier, N, F, B, D, lam, gamma, lr, mcw, data.cuts)
    bins_l = data.bins.long()
    bins_d, g_d, h_d = data.bins.cuda(), data.g.cuda(), data.h.cuda()
    gr = ext.GbdtGrower(bins_d, data.cuts.cuda(), B, D, lam, gamma, lr, mcw)
    rpb = gr.rows_per_chunk()
    if tier == 1:
        assert 4 * N < CAP and rpb == _rpb(N) and rpb & (rpb - 1) == 0
        wg, wh = data.g.long(), data.h.long()
    else:
        wg, wh = data.g.double(), data.h.double()
    step = torch.tensor([rpb * float(data.g.abs().max()) / 2 ** 30, rpb * float(data.h.max()) / 2 ** 30],
                        dtype=torch.float64)
    heap = (1 << (D + 1)) - 1

    # a tree grown before (other gradients): begin_tree has state to reset
    gr.grow_local(g_d.flip(0).contiguous(), h_d.flip(0).contiguous())
    root_view = gr.begin_tree(g_d, h_d)
    st = gr.debug_state(0)
    rows, pos = _cpu(st["rows"]).long(), _cpu(st["node_pos"]).long()
    _same(rows, torch.arange(N), f"{name}: begin_tree: rows")
    _same(pos, torch.zeros(N, dtype=torch.long), f"{name}: begin_tree: node_pos")
    lo, hi = _cpu(st["lo"]).long(), _cpu(st["hi"]).long()
    assert lo.tolist() == [0] and hi.tolist() == [N] and _cpu(st["exists"]).tolist() == [1], (lo, hi)
    feat, tbin, thr, val = (_cpu(t) for t in gr.tree())
    assert feat.numel() == heap
    _same(feat, torch.full((heap,), -1, dtype=torch.int32), f"{name}: begin_tree: feat")
    _same(tbin, torch.full((heap,), -1, dtype=torch.int32), f"{name}: begin_tree: tbin")
    _same(_bits(thr), torch.zeros(heap, dtype=torch.int32), f"{name}: begin_tree: thr bits")
    _same(_bits(val), torch.zeros(heap, dtype=torch.int32), f"{name}: begin_tree: val bits")
    _same(_bits(_cpu(st["gh_max"])), _bits(torch.stack([data.g.abs().max(), data.h.max()])),
          f"{name}: begin_tree: gh_max bits")
    _same(_cpu(st["built"]), torch.zeros_like(_cpu(st["built"])), f"{name}: begin_tree: built_")
    hist_dev = _cpu(st["hist_cur"])[:1]
    _same(_cpu(root_view), hist_dev, f"{name}: begin_tree: returned root vs hist_cur[0]")
    if tier == 1:
        href = _level_hist(bins_l, wg, wh, rows, pos, 0, 1, B)
        _same(hist_dev.double(), href.double(), f"{name}: root histogram [node, f, b, (g, h)]")
        bound = None
    else:
        href, cnt = _level_hist(bins_l, wg, wh, rows, pos, 0, 1, B, count=True)
        bound = _hist_bound(href, cnt, step)
        r = ctx.worst("hist_root", (hist_dev.double() - href).abs(), bound)
        assert r <= 1.0, f"{name}: root histogram off by {r:.3g} x its bound"

    for d in range(D + 1):
        L, h0, last = 1 << d, (1 << d) - 1, d == D
        gr.level_a(d, pick_in_a)
        st = gr.debug_state(d)
        feat, tbin, thr, val = (_cpu(t) for t in gr.tree())
        split, tot, exists = _cpu(st["split"])[:L], _cpu(st["tot"])[:L], _cpu(st["exists"])
        exists_next = None if last else _cpu(gr.debug_state(d + 1)["exists"])
        _check_decisions(ctx, d, href if tier == 1 else hist_dev.double(), exists, split, feat, tbin, thr, val, tot,
                         exists_next)
        rows_d, pos_d = _cpu(st["rows"]).long(), _cpu(st["node_pos"]).long()
        if last:
            _same(rows_d, rows, f"{name}: level {d} (last): rows moved", pos)
            _same(pos_d, pos, f"{name}: level {d} (last): node_pos changed", pos)
            break
        # partition: the stable split of every split node's segment, nothing else moves
        nrows, npos, lon, hin = _ref_partition(bins_l, rows, pos, lo, hi, split, feat, tbin, h0)
        _same(rows_d, nrows, f"{name}: level {d}: rows after the partition [position]", pos)
        _same(pos_d, npos, f"{name}: level {d}: node_pos after the partition [position]", pos)
        stn = gr.debug_state(d + 1)
        _same(_cpu(stn["lo"]).long(), lon, f"{name}: level {d}: lo[{d + 1}] [child]")
        _same(_cpu(stn["hi"]).long(), hin, f"{name}: level {d}: hi[{d + 1}] [child]")
        _same(_cpu(st["cnt"])[:2 * L].double(), (hin - lon).double(), f"{name}: level {d}: cnt [child]")
        ctx.stats["empty"] += int(((hin - lon) == 0).sum())
        size = (hin - lon).view(L, 2)
        bc_ref = 2 * torch.arange(L) + (size[:, 0] > size[:, 1]).long()  # the smaller child, ties -> left
        blo_ref, bhi_ref = lon[bc_ref], hin[bc_ref]

        def check_pick(when):
            s = gr.debug_state(d)
            _same(_cpu(s["build_child"])[:L].long(), bc_ref, f"{name}: level {d}: build_child {when} [parent]")
            _same(_cpu(s["blo"])[:L].long(), blo_ref, f"{name}: level {d}: blo {when} [parent]")
            _same(_cpu(s["bhi"])[:L].long(), bhi_ref, f"{name}: level {d}: bhi {when} [parent]")
        if pick_in_a:
            check_pick("after level_a(pick)")
        rows, pos, lo, hi = nrows, npos, lon, hin

        # the smaller children's histograms
        parent_c = hist_dev
        built_c = _cpu(gr.level_b(d, not pick_in_a))
        check_pick("after level_b")
        assert built_c.shape == (L, F, B, 2)
        whole = _cpu(gr.debug_state(d)["built"])
        _same(whole[:L], built_c, f"{name}: level {d}: level_b's result is not a view of built_")
        _same(whole[L:], torch.zeros_like(whole[L:]), f"{name}: level {d}: built_ past the level's parents")
        sp4 = split.bool()[:, None, None, None]
        if tier == 1:
            hnext = _level_hist(bins_l, wg, wh, rows, pos, 2 * L - 1, 2 * L, B)
            _same(built_c.double(), (hnext[bc_ref] * sp4).double(),
                  f"{name}: level {d}: built [parent, f, b, (g, h)]", h0 + torch.arange(L)[:, None, None, None]
                  .expand(L, F, B, 2))
        else:
            hnext, cnt = _level_hist(bins_l, wg, wh, rows, pos, 2 * L - 1, 2 * L, B, count=True)
            base = _hist_bound(hnext, cnt, step)
            _same(built_c * ~sp4, torch.zeros_like(built_c), f"{name}: level {d}: built under non-split parents")
            r = ctx.worst("hist_built", (built_c.double() - hnext[bc_ref] * sp4).abs(), base[bc_ref])
            assert r <= 1.0, f"{name}: level {d}: built histogram off by {r:.3g} x its bound"

        # children's histograms: built one copied, sibling = parent - built, zero below a leaf
        gr.level_c(d)
        st = gr.debug_state(d + 1)
        nxt = _cpu(st["hist_cur"])[:2 * L]
        own = (2 * L - 1 + torch.arange(2 * L))[:, None, None, None].expand(2 * L, F, B, 2)
        exp = torch.zeros_like(nxt)
        exp[bc_ref] = built_c
        exp[bc_ref ^ 1] = (parent_c - built_c) * sp4
        exp = exp * sp4.repeat_interleave(2, 0)
        _same(_bits(nxt + 0.0), _bits(exp + 0.0), f"{name}: level {d}: hist_cur after level_c [child, f, b, (g, h)] "
              "vs built / parent - built in fp32", own)
        whole = _cpu(st["built"])
        _same(whole, torch.zeros_like(whole), f"{name}: level {d}: built_ after level_c")
        if tier == 1:
            _same(nxt.double(), hnext.double(), f"{name}: level {d}: hist_cur after level_c vs the int64 histogram", own)
        else:
            nb = torch.zeros_like(base)
            nb[bc_ref] = base[bc_ref]
            nb[bc_ref ^ 1] = bound + base[bc_ref] + U32 * nxt[bc_ref ^ 1].double().abs()
            live = sp4.repeat_interleave(2, 0).expand_as(nb)
            err = (nxt.double() - hnext).abs()
            sib = torch.zeros(2 * L, dtype=torch.bool)
            sib[bc_ref ^ 1] = True
            sib = sib[:, None, None, None].expand_as(nb) & live
            if bool(sib.any()):
                r = ctx.worst("hist_sibling", err[sib], nb[sib])
                assert r <= 1.0, f"{name}: level {d}: subtracted histogram off by {r:.3g} x its bound"
            bound = torch.where(live, nb, torch.full_like(nb, 1e-9))
        hist_dev, href = nxt, hnext

    # leaves
    leaf = _ref_leaf(bins_l, feat, tbin, D)
    own = torch.empty(N, dtype=torch.long)
    own[rows] = pos
    _same(own, leaf, f"{name}: the walker's row -> node map vs walking the tree arrays [row]")
    K, k = 3, 1
    pred0 = torch.randn(N, K, generator=torch.Generator().manual_seed(N))
    pred = pred0.clone().cuda()
    gr.add_leaf(pred, k)
    _same(_cpu(gr.node_of_row()).long(), leaf, f"{name}: node_of_row [row]")
    exp = pred0.clone()
    exp[:, k] = pred0[:, k] + val[leaf]
    _same(_cpu(pred), exp, f"{name}: pred after add_leaf [row, column]")
    tree = [_cpu(t) for t in gr.tree()]
    _same(_cpu(gr.heap_packed()), torch.stack([tree[0].float(), tree[1].float(), tree[2], tree[3]]),
          f"{name}: heap_packed vs tree()")
    if tier == 1:
        g2 = ext.GbdtGrower(bins_d, data.cuts.cuda(), B, D, lam, gamma, lr, mcw)
        g2.grow_local(g_d, h_d)
        for a, b_, what in zip(g2.tree(), tree, ("feat", "tbin", "thr", "val")):
            _same(_bits(_cpu(a)) if a.dtype == torch.float32 else _cpu(a),
                  _bits(b_) if b_.dtype == torch.float32 else b_, f"{name}: grow_local's {what}")
        s2 = g2.debug_state(D)
        _same(_cpu(s2["rows"]).long(), rows, f"{name}: grow_local's rows")
        _same(_cpu(s2["node_pos"]).long(), pos, f"{name}: grow_local's node_pos")
    torch.cuda.synchronize()
    return ctx


def _report(ctx):
    print(f"[{ctx.name}] splits {ctx.stats['split']}, worst error / bound: "
          + ", ".join(f"{k} {v:.3g}" for k, v in sorted(ctx.ratio.items())))


# ---------------------------------------------------------------- Tier 1 (GPU)
@gpu
@pytest.mark.parametrize("pick_in_a", [True, False], ids=["pick_a", "pick_b"])
@pytest.mark.parametrize("knobs", sorted(DISPATCH))
def test_gpu_grower_exact_walk_dispatch(knobs, pick_in_a):
    """The first geometry under every dispatch setting, with the smaller child picked by ``level_a`` or by
    ``level_b`` (pick_small_kernel, the several-ranks sequence): the same reference, so the same result."""
    c, data = TIER1["base"], _tier1("base")
    plan, scan, rows, pack = DISPATCH[knobs]
    with _dispatch(plan, scan, rows, pack):
        ctx = _walk(f"base/{knobs}", 1, data, c.D, c.mcw, c.gamma, LR1, pick_in_a)
    _report(ctx)
    assert ctx.stats["split"] >= 8 and ctx.stats["tie_nodes"] >= 1 and ctx.stats["const_feature_nodes"] >= 1, ctx.stats


@gpu
@pytest.mark.parametrize("pick_in_a", [True, False], ids=["pick_a", "pick_b"])
@pytest.mark.parametrize("name", [n for n in TIER1 if n != "base"])
def test_gpu_grower_exact_walk(name, pick_in_a):
    c, data = TIER1[name], _tier1(name)
    with _dispatch():
        ctx = _walk(name, 1, data, c.D, c.mcw, c.gamma, LR1, pick_in_a)
    _report(ctx)
    s = ctx.stats
    if name in ("zero_g", "root_only"):
        assert s["split"] == 0, s
    elif name == "leafy":
        assert s["leaf_beside_split"] >= 1 and s["tie_nodes"] >= 1, s
    elif name == "deep":
        assert s["split"] >= 200 and s["empty"] >= 256 and s["tie_nodes"] >= 1, s
    else:
        assert s["split"] >= 3 and s["tie_nodes"] >= 1, s
    assert s["inf_thr"] >= (1 if c.ncut else 0), s


@gpu
def test_gpu_decide_keeps_nonexistent_nodes_unsplit():
    """decide_kernel's ``exists`` guard.  Below a leaf the histogram slots are zero, which alone keeps such a
    node unsplit whenever min_child_weight > 0 -- so the guard is invisible to a walk.  Here g == 0 keeps
    the root a leaf (gain 0 is not > gamma = 0), then a histogram with one very good split is written into
    the two level-1 slots through the ``debug_state`` view: the nodes do not exist, so they must stay
    unsplit with feat = -1 and val = +0.  The same histogram in the root's slot (which exists) does split."""
    c, data = TIER1["zero_g"], _tier1("zero_g")
    ext = _ext()
    B, F = c.B, c.F
    args = (data.bins.cuda(), data.cuts.cuda(), B, 2, LAM, 0.0, LR1, 1.0)
    good = torch.zeros(F, B, 2)
    good[0, 0] = torch.tensor([1000.0, 100.0])
    good[0, 1] = torch.tensor([-1000.0, 100.0])
    with _dispatch():
        gr = ext.GbdtGrower(*args)
        gr.begin_tree(data.g.cuda(), data.h.cuda())
        gr.level_a(0, True)
        gr.level_b(0, False)
        gr.level_c(0)
        st = gr.debug_state(1)
        assert _cpu(st["exists"]).tolist() == [0, 0]
        rows0, pos0 = _cpu(st["rows"]), _cpu(st["node_pos"])
        st["hist_cur"][:2] = good.cuda()
        gr.level_a(1, True)
        st = gr.debug_state(1)
        feat, tbin, thr, val = (_cpu(t) for t in gr.tree())
        assert feat.tolist() == [-1] * 7 and tbin.tolist() == [-1] * 7, (feat, tbin)
        assert _bits(thr)[1:].tolist() == [0] * 6 and _bits(val)[1:].tolist() == [0] * 6, (thr, val)
        assert _cpu(st["split"])[:2].tolist() == [0, 0]
        assert _cpu(gr.debug_state(2)["exists"]).tolist() == [0] * 4
        _same(_cpu(st["rows"]), rows0, "rows moved under non-existing nodes")
        _same(_cpu(st["node_pos"]), pos0, "node_pos changed under non-existing nodes")
        # the control: the root exists, and the same histogram splits it at (0, 0)
        gr = ext.GbdtGrower(*args)
        gr.begin_tree(data.g.cuda(), data.h.cuda())
        gr.debug_state(0)["hist_cur"][:1] = good.cuda()
        gr.level_a(0, True)
        feat, tbin, _, _ = (_cpu(t) for t in gr.tree())
        assert (int(feat[0]), int(tbin[0])) == (0, 0) and _cpu(gr.debug_state(0)["split"])[:1].tolist() == [1]
        torch.cuda.synchronize()


# ---------------------------------------------------------------- Tier 2 (GPU)
def _xy(N, F, seed):
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(N, F, generator=gen)
    y = ((X[:, 0] - X[:, 1] * X[:, 2] + 0.2 * torch.randn(N, generator=gen)) > 0).long()
    return X, y


def _tier2_logistic(N, F, B):
    """g / h of binary:logistic after a few rounds of the device grower (confident rows beside uncertain
    ones: hessians over several decades), on the model's own cuts and bins."""
    X, y = _xy(N, F, 11)
    m = HistGBDT(GBDTParams(objective="binary:logistic", n_estimators=12, max_depth=5, max_bin=B, learning_rate=1.0),
                 "cuda")
    m.fit_cuts(X.cuda())
    pred = m.fit(X, y)
    g, h = m._grad_hess(pred, y.cuda())
    bins = m.quantise(X.cuda())
    return Data(bins.cpu().contiguous(), g[:, 0].cpu().contiguous(), h[:, 0].cpu().contiguous(), m.cuts.cpu(), B)


def _tier2_skewed(N, F, B):
    """The inputs of test_gpu_quantised_hist_tiny_and_skewed_hessians: g ~ N(0, 1e-3) with 1 % at +-1, h
    in 1e-9 .. 1e-6 with 10 % at 0.25."""
    gen = torch.Generator().manual_seed(7)
    bins = torch.randint(0, B, (N, F), generator=gen, dtype=torch.uint8)
    g = torch.randn(N, generator=gen) * 1e-3
    hot = torch.rand(N, generator=gen) < 0.01
    g[hot] = torch.sign(torch.randn(int(hot.sum()), generator=gen))
    h = torch.exp(torch.empty(N).uniform_(-20.7, -13.8, generator=gen))
    big = torch.rand(N, generator=gen) < 0.1
    h[big] = 0.25
    return Data(bins, g.contiguous(), h.contiguous(), _cuts(F, B), B)


@gpu
@pytest.mark.parametrize("kind", ["logistic", "skewed"])
@pytest.mark.parametrize("F,B", [(8, 32), (28, 256)])
def test_gpu_grower_realistic_walk(F, B, kind):
    """Tier 2: the same walk on inexact data; prints the worst error / bound ratio per stage."""
    N, D = 6037, 4
    with _dispatch():
        data = (_tier2_logistic if kind == "logistic" else _tier2_skewed)(N, F, B)
        span = float(data.h.max() / data.h.min())
        ctx = _walk(f"{kind}/f{F}_b{B}", 2, data, D, 1.0, 0.0, 0.3, kind == "logistic")
    print(f"[{ctx.name}] hessian max / min {span:.3g}")
    _report(ctx)
    assert ctx.stats["split"] >= 3 and span > 1e3, (ctx.stats, span)


# ---------------------------------------------------------------- CPU self-checks
@pytest.mark.parametrize("name", sorted(TIER1))
def test_tier1_inputs_are_exact(name):
    """4 N < 2^24 and power-of-two fixed-point scales for every Tier 1 case."""
    rpb = _exactness_conditions(name)
    assert rpb == 256  # every case here is at most 512 chunks of 256 rows


def test_int64_histogram_equals_fp64_index_add():
    data = _tier1("f7_b16")
    N, F = data.bins.shape
    B = 16
    gen = torch.Generator().manual_seed(3)
    rows = torch.randperm(N, generator=gen)
    pos = torch.randint(2, 9, (N,), generator=gen)  # heap nodes 2 .. 8: level 2 is 3 .. 6
    got, cnt = _level_hist(data.bins.long(), data.g.long(), data.h.long(), rows, pos, 3, 4, B), None
    ref = torch.zeros(4, F, B, 2, dtype=torch.float64)
    for i in range(4):
        r = rows[pos == 3 + i]
        for f in range(F):
            ref[i, f, :, 0].index_add_(0, data.bins[r, f].long(), data.g[r].double())
            ref[i, f, :, 1].index_add_(0, data.bins[r, f].long(), data.h[r].double())
    assert torch.equal(got.double(), ref)
    got64, cnt = _level_hist(data.bins.long(), data.g.double(), data.h.double(), rows, pos, 3, 4, B, count=True)
    assert torch.equal(got64, ref)
    assert float(cnt[:, 0].sum()) == float(((pos >= 3) & (pos < 7)).sum())
    assert torch.equal(cnt.sum(2), cnt.sum(2)[:, :1].expand(4, F))


@pytest.mark.parametrize("name", ["base", "leafy", "f7_b16", "tiny", "zero_g", "root_only"])
def test_reference_accepts_torch_grower_tree(name):
    """The walker's reference side on a tree of the torch grower: with exact integers its fp32 histograms
    are exact, so each of its decisions must pass the optimality check; the partition rule and the leaf
    walk must reproduce its row -> leaf map."""
    c, data = TIER1[name], _tier1(name)
    _exactness_conditions(name)
    N, F, B, D = c.N, c.F, c.B, c.D
    m = HistGBDT(GBDTParams(max_depth=D, max_bin=B, reg_lambda=LAM, gamma=c.gamma, min_child_weight=c.mcw,
                            learning_rate=LR1), "cpu")
    m.cuts = data.cuts
    tree, leaf_of_row = m._grow(data.bins, data.g, data.h, N)
    heap = (1 << (D + 1)) - 1
    feat = torch.full((heap,), -1, dtype=torch.int32)
    tbin = torch.full((heap,), -1, dtype=torch.int32)
    thr, val = torch.zeros(heap), torch.zeros(heap)
    exists = torch.zeros(heap, dtype=torch.int32)
    to_heap = {0: 0}
    order = [0]
    for nid in order:  # list id -> heap id, breadth first
        hid = to_heap[nid]
        exists[hid] = 1
        val[hid] = tree.value[nid]
        if tree.feature[nid] >= 0:
            feat[hid], tbin[hid], thr[hid] = tree.feature[nid], tree.split_bin[nid], tree.threshold[nid]
            to_heap[tree.left[nid]], to_heap[tree.right[nid]] = 2 * hid + 1, 2 * hid + 2
            order += [tree.left[nid], tree.right[nid]]
    ctx = Ctx(f"cpu/{name}", 1, N, F, B, D, LAM, c.gamma, LR1, c.mcw, data.cuts)
    bins_l = data.bins.long()
    rows, pos = torch.arange(N), torch.zeros(N, dtype=torch.long)
    lo, hi = torch.tensor([0]), torch.tensor([N])
    for d in range(D + 1):
        L, h0 = 1 << d, (1 << d) - 1
        hist = _level_hist(bins_l, data.g.long(), data.h.long(), rows, pos, h0, L, B)
        split = (feat[h0:h0 + L] >= 0).int()
        tot = torch.stack([hist[:, 0, :, 0].sum(1), hist[:, 0, :, 1].sum(1)], 1).float()
        nxt = None if d == D else exists[2 * L - 1:4 * L - 1]
        _check_decisions(ctx, d, hist, exists[h0:h0 + L], split, feat, tbin, thr, val, tot, nxt,
                         val_nodes=~split.bool())
        if d < D:
            rows, pos, lo, hi = _ref_partition(bins_l, rows, pos, lo, hi, split, feat, tbin, h0)
    own = torch.empty(N, dtype=torch.long)
    own[rows] = pos
    leaf = _ref_leaf(bins_l, feat, tbin, D)
    assert torch.equal(own, leaf)
    assert torch.equal(torch.tensor([to_heap[int(v)] for v in leaf_of_row.tolist()]), leaf)
    if name in ("base", "leafy", "f7_b16"):
        assert ctx.stats["split"] >= 3 and ctx.stats["tie_nodes"] >= 1 and ctx.stats["const_feature_nodes"] >= 1
    if name == "leafy":
        assert ctx.stats["leaf_beside_split"] >= 1, ctx.stats
    assert ctx.stats["inf_thr"] >= (1 if c.ncut else 0), ctx.stats


def test_reference_rejects_wrong_decisions():
    """The checks bite: a second-best candidate, the tie's upper bin, a moved row and a missed split fail."""
    c, data = TIER1["base"], _tier1("base")
    N, F, B = c.N, c.F, c.B
    ctx = Ctx("cpu/reject", 1, N, F, B, 1, LAM, 0.0, LR1, 1.0, data.cuts)
    bins_l = data.bins.long()
    rows, pos = torch.arange(N), torch.zeros(N, dtype=torch.long)
    hist = _level_hist(bins_l, data.g.long(), data.h.long(), rows, pos, 0, 1, B)
    tot = torch.stack([hist[:, 0, :, 0].sum(1), hist[:, 0, :, 1].sum(1)], 1).float()
    t0 = (B // 2) // 2 * 2
    Gn, Hn = float(tot[0, 0]), float(tot[0, 1])

    def run(f, b, split=1):
        feat = torch.tensor([f if split else -1, -1, -1], dtype=torch.int32)
        tbin = torch.tensor([b if split else -1, -1, -1], dtype=torch.int32)
        thr = torch.tensor([float(data.cuts[f, b]) if split else 0.0, 0.0, 0.0])
        val = torch.tensor([-Gn / (Hn + 1.0) * 0.5, 0.0, 0.0])
        _check_decisions(ctx, 0, hist, torch.tensor([1], dtype=torch.int32), torch.tensor([split], dtype=torch.int32),
                         feat, tbin, thr, val, tot, torch.tensor([split, split], dtype=torch.int32))
    run(2, t0)  # the planted split passes
    with pytest.raises(AssertionError, match="tie rule"):
        run(2, t0 + 1)
    with pytest.raises(AssertionError, match="tie rule"):
        run(5, t0)
    with pytest.raises(AssertionError, match="best candidate"):
        run(2, t0 + 2)
    with pytest.raises(AssertionError, match="not split although"):
        run(2, t0, split=0)
    nr, npos, lon, hin = _ref_partition(bins_l, rows, pos, torch.tensor([0]), torch.tensor([N]),
                                        torch.tensor([1]), torch.tensor([2]), torch.tensor([t0]), 0)
    assert torch.equal(nr[:int(hin[0])], rows[bins_l[:, 2] <= t0]) and torch.equal(nr[int(hin[0]):],
                                                                                  rows[bins_l[:, 2] > t0])
    bad = nr.clone()
    bad[[3, 4]] = bad[[4, 3]]
    with pytest.raises(AssertionError, match=r"first difference at \(3,\)"):
        _same(bad, nr, "rows")
