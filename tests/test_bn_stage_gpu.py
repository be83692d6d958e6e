"""Staged BatchNorm entry points (csrc/bn_act.hip, ``bn_stage_*``) against int64 / fp64 references.

The ResNet engine drives BatchNorm through these stages, and other GPU tests use them as *their*
reference, so each stage gets a ground truth of its own here:

* Tier 1 -- small-integer data.  fp32 sums of small integers are exact in any order, so every sum is
  compared with ``atol = 0`` against an int64 reference: a dropped or doubled row, a wrong replica,
  channel or mask bit changes the result.
* Tier 2 -- realistic data against hand-written fp64 references, with bounds derived from the number
  formats (half a bf16 ulp = 2^-8 relative, plus slack for the fp32 arithmetic).
* CPU self-checks (no ``gpu`` marker) -- the fp64 references agree with double-precision autograd
  through ``F.batch_norm``, and a plain fp32 emulation of the stages stays inside the Tier 2 bounds,
  so a correct implementation passes.

The bound tests print their worst ``error / bound`` ratio and excluded share (``pytest -rA`` shows them).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

REP = 32  # accumulator replicas (kReplicas)
MOM, EPS = 0.1, 1e-5
U_BF16 = 2.0 ** -8   # half a bf16 ulp, relative
U_F32 = 2.0 ** -20   # slack for a handful of fp32 roundings (each 2^-24), relative to the sum of magnitudes
U_SUM = 2.0 ** -16   # fp32 add chain shorter than 2^8 adds, each 2^-24, relative to sum(|terms|)
EXCL_CAP = 1e-3      # share of elements whose sign is decided inside the fp32 slack

# M, C: the smallest shapes that reach every branch of make_tiling / plan_reduce / apply_gx
SHAPES = [
    (1, 8),        # one row, one channel group, Mf == 1 guard of the unbiased variance
    (7, 24),       # TPR 3, RPI 85: thread 255 idle, M < RPI
    (197, 64),     # odd M, TPR 8, RPI 32
    (196, 64),     # multiple of 4 (exact broadcast case)
    (4231, 264),   # 33 channel groups: gy 2, one live lane in the second y-block; reduce gx 34 wraps the replicas
    (98, 2048),    # the real last stage (2 images of 7x7), gy 8
    (16411, 64),   # narrow C, reduce gx 33 wraps the replicas, 4-way unrolled stats loop
]
WRAP_SHAPES = [(4231, 264), (16411, 64)]
CHAIN_SHAPES = [(197, 64), (4231, 264)]
PDTYPES = [torch.float32, torch.bfloat16]


def _ext():
    from kubedl_amd.ops import _ext
    return _ext.load()


# ---------------------------------------------------------------- workspace layout
def _views(ws, C):
    """Views of one BN layer's fp32 workspace (``bn_workspace_floats(C)`` values, zero on first use):

        [32][2C]  forward accumulators   sum(x - K), sum((x - K)^2)    at 0
        [32][2C]  backward accumulators  sum(g), sum(g (x - mean))     at 32*2*C
        [2C]      forward coefficients   scale | shift                 at bn_coef_offset(C) = 32*4*C
        [3C]      backward coefficients  k | c1 | c0                   right after the forward ones

    Block b adds into replica row b % 32; the finalize kernels sum the 32 rows and re-zero them."""
    a = REP * 2 * C
    off = 2 * a
    return {"facc": ws[:a].view(REP, 2, C), "bacc": ws[a:2 * a].view(REP, 2, C),
            "fcoef": ws[off:off + 2 * C].view(2, C), "bcoef": ws[off + 2 * C:off + 5 * C].view(3, C)}


def _ws(C):
    return torch.zeros(_ext().bn_workspace_floats(C), device="cuda")


def _sums(acc):
    """Replica-summed accumulators as fp64 [2, C] on the CPU."""
    return acc.double().sum(0).cpu()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _plan(M, C):
    """TPR, RPI, gy and the reduce / apply grid widths for bf16 [M, C] (make_tiling, plan_reduce, apply_gx)."""
    CG = C // 8
    TPR = min(CG, 32)
    RPI = 256 // TPR
    gy = -(-CG // TPR)
    target = max(1024 // gy, 1)
    min_rows = max(RPI * 16, 128)
    gx = max(min(-(-M // min_rows), target), 1)
    rpb = -(-(-(-M // gx)) // RPI) * RPI
    gx = max(-(-M // rpb), 1)
    agx = max(min(-(-M // (2 * RPI)), max(2048 // gy, 1)), 1)
    return {"TPR": TPR, "RPI": RPI, "gy": gy, "gx": gx, "apply_gx": agx}


def _unpack(mb, C):
    """[M, C/8] mask bytes -> [M, C] 0/1: bit i of byte [r, c/8] stands for channel 8*(c/8)+i."""
    M = mb.shape[0]
    return ((mb.long().unsqueeze(-1) >> torch.arange(8)) & 1).reshape(M, C)


def _pack(bits):
    M, C = bits.shape
    return (bits.long().view(M, C // 8, 8) << torch.arange(8)).sum(-1).to(torch.uint8)


def _dev(t):  # integer / float CPU tensor -> bf16 on the GPU (a copy: the cached cases stay unchanged)
    return t.to(torch.bfloat16).cuda()


# ---------------------------------------------------------------- inputs (built once, never modified)
@functools.lru_cache(maxsize=None)
def _int_case(M, C):
    """Small integers (int64, CPU): x, x2 in 0..3 with x[0] = 0 (the stats kernel shifts by x[0, c]),
    dy in -2..2, integer means, random mask bytes.  Every sum stays far below 2^24."""
    g = torch.Generator().manual_seed(7919 * M + C)
    x = torch.randint(0, 4, (M, C), generator=g)
    x[0] = 0
    return {"x": x, "x2": torch.randint(0, 4, (M, C), generator=g),
            "dy": torch.randint(-2, 3, (M, C), generator=g),
            "res": torch.randint(-1, 2, (M, C), generator=g),
            "mean": torch.randint(0, 4, (C,), generator=g), "mean2": torch.randint(0, 4, (C,), generator=g),
            "mb": torch.randint(0, 256, (M, C // 8), generator=g, dtype=torch.uint8)}


@functools.lru_cache(maxsize=None)
def _float_case(M, C):
    """Realistic data as in test_ops_gpu.py (CPU; activations already rounded to bf16)."""
    g = torch.Generator().manual_seed(104729 * M + C)

    def act(scale, shift):
        return (torch.randn(M, C, generator=g) * scale + shift).bfloat16()

    d = {"x": act(2, 3), "xd": act(2, 3), "res": act(1, 0), "dy": act(1, 0),
         "mb": torch.randint(0, 256, (M, C // 8), generator=g, dtype=torch.uint8)}
    for s in ("", "d"):
        d["gamma" + s] = torch.rand(C, generator=g) + 0.5
        d["beta" + s] = torch.randn(C, generator=g)
        d["rm" + s] = torch.randn(C, generator=g)
        d["rv" + s] = torch.rand(C, generator=g) + 0.5
    return d


# ---------------------------------------------------------------- fp64 references, written by hand
def _ref_moments(x64):
    mean = x64.mean(0)
    return mean, ((x64 - mean) ** 2).mean(0)  # biased variance


def _ref_finalize(x64, gamma64, beta64, rm64, rv64):
    M = x64.shape[0]
    mean, var = _ref_moments(x64)
    # M == 1 has no unbiased estimate; the kernel's rule is unbiased = biased there
    unbiased = var * M / (M - 1) if M > 1 else var
    invstd = (var + EPS).rsqrt()
    sc = gamma64 * invstd
    return {"mean": mean, "var": var, "invstd": invstd, "rm": (1 - MOM) * rm64 + MOM * mean,
            "rv": (1 - MOM) * rv64 + MOM * unbiased, "sc": sc, "sf": beta64 - mean * sc}


def _ref_bn(x64, gamma64, beta64):
    """Training-mode BN forward in fp64, differentiable."""
    mean, var = _ref_moments(x64)
    return (x64 - mean) * (var + EPS).rsqrt() * gamma64 + beta64


def _close(got, ref, tol):
    torch.testing.assert_close(got.double().cpu(), ref, atol=tol, rtol=tol)


# ---------------------------------------------------------------- bound checkers (CPU, fp64)
def _check_fwd_apply(tag, y, bits, x, sc, sf, res=None, xd=None, scd=None, sfd=None, relu=True):
    """|y - act(o)| <= 2^-8 |o| + 2^-20 T with T = |x sc| + |sf| + |res| (+ |xd scd| + |sfd|); the mask bit
    equals o > 0 wherever |o| > 2^-20 T; at most 0.1 % of the elements fall under that threshold."""
    x, sc, sf = x.double(), sc.double(), sf.double()
    o = x * sc + sf
    T = (x * sc).abs() + sf.abs()
    if res is not None:
        o = o + res.double()
        T = T + res.double().abs()
    if xd is not None:
        o = o + xd.double() * scd.double() + sfd.double()
        T = T + (xd.double() * scd.double()).abs() + sfd.double().abs()
    ref = o.clamp_min(0) if relu else o
    bound = U_BF16 * o.abs() + U_F32 * T
    err = (y.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    live = o.abs() > U_F32 * T
    excl = 1.0 - live.double().mean().item()
    print(f"fwd_apply[{tag}] worst err/bound {ratio:.3f} excluded {excl:.2e}")
    assert bool((err <= bound).all()), f"{tag}: err/bound {ratio}"
    if bits is not None:
        assert excl <= EXCL_CAP, f"{tag}: {excl} of the elements inside the slack"
        assert torch.equal(bits.bool()[live], (o > 0)[live]), f"{tag}: mask bit != (o > 0)"
    return ratio, excl


def _check_bwd_apply(tag, dx, g, x, k, c1, c0, live=None):
    """|dx - ref| <= 2^-8 |ref| + 2^-20 (|k g| + |c1 x| + |c0|), ref = k g + c1 x + c0."""
    g, x, k, c1, c0 = g.double(), x.double(), k.double(), c1.double(), c0.double()
    ref = k * g + c1 * x + c0
    bound = U_BF16 * ref.abs() + U_F32 * ((k * g).abs() + (c1 * x).abs() + c0.abs())
    err = (dx.double() - ref).abs()
    if live is not None:
        err, bound = err[live], bound[live]
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"bwd_apply[{tag}] worst err/bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{tag}: err/bound {ratio}"
    return ratio


def _check_sums(tag, got, ta, tb):
    """Per channel |got - sum(terms)| <= 2^-16 sum(|terms|).  The kernels' fp32 add chain -- a lane's rows,
    the RPI fold, the atomics of one replica, the 32 replicas -- is shorter than 2^8 adds at SHAPES."""
    worst = 0.0
    for name, gsum, t in (("a", got[0], ta), ("b", got[1], tb)):
        t = t.double()
        err = (gsum.double() - t.sum(0)).abs()
        bound = U_SUM * t.abs().sum(0)
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), f"{tag} sum {name}: err/bound {ratio}"
    print(f"sums[{tag}] worst err/bound {worst:.3f}")
    return worst


def _sign_slack(x, sc, sf):
    """Elements whose sign of x sc + sf lies inside the fp32 slack: |x sc + sf| <= 2^-20 (|x sc| + |sf|)."""
    x, sc, sf = x.double(), sc.double(), sf.double()
    o = x * sc + sf
    return o, o.abs() <= U_F32 * ((x * sc).abs() + sf.abs())


# ---------------------------------------------------------------- GPU pipeline helpers
def _params(d, pd, s=""):
    return {"gamma": d["gamma" + s].to(pd).cuda(), "beta": d["beta" + s].to(pd).cuda(),
            "rm": d["rm" + s].clone().cuda(), "rv": d["rv" + s].clone().cuda()}


def _fwd_finalize(x, ws, M, C, p, training=True, shift=None):
    sm = torch.empty(C, device="cuda")
    si = torch.empty(C, device="cuda")
    _ext().bn_stage_fwd_finalize(None if shift is not None else x, shift, ws, M, C, p["gamma"], p["beta"], p["rm"],
                                 p["rv"], sm, si, training, MOM, EPS)
    return sm, si


def _stats_finalize(x, ws, M, C, p):
    _ext().bn_stage_fwd_stats(x, ws, M, C)
    return _fwd_finalize(x, ws, M, C, p)


def _bwd_finalize(ws, M, C, p, sm, si, training=True):
    dg = torch.empty_like(p["gamma"])
    db = torch.empty_like(p["gamma"])
    _ext().bn_stage_bwd_finalize(ws, M, C, p["gamma"], sm, si, dg, db, training)
    return dg, db


# ================================================================ Tier 1: exact, small integers
@gpu
def test_workspace_layout_matches_bindings():
    ext = _ext()
    for C in (8, 264, 2048):
        assert ext.bn_coef_offset(C) == REP * 4 * C
        assert ext.bn_workspace_floats(C) >= REP * 4 * C + 5 * C


@gpu
@pytest.mark.parametrize("M,C", SHAPES)
def test_fwd_stats_exact(M, C):
    d = _int_case(M, C)
    ws = _ws(C)
    _ext().bn_stage_fwd_stats(_dev(d["x"]), ws, M, C)
    v = _views(ws, C)
    ref = torch.stack([d["x"].sum(0), (d["x"] * d["x"]).sum(0)]).double()
    assert torch.equal(_sums(v["facc"]), ref)
    assert not ws[REP * 2 * C:].any(), "stats wrote outside the forward accumulators"
    if (M, C) in WRAP_SHAPES:
        assert _plan(M, C)["gx"] > REP
        assert int((v["facc"] != 0).any(-1).any(-1).sum()) > 1, "all blocks added into one replica row"


@gpu
@pytest.mark.parametrize("mask_x", [False, True])
@pytest.mark.parametrize("M,C,pd", [(M, C, torch.float32) for M, C in SHAPES] + [(197, 64, torch.bfloat16)])
def test_bwd_reduce_exact(M, C, pd, mask_x):
    d = _int_case(M, C)
    gamma = torch.ones(C, device="cuda", dtype=pd)
    beta = torch.zeros(C, device="cuda", dtype=pd)
    invstd = torch.ones(C, device="cuda")
    if mask_x:
        # scale 1, shift -1.5: x - 1.5 is never 0, so the mask x > 1.5 is unambiguous; terms are multiples of 0.5
        mean = torch.full((C,), 1.5)
        g = d["dy"] * (d["x"] >= 2)
    else:
        mean = d["mean"].float()
        g = d["dy"]
    ws = _ws(C)
    _ext().bn_stage_bwd_reduce(_dev(d["dy"]), _dev(d["x"]), gamma, beta, mean.cuda(), invstd, ws, M, C, mask_x)
    v = _views(ws, C)
    ref = torch.stack([g.double().sum(0), (g.double() * (d["x"].double() - mean.double())).sum(0)])
    assert torch.equal(_sums(v["bacc"]), ref)
    assert not v["facc"].any(), "backward reduce wrote into the forward accumulators"
    if (M, C) in WRAP_SHAPES:
        assert int((v["bacc"] != 0).any(-1).any(-1).sum()) > 1


@gpu
@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("M,C", SHAPES)
def test_bwd_mask_reduce_exact(M, C, second):
    d = _int_case(M, C)
    g = d["dy"] * _unpack(d["mb"], C)
    ws, ws2 = _ws(C), _ws(C)
    gout = torch.full((M, C), 77.0, device="cuda", dtype=torch.bfloat16)
    extra = (_dev(d["x2"]), d["mean2"].float().cuda(), ws2) if second else (None, None, None)
    _ext().bn_stage_bwd_mask_reduce(_dev(d["dy"]), 0, 1.0, d["mb"].cuda(), _dev(d["x"]), d["mean"].float().cuda(),
                                    gout, ws, M, C, *extra)
    assert torch.equal(gout.double().cpu(), g.double())
    ref = torch.stack([g.sum(0), (g * (d["x"] - d["mean"])).sum(0)]).double()
    assert torch.equal(_sums(_views(ws, C)["bacc"]), ref)
    if second:
        ref2 = torch.stack([g.sum(0), (g * (d["x2"] - d["mean2"])).sum(0)]).double()
        assert torch.equal(_sums(_views(ws2, C)["bacc"]), ref2)
    else:
        assert not ws2.any()


@gpu
@pytest.mark.parametrize("second", [False, True])
def test_bwd_mask_reduce_broadcast_exact(second):
    """dy is one row per image ([M/4, C], multiples of 4), scaled by 0.25 inside the kernel: still integers."""
    M, C, rows = 196, 64, 4
    d = _int_case(M, C)
    dy_img = 4 * d["dy"][:M // rows]
    g = (dy_img // 4).repeat_interleave(rows, 0) * _unpack(d["mb"], C)
    ws, ws2 = _ws(C), _ws(C)
    gout = torch.full((M, C), 77.0, device="cuda", dtype=torch.bfloat16)
    extra = (_dev(d["x2"]), d["mean2"].float().cuda(), ws2) if second else (None, None, None)
    _ext().bn_stage_bwd_mask_reduce(_dev(dy_img), rows, 0.25, d["mb"].cuda(), _dev(d["x"]),
                                    d["mean"].float().cuda(), gout, ws, M, C, *extra)
    assert torch.equal(gout.double().cpu(), g.double())
    ref = torch.stack([g.sum(0), (g * (d["x"] - d["mean"])).sum(0)]).double()
    assert torch.equal(_sums(_views(ws, C)["bacc"]), ref)
    if second:
        ref2 = torch.stack([g.sum(0), (g * (d["x2"] - d["mean2"])).sum(0)]).double()
        assert torch.equal(_sums(_views(ws2, C)["bacc"]), ref2)


@gpu
@pytest.mark.parametrize("M,C", [(197, 64), (4231, 264)])
def test_workspace_self_cleaning_and_isolation(M, C):
    """Each finalize zeroes its own accumulators and leaves the other direction's coefficients bit-identical
    (the engine runs a weight gradient that reads the forward coefficients beside the backward finalize)."""
    ext = _ext()
    d = _int_case(M, C)
    x, dy = _dev(d["x"]), _dev(d["dy"])
    mean, invstd = d["mean"].float().cuda(), torch.ones(C, device="cuda")
    p = {"gamma": torch.rand(C, device="cuda") + 0.5, "beta": torch.randn(C, device="cuda"),
         "rm": torch.zeros(C, device="cuda"), "rv": torch.ones(C, device="cuda")}
    ref_f = torch.stack([d["x"].sum(0), (d["x"] * d["x"]).sum(0)]).double()
    ref_b = torch.stack([d["dy"].sum(0), (d["dy"] * (d["x"] - d["mean"])).sum(0)]).double()
    ws = _ws(C)
    v = _views(ws, C)
    v["bcoef"].copy_(torch.randn(3, C))  # sentinel: the forward finalize must not touch it
    for _ in range(2):
        ext.bn_stage_fwd_stats(x, ws, M, C)
        assert torch.equal(_sums(v["facc"]), ref_f)
        before = v["bcoef"].clone()
        _fwd_finalize(x, ws, M, C, p)
        assert not v["facc"].any(), "forward accumulators not re-zeroed"
        assert _bits_equal(v["bcoef"], before), "forward finalize touched the backward coefficients"
        assert bool((v["fcoef"][0] != 0).all())
        ext.bn_stage_bwd_reduce(dy, x, p["gamma"], p["beta"], mean, invstd, ws, M, C, False)
        assert torch.equal(_sums(v["bacc"]), ref_b)
        before = v["fcoef"].clone()
        _bwd_finalize(ws, M, C, p, mean, invstd)
        assert not v["bacc"].any(), "backward accumulators not re-zeroed"
        assert _bits_equal(v["fcoef"], before), "backward finalize touched the forward coefficients"
        assert not v["facc"].any()


@gpu
@pytest.mark.parametrize("data", ["int", "float"])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("M,C", SHAPES)
def test_fwd_apply_mask_equals_stored_output(M, C, dual, data):
    """Every mask bit equals y > 0 of the stored bf16 y.  The integer case (scale 1, shift -2 written straight
    into the workspace) puts a quarter of the pre-activations at exactly 0."""
    ext = _ext()
    ws, wsd = _ws(C), _ws(C)
    if data == "int":
        d = _int_case(M, C)
        x, other = _dev(d["x"]), _dev(d["x2"] - 1 if dual else d["res"])
        _views(ws, C)["fcoef"].copy_(torch.stack([torch.ones(C), torch.full((C,), -2.0)]))
        _views(wsd, C)["fcoef"].copy_(torch.stack([torch.ones(C), torch.zeros(C)]))
    else:
        d = _float_case(M, C)
        x, other = d["x"].cuda(), (d["xd"] if dual else d["res"]).cuda()
        _stats_finalize(x, ws, M, C, _params(d, torch.float32))
        if dual:
            _stats_finalize(other, wsd, M, C, _params(d, torch.float32, "d"))
    y = torch.full((M, C), -5.0, device="cuda", dtype=torch.bfloat16)
    mb = torch.full((M, C // 8), 0xA5, device="cuda", dtype=torch.uint8)
    if dual:
        ext.bn_stage_fwd_apply(x, ws, None, other, wsd, y, mb, M, C, True)
    else:
        ext.bn_stage_fwd_apply(x, ws, other, None, None, y, mb, M, C, True)
    assert torch.equal(mb.cpu(), _pack(y.cpu() > 0))
    assert bool((y >= 0).all())
    if data == "int":
        o = d["x"] - 2 + (d["x2"] - 1 if dual else d["res"])
        assert torch.equal(y.double().cpu(), o.clamp_min(0).double())


# ================================================================ Tier 2: fp64 references, realistic data
def _assert_finalize(got, ref, tol_a, tol_b):
    for name in ("mean", "rm", "sc", "sf"):
        _close(got[name], ref[name], tol_a)
    for name in ("invstd", "rv"):
        _close(got[name], ref[name], tol_b)


@gpu
@pytest.mark.parametrize("pd", PDTYPES)
@pytest.mark.parametrize("M,C", SHAPES)
def test_fwd_finalize_training_vs_fp64(M, C, pd):
    d = _float_case(M, C)
    p = _params(d, pd)
    ws = _ws(C)
    sm, si = _stats_finalize(d["x"].cuda(), ws, M, C, p)
    v = _views(ws, C)
    ref = _ref_finalize(d["x"].double(), p["gamma"].double().cpu(), p["beta"].double().cpu(), d["rm"].double(),
                        d["rv"].double())
    _assert_finalize({"mean": sm, "invstd": si, "rm": p["rm"], "rv": p["rv"], "sc": v["fcoef"][0],
                      "sf": v["fcoef"][1]}, ref, 1e-4, 1e-3)
    assert not v["facc"].any()


@gpu
@pytest.mark.parametrize("std", [0.01, 0.5])
def test_fwd_finalize_large_mean(std):
    """|mean| >> std at 100: the per-channel shift K = x[0, c] keeps the variance from cancelling.  std 0.01 is
    the case of test_bn_large_mean_stability (bf16 has a 0.5 ulp at 100, so it is all but constant); std 0.5
    keeps a real variance after the rounding."""
    M, C = 197, 64
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(M, C, generator=g) * std + 100.0).bfloat16()
    d = _float_case(M, C)
    p = _params(d, torch.float32)
    ws = _ws(C)
    sm, si = _stats_finalize(x.cuda(), ws, M, C, p)
    v = _views(ws, C)
    ref = _ref_finalize(x.double(), d["gamma"].double(), d["beta"].double(), d["rm"].double(), d["rv"].double())
    _assert_finalize({"mean": sm, "invstd": si, "rm": p["rm"], "rv": p["rv"], "sc": v["fcoef"][0],
                      "sf": v["fcoef"][1]}, ref, 2e-3, 2e-3)


@gpu
@pytest.mark.parametrize("pd", PDTYPES)
@pytest.mark.parametrize("M,C", [(7, 24), (197, 64), (4231, 264)])
def test_fwd_finalize_external_shift_aliasing_running_mean(M, C, pd):
    """The engine's call after a GEMM-epilogue reduction: ``x=None, shift=rm, rm=rm``, the sums taken around
    K = running_mean.  K is read before running_mean is updated in place.  rm is drawn with
    |mean - K| <= 3 std: the range this path is designed for (the running mean tracks the batch mean; a K
    many std away would cancel in E[d^2] - E[d]^2)."""
    d = _float_case(M, C)
    x64 = d["x"].double()
    mean, var = _ref_moments(x64)
    g = torch.Generator().manual_seed(11)
    k_old = (mean + (torch.rand(C, generator=g, dtype=torch.float64) * 2 - 1) * 2.9 * var.sqrt()).float()
    K = k_old.double()
    assert bool(((mean - K).abs() <= 3 * var.sqrt()).all())
    s1, s2 = (x64 - K).sum(0), ((x64 - K) ** 2).sum(0)
    rows = torch.randperm(REP, generator=g)[:5]
    w = torch.rand(5, C, generator=g, dtype=torch.float64) + 0.1
    w = w / w.sum(0)
    acc = torch.zeros(REP, 2, C)
    acc[rows, 0] = (s1 * w).float()
    acc[rows, 1] = (s2 * w).float()
    ws = _ws(C)
    v = _views(ws, C)
    v["facc"].copy_(acc)
    p = _params(d, pd)
    p["rm"] = k_old.clone().cuda()
    sm, si = _fwd_finalize(None, ws, M, C, p, shift=p["rm"])
    ref = _ref_finalize(x64, p["gamma"].double().cpu(), p["beta"].double().cpu(), K, d["rv"].double())
    _assert_finalize({"mean": sm, "invstd": si, "rm": p["rm"], "rv": p["rv"], "sc": v["fcoef"][0],
                      "sf": v["fcoef"][1]}, ref, 1e-4, 1e-3)
    _close(p["rm"], 0.9 * K + 0.1 * mean, 1e-4)
    assert not v["facc"].any()


@gpu
@pytest.mark.parametrize("pd", PDTYPES)
@pytest.mark.parametrize("M,C", [(197, 64), (98, 2048)])
def test_finalize_eval_vs_fp64(M, C, pd):
    ext = _ext()
    d = _float_case(M, C)
    p = _params(d, pd)
    x, dy = d["x"].cuda(), d["dy"].cuda()
    ws = _ws(C)
    v = _views(ws, C)
    sm, si = _fwd_finalize(x, ws, M, C, p, training=False)
    assert torch.equal(sm.cpu(), d["rm"]), "eval: save_mean must be running_mean"
    assert torch.equal(p["rm"].cpu(), d["rm"]) and torch.equal(p["rv"].cpu(), d["rv"])
    g64, b64 = p["gamma"].double().cpu(), p["beta"].double().cpu()
    invstd = (d["rv"].double() + EPS).rsqrt()
    _close(si, invstd, 1e-3)
    _close(v["fcoef"][0], g64 * invstd, 1e-4)
    _close(v["fcoef"][1], b64 - d["rm"].double() * g64 * invstd, 1e-4)
    ext.bn_stage_bwd_reduce(dy, x, p["gamma"], p["beta"], sm, si, ws, M, C, False)
    dg, db = _bwd_finalize(ws, M, C, p, sm, si, training=False)
    assert not v["bacc"].any()
    assert not v["bcoef"][1].any() and not v["bcoef"][2].any(), "eval: c1 and c0 must be exactly 0"
    _close(v["bcoef"][0], g64 * si.double().cpu(), 1e-4)
    # dbeta = sum(dy), dgamma = sum(dy (x - mean)) invstd: the fp32 chain bound of _check_sums, one more fp32
    # product, and half a bf16 ulp where the parameters (hence their gradients) are bf16
    dy64, xc = d["dy"].double(), d["x"].double() - sm.double().cpu()
    out_ulp = U_BF16 if pd == torch.bfloat16 else 0.0
    ref_db, ref_dg = dy64.sum(0), (dy64 * xc).sum(0) * si.double().cpu()
    assert bool(((db.double().cpu() - ref_db).abs() <= U_SUM * dy64.abs().sum(0) + out_ulp * ref_db.abs()).all())
    assert bool(((dg.double().cpu() - ref_dg).abs() <= U_SUM * (dy64 * xc).abs().sum(0) * si.double().cpu()
                 + (U_F32 + out_ulp) * ref_dg.abs()).all())


FWD_FORMS = ["plain", "relu", "relu_res", "relu_res_mask", "res", "dual", "dual_mask"]


@gpu
@pytest.mark.parametrize("M,C", SHAPES)
def test_fwd_apply_all_forms_vs_fp64(M, C):
    ext = _ext()
    d = _float_case(M, C)
    x, xd, res = d["x"].cuda(), d["xd"].cuda(), d["res"].cuda()
    ws, wsd = _ws(C), _ws(C)
    _stats_finalize(x, ws, M, C, _params(d, torch.float32))
    _stats_finalize(xd, wsd, M, C, _params(d, torch.bfloat16, "d"))
    sc, sf = _views(ws, C)["fcoef"].cpu()
    scd, sfd = _views(wsd, C)["fcoef"].cpu()
    for form in FWD_FORMS:
        relu = form != "plain" and form != "res"
        with_mask = form.endswith("mask")
        y = torch.full((M, C), -5.0, device="cuda", dtype=torch.bfloat16)
        mb = torch.full((M, C // 8), 0xA5, device="cuda", dtype=torch.uint8) if with_mask else None
        if form.startswith("dual"):
            ext.bn_stage_fwd_apply(x, ws, None, xd, wsd, y, mb, M, C, True)
            kw = {"xd": d["xd"], "scd": scd, "sfd": sfd}
        else:
            with_res = "res" in form
            ext.bn_stage_fwd_apply(x, ws, res if with_res else None, None, None, y, mb, M, C, relu)
            kw = {"res": d["res"]} if with_res else {}
        bits = _unpack(mb.cpu(), C) if with_mask else None
        _check_fwd_apply(f"{form} {M}x{C}", y.cpu(), bits, d["x"], sc, sf, relu=relu, **kw)


@gpu
@pytest.mark.parametrize("pd", PDTYPES)
@pytest.mark.parametrize("M,C", SHAPES)
def test_bwd_apply_all_forms_vs_fp64(M, C, pd):
    """bn_stage_bwd_apply (single, dual) and bn_stage_bwd_apply_maskx against k g + c1 x + c0 in fp64, with the
    coefficients read back from the workspace (themselves checked by the chain tests below)."""
    ext = _ext()
    d = _float_case(M, C)
    x, xd, dy = d["x"].cuda(), d["xd"].cuda(), d["dy"].cuda()
    p, pdl = _params(d, pd), _params(d, pd, "d")
    ws, wsd = _ws(C), _ws(C)
    sm, si = _stats_finalize(x, ws, M, C, p)
    smd, sid = _stats_finalize(xd, wsd, M, C, pdl)
    # single and dual: the gradient arrives already masked, any g serves
    ext.bn_stage_bwd_reduce(dy, x, p["gamma"], p["beta"], sm, si, ws, M, C, False)
    ext.bn_stage_bwd_reduce(dy, xd, pdl["gamma"], pdl["beta"], smd, sid, wsd, M, C, False)
    _bwd_finalize(ws, M, C, p, sm, si)
    _bwd_finalize(wsd, M, C, pdl, smd, sid)
    k, c1, c0 = _views(ws, C)["bcoef"].cpu()
    kd, c1d, c0d = _views(wsd, C)["bcoef"].cpu()
    dx = torch.full((M, C), 9.0, device="cuda", dtype=torch.bfloat16)
    ext.bn_stage_bwd_apply(dy, x, ws, dx, None, None, None, M, C)
    _check_bwd_apply(f"single {M}x{C}", dx.cpu(), d["dy"], d["x"], k, c1, c0)
    dx.fill_(9.0)
    dxd = torch.full((M, C), 9.0, device="cuda", dtype=torch.bfloat16)
    ext.bn_stage_bwd_apply(dy, x, ws, dx, xd, wsd, dxd, M, C)
    _check_bwd_apply(f"dual.x {M}x{C}", dx.cpu(), d["dy"], d["x"], k, c1, c0)
    _check_bwd_apply(f"dual.xd {M}x{C}", dxd.cpu(), d["dy"], d["xd"], kd, c1d, c0d)
    # maskx: the ReLU mask is recomputed as x scale + shift > 0
    sc, sf = _views(ws, C)["fcoef"].cpu()
    o, slack = _sign_slack(d["x"], sc, sf)
    excl = slack.double().mean().item()
    print(f"bwd_apply[maskx {M}x{C}] excluded {excl:.2e}")
    assert excl <= EXCL_CAP
    ext.bn_stage_bwd_reduce(dy, x, p["gamma"], p["beta"], sm, si, ws, M, C, True)
    _bwd_finalize(ws, M, C, p, sm, si)
    k, c1, c0 = _views(ws, C)["bcoef"].cpu()
    dx.fill_(9.0)
    ext.bn_stage_bwd_apply_maskx(dy, x, p["gamma"], p["beta"], sm, si, ws, dx, M, C)
    _check_bwd_apply(f"maskx {M}x{C}", dx.cpu(), d["dy"].double() * (o > 0), d["x"], k, c1, c0, live=~slack)


@gpu
@pytest.mark.parametrize("M,C", SHAPES)
def test_float_reductions_vs_fp64(M, C):
    ext = _ext()
    d = _float_case(M, C)
    x, xd = d["x"].cuda(), d["xd"].cuda()
    x64, xd64, dy64 = d["x"].double(), d["xd"].double(), d["dy"].double()
    p = _params(d, torch.float32)
    ws, wsd = _ws(C), _ws(C)
    v, vd = _views(ws, C), _views(wsd, C)
    # forward stats: sums around K = x[0, c]
    ext.bn_stage_fwd_stats(x, ws, M, C)
    dk = x64 - x64[0]
    _check_sums(f"stats {M}x{C}", _sums(v["facc"]), dk, dk * dk)
    sm, si = _fwd_finalize(x, ws, M, C, p)
    smd, _ = _stats_finalize(xd, wsd, M, C, _params(d, torch.float32, "d"))
    xc, xdc = x64 - sm.double().cpu(), xd64 - smd.double().cpu()
    # backward reduce, no mask
    ext.bn_stage_bwd_reduce(d["dy"].cuda(), x, p["gamma"], p["beta"], sm, si, ws, M, C, False)
    _check_sums(f"bwd_reduce {M}x{C}", _sums(v["bacc"]), dy64, dy64 * xc)
    v["bacc"].zero_()
    # backward reduce, mask from x: the gradient is zeroed where the sign of x scale + shift lies inside the
    # fp32 slack, so that every term of the reference is decided
    o, slack = _sign_slack(d["x"], *v["fcoef"].cpu())
    assert slack.double().mean().item() <= EXCL_CAP
    dyz = d["dy"].clone()
    dyz[slack] = 0
    gz = dyz.double() * (o > 0)
    ext.bn_stage_bwd_reduce(dyz.cuda(), x, p["gamma"], p["beta"], sm, si, ws, M, C, True)
    _check_sums(f"bwd_reduce_maskx {M}x{C}", _sums(v["bacc"]), gz, gz * xc)
    v["bacc"].zero_()
    # masked gradient + both BNs' sums
    g = dy64 * _unpack(d["mb"], C)
    gout = torch.full((M, C), 77.0, device="cuda", dtype=torch.bfloat16)
    ext.bn_stage_bwd_mask_reduce(d["dy"].cuda(), 0, 1.0, d["mb"].cuda(), x, sm, gout, ws, M, C, xd, smd, wsd)
    assert torch.equal(gout.double().cpu(), g)
    _check_sums(f"mask_reduce {M}x{C}", _sums(v["bacc"]), g, g * xc)
    _check_sums(f"mask_reduce.2 {M}x{C}", _sums(vd["bacc"]), g, g * xdc)


@gpu
def test_float_mask_reduce_pooled_broadcast():
    """The pooling head's gradient: one dy row per image, scaled by 1/49 and rounded to bf16 in the kernel."""
    M, C, hw = 98, 2048, 49
    d = _float_case(M, C)
    x = d["x"].cuda()
    ws = _ws(C)
    sm, _ = _stats_finalize(x, ws, M, C, _params(d, torch.float32))
    dy_img = d["dy"][:M // hw].contiguous()
    scaled = (dy_img.float() * torch.tensor(1.0 / hw, dtype=torch.float32)).bfloat16()  # as the kernel rounds it
    g = scaled.double().repeat_interleave(hw, 0) * _unpack(d["mb"], C)
    gout = torch.full((M, C), 77.0, device="cuda", dtype=torch.bfloat16)
    _ext().bn_stage_bwd_mask_reduce(dy_img.cuda(), hw, 1.0 / hw, d["mb"].cuda(), x, sm, gout, ws, M, C, None, None,
                                    None)
    assert torch.equal(gout.double().cpu(), g)
    _check_sums("mask_reduce 1/49", _sums(_views(ws, C)["bacc"]), g, g * (d["x"].double() - sm.double().cpu()))


def _scaled_close(got, ref, tol):
    s = max(1.0, ref.abs().max().item())
    torch.testing.assert_close(got.double().cpu() / s, ref / s, atol=tol, rtol=tol)


@gpu
@pytest.mark.parametrize("pd", PDTYPES)
@pytest.mark.parametrize("M,C", CHAIN_SHAPES)
def test_chain_bn_relu_vs_fp64_autograd(M, C, pd):
    """stats -> finalize -> apply(relu), then bwd_reduce(mask from x) -> bwd_finalize -> apply_maskx, against
    double-precision autograd of relu(BN(x)).  The reference takes the ReLU mask from the kernel's own output
    (checked against fp64 by the apply tests above)."""
    ext = _ext()
    d = _float_case(M, C)
    x, dy = d["x"].cuda(), d["dy"].cuda()
    p = _params(d, pd)
    ws = _ws(C)
    sm, si = _stats_finalize(x, ws, M, C, p)
    y = torch.empty_like(x)
    ext.bn_stage_fwd_apply(x, ws, None, None, None, y, None, M, C, True)
    ext.bn_stage_bwd_reduce(dy, x, p["gamma"], p["beta"], sm, si, ws, M, C, True)
    dg, db = _bwd_finalize(ws, M, C, p, sm, si)
    dx = torch.empty_like(x)
    ext.bn_stage_bwd_apply_maskx(dy, x, p["gamma"], p["beta"], sm, si, ws, dx, M, C)

    xr = d["x"].double().requires_grad_(True)
    gr = p["gamma"].double().cpu().requires_grad_(True)
    br = p["beta"].double().cpu().requires_grad_(True)
    out = _ref_bn(xr, gr, br) * (y.cpu() > 0)
    out.backward(d["dy"].double())
    _close(y, out.detach(), 3e-2)
    _close(dx, xr.grad, 5e-2)
    _scaled_close(dg, gr.grad, 5e-2)
    _scaled_close(db, br.grad, 5e-2)


@gpu
@pytest.mark.parametrize("pd", PDTYPES)
@pytest.mark.parametrize("M,C", CHAIN_SHAPES)
def test_chain_dual_tail_vs_fp64_autograd(M, C, pd):
    """The bottleneck tail relu(BN1(x) + BN2(xd)) with its packed mask: dual apply, mask_reduce feeding both
    BNs' sums, two backward finalizes, dual backward apply, against double-precision autograd."""
    ext = _ext()
    d = _float_case(M, C)
    x, xd, dy = d["x"].cuda(), d["xd"].cuda(), d["dy"].cuda()
    p, pdl = _params(d, pd), _params(d, pd, "d")
    ws, wsd = _ws(C), _ws(C)
    sm, si = _stats_finalize(x, ws, M, C, p)
    smd, sid = _stats_finalize(xd, wsd, M, C, pdl)
    y = torch.empty_like(x)
    mb = torch.empty(M, C // 8, device="cuda", dtype=torch.uint8)
    ext.bn_stage_fwd_apply(x, ws, None, xd, wsd, y, mb, M, C, True)
    g = torch.empty_like(x)
    ext.bn_stage_bwd_mask_reduce(dy, 0, 1.0, mb, x, sm, g, ws, M, C, xd, smd, wsd)
    dg, db = _bwd_finalize(ws, M, C, p, sm, si)
    dgd, dbd = _bwd_finalize(wsd, M, C, pdl, smd, sid)
    dx, dxd = torch.empty_like(x), torch.empty_like(x)
    ext.bn_stage_bwd_apply(g, x, ws, dx, xd, wsd, dxd, M, C)

    leaves = [d["x"].double(), p["gamma"].double().cpu(), p["beta"].double().cpu(),
              d["xd"].double(), pdl["gamma"].double().cpu(), pdl["beta"].double().cpu()]
    xr, gr, br, xdr, gdr, bdr = [t.requires_grad_(True) for t in leaves]
    out = (_ref_bn(xr, gr, br) + _ref_bn(xdr, gdr, bdr)) * _unpack(mb.cpu(), C)
    out.backward(d["dy"].double())
    _close(y, out.detach(), 3e-2)
    _close(dx, xr.grad, 5e-2)
    _close(dxd, xdr.grad, 5e-2)
    for got, ref in ((dg, gr.grad), (db, br.grad), (dgd, gdr.grad), (dbd, bdr.grad)):
        _scaled_close(got, ref, 5e-2)


@gpu
def test_rejected_arguments():
    """C % 8 != 0 is refused by every row-tiled entry point on the host, before any launch; the dual forward
    apply has no form without ReLU."""
    ext = _ext()
    M, C = 4, 12
    ws = _ws(C)
    a = torch.zeros(M, C, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros_like(a)
    out2 = torch.zeros_like(a)
    mb = torch.zeros(M * C // 8 + 1, device="cuda", dtype=torch.uint8)
    f = torch.ones(C, device="cuda")
    calls = {
        "fwd_stats": lambda: ext.bn_stage_fwd_stats(a, ws, M, C),
        "fwd_apply": lambda: ext.bn_stage_fwd_apply(a, ws, None, None, None, out, None, M, C, True),
        "bwd_mask_reduce": lambda: ext.bn_stage_bwd_mask_reduce(a, 0, 1.0, mb, a, f, out, ws, M, C, None, None, None),
        "bwd_reduce": lambda: ext.bn_stage_bwd_reduce(a, a, f, f, f, f, ws, M, C, False),
        "bwd_apply_maskx": lambda: ext.bn_stage_bwd_apply_maskx(a, a, f, f, f, f, ws, out, M, C),
        "bwd_apply": lambda: ext.bn_stage_bwd_apply(a, a, ws, out, None, None, None, M, C),
        "bwd_apply_dual": lambda: ext.bn_stage_bwd_apply(a, a, ws, out, a, ws, out2, M, C),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=r"invalid argument|C % 8"):
            call()
        assert not out.any() and not out2.any() and not ws.any(), f"{name} launched before refusing C = 12"
    M, C = 4, 8
    ws = _ws(C)
    a = torch.zeros(M, C, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros_like(a)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ext.bn_stage_fwd_apply(a, ws, None, a, ws, out, None, M, C, False)
    torch.cuda.synchronize()


# ================================================================ CPU self-checks (no GPU needed)
def test_plan_mirror_reaches_the_branches_named_in_shapes():
    """The comments beside SHAPES, checked against the Python mirror of the launch plans."""
    assert _plan(7, 24) == {"TPR": 3, "RPI": 85, "gy": 1, "gx": 1, "apply_gx": 1}
    assert (_plan(197, 64)["TPR"], _plan(197, 64)["RPI"]) == (8, 32)
    p = _plan(4231, 264)
    assert (p["TPR"], p["gy"], p["gx"]) == (32, 2, 34)
    assert _plan(98, 2048)["gy"] == 8
    p = _plan(16411, 64)
    assert p["gx"] == 33 and 16411 > 3 * p["gx"] * p["RPI"]  # the 4-way unrolled stats loop runs


@pytest.mark.parametrize("M,C", [s for s in SHAPES if s[0] > 1])
def test_cpu_fp64_references_match_autograd_batch_norm(M, C):
    d = _float_case(M, C)
    x64, g64, b64 = d["x"].double(), d["gamma"].double(), d["beta"].double()
    ref = _ref_finalize(x64, g64, b64, d["rm"].double(), d["rv"].double())
    rm, rv = d["rm"].double(), d["rv"].double()
    xa, ga, ba = [t.clone().requires_grad_(True) for t in (x64, g64, b64)]
    ya = F.batch_norm(xa, rm, rv, ga, ba, True, MOM, EPS)
    tol = {"atol": 1e-10, "rtol": 1e-10}
    torch.testing.assert_close(ref["rm"], rm, **tol)
    torch.testing.assert_close(ref["rv"], rv, **tol)
    torch.testing.assert_close(x64 * ref["sc"] + ref["sf"], ya.detach(), **tol)
    torch.testing.assert_close((ref["var"] + EPS).rsqrt(), ref["invstd"], **tol)
    xb, gb, bb = [t.clone().requires_grad_(True) for t in (x64, g64, b64)]
    yb = _ref_bn(xb, gb, bb)
    torch.testing.assert_close(yb.detach(), ya.detach(), **tol)
    mask = ya.detach() > 0
    (ya * mask).backward(d["dy"].double())
    (yb * mask).backward(d["dy"].double())
    for a, b in ((xa, xb), (ga, gb), (ba, bb)):
        s = max(1.0, a.grad.abs().max().item())
        torch.testing.assert_close(b.grad / s, a.grad / s, **tol)


def _emu_finalize(x, gamma, beta):
    """fp32 torch: mean, invstd, scale, shift."""
    xf = x.float()
    mean = xf.mean(0)
    var = ((xf - mean) ** 2).mean(0)
    invstd = (var + EPS).rsqrt()
    sc = gamma.float() * invstd
    return mean, invstd, sc, beta.float() - mean * sc


def _emu_reduce(ta, tb, M, C):
    """fp32 sums of [M, C] terms in the kernels' order: a lane's grid-strided rows, the RPI fold, one add per
    block into replica b % 32, the 32 replicas."""
    pl = _plan(M, C)
    step = pl["gx"] * pl["RPI"]
    iters = -(-M // step)
    out = []
    for t in (ta, tb):
        t = torch.cat([t.float(), torch.zeros(iters * step - M, C)]).view(iters, pl["gx"], pl["RPI"], C)
        lane = torch.zeros(pl["gx"], pl["RPI"], C)
        for i in range(iters):
            lane = lane + t[i]
        blk = lane[:, 0].clone()
        for r in range(1, pl["RPI"]):
            blk = blk + lane[:, r]
        rep = torch.zeros(REP, C)
        for b in range(pl["gx"]):
            rep[b % REP] = rep[b % REP] + blk[b]
        tot = torch.zeros(C)
        for r in range(REP):
            tot = tot + rep[r]
        out.append(tot)
    return torch.stack(out)


@pytest.mark.parametrize("M,C", SHAPES)
def test_cpu_fp32_emulation_stays_inside_the_bounds(M, C):
    """A plain fp32 implementation of the apply and reduce stages passes the Tier 2 checks at every shape."""
    d = _float_case(M, C)
    xf, xdf, rf, dyf = d["x"].float(), d["xd"].float(), d["res"].float(), d["dy"].float()
    mean, invstd, sc, sf = _emu_finalize(d["x"], d["gamma"], d["beta"])
    meand, invstdd, scd, sfd = _emu_finalize(d["xd"], d["gammad"].bfloat16(), d["betad"].bfloat16())
    # forward apply
    for relu, with_res in ((False, False), (True, False), (True, True), (False, True)):
        o = xf * sc + sf + (rf if with_res else 0)
        y = (o.clamp_min(0) if relu else o).bfloat16()
        _check_fwd_apply(f"emu relu={relu} res={with_res} {M}x{C}", y, (o > 0) if relu and with_res else None,
                         d["x"], sc, sf, res=d["res"] if with_res else None, relu=relu)
    o = (xf * sc + sf) + (xdf * scd + sfd)
    _check_fwd_apply(f"emu dual {M}x{C}", o.clamp_min(0).bfloat16(), o > 0, d["x"], sc, sf, xd=d["xd"], scd=scd,
                     sfd=sfd)
    # reductions
    dk = xf - xf[0]
    _check_sums(f"emu stats {M}x{C}", _emu_reduce(dk, dk * dk, M, C), dk.double(), dk.double() ** 2)
    xc64 = d["x"].double() - mean.double()
    _check_sums(f"emu bwd_reduce {M}x{C}", _emu_reduce(dyf, dyf * (xf - mean), M, C), d["dy"].double(),
                d["dy"].double() * xc64)
    o64, slack = _sign_slack(d["x"], sc, sf)
    excl = slack.double().mean().item()
    assert excl <= EXCL_CAP
    dyz = dyf.clone()
    dyz[slack] = 0
    gz = dyz * ((xf * sc + sf) > 0)
    assert torch.equal(gz.double(), dyz.double() * (o64 > 0)), "fp32 and fp64 masks differ outside the slack"
    _check_sums(f"emu bwd_reduce_maskx {M}x{C}", _emu_reduce(gz, gz * (xf - mean), M, C), gz.double(),
                gz.double() * xc64)
    g = dyf * _unpack(d["mb"], C)
    _check_sums(f"emu mask_reduce {M}x{C}", _emu_reduce(g, g * (xf - mean), M, C), g.double(), g.double() * xc64)
    _check_sums(f"emu mask_reduce.2 {M}x{C}", _emu_reduce(g, g * (xdf - meand), M, C), g.double(),
                g.double() * (d["xd"].double() - meand.double()))
    # backward apply: coefficients as the backward finalize forms them, in fp32
    sa, sb = _emu_reduce(dyf, dyf * (xf - mean), M, C)
    k = d["gamma"] * invstd
    c1 = -k * invstd * (sb * invstd) / M
    c0 = -k * sa / M - c1 * mean
    dx = (k * dyf + (c1 * xf + c0)).bfloat16()
    _check_bwd_apply(f"emu single {M}x{C}", dx, d["dy"], d["x"], k, c1, c0)
    gm = dyf * ((xf * sc + sf) > 0)
    dx = (k * gm + (c1 * xf + c0)).bfloat16()
    _check_bwd_apply(f"emu maskx {M}x{C}", dx, d["dy"].double() * (o64 > 0), d["x"], k, c1, c0, live=~slack)
