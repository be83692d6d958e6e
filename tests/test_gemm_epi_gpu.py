"""Conv GEMM prologues / epilogues and the in-GEMM BN finalize against int64 / fp64 references.

Almost all of the ResNet step runs through ``conv1x1_gemm`` / ``conv3x3_gemm`` / ``conv3x3_s2_dgrad``, the
weight gradients ``conv1x1_wgrad`` / ``conv3x3_wgrad`` and the BN finalize that ``bn_fin_arm`` folds into the
GEMM's last arriving blocks (csrc/gemm_epi.h, csrc/bn_fin.h).  Each gets a ground truth of its own here:

* Tier 1 -- small-integer data (A and gradients in -2..2, weights in -1..1, integer coefficients, mask shifts
  at integer + 0.5 so that ``x a + b`` is never 0).  Every fp32 accumulation is then an exact integer in any
  order and every bf16 store the round-to-nearest-even of an exact integer, so outputs, replica-summed
  accumulators, written-through tensors and mask bytes are compared bit for bit (``atol = 0``) with an int64
  reference that rounds (``.float().bfloat16()``) exactly where the kernel stores or re-reads bf16: the
  accumulator into the LDS tile, the residual add, A' of the prologues.  A dropped, doubled or misplaced row,
  a wrong tap, replica or mask bit changes the result.  Every reference asserts that the sum of absolute
  terms of each of its sums stays below 2^24 (a condition on the inputs, not a tolerance).
* Tier 2 -- realistic data: the armed GEMM's finalize against fp64 references built from the *stored* bf16
  output, with the bounds of tests/test_bn_stage_gpu.py, plus the bookkeeping (replicas re-zeroed, the other
  direction untouched, tile counters back at zero, a second launch bit-identical).
* CPU self-checks (no ``gpu`` marker) -- the int64 references equal ``F.conv2d`` / ``conv2d_input`` /
  ``conv2d_weight`` in fp64, the 2^24 condition holds for every parametrized case, and a plain fp32
  emulation of both finalizes stays inside the Tier 2 bounds.

The Tier 2 tests print their worst ``error / bound`` ratios (``pytest -rA`` shows them).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_bn_stage_gpu import (EPS, MOM, REP, U_BF16, U_F32, U_SUM, _assert_finalize, _bits_equal, _close, _pack,
                               _ref_finalize, _unpack, _views, _ws)

gpu = pytest.mark.gpu
CAP = 2 ** 24
NAN = float("nan")
PDTYPES = [torch.float32, torch.bfloat16]


def _ext():
    from kubedl_amd.ops import _ext
    return _ext.load()


@pytest.fixture(autouse=True)
def _restore_dispatch():
    """Every test leaves the dispatch knobs at their defaults (as tests/test_igemm_gpu.py does)."""
    yield
    if torch.cuda.is_available():
        ext = _ext()
        ext.set_gemm_core(-1)
        ext.set_igemm_cfg(-1)
        ext.set_halo3x3(1)
        ext.set_wgrad_big(-1)


def _dispatch(core=-1, cfg=-1, big=-1):
    ext = _ext()
    ext.set_gemm_core(core)
    ext.set_igemm_cfg(cfg)
    ext.set_wgrad_big(big)


# ---------------------------------------------------------------- small helpers
def _rne(t):
    """int64 -> the integer its bf16 round-to-nearest-even store holds (``.float()`` is exact below 2^24)."""
    return t.float().bfloat16().double().long()


def _dev(t):
    return t.to(torch.bfloat16).cuda()


def _fdev(t):
    return t.float().cuda()


def _budget(*terms):
    """The condition of Tier 1: per channel, the sum of absolute terms of every sum stays below 2^24."""
    worst = 0
    for t in terms:
        worst = max(worst, int(t.abs().sum(0).max()))
    assert worst < CAP, f"sum of absolute terms {worst} >= 2^24: narrow the input ranges"
    return worst


def _mm(a, w):
    """[M, K] x [N, K]^T in int64; the fp32 accumulation is exact while sum |a||w| < 2^24."""
    assert int((a.abs() @ w.abs().t()).max()) < CAP
    return a @ w.t()


def _gemm(A, W, C, M, N, K, **kw):
    args = dict(Hout=0, Wout=0, Hin=0, Win=0, stride=1, pro_coef=None, epi=0, shift=None, acc=None, ex=None,
                emean=None, ecoef=None, eres=None, res_stride=1, res_H=0, res_W=0, ebits=None, ex2=None,
                emean2=None, acc2=None)
    args.update(kw)
    _ext().conv1x1_gemm(A, W, C, M, N, K, args["Hout"], args["Wout"], args["Hin"], args["Win"], args["stride"],
                        args["pro_coef"], args["epi"], args["shift"], args["acc"], args["ex"], args["emean"],
                        args["ecoef"], args["eres"], args["res_stride"], args["res_H"], args["res_W"], args["ebits"],
                        args["ex2"], args["emean2"], args["acc2"])


def _acc_sums(ws, C, fwd):
    v = _views(ws, C)
    return (v["facc"] if fwd else v["bacc"]).double().sum(0).cpu()


def _assert_same(got, ref, tag):
    """Bit-for-bit comparison of every tensor the reference names."""
    assert set(ref) <= set(got), f"{tag}: missing outputs {set(ref) - set(got)}"
    for name, r in ref.items():
        g = got[name].cpu()
        assert g.shape == r.shape, f"{tag} {name}: shape {tuple(g.shape)} != {tuple(r.shape)}"
        if r.dtype == torch.uint8:
            assert torch.equal(g, r), f"{tag} {name}: {(g != r).sum().item()} mask bytes differ"
            continue
        g = g.double()
        assert not g.isnan().any(), f"{tag} {name}: {int(g.isnan().any(-1).sum())} rows never written"
        bad = g != r.double()
        if bad.any():
            pytest.fail(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} values differ, first at "
                        f"{bad.nonzero()[0].tolist()}: got {g[bad][0].item()} expected {r.double()[bad][0].item()}",
                        pytrace=False)


# ---------------------------------------------------------------- Tier 1 inputs (built once, never modified)
@functools.lru_cache(maxsize=None)
def _int_operands(M, N, K, rows_in=0):
    """CPU int64 operands of one [M, N, K] GEMM: A (``rows_in`` rows when gathered) and gradients in -2..2,
    weights in -1..1, BN inputs in 0..3, integer means / shifts / coefficients, mask shifts at integer + 0.5."""
    g = torch.Generator().manual_seed(7919 * M + 31 * N + K)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g)

    return {"A": ri(-2, 2, rows_in or M, K), "W": ri(-1, 1, N, K),
            "x": ri(0, 3, M, N), "x2": ri(0, 3, M, N), "mean": ri(0, 3, N), "mean2": ri(0, 3, N),
            "shift": ri(-2, 2, N), "ea": ri(1, 2, N), "eb": ri(-3, 0, N).double() - 0.5,
            "mb": torch.randint(0, 256, (M, N // 8), generator=g, dtype=torch.uint8), "res": ri(-2, 2, M, N),
            "psc": ri(1, 2, K), "psf": ri(-2, 1, K),
            "bx": ri(0, 3, M, K), "bk": ri(1, 2, K), "bc1": ri(-1, 1, K), "bc0": ri(-1, 1, K),
            "rres": ri(-2, 2, M, K), "rsc": ri(1, 2, K), "rsf": ri(-2, 1, K), "rscd": ri(-1, 1, K), "rsfd": ri(-1, 1, K)}


# ---------------------------------------------------------------- int64 references
def _ref_epilogue(acc, epi, d, res=None, res_geom=None, x2=False):
    """The epilogue of csrc/gemm_epi.h on the exact accumulator ``acc`` [M, N] (int64).  Returns the expected
    output, the replica-summed accumulators, and asserts the 2^24 condition on every sum it forms."""
    M, N = acc.shape
    y = _rne(acc)  # the accumulator tile is rounded to bf16 into LDS
    ref = {}
    if epi == 0:
        ref["C"] = y
    elif epi == 1:
        dd = y - d["shift"]
        _budget(dd, dd * dd)
        ref["C"] = y
        ref["acc"] = torch.stack([dd.sum(0), (dd * dd).sum(0)])
    elif epi == 2:
        live = (d["x"].double() * d["ea"].double() + d["eb"]) > 0  # never 0: the shift is an integer + 0.5
        g = y * live
        t = g * (d["x"] - d["mean"])
        _budget(g, t)
        ref["C"] = g
        ref["acc"] = torch.stack([g.sum(0), t.sum(0)])
    else:
        if res_geom is None:
            has, full = torch.ones(M, dtype=torch.bool), res
        else:  # strided residual: rows (h % s == 0, w % s == 0) of each res_H x res_W image receive one
            nb, H, W, s = res_geom
            Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
            full = torch.zeros(nb, H, W, N, dtype=torch.long)
            full[:, ::s, ::s] = res.view(nb, Ho, Wo, N)
            has = torch.zeros(nb, H, W, dtype=torch.bool)
            has[:, ::s, ::s] = True
            full, has = full.view(M, N), has.view(M)
        y = torch.where(has[:, None], _rne(y + full), y)  # the sum is rounded to bf16 again
        if epi == 4:
            ref["C"] = y
        else:
            g = y * _unpack(d["mb"], N)
            t = g * (d["x"] - d["mean"])
            _budget(g, t)
            ref["C"] = g
            ref["acc"] = torch.stack([g.sum(0), t.sum(0)])
            if x2:
                t2 = g * (d["x2"] - d["mean2"])
                _budget(t2)
                ref["acc2"] = torch.stack([g.sum(0), t2.sum(0)])
    return ref


def _ref_pro_fwd(a, sc, sf):
    """relu(a scale + shift), stored as bf16 (the A staging of PRO_FWD, the halo kernels' input transform)."""
    return _rne((a * sc + sf).clamp_min(0))


def _gather_rows(a, nb, H, W, stride):
    """Rows (n, oh s, ow s) of an [nb H W, K] tensor: the stride-s 1x1 conv's A rows."""
    K = a.shape[1]
    return a.view(nb, H, W, K)[:, ::stride, ::stride].reshape(-1, K)


def _patches(x, stride):
    """[nb, H, W, Cin] -> [nb Ho Wo, 9 Cin] in (r, s, cin) order: the implicit GEMM's A of a 3x3 / pad 1 conv
    against weights [Cout][3][3][Cin] (channels_last OIHW).  Padding taps are zero."""
    nb, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.zeros(nb, H + 2, W + 2, Cin, dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    cols = [xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]
            for r in range(3) for s in range(3)]
    return torch.stack(cols, 3).reshape(nb * Ho * Wo, 9 * Cin)


def _ref_s2_dgrad(dy, w, Hx, Wx):
    """dx [nb, Hx, Wx, Cin] of conv2d(x, w, stride 2, pad 1) for dy [nb, Hd, Wd, Cout], w [Cout, Cin, 3, 3]: each
    dy pixel (oh, ow) adds dy w[:, :, r, s] to dx pixel (2 oh - 1 + r, 2 ow - 1 + s)."""
    nb, Hd, Wd, Cout = dy.shape
    Cin = w.shape[1]
    dxp = torch.zeros(nb, 2 * Hd + 1, 2 * Wd + 1, Cin, dtype=dy.dtype)
    for r in range(3):
        for s in range(3):
            dxp[:, r:r + 2 * Hd:2, s:s + 2 * Wd:2] += dy @ w[:, :, r, s]
    return dxp[:, 1:1 + Hx, 1:1 + Wx].contiguous()


# ================================================================ Tier 1: conv1x1_gemm
# nb, H, W of the output rows (M = nb H W): odd images, M never a multiple of the row tile
G_SMALL = (1, 5, 9)      # M = 45: below one tile; the launcher pads the grid to 8 blocks, 7 of them inactive
G_MID = (3, 7, 11)       # M = 231: two 128-row tiles, the second ragged
G_LONG = (13, 7, 11)     # M = 1001
G_BIG = (24, 5, 25)      # M = 3000

# (geom, N, K, epi, variant); variant tokens joined by "+": x2 (second BN input), rs2 (strided residual), s2
# (stride-2 row gather), pro (BN + ReLU prologue), bwd (backward-apply prologue), thru (its write-through),
# res / res2 (residual prologues, plain and dual)
# (STATS' statistics-only form, ``p.C == nullptr`` in gemm_epi.h, cannot be reached from Python: the
# conv1x1_gemm binding takes the output tensor as a required argument, so it has no case here.)
REG_TILES = [(64, 128), (128, 64), (128, 512)]  # N, K -> 128x64 | 32-deep config 5 under STATS | 128x128


def _reg_cases():
    cases = []
    for N, K in REG_TILES:
        for epi in range(5):
            cases.append((G_MID, N, K, epi, ""))
        cases += [(G_MID, N, K, 3, "x2"), (G_MID, N, K, 3, "rs2"), (G_MID, N, K, 3, "x2+rs2"), (G_MID, N, K, 4, "rs2")]
        cases += [(G_MID, N, K, 0, "pro"), (G_MID, N, K, 1, "pro"), (G_MID, N, K, 1, "pro+s2"), (G_MID, N, K, 0, "s2")]
        cases += [(G_MID, N, K, 1, "res"), (G_MID, N, K, 1, "res2")]
    for epi in (1, 2, 3, 4):
        cases.append((G_SMALL, 128, 64, epi, "x2" if epi == 3 else ""))
    cases += [(G_SMALL, 64, 128, 1, "pro"), (G_SMALL, 64, 128, 1, "res2"), (G_SMALL, 64, 128, 2, "bwd+thru")]
    # backward-apply prologue: 128-wide tiles to K = 512, 64-wide beyond
    for N, K in [(128, 512), (128, 576), (64, 128), (256, 1024)]:
        for epi in (0, 2, 3, 4):
            cases.append((G_MID, N, K, epi, "bwd+thru" if epi in (0, 3) else "bwd"))
    cases += [(G_LONG, 128, 1024, 3, "bwd+thru+x2+rs2"), (G_BIG, 256, 1024, 1, ""), (G_BIG, 256, 1024, 2, "")]
    return cases


def _dma_cases():
    cases = []
    for epi in range(5):
        cases.append((G_LONG, 256, 512, epi, ""))
        cases.append((G_MID, 256, 512, epi, "x2" if epi == 3 else ""))  # M below every DMA row tile but 128
    cases += [(G_LONG, 256, 512, 0, "s2"), (G_LONG, 256, 512, 1, "s2"), (G_LONG, 256, 512, 3, "x2+rs2"),
              (G_LONG, 256, 512, 4, "rs2"), (G_BIG, 256, 1024, 1, ""), (G_BIG, 256, 1024, 2, "")]
    return cases


REG_CASES = _reg_cases()
DMA_CASES = _dma_cases()


def _case_id(c):
    (nb, H, W), N, K, epi, var = c
    return f"{nb}x{H}x{W}-N{N}-K{K}-epi{epi}{'-' + var if var else ''}"


@functools.lru_cache(maxsize=None)
def _gemm1_ref(geom, N, K, epi, var):
    """Inputs (dict of CPU tensors) and the expected outputs of one conv1x1_gemm case."""
    nb, H, W = geom
    M = nb * H * W
    var = var.split("+")
    s2 = "s2" in var
    Hin, Win = (2 * H - 1, 2 * W) if s2 else (H, W)  # an odd and an even input size
    d = dict(_int_operands(M, N, K, nb * Hin * Win if s2 else 0))
    a = d["A"]
    ref = {}
    if "pro" in var:
        a = _ref_pro_fwd(a, d["psc"], d["psf"])
    if s2:
        a = _gather_rows(a, nb, Hin, Win, 2)
    if "bwd" in var:
        a = _rne(d["bk"] * a + d["bc1"] * d["bx"] + d["bc0"])
        if "thru" in var:
            ref["thru"] = a
    if "res" in var or "res2" in var:
        dual = "res2" in var
        o = a * d["rsc"] + d["rsf"] + (d["rres"] * d["rscd"] + d["rsfd"] if dual else d["rres"])
        a = _rne(o.clamp_min(0))
        ref["xout"] = a
        ref["obits"] = _pack(o > 0)
    rs2 = "rs2" in var
    res, res_geom = d["res"], None
    if rs2:
        res_geom = (nb, H, W, 2)
        res = d["res"][:nb * ((H + 1) // 2) * ((W + 1) // 2)]
        d["res_s"] = res
    ref.update(_ref_epilogue(_mm(a, d["W"]), epi, d, res=res, res_geom=res_geom, x2="x2" in var))
    d.update(Hin=Hin, Win=Win, s2=s2)
    return d, ref


def _gemm1_run(geom, N, K, epi, var):
    ext = _ext()
    nb, H, W = geom
    M = nb * H * W
    d, ref = _gemm1_ref(geom, N, K, epi, var)
    var = var.split("+")
    ws, ws2 = _ws(N), _ws(N)
    C = torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16)
    kw = {"epi": epi}
    got = {"C": C}
    if d["s2"]:
        kw.update(Hout=H, Wout=W, Hin=d["Hin"], Win=d["Win"], stride=2)
    if "pro" in var:
        kw["pro_coef"] = _fdev(torch.cat([d["psc"], d["psf"]]))
    if epi == 1:
        kw.update(shift=_fdev(d["shift"]), acc=_views(ws, N)["facc"])
    if epi in (2, 3):
        kw.update(ex=_dev(d["x"]), emean=_fdev(d["mean"]), acc=_views(ws, N)["bacc"])
    if epi == 2:
        kw["ecoef"] = torch.cat([d["ea"].double(), d["eb"]]).float().cuda()
    if epi in (3, 4):
        kw["eres"] = _dev(d["res_s"] if "rs2" in var else d["res"])
        if "rs2" in var:
            kw.update(res_stride=2, res_H=H, res_W=W)
    if epi == 3:
        kw["ebits"] = d["mb"].cuda()
        if "x2" in var:
            kw.update(ex2=_dev(d["x2"]), emean2=_fdev(d["mean2"]), acc2=_views(ws2, N)["bacc"])
    if "bwd" in var:
        wsb = _ws(K)
        _views(wsb, K)["bcoef"].copy_(torch.stack([d["bk"], d["bc1"], d["bc0"]]).float())
        thru = torch.full((M, K), NAN, device="cuda", dtype=torch.bfloat16) if "thru" in var else None
        keep = _dev(d["bx"])  # the arming holds raw pointers: its operands stay alive until the launch
        ext.bn_bwd_pro_arm(keep, wsb, K, thru)
        if thru is not None:
            got["thru"] = thru
    if "res" in var or "res2" in var:
        got["xout"] = torch.full((M, K), NAN, device="cuda", dtype=torch.bfloat16)
        got["obits"] = torch.full((M, K // 8), 0x5A, device="cuda", dtype=torch.uint8)
        coefd = _fdev(torch.cat([d["rscd"], d["rsfd"]])) if "res2" in var else None
        keep = (_dev(d["rres"]), _fdev(torch.cat([d["rsc"], d["rsf"]])))  # (raw pointers, as above)
        ext.bn_res_pro_arm(keep[0], keep[1], K, got["xout"], got["obits"], coefd)
    _gemm(_dev(d["A"]), _dev(d["W"]), C, M, N, K, **kw)
    if epi in (1, 2, 3):  # read before any finalize
        got["acc"] = _acc_sums(ws, N, epi == 1)
        other = _views(ws, N)["bacc" if epi == 1 else "facc"]
        assert not other.any(), "the epilogue added into the other direction's replicas"
    if "acc2" in ref:
        got["acc2"] = _acc_sums(ws2, N, False)
    else:
        assert not ws2.any()
    return got, ref


@gpu
@pytest.mark.parametrize("case", REG_CASES, ids=_case_id)
def test_conv1x1_gemm_register_core_exact(case):
    _dispatch(core=0)
    got, ref = _gemm1_run(*case)
    _assert_same(got, ref, _case_id(case))


@gpu
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("case", DMA_CASES, ids=_case_id)
def test_conv1x1_gemm_dma_core_exact(case, cfg):
    """N = 256 is a multiple of every config's tile width, so the forced config is the one that runs."""
    _dispatch(core=1, cfg=cfg)
    got, ref = _gemm1_run(*case)
    _assert_same(got, ref, f"cfg{cfg} {_case_id(case)}")


# ================================================================ Tier 1: conv3x3_gemm
# nb, H, W, Cin, Cout, stride, epi, pro, aout
C3_DMA = [(3, 7, 11, 64, 128, s, e, False, False) for s in (1, 2) for e in (0, 1, 2)]
C3_CFG = [(3, 7, 11, 64, 256, 2, 1, False, False), (3, 7, 11, 64, 256, 1, 2, False, False)]
C3_REG = ([(3, 7, 11, 64, 128, s, e, True, False) for s in (1, 2) for e in (0, 1)] +
          [(3, 7, 11, 64, 64, 1, 2, False, False), (2, 5, 3, 128, 128, 2, 1, True, False)])
# the halo kernel's only geometry: 56 x 56, Cin = Cout = 64 (csrc/halo3x3.hip)
C3_HALO = [(1, 56, 56, 64, 64, 1, 0, False, False), (1, 56, 56, 64, 64, 1, 1, False, False),
           (1, 56, 56, 64, 64, 1, 2, False, False), (1, 56, 56, 64, 64, 1, 1, True, False),
           (1, 56, 56, 64, 64, 1, 1, True, True)]


@functools.lru_cache(maxsize=None)
def _conv3_ref(nb, H, W, Cin, Cout, stride, epi, pro, aout):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = nb * Ho * Wo
    d = dict(_int_operands(M, Cout, 9 * Cin, nb * H * W))
    x = d["A"][:, :Cin]                       # the input rows [nb H W, Cin]
    psc, psf = d["psc"][:Cin], d["psf"][:Cin]
    ref = {}
    a = x
    if pro:
        a = _ref_pro_fwd(x, psc, psf)
        if aout:
            ref["aout"] = a
    acc = _mm(_patches(a.view(nb, H, W, Cin), stride), d["W"])
    ref.update(_ref_epilogue(acc, epi, d))
    d.update(x=d["x"], xin=x, psc3=psc, psf3=psf)
    return d, ref


def _conv3_run(nb, H, W, Cin, Cout, stride, epi, pro, aout):
    ext = _ext()
    d, ref = _conv3_ref(nb, H, W, Cin, Cout, stride, epi, pro, aout)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = nb * Ho * Wo
    ws = _ws(Cout)
    C = torch.full((M, Cout), NAN, device="cuda", dtype=torch.bfloat16)
    got = {"C": C}
    coef = _fdev(torch.cat([d["psc3"], d["psf3"]])) if pro else None
    shift = acc = ex = emean = ecoef = None
    if epi == 1:
        shift, acc = _fdev(d["shift"]), _views(ws, Cout)["facc"]
    if epi == 2:
        ex, emean, acc = _dev(d["x"]), _fdev(d["mean"]), _views(ws, Cout)["bacc"]
        ecoef = torch.cat([d["ea"].double(), d["eb"]]).float().cuda()
    if aout:
        got["aout"] = torch.full((nb * H * W, Cin), NAN, device="cuda", dtype=torch.bfloat16)
        ext.conv3x3_aout_arm(got["aout"])
    ext.conv3x3_gemm(_dev(d["xin"]), _dev(d["W"]), C, nb, H, W, Cin, Cout, stride, coef, epi, shift, acc, ex, emean,
                     ecoef)
    if epi:
        got["acc"] = _acc_sums(ws, Cout, epi == 1)
    return got, ref


@gpu
@pytest.mark.parametrize("case", C3_DMA + C3_HALO, ids=str)
def test_conv3x3_gemm_exact(case):
    got, ref = _conv3_run(*case)
    _assert_same(got, ref, str(case))


@gpu
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("case", C3_CFG, ids=str)
def test_conv3x3_gemm_forced_config_exact(case, cfg):
    _dispatch(core=1, cfg=cfg)
    got, ref = _conv3_run(*case)
    _assert_same(got, ref, f"cfg{cfg} {case}")


@gpu
@pytest.mark.parametrize("case", C3_REG, ids=str)
def test_conv3x3_gemm_register_core_exact(case):
    _dispatch(core=0)
    got, ref = _conv3_run(*case)
    _assert_same(got, ref, str(case))


@gpu
def test_conv3x3_gemm_halo_off_matches_the_same_reference():
    """The halo geometry on the implicit GEMM (set_halo3x3(0)): one reference, two kernels."""
    _ext().set_halo3x3(0)
    case = C3_HALO[1]
    got, ref = _conv3_run(*case)
    _assert_same(got, ref, f"halo off {case}")


# ================================================================ Tier 1: conv3x3_s2_dgrad
# nb, Hd, Wd, Cd, N, epi, odd: mc = nb Hd Wd rows per sub-pixel class, padded to whole tiles by the launcher
S2_CASES = ([(3, 7, 13, 64, 256, e, odd) for e in (0, 2) for odd in (False, True)] +   # mc = 273: ragged second tile
            [(2, 4, 6, 64, 256, e, odd) for e in (0, 2) for odd in (False, True)])     # mc = 48: below one tile


@functools.lru_cache(maxsize=None)
def _s2_ref(nb, Hd, Wd, Cd, N, epi, odd):
    Hx, Wx = (2 * Hd - 1, 2 * Wd - 1) if odd else (2 * Hd, 2 * Wd)
    Mdx = nb * Hx * Wx
    d = dict(_int_operands(Mdx, N, 9 * Cd, nb * Hd * Wd))
    dy = d["A"][:, :Cd]
    w = d["W"].view(N, 3, 3, Cd).permute(3, 0, 1, 2).contiguous()  # the conv weight [Cout = Cd, Cin = N, 3, 3]
    for r in range(3):
        for s in range(3):
            assert int((dy.abs() @ w[:, :, r, s].abs()).max()) * 4 < CAP
    dx = _ref_s2_dgrad(dy.view(nb, Hd, Wd, Cd), w, Hx, Wx).view(Mdx, N)
    d.update(dy=dy, w=w, Hx=Hx, Wx=Wx)
    return d, _ref_epilogue(dx, epi, d)


def _s2_run(nb, Hd, Wd, Cd, N, epi, odd):
    from kubedl_amd.ops.conv import s2_dgrad_weights
    d, ref = _s2_ref(nb, Hd, Wd, Cd, N, epi, odd)
    Mdx = nb * d["Hx"] * d["Wx"]
    ws = _ws(N)
    dx = torch.full((Mdx, N), NAN, device="cuda", dtype=torch.bfloat16)
    ball = s2_dgrad_weights(d["w"].float().cuda())
    acc = ex = emean = ecoef = None
    if epi == 2:
        ex, emean, acc = _dev(d["x"]), _fdev(d["mean"]), _views(ws, N)["bacc"]
        ecoef = torch.cat([d["ea"].double(), d["eb"]]).float().cuda()
    _ext().conv3x3_s2_dgrad(_dev(d["dy"]), ball, dx, nb, Hd, Wd, Cd, N, epi, acc, ex, emean, ecoef, d["Hx"], d["Wx"])
    got = {"C": dx}
    if epi:
        got["acc"] = _acc_sums(ws, N, False)
    return got, ref


@gpu
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("case", S2_CASES, ids=str)
def test_conv3x3_s2_dgrad_exact(case, cfg):
    """Every forced config and the by-shape pick.  MASKX with config 0 forced is the variant igemm() reroutes
    to 256x128 tiles (it computed wrong rows on 256x256): exact here, whichever tile serves it."""
    _dispatch(cfg=cfg)
    got, ref = _s2_run(*case)
    _assert_same(got, ref, f"cfg{cfg} {case}")


# ================================================================ Tier 1: weight gradients
# N, K, stride, pro, gpro
WG_SHAPES = [(64, 64), (128, 256), (256, 256)]
WG_CASES = [(N, K, s, p, False) for N, K in WG_SHAPES for s, p in ((1, False), (2, True), (1, True), (2, False))]
WG_GPRO = [(N, K, s, p, True) for N, K in WG_SHAPES for s, p in ((1, False), (1, True), (2, False))]
WG_GEOM = (3, 12, 9)      # the input images; stride 2 gives 6 x 5 outputs: M = 90 / 324, ragged last split
WG_MANY = (8, 28, 27)     # M = 6048: conv1x1_wgrad_splits > 16, ragged last split


@functools.lru_cache(maxsize=None)
def _wg1_ref(geom, N, K, stride, pro, gpro):
    nb, H, W = geom
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = nb * Ho * Wo
    d = dict(_int_operands(M, N, K, nb * H * W))
    a = d["A"]
    if pro:
        a = _ref_pro_fwd(a, d["psc"], d["psf"])
    a = _gather_rows(a, nb, H, W, stride)
    g = d["res"]  # [M, N] in -2..2
    if gpro:      # G' = k g + c1 gx + c0 per output channel, stored as bf16
        d["gk"], d["gc1"], d["gc0"] = d["ea"], d["mean"] - 1, d["shift"].clamp(-1, 1)
        g = _rne(d["gk"] * g + d["gc1"] * d["x"] + d["gc0"])
    assert int((g.abs().t() @ a.abs()).max()) < CAP
    d["M"] = M
    return d, g.t() @ a


def _wg1_run(geom, N, K, stride, pro, gpro, core, big=-1):
    ext = _ext()
    _dispatch(core=core, big=big)
    nb, H, W = geom
    d, ref = _wg1_ref(geom, N, K, stride, pro, gpro)
    M = d["M"]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    G, A = _dev(d["res"]), _dev(d["A"])
    coef = _fdev(torch.cat([d["psc"], d["psf"]])) if pro else None
    slabs = ext.conv1x1_wgrad_splits(M, N, K)
    if gpro:
        wsb = _ws(N)
        _views(wsb, N)["bcoef"].copy_(torch.stack([d["gk"], d["gc1"], d["gc0"]]).float())
        gx = _dev(d["x"])
    tag = f"wgrad {geom} N{N} K{K} s{stride} pro{pro} gpro{gpro} core{core} big{big}"
    for scale, bf in ((1.0, False), (1.0, True), (0.5, True)):
        dw32 = torch.full((slabs * N * K,), NAN, device="cuda")  # no initialisation required
        dW = torch.full((N, K), NAN, device="cuda", dtype=torch.bfloat16) if bf else None
        if gpro:
            ext.bn_bwd_pro_arm(gx, wsb, N, None)
        ext.conv1x1_wgrad(G, A, coef, dw32, dW, scale, M, N, K, Ho, Wo, H, W, stride)
        if bf:  # the RNE rounding of the exact sum, times the power-of-two scale
            _assert_same({"dW": dW}, {"dW": _rne(ref).double() * scale}, f"{tag} bf16 x{scale}")
        else:
            _assert_same({"dw32": dw32[:N * K].view(N, K)}, {"dw32": ref}, f"{tag} fp32")
    return slabs


@gpu
@pytest.mark.parametrize("core", [0, 1])
@pytest.mark.parametrize("case", WG_CASES, ids=str)
def test_conv1x1_wgrad_exact(case, core):
    _wg1_run(WG_GEOM, *case, core=core)


@gpu
@pytest.mark.parametrize("case", WG_GPRO, ids=str)
def test_conv1x1_wgrad_g_prologue_exact(case):
    _wg1_run(WG_GEOM, *case, core=1)


@gpu
@pytest.mark.parametrize("core,big", [(0, -1), (1, -1), (1, 2)])
@pytest.mark.parametrize("N,K", [(64, 64), (256, 256)])
def test_conv1x1_wgrad_many_splits_exact(N, K, core, big):
    """Tens of split-M slabs folded by every reduce group, a ragged last split; (256, 256) with
    set_wgrad_big(2) runs the 256 x 256 tiles."""
    _dispatch(core=core, big=big)
    nb, H, W = WG_MANY
    assert _ext().conv1x1_wgrad_splits(nb * H * W, N, K) > 16
    _wg1_run(WG_MANY, N, K, 1, False, False, core=core, big=big)


# nb, H, W, Cin, Cout, stride, pro
WG3_CASES = [(4, 12, 10, 64, 64, 1, False), (4, 9, 9, 128, 64, 2, False), (4, 7, 7, 256, 256, 1, False),
             (4, 13, 13, 256, 256, 2, False), (4, 12, 10, 64, 64, 1, True),
             (1, 56, 56, 64, 64, 1, False), (1, 56, 56, 64, 64, 1, True)]  # the last two: the halo kernel


@functools.lru_cache(maxsize=None)
def _wg3_ref(nb, H, W, Cin, Cout, stride, pro):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = nb * Ho * Wo
    d = dict(_int_operands(M, Cout, Cin, nb * H * W))
    a = _ref_pro_fwd(d["A"], d["psc"], d["psf"]) if pro else d["A"]
    p = _patches(a.view(nb, H, W, Cin), stride)
    g = d["res"]
    assert int((g.abs().t() @ p.abs()).max()) < CAP
    return d, g.t() @ p  # [Cout, 9 Cin] = OHWI


@gpu
@pytest.mark.parametrize("case", WG3_CASES, ids=str)
def test_conv3x3_wgrad_exact(case):
    """Both workspace sizes of test_dma_wgrad_3x3 (conv1x1_wgrad_splits: 128 tiles; conv3x3_wgrad_slabs: 256 tiles
    / the halo kernel's slabs), fp32 and bf16 outputs."""
    ext = _ext()
    nb, H, W, Cin, Cout, stride, pro = case
    d, ref = _wg3_ref(*case)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = nb * Ho * Wo
    G, A = _dev(d["res"]), _dev(d["A"])
    coef = _fdev(torch.cat([d["psc"], d["psf"]])) if pro else None
    for slabs in (ext.conv1x1_wgrad_splits(M, Cout, 9 * Cin), ext.conv3x3_wgrad_slabs(nb, H, W, Cin, Cout, stride)):
        for scale, bf in ((1.0, False), (0.5, True)):
            dw32 = torch.full((slabs * Cout * 9 * Cin,), NAN, device="cuda")
            dW = torch.full((Cout, 9 * Cin), NAN, device="cuda", dtype=torch.bfloat16) if bf else None
            ext.conv3x3_wgrad(G, A, coef, dw32, dW, scale, nb, H, W, Cin, Cout, stride)
            tag = f"wgrad3x3 {case} slabs {slabs}"
            if bf:
                _assert_same({"dW": dW}, {"dW": _rne(ref).double() * scale}, tag + " bf16")
            else:
                _assert_same({"dw32": dw32[:Cout * 9 * Cin].view(Cout, 9 * Cin)}, {"dw32": ref}, tag + " fp32")


GRAM_CASES = [(231, 64), (1001, 128), (231, 256), (3000, 512)]


@functools.lru_cache(maxsize=None)
def _gram_ref(M, K):
    d = _int_operands(M, 64, K)
    a = _ref_pro_fwd(d["A"], d["psc"], d["psf"])
    assert int((a.t() @ a).max()) < CAP
    return d, a.t() @ a, a.sum(0)


@gpu
@pytest.mark.parametrize("M,K", GRAM_CASES)
def test_conv1x1_gram_exact(M, K):
    """Q = a^T a and s = 1^T a of a = relu(X scale + shift): integers."""
    ext = _ext()
    d, Q, s = _gram_ref(M, K)
    ws = torch.full((ext.conv1x1_gram_floats(M, K),), NAN, device="cuda")
    ext.conv1x1_gram(_dev(d["A"]), _fdev(torch.cat([d["psc"], d["psf"]])), ws, M, K)
    _assert_same({"Q": ws[:K * K].view(K, K), "s": ws[K * K:K * K + K]}, {"Q": Q, "s": s}, f"gram {M}x{K}")


# ================================================================ Tier 2: the in-GEMM BN finalize
class _Layer:
    """One BN layer as the engine holds it: workspace, parameters, saved statistics, gradients, and the
    finalize descriptor in the workspace tail."""

    def __init__(self, C, pd, seed):
        g = torch.Generator().manual_seed(seed)
        self.C, self.pd = C, pd
        self.ws = _ws(C)
        self.gamma = (torch.rand(C, generator=g) + 0.5).to(pd).cuda()
        self.beta = torch.randn(C, generator=g).to(pd).cuda()
        self.rm = torch.randn(C, generator=g).cuda()
        self.rv = (torch.rand(C, generator=g) + 0.5).cuda()
        self.sm = torch.zeros(C, device="cuda")
        self.si = torch.ones(C, device="cuda")
        self.dg = torch.zeros(C, device="cuda", dtype=pd)
        self.db = torch.zeros(C, device="cuda", dtype=pd)
        self.v = _views(self.ws, C)
        _ext().bn_fin_desc(self.ws, self.gamma, self.beta, self.rm, self.rv, self.sm, self.si, self.dg, self.db, MOM,
                           EPS)

    def counters(self):
        off = REP * 4 * self.C + 5 * self.C + 32  # fin_desc_off(C) + the descriptor's 32 floats
        return self.ws[off:off + 64].view(torch.int32)

    def params(self):
        return {"gamma": self.gamma, "beta": self.beta, "rm": self.rm, "rv": self.rv}


def _ulps(a, b):
    """Largest distance in fp32 ulps between two fp32 tensors of equal sign pattern."""
    ia, ib = a.float().contiguous().view(torch.int32).long(), b.float().contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


RATIOS = {}


def _note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)


def _check_fwd_fin(tag, got, y64, gamma64, beta64, K64, rv64):
    """save_mean / save_invstd / running stats / scale | shift against the fp64 finalize of the stored output
    with the old running mean as K, at the bounds of test_fwd_finalize_external_shift_aliasing_running_mean."""
    ref = _ref_finalize(y64, gamma64, beta64, K64, rv64)
    _assert_finalize(got, ref, 1e-4, 1e-3)
    _close(got["rm"], 0.9 * K64 + 0.1 * y64.mean(0), 1e-4)
    for name, tol in (("mean", 1e-4), ("invstd", 1e-3), ("rm", 1e-4), ("rv", 1e-3), ("sc", 1e-4), ("sf", 1e-4)):
        err = (got[name].double().cpu() - ref[name]).abs()
        ratio = (err / (tol + tol * ref[name].abs())).max().item()
        _note("fwd " + name, ratio)
        print(f"fwd_fin[{tag}] {name} worst err/bound {ratio:.3f}")
    return ref


def _check_bwd_fin(tag, got, g64, x64, mean64, is64, gamma64, M, bf16, chain=1.0):
    """dgamma / dbeta at the bound of test_finalize_eval_vs_fp64 (the U_SUM chain bound, one fp32 product, half a
    bf16 ulp for bf16 parameters), k | c1 | c0 at the staged-finalize tests' 1e-4.  ``chain`` scales U_SUM
    where the add chain exceeds 2^8 (1.0 at every shape used here, see test_in_gemm_finalize_backward)."""
    xc = x64 - mean64
    ref_db, ref_dg = g64.sum(0), (g64 * xc).sum(0) * is64
    out_ulp = U_BF16 if bf16 else 0.0
    b_db = U_SUM * chain * g64.abs().sum(0) + out_ulp * ref_db.abs()
    b_dg = U_SUM * chain * (g64 * xc).abs().sum(0) * is64 + (U_F32 + out_ulp) * ref_dg.abs()
    e_db = (got["db"].double().cpu() - ref_db).abs()
    e_dg = (got["dg"].double().cpu() - ref_dg).abs()
    r_db = (e_db / b_db.clamp_min(1e-300)).max().item()
    r_dg = (e_dg / b_dg.clamp_min(1e-300)).max().item()
    print(f"bwd_fin[{tag}] dbeta worst err/bound {r_db:.3f} dgamma {r_dg:.3f}")
    _note("bwd dbeta", r_db)
    _note("bwd dgamma", r_dg)
    assert bool((e_db <= b_db).all()), f"{tag}: dbeta err/bound {r_db}"
    assert bool((e_dg <= b_dg).all()), f"{tag}: dgamma err/bound {r_dg}"
    k = gamma64 * is64
    c1 = -k * is64 * ref_dg / M
    c0 = -k * ref_db / M - c1 * mean64
    for name, got_c, ref_c in (("k", got["k"], k), ("c1", got["c1"], c1), ("c0", got["c0"], c0)):
        err = (got_c.double().cpu() - ref_c).abs()
        ratio = (err / (1e-4 + 1e-4 * ref_c.abs())).max().item()
        _note("bwd " + name, ratio)
        print(f"bwd_fin[{tag}] {name} worst err/bound {ratio:.3f}")
        _close(got_c, ref_c, 1e-4)


def _draw_rm(y64, seed):
    """A running mean within +-2 standard deviations of the batch mean of the conv output: the range
    test_fwd_finalize_external_shift_aliasing_running_mean documents for sums taken around K = running_mean."""
    g = torch.Generator().manual_seed(seed)
    mean, std = y64.mean(0), y64.std(0, unbiased=False)
    return (mean + (torch.rand(y64.shape[1], generator=g, dtype=torch.float64) * 2 - 1) * 2 * std).float()


def _fwd_got(L):
    return {"mean": L.sm.clone(), "invstd": L.si.clone(), "rm": L.rm.clone(), "rv": L.rv.clone(),
            "sc": L.v["fcoef"][0].clone(), "sf": L.v["fcoef"][1].clone()}


def _bwd_got(L):
    return {"dg": L.dg.clone(), "db": L.db.clone(), "k": L.v["bcoef"][0].clone(), "c1": L.v["bcoef"][1].clone(),
            "c0": L.v["bcoef"][2].clone()}


def _run_forward(tag, C, M, pd, launch, seed=1, integer=False):
    """``launch(y, shift, acc)`` runs the STATS GEMM into ``y`` [M, C].  Unarmed once to see the output's
    statistics, then armed twice on one layer with running_mean / running_var restored in between; every
    forward check of Tier 2 on the result.

    The two armed launches are compared bit for bit on integer data (``integer``: the caller rounded its
    operands, the running mean is rounded here, every replica sum is exact and so independent of the order in
    which the blocks' atomics arrive).  On float data three or more blocks may add into one replica slot
    (256x64 and 128x128 DMA tiles at M = 4231: blocks r, r + 32, r + 64 of 72 share a channel tile) and fp32
    addition does not associate, so there both launches are held to the fp64 bounds instead and their
    difference is printed."""
    ext = _ext()
    L = _Layer(C, pd, seed)
    y = torch.full((M, C), NAN, device="cuda", dtype=torch.bfloat16)
    launch(y, L.rm, _ws(C)[:REP * 2 * C])
    y64 = y.double().cpu()
    assert not y64.isnan().any()
    rm_old, rv_old = _draw_rm(y64, seed).cuda(), L.rv.clone()
    if integer:
        rm_old.round_()
        dd = y64 - rm_old.double().cpu()
        _budget(dd, dd * dd)
    L.rm.copy_(rm_old)
    L.v["bacc"].copy_(torch.randn(REP, 2, C))    # sentinels: the forward finalize must not touch them
    L.v["bcoef"].copy_(torch.randn(3, C))
    before = (L.v["bacc"].clone(), L.v["bcoef"].clone())
    runs = []
    for _ in range(2):
        L.rm.copy_(rm_old)
        L.rv.copy_(rv_old)
        y.fill_(NAN)
        ext.bn_fin_arm(L.ws, None, C, M)
        launch(y, L.rm, L.v["facc"])
        torch.cuda.synchronize()
        assert torch.equal(y.double().cpu(), y64), f"{tag}: the armed launch stored a different output"
        assert not L.v["facc"].any(), f"{tag}: forward replicas not re-zeroed"
        assert not L.counters().any(), f"{tag}: tile counters not back at zero"
        assert _bits_equal(L.v["bacc"], before[0]) and _bits_equal(L.v["bcoef"], before[1]), \
            f"{tag}: the forward finalize touched the backward replicas / coefficients"
        runs.append(_fwd_got(L))
    for name in runs[0]:
        if integer:
            assert _bits_equal(runs[0][name], runs[1][name]), f"{tag}: {name} differs between two identical launches"
        else:
            print(f"fwd_fin[{tag}] {name} run to run: {_ulps(runs[0][name], runs[1][name])} ulp")
    if not integer:
        for got in runs:
            _check_fwd_fin(tag, got, y64, L.gamma.double().cpu(), L.beta.double().cpu(), rm_old.double().cpu(),
                           rv_old.double().cpu())
    return L, y


def _prepare_backward(L, ex):
    """The forward of the layer whose backward the GEMM finalizes, on the same workspace, through the staged
    kernels: save_mean, save_invstd and scale | shift of ``ex`` (forward, then backward on one workspace)."""
    ext = _ext()
    M, C = ex.shape
    ext.bn_stage_fwd_stats(ex, L.ws, M, C)
    ext.bn_stage_fwd_finalize(ex, None, L.ws, M, C, L.gamma, L.beta, L.rm, L.rv, L.sm, L.si, True, MOM, EPS)
    L.v["facc"].copy_(torch.randn(REP, 2, C))    # sentinel: the backward finalize must not touch it
    return L.v["facc"].clone(), L.v["fcoef"].clone()


def _run_backward(tag, C, M, pd, launch, ex, ex2=None, fin_M=None, seed=2, integer=False):
    """``launch(g, L, L2)`` runs the MASKX / RESBITS GEMM into ``g`` [M, C] with L's (L2's) backward replicas,
    save_mean and scale | shift.  Armed twice; every backward check of Tier 2 on the result (``integer`` as in
    _run_forward: save_mean is rounded here, so that g' (x - mean) is an integer)."""
    ext = _ext()
    fin_M = fin_M or M
    L = _Layer(C, pd, seed)
    L2 = _Layer(C, pd, seed + 100) if ex2 is not None else None
    before = _prepare_backward(L, ex)
    before2 = _prepare_backward(L2, ex2) if L2 is not None else None
    if integer:
        for layer in (L, L2):
            if layer is not None:
                layer.sm.round_()
    g = torch.full((M, C), NAN, device="cuda", dtype=torch.bfloat16)
    runs = []
    for _ in range(2):
        g.fill_(NAN)
        ext.bn_fin_arm(L.ws, L2.ws if L2 is not None else None, C, fin_M)
        launch(g, L, L2)
        torch.cuda.synchronize()
        for layer, bef in ((L, before), (L2, before2)):
            if layer is None:
                continue
            assert not layer.v["bacc"].any(), f"{tag}: backward replicas not re-zeroed"
            assert not layer.counters().any(), f"{tag}: tile counters not back at zero"
            assert _bits_equal(layer.v["facc"], bef[0]) and _bits_equal(layer.v["fcoef"], bef[1]), \
                f"{tag}: the backward finalize touched the forward replicas / coefficients"
        runs.append((_bwd_got(L), _bwd_got(L2) if L2 is not None else None, g.clone()))
    assert not g.isnan().any()
    assert torch.equal(runs[0][2], runs[1][2])
    g64 = g.double().cpu()
    for a, b in ((runs[0][0], runs[1][0]), (runs[0][1], runs[1][1])):
        if a is not None:
            for name in a:
                if integer:
                    assert _bits_equal(a[name], b[name]), f"{tag}: {name} differs between two identical launches"
                else:
                    print(f"bwd_fin[{tag}] {name} run to run: {_ulps(a[name].float(), b[name].float())} ulp")
    for layer, x, sfx, i in ((L, ex, "", 0), (L2, ex2, ".2", 1)):
        if layer is None:
            continue
        x64, mean64 = x.double().cpu(), layer.sm.double().cpu()
        if integer:
            _budget(g64, g64 * (x64 - mean64))
            continue
        for run in runs:
            _check_bwd_fin(tag + sfx, run[i], g64, x64, mean64, layer.si.double().cpu(), layer.gamma.double().cpu(),
                           fin_M, pd == torch.bfloat16)
    return L, L2, g


def _float_gemm(M, N, K, seed, rows_in=0, integer=False):
    """Realistic GEMM operands; ``integer``: rounded to small integers (A in about -4..4, W in -1..1)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(rows_in or M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    if integer:
        return A.round().bfloat16().cuda(), W.round().clamp(-1, 1).bfloat16().cuda()
    return A.bfloat16().cuda(), (W / K ** 0.5).bfloat16().cuda()


def _float_act(M, C, seed, scale=2.0, shift=3.0, integer=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(M, C, generator=g) * scale + shift
    return (t.round() if integer else t).bfloat16().cuda()


def _coef(integer, *parts):
    """Per-channel fp32 coefficient rows on the GPU (``integer``: rounded)."""
    t = torch.cat(parts)
    return (t.round() if integer else t).float().cuda()


# entry, core, cfg, M, C, K: every forward entry point the engine arms
T2_FWD = ([("gemm", 0, -1, M, C, K) for M in (45, 4231) for C, K in REG_TILES] +
          [("gemm_pro", 0, -1, 231, 64, 128), ("gemm_res", 0, -1, 231, 64, 256), ("gemm_res2", 0, -1, 231, 128, 256)] +
          [("gemm", 1, cfg, M, 256, 512) for cfg in range(5) for M in (45, 4231)] +
          [("gemm", 1, 3, 231, 2048, 64)] +          # 32 N-tiles of 256x64: the last forward counter slot
          [("conv3", -1, -1, 231, 64, 64), ("conv3s2", -1, -1, 72, 128, 64), ("halo", -1, -1, 3136, 64, 64),
           ("halo_pro", -1, -1, 3136, 64, 64)])


@gpu
@pytest.mark.parametrize("data", ["float", "int"])
@pytest.mark.parametrize("pd", PDTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", T2_FWD, ids=str)
def test_in_gemm_finalize_forward(case, pd, data):
    """Epilogue STATS + fin_fwd_channel.  K = running_mean is read before it is updated in place: the reference
    takes the old value, and ``rm_new = 0.9 K + 0.1 mean`` is checked on its own.  ``float``: the fp64 bounds;
    ``int``: the same launches on rounded operands, where two armed launches are bit-identical."""
    ext = _ext()
    entry, core, cfg, M, C, K = case
    integer = data == "int"
    _dispatch(core=core, cfg=cfg)
    if entry.startswith("gemm"):
        A, W = _float_gemm(M, C, K, 17, integer=integer)
        pro = res = None
        if entry == "gemm_pro":
            pro = _coef(integer, torch.rand(K) + 0.5, torch.randn(K))
        if entry in ("gemm_res", "gemm_res2"):
            res = _float_act(M, K, 19, 1.0, 0.0, integer)
            coef = _coef(integer, torch.rand(K) + 0.5, torch.randn(K) * 0.5)
            coefd = _coef(integer, torch.rand(K) + 0.5, torch.randn(K) * 0.5) if entry == "gemm_res2" else None
            xout = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
            bits = torch.empty(M, K // 8, device="cuda", dtype=torch.uint8)

        def launch(y, shift, acc):
            if res is not None:
                ext.bn_res_pro_arm(res, coef, K, xout, bits, coefd)
            _gemm(A, W, y, M, C, K, pro_coef=pro, epi=1, shift=shift, acc=acc)
    else:
        nb, H, Wd, stride = {"conv3": (3, 7, 11, 1), "conv3s2": (3, 7, 11, 2)}.get(entry, (1, 56, 56, 1))
        A, W = _float_gemm(M, C, 9 * K, 23, rows_in=nb * H * Wd, integer=integer)
        A = A[:, :K].contiguous()
        pro = _coef(integer, torch.rand(K) + 0.5, torch.randn(K) * 0.5) if entry == "halo_pro" else None

        def launch(y, shift, acc):
            ext.conv3x3_gemm(A, W, y, nb, H, Wd, K, C, stride, pro, 1, shift, acc, None, None, None)
    _run_forward(str(case), C, M, pd, launch, integer=integer)


# entry, core, cfg, M, C, K
T2_BWD = ([("maskx", 0, -1, M, C, K) for M in (45, 4231) for C, K in REG_TILES] +
          [("resbits", 0, -1, M, C, K) for M in (45, 4231) for C, K in REG_TILES[:2]] +
          [("dual", 0, -1, 4231, 64, 128), ("dual", 0, -1, 45, 128, 512), ("dual", 1, 0, 4231, 256, 512)] +
          [("maskx_bwdpro", 0, -1, 231, 128, 512), ("resbits_bwdpro", 0, -1, 231, 128, 576),
           ("maskx_bwdpro", 0, -1, 231, 2048, 576)] +   # 32 N-tiles of 128x64: backward counter slot 63
          [(e, 1, cfg, M, 256, 512) for cfg in range(5) for e, M in (("maskx", 4231), ("resbits", 45))] +
          [("conv3", -1, -1, 231, 64, 64), ("halo", -1, -1, 3136, 64, 64),
           ("s2", -1, -1, 3 * 14 * 26, 256, 64), ("s2odd", -1, -1, 3 * 13 * 25, 256, 64)])


@gpu
@pytest.mark.parametrize("data", ["float", "int"])
@pytest.mark.parametrize("pd", PDTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", T2_BWD, ids=str)
def test_in_gemm_finalize_backward(case, pd, data):
    """Epilogues MASKX / RESBITS (single and dual) + fin_bwd_channel, against sums of the stored masked gradient.

    U_SUM assumes fewer than 2^8 chained fp32 adds per channel.  The epilogue's chain at M = 4231, the largest
    shape here (gemm_epi.h: CPR = BN / 8 chunks per row, RPP = threads / CPR rows per pass, NP = BM / RPP rows
    per thread per tile):

        tile      threads  RPP  NP
        128x128   256      16   8      (also the 32-deep config 5)
        128x64    256      32   4
        256x64    256      32   8
        256x128   512      32   8
        256x256   512      16   16

    times one tile per block (34 or 17 row tiles never exceed one round of resident blocks), then the RPP fold
    (16 or 32 adds), then the atomics of the blocks b = r (mod 32) that share a channel tile (at most 3: 72
    blocks on 128x128 / 256x64 at N = 256), then the finalize's 32 replicas: at most 16 + 32 + 3 + 32 = 83 adds.
    The halo kernel (224-pixel tiles, 448 threads, BN = 64: RPP 56, NP 4; 14 tiles on 14 blocks at M = 3136)
    chains 4 + 56 + 1 + 32 = 93 adds, the s2 dgrad (four classes of at most 3 tiles, one tile per block, fewer
    than 32 blocks) at most 16 + 32 + 1 + 32 = 81.  All below 2^8: ``chain`` = 1.0 everywhere.
    ``data`` as in test_in_gemm_finalize_forward."""
    ext = _ext()
    entry, core, cfg, M, C, K = case
    integer = data == "int"
    _dispatch(core=core, cfg=cfg)
    ex = _float_act(M, C, 29, integer=integer)
    ex2 = _float_act(M, C, 31, integer=integer) if entry == "dual" else None
    fin_M = M
    if entry in ("conv3", "halo"):
        nb, H, Wd = (3, 7, 11) if entry == "conv3" else (1, 56, 56)
        A, W = _float_gemm(M, C, 9 * K, 37, integer=integer)
        A = A[:, :K].contiguous()

        def launch(g, L, L2):
            ext.conv3x3_gemm(A, W, g, nb, H, Wd, K, C, 1, None, 2, None, L.v["bacc"], ex, L.sm, L.v["fcoef"].view(-1))
    elif entry in ("s2", "s2odd"):
        from kubedl_amd.ops.conv import s2_dgrad_weights
        nb, Hd, Wd = 3, 7, 13
        Hx, Wx = (2 * Hd - 1, 2 * Wd - 1) if entry == "s2odd" else (2 * Hd, 2 * Wd)
        gen = torch.Generator().manual_seed(41)
        dy, w = torch.randn(nb * Hd * Wd, K, generator=gen), torch.randn(K, C, 3, 3, generator=gen)
        dy = (dy.round() if integer else dy).bfloat16().cuda()
        ball = s2_dgrad_weights((w.round().clamp(-1, 1) if integer else w / (3 * K ** 0.5)).cuda())

        def launch(g, L, L2):
            ext.conv3x3_s2_dgrad(dy, ball, g, nb, Hd, Wd, K, C, 2, L.v["bacc"], ex, L.sm, L.v["fcoef"].view(-1), Hx, Wx)
    else:
        A, W = _float_gemm(M, C, K, 43, integer=integer)
        res = _float_act(M, C, 47, 1.0, 0.0, integer)
        gen = torch.Generator().manual_seed(53)
        mb = torch.randint(0, 256, (M, C // 8), generator=gen, dtype=torch.uint8).cuda()
        bwdpro = entry.endswith("bwdpro")
        if bwdpro:
            bx = _float_act(M, K, 59, integer=integer)
            wsb = _ws(K)
            bc = torch.randn(3, K, generator=gen)
            _views(wsb, K)["bcoef"].copy_(bc.round().clamp(-1, 1) if integer else bc * 0.5)

        def launch(g, L, L2):
            if bwdpro:
                ext.bn_bwd_pro_arm(bx, wsb, K, None)
            if entry.startswith("maskx"):
                _gemm(A, W, g, M, C, K, epi=2, ex=ex, emean=L.sm, ecoef=L.v["fcoef"].view(-1), acc=L.v["bacc"])
            else:
                kw = dict(ex2=ex2, emean2=L2.sm, acc2=L2.v["bacc"]) if L2 is not None else {}
                _gemm(A, W, g, M, C, K, epi=3, ex=ex, emean=L.sm, acc=L.v["bacc"], eres=res, ebits=mb, **kw)
    _run_backward(str(case), C, M, pd, launch, ex, ex2, fin_M, integer=integer)


@gpu
@pytest.mark.parametrize("pd", PDTYPES, ids=["f32", "bf16"])
def test_in_gemm_finalize_forward_then_backward_on_one_workspace(pd):
    """As in an engine step: the armed forward conv finalizes BN(y), the armed dgrad of the next layer masks by
    relu(BN(y)) and finalizes the same BN's backward from the statistics the first launch saved."""
    ext = _ext()
    _dispatch(core=0)
    M, C, K, N2 = 4231, 128, 64, 256
    A, W = _float_gemm(M, C, K, 61)

    def fwd(y, shift, acc):
        _gemm(A, W, y, M, C, K, epi=1, shift=shift, acc=acc)

    L, y = _run_forward("chain fwd", C, M, pd, fwd, seed=5)
    L.v["bacc"].zero_()  # (_run_forward left its sentinel there)
    fwd_state = (L.v["fcoef"].clone(), L.sm.clone(), L.si.clone())
    dy, Wt = _float_gemm(M, C, N2, 67)
    g = torch.full((M, C), NAN, device="cuda", dtype=torch.bfloat16)
    ext.bn_fin_arm(L.ws, None, C, M)
    _gemm(dy, Wt, g, M, C, N2, epi=2, ex=y, emean=L.sm, ecoef=L.v["fcoef"].view(-1), acc=L.v["bacc"])
    torch.cuda.synchronize()
    assert not L.v["bacc"].any() and not L.v["facc"].any() and not L.counters().any()
    assert _bits_equal(L.v["fcoef"], fwd_state[0]) and _bits_equal(L.sm, fwd_state[1]) and _bits_equal(L.si, fwd_state[2])
    _check_bwd_fin("chain bwd", _bwd_got(L), g.double().cpu(), y.double().cpu(), L.sm.double().cpu(),
                   L.si.double().cpu(), L.gamma.double().cpu(), M, pd == torch.bfloat16)


@gpu
@pytest.mark.parametrize("geom,N,K", [(G_MID, 64, 128), (G_BIG, 256, 1024)])
def test_armed_finalize_vs_staged_finalize_on_exact_sums(geom, N, K):
    """On Tier 1 data the replica contents are exact, so the armed launch and the unarmed launch followed by
    bn_stage_fwd_finalize / bn_stage_bwd_finalize start from identical sums: what differs is the finalize
    arithmetic alone (bn_fin.h: "the same fp32 expressions").  The difference is printed in ulps; the gate is
    the fp64 bound, which both results satisfy."""
    ext = _ext()
    _dispatch(core=0)
    nb, H, W = geom
    M = nb * H * W
    d, ref = _gemm1_ref(geom, N, K, 1, "")
    A, Wt = _dev(d["A"]), _dev(d["W"])
    y64 = ref["C"].double()
    rm0 = d["shift"].float()
    outs = []
    for armed in (True, False):
        L = _Layer(N, torch.float32, 3)
        L.rm.copy_(rm0)
        rv0 = L.rv.clone()
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        if armed:
            ext.bn_fin_arm(L.ws, None, N, M)
        _gemm(A, Wt, y, M, N, K, epi=1, shift=L.rm, acc=L.v["facc"])
        if not armed:
            ext.bn_stage_fwd_finalize(None, L.rm, L.ws, M, N, L.gamma, L.beta, L.rm, L.rv, L.sm, L.si, True, MOM, EPS)
        got = _fwd_got(L)
        _check_fwd_fin(f"int {'armed' if armed else 'staged'} {M}x{N}", got, y64, L.gamma.double().cpu(),
                       L.beta.double().cpu(), rm0.double(), rv0.double().cpu())
        # backward of the same layer: MASKX dgrad with ex = an integer tensor, exact sums again
        db_, refb = _gemm1_ref(geom, N, K, 2, "")
        g = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        if armed:
            ext.bn_fin_arm(L.ws, None, N, M)
        L.sm.copy_(db_["mean"].float())
        _gemm(A, Wt, g, M, N, K, epi=2, ex=_dev(db_["x"]), emean=L.sm,
              ecoef=torch.cat([db_["ea"].double(), db_["eb"]]).float().cuda(), acc=L.v["bacc"])
        if not armed:
            ext.bn_stage_bwd_finalize(L.ws, M, N, L.gamma, L.sm, L.si, L.dg, L.db, True)
        gotb = _bwd_got(L)
        _check_bwd_fin(f"int {'armed' if armed else 'staged'} {M}x{N}", gotb, refb["C"].double(), db_["x"].double(),
                       db_["mean"].double(), L.si.double().cpu(), L.gamma.double().cpu(), M, False)
        outs.append({**got, **gotb})
    for name in outs[0]:
        print(f"armed vs staged finalize [{M}x{N}] {name}: {_ulps(outs[0][name].float(), outs[1][name].float())} ulp")


@gpu
def test_in_gemm_finalize_rejected_arguments():
    """bn_fin_arm refuses C outside 64..2048 or C % 64 != 0; an armed GEMM refuses N != C, an epilogue without BN
    sums, and an ``acc`` / ``acc2`` that is not the armed workspace's replica block (the finalize would read
    zeros and write plausible coefficients).  A launch that raises also disarms."""
    ext = _ext()
    _dispatch(core=0)
    for C in (32, 2112, 96):
        with pytest.raises(RuntimeError, match="bn_fin_arm"):
            ext.bn_fin_arm(torch.zeros(ext.bn_workspace_floats(C), device="cuda"), None, C, 100)
    M, N, K = 231, 128, 64
    A, W = _float_gemm(M, N, K, 71)
    ex = _float_act(M, N, 73)
    res = _float_act(M, N, 79, 1.0, 0.0)
    mb = torch.zeros(M, N // 8, device="cuda", dtype=torch.uint8)
    y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    L, L2, Lo = _Layer(N, torch.float32, 7), _Layer(N, torch.float32, 8), _Layer(N, torch.float32, 9)
    L256 = _Layer(256, torch.float32, 10)
    sentinel = torch.randn(5, N, device="cuda")
    for layer in (L, L2, Lo):
        layer.v["fcoef"].copy_(sentinel[:2])
        layer.v["bcoef"].copy_(sentinel[2:])
    mask = dict(ex=ex, emean=L.sm, ecoef=torch.ones(2 * N, device="cuda"))
    rb = dict(ex=ex, emean=L.sm, eres=res, ebits=mb)
    bad = {
        "N != C": (L256, None, dict(epi=1, shift=L.rm, acc=L.v["facc"])),
        "epi 0": (L, None, dict(epi=0)),
        "epi 4": (L, None, dict(epi=4, eres=res)),
        "stats acc of another workspace": (L, None, dict(epi=1, shift=L.rm, acc=Lo.v["facc"])),
        "stats acc = backward block": (L, None, dict(epi=1, shift=L.rm, acc=L.v["bacc"].view(-1))),
        "maskx acc = forward block": (L, None, dict(epi=2, acc=L.v["facc"], **mask)),
        "maskx acc = whole workspace": (L, None, dict(epi=2, acc=L.ws, **mask)),
        "resbits acc2 of another workspace": (L, L2, dict(epi=3, acc=L.v["bacc"], ex2=ex, emean2=L2.sm,
                                                          acc2=Lo.v["bacc"], **rb)),
        "resbits ws2 armed without acc2": (L, L2, dict(epi=3, acc=L.v["bacc"], **rb)),
        "ws2 armed under maskx": (L, L2, dict(epi=2, acc=L.v["bacc"], **mask)),
    }
    for name, (layer, layer2, kw) in bad.items():
        ext.bn_fin_arm(layer.ws, layer2.ws if layer2 is not None else None, layer.C, M)
        with pytest.raises(RuntimeError, match="bn_fin_arm"):
            _gemm(A, W, y, M, N, K, **kw)
        # the refused launch disarmed: this one finalizes nothing
        _gemm(A, W, y, M, N, K, epi=1, shift=Lo.rm, acc=Lo.v["facc"])
        torch.cuda.synchronize()
        for lay in (L, L2, Lo):
            got = torch.cat([lay.v["fcoef"], lay.v["bcoef"]])
            assert _bits_equal(got, sentinel), f"{name}: a finalize ran after the refused launch"
        assert Lo.v["facc"].any() and not Lo.counters().any()
        Lo.v["facc"].zero_()
    # the 3x3 entry points go through the same check
    nb, H, Wd, Ci = 3, 7, 11, 64
    A3, W3 = _float_gemm(M, N, 9 * Ci, 83)
    ext.bn_fin_arm(L.ws, None, N, M)
    with pytest.raises(RuntimeError, match="bn_fin_arm"):
        ext.conv3x3_gemm(A3[:, :Ci].contiguous(), W3, y, nb, H, Wd, Ci, N, 1, None, 1, L.rm, Lo.v["facc"], None, None,
                         None)
    assert _bits_equal(torch.cat([L.v["fcoef"], L.v["bcoef"]]), sentinel)


# ================================================================ CPU self-checks (no GPU needed)
def _all_tier1_refs():
    for c in sorted(set(REG_CASES + DMA_CASES), key=_case_id):
        yield _case_id(c), functools.partial(_gemm1_ref, *c)
    for c in C3_DMA + C3_CFG + C3_REG + C3_HALO:
        yield str(c), functools.partial(_conv3_ref, *c)
    for c in S2_CASES:
        yield str(c), functools.partial(_s2_ref, *c)
    for c in WG_CASES + WG_GPRO:
        yield str(c), functools.partial(_wg1_ref, WG_GEOM, *c)
    for N, K in [(64, 64), (256, 256)]:
        yield f"many {N} {K}", functools.partial(_wg1_ref, WG_MANY, N, K, 1, False, False)
    for c in WG3_CASES:
        yield str(c), functools.partial(_wg3_ref, *c)
    for c in GRAM_CASES:
        yield str(c), functools.partial(_gram_ref, *c)


def test_cpu_every_tier1_case_keeps_its_sums_below_2_24():
    """Each reference asserts the condition while it is built (``_budget``, ``_mm``): building all of them is
    the check.  A badly chosen input fails here, loudly, and cannot weaken a comparison."""
    n = 0
    for name, build in _all_tier1_refs():
        build()
        n += 1
    assert n > 100


def _f64_nchw(rows, nb, H, W):
    return rows.double().view(nb, H, W, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("stride", [1, 2])
def test_cpu_int64_conv_references_match_fp64_convolutions(stride):
    nb, H, W, Cin, Cout = 3, 7, 11, 64, 128
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d = _int_operands(nb * Ho * Wo, Cout, 9 * Cin, nb * H * W)
    x = d["A"][:, :Cin]
    w = d["W"].view(Cout, 3, 3, Cin)
    w_oihw = w.permute(0, 3, 1, 2).double()
    x_nchw = _f64_nchw(x, nb, H, W)
    # 3x3 forward (patches x OHWI weights) and its weight gradient
    y = _mm(_patches(x.view(nb, H, W, Cin), stride), d["W"])
    assert torch.equal(_f64_nchw(y, nb, Ho, Wo), F.conv2d(x_nchw, w_oihw, stride=stride, padding=1))
    g = d["res"]
    dw = (g.t() @ _patches(x.view(nb, H, W, Cin), stride)).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(x_nchw, (Cout, Cin, 3, 3), _f64_nchw(g, nb, Ho, Wo), stride=stride, padding=1)
    assert torch.equal(dw.double(), ref)
    # 1x1 forward with the row gather, and its weight gradient
    w1 = d["W"][:, :Cin]
    y1 = _mm(_gather_rows(x, nb, H, W, stride), w1)
    assert torch.equal(_f64_nchw(y1, nb, Ho, Wo), F.conv2d(x_nchw, w1.double().view(Cout, Cin, 1, 1), stride=stride))
    dw1 = g.t() @ _gather_rows(x, nb, H, W, stride)
    ref1 = torch.nn.grad.conv2d_weight(x_nchw, (Cout, Cin, 1, 1), _f64_nchw(g, nb, Ho, Wo), stride=stride)
    assert torch.equal(dw1.double(), ref1.view(Cout, Cin))
    if stride == 1:
        # the stride-1 3x3 data gradient is the same implicit GEMM on the flipped, transposed weights
        wd = w_oihw.flip(2, 3).transpose(0, 1).permute(0, 2, 3, 1).reshape(Cin, 9 * Cout).long()
        dx = _mm(_patches(g.view(nb, H, W, Cout), 1), wd)
        refx = torch.nn.grad.conv2d_input((nb, Cin, H, W), w_oihw, _f64_nchw(g, nb, H, W), padding=1)
        assert torch.equal(_f64_nchw(dx, nb, H, W), refx)


@pytest.mark.parametrize("odd", [False, True])
def test_cpu_int64_s2_dgrad_reference_matches_fp64_conv2d_input(odd):
    from kubedl_amd.ops.conv import s2_dgrad_reference
    nb, Hd, Wd, Cd, N = 3, 7, 13, 64, 256
    d, ref = _s2_ref(nb, Hd, Wd, Cd, N, 0, odd)
    Hx, Wx = d["Hx"], d["Wx"]
    dy = _f64_nchw(d["dy"], nb, Hd, Wd)
    truth = torch.nn.grad.conv2d_input((nb, N, Hx, Wx), d["w"].double(), dy, stride=2, padding=1)
    dx = _ref_s2_dgrad(d["dy"].view(nb, Hd, Wd, Cd), d["w"], Hx, Wx)
    assert torch.equal(dx.double().permute(0, 3, 1, 2), truth)
    if not odd:  # and the sub-pixel class decomposition the kernel's weight layout follows
        assert torch.equal(s2_dgrad_reference(dy, d["w"].double()), truth)


def test_cpu_strided_residual_reference_matches_fp64_conv2d_input():
    """d(identity) of a stride-2 1x1 downsample input: the residual lands on rows (h % 2 == 0, w % 2 == 0), as
    conv2d_input of an identity 1x1 / stride 2 conv scatters it."""
    nb, H, W = G_MID
    N, K = 64, 128
    d, ref = _gemm1_ref(G_MID, N, K, 4, "rs2")
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    eye = torch.eye(N, dtype=torch.float64).view(N, N, 1, 1)
    scat = torch.nn.grad.conv2d_input((nb, N, H, W), eye, _f64_nchw(d["res_s"], nb, Ho, Wo), stride=2)
    y = _rne(_mm(d["A"], d["W"])).double()
    expect = y + scat.permute(0, 2, 3, 1).reshape(-1, N)   # |values| < 256: the bf16 re-rounding is exact
    assert int(expect.abs().max()) < 256
    assert torch.equal(ref["C"].double(), expect)


def _emu_fwd_fin(y, K, gamma, beta, rv, M):
    """fin_fwd_channel in plain fp32 torch."""
    d = y.float() - K
    s1, s2 = d.sum(0), (d * d).sum(0)
    inv_m = torch.tensor(1.0 / M)
    m1 = s1 * inv_m
    var = (s2 * inv_m - m1 * m1).clamp_min(0)
    mean = K + m1
    invstd = (var + EPS).rsqrt()
    unb = var * M / (M - 1) if M > 1 else var
    sc = gamma.float() * invstd
    return {"mean": mean, "invstd": invstd, "rm": (1 - MOM) * K + MOM * mean, "rv": (1 - MOM) * rv + MOM * unb, "sc": sc,
            "sf": beta.float() - mean * sc}


@pytest.mark.parametrize("pd", PDTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("M,C", [(45, 64), (4231, 256), (231, 2048)])
def test_cpu_fp32_emulation_of_both_finalizes_stays_inside_the_bounds(M, C, pd):
    """A plain fp32 implementation of fin_fwd_channel / fin_bwd_channel passes the Tier 2 checks."""
    g = torch.Generator().manual_seed(97 * M + C)
    y = torch.randn(M, C, generator=g).bfloat16()
    gamma = (torch.rand(C, generator=g) + 0.5).to(pd)
    beta = torch.randn(C, generator=g).to(pd)
    rv = torch.rand(C, generator=g) + 0.5
    K = _draw_rm(y.double(), 3)
    got = _emu_fwd_fin(y, K, gamma, beta, rv, M)
    _check_fwd_fin(f"emu {M}x{C}", got, y.double(), gamma.double(), beta.double(), K.double(), rv.double())
    x = (torch.randn(M, C, generator=g) * 2 + 3).bfloat16()
    gr = (torch.randn(M, C, generator=g) * (torch.rand(M, C, generator=g) > 0.5)).bfloat16()
    mean = x.float().mean(0)
    is_ = (x.float().var(0, unbiased=False) + EPS).rsqrt()
    a, b = gr.float().sum(0), (gr.float() * (x.float() - mean)).sum(0)
    dg, db = b * is_, a
    k = gamma.float() * is_
    c1 = -k * is_ * dg / M
    c0 = -k * db / M - c1 * mean
    gotb = {"dg": dg.to(pd), "db": db.to(pd), "k": k, "c1": c1, "c0": c0}
    _check_bwd_fin(f"emu {M}x{C}", gotb, gr.double(), x.double(), mean.double(), is_.double(), gamma.double(), M,
                   pd == torch.bfloat16)
