"""The inference epilogues of the conv GEMMs, ``bn_infer_coefs`` and ``head_eval`` against exact references.

* Tier 1 (the method of tests/test_gemm_epi_gpu.py): small-integer operands, integer ``scale`` in 1..2 and
  ``shift`` in -2..1, ``res`` in -2..2, outputs pre-filled with NaN, compared bit for bit with an int64
  reference that rounds where the kernel does -- the accumulator into the LDS tile, and the store.
* Identity: on realistic float data ``conv1x1_bn`` / ``conv3x3_bn`` equal, bit for bit, ``bn_stage_fwd_apply``
  run on the ``EPI_PLAIN`` output of the same GEMM with the same coefficients (csrc/gemm_epi.h nests the
  arithmetic as csrc/bn_act.hip bn_fwd_apply_kernel does).  The main loop and the tile do not depend on the
  epilogue, with one exception: the 56x56 / 64-channel 3x3 runs PLAIN on the halo kernel, which does not have
  the inference epilogues; there both sides are compared on the implicit GEMM (``set_halo3x3(0)``).
* ``bn_infer_coefs`` against fp64 with bounds counted from its roundings; ``head_eval`` against
  ``head_forward`` (loss rows bit-equal), the tie rule applied in torch to its own logits, exact counts.
* CPU self-checks: the 2^24 condition of every Tier 1 case and the int64 reference against an fp64 composition.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_bn_stage_gpu import _bits_equal, _views, _ws
from test_gemm_epi_gpu import (CAP, G_BIG, G_LONG, G_MID, G_SMALL, NAN, _assert_same, _dev, _ext, _fdev, _gather_rows,
                               _gemm, _int_operands, _patches, _rne)

gpu = pytest.mark.gpu
EPI_BN, EPI_BN_RELU, EPI_BN_RES_RELU = 7, 8, 9
EPIS = (EPI_BN, EPI_BN_RELU, EPI_BN_RES_RELU)


@pytest.fixture(autouse=True)
def _restore_dispatch():
    yield
    if torch.cuda.is_available():
        ext = _ext()
        ext.set_gemm_core(-1)
        ext.set_igemm_cfg(-1)
        ext.set_halo3x3(1)


# ---------------------------------------------------------------- cases
# (geom, N, K, epi, s2)
REG_CASES = [(g, N, K, e, False) for g in (G_MID, G_SMALL) for N, K in [(64, 128), (128, 64), (128, 512)]
             for e in EPIS]
REG_CASES += [(G_MID, N, K, e, True) for N, K in [(64, 128), (128, 64), (128, 512)] for e in (EPI_BN, EPI_BN_RELU)]
DMA_CASES = [(g, N, K, e, False) for g, N, K in [(G_LONG, 256, 512), (G_MID, 256, 512), (G_BIG, 256, 1024),
                                                 (G_BIG, 2048, 512)] for e in EPIS]
DMA_CASES += [(G_LONG, 256, 512, e, True) for e in (EPI_BN, EPI_BN_RELU)]
# the LDS-DMA configs the inference epilogues are instantiated for, and what a forced config runs
# (csrc/igemm.hip igemm_infer_cfg: the three-stage config 4 runs on its two-stage twin, config 1)
CFG_RUNS = {0: 0, 1: 1, 2: 2, 3: 3, 4: 1}
CFG_CASES = [(G_LONG, 256, 512, e, False) for e in EPIS] + [(G_LONG, 256, 512, EPI_BN, True)]
# nb, H, W, Cin, Cout, stride (all with EPI_BN_RELU); the last is the halo geometry
C3_CASES = [(3, 7, 11, 64, 64, 1), (2, 5, 3, 128, 128, 2), (2, 9, 9, 64, 128, 2), (1, 56, 56, 64, 64, 1)]


def _case_id(c):
    (nb, H, W), N, K, epi, s2 = c
    return f"{nb}x{H}x{W}-N{N}-K{K}-epi{epi}{'-s2' if s2 else ''}"


def _mm(a, w):
    """[M, K] x [N, K]^T of small integers through fp64 (exact: every sum is far below 2^53), with Tier 1's
    condition asserted: the sum of absolute terms of every accumulator stays below 2^24."""
    assert float((a.abs().double() @ w.abs().double().t()).max()) < CAP
    return (a.double() @ w.double().t()).long()


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, rows_in=0):
    d = dict(_int_operands(M, N, K, rows_in))
    g = torch.Generator().manual_seed(104729 * M + 17 * N + K)
    d["bsc"] = torch.randint(1, 3, (N,), generator=g)    # scale in 1..2
    d["bsf"] = torch.randint(-2, 2, (N,), generator=g)   # shift in -2..1
    return d


def _ref_bn(acc, epi, d):
    """csrc/gemm_epi.h EPI_BN*: the accumulator rounded to bf16 into the LDS tile, then
    relu(y scale + shift + res) in exact integers, rounded once at the store."""
    y = _rne(acc)
    o = y * d["bsc"] + d["bsf"]
    worst = y.abs() * d["bsc"].abs() + d["bsf"].abs()
    if epi == EPI_BN_RES_RELU:
        o = o + d["res"]
        worst = worst + d["res"].abs()
    assert int(worst.max()) < CAP
    if epi != EPI_BN:
        o = o.clamp_min(0)
    return _rne(o)


@functools.lru_cache(maxsize=None)
def _gemm_ref(geom, N, K, epi, s2):
    nb, H, W = geom
    M = nb * H * W
    Hin, Win = (2 * H - 1, 2 * W) if s2 else (H, W)
    d = dict(_operands(M, N, K, nb * Hin * Win if s2 else 0))
    a = _gather_rows(d["A"], nb, Hin, Win, 2) if s2 else d["A"]
    d.update(Hin=Hin, Win=Win)
    return d, {"C": _ref_bn(_mm(a, d["W"]), epi, d)}


def _coef(d):
    return _fdev(torch.cat([d["bsc"], d["bsf"]]))


def _gemm_run(geom, N, K, epi, s2):
    nb, H, W = geom
    M = nb * H * W
    d, ref = _gemm_ref(geom, N, K, epi, s2)
    C = torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16)
    _ext().conv1x1_bn(_dev(d["A"]), _dev(d["W"]), C, M, N, K, H, W, d["Hin"], d["Win"], 2 if s2 else 1, _coef(d),
                      epi != EPI_BN, _dev(d["res"]) if epi == EPI_BN_RES_RELU else None)
    return {"C": C}, ref


@functools.lru_cache(maxsize=None)
def _conv3_ref(nb, H, W, Cin, Cout, stride):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d = dict(_operands(nb * Ho * Wo, Cout, 9 * Cin, nb * H * W))
    d["xin"] = d["A"][:, :Cin]
    acc = _mm(_patches(d["xin"].reshape(nb, H, W, Cin), stride), d["W"])
    return d, {"C": _ref_bn(acc, EPI_BN_RELU, d)}


def _conv3_run(nb, H, W, Cin, Cout, stride):
    d, ref = _conv3_ref(nb, H, W, Cin, Cout, stride)
    M = ref["C"].shape[0]
    C = torch.full((M, Cout), NAN, device="cuda", dtype=torch.bfloat16)
    _ext().conv3x3_bn(_dev(d["xin"]), _dev(d["W"]), C, nb, H, W, Cin, Cout, stride, _coef(d), True)
    return {"C": C}, ref


# ================================================================ CPU self-check (issue item 7)
def test_cpu_every_infer_case_keeps_its_sums_below_2_24_and_matches_fp64():
    """Every Tier 1 case below satisfies the 2^24 condition (asserted while the reference is built), and the
    int64 reference equals the fp64 composition relu(conv scale + shift + res) -- conv rounded to bf16 as the
    LDS tile holds it -- rounded once to bf16."""
    def check(x_nhwc, w_oihw, stride, pad, d, epi, ref):
        conv = F.conv2d(x_nhwc.permute(0, 3, 1, 2).double(), w_oihw.double(), stride=stride, padding=pad)
        conv = conv.permute(0, 2, 3, 1).reshape(-1, w_oihw.shape[0])
        o = conv.float().bfloat16().double() * d["bsc"].double() + d["bsf"].double()
        if epi == EPI_BN_RES_RELU:
            o = o + d["res"].double()
        if epi != EPI_BN:
            o = o.clamp_min(0)
        assert torch.equal(o.float().bfloat16().double(), ref["C"].double())

    for case in sorted(set(REG_CASES + DMA_CASES + CFG_CASES), key=_case_id):
        (nb, H, W), N, K, epi, s2 = case
        d, ref = _gemm_ref(*case)
        check(d["A"].view(nb, d["Hin"], d["Win"], K), d["W"].view(N, K, 1, 1), 2 if s2 else 1, 0, d, epi, ref)
    for nb, H, W, Cin, Cout, stride in C3_CASES:
        d, ref = _conv3_ref(nb, H, W, Cin, Cout, stride)
        w = d["W"].view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
        check(d["xin"].reshape(nb, H, W, Cin), w, stride, 1, d, EPI_BN_RELU, ref)


# ================================================================ Tier 1 on the GPU (issue item 8)
@gpu
@pytest.mark.parametrize("case", REG_CASES, ids=_case_id)
def test_conv1x1_bn_register_core_exact(case):
    ext = _ext()
    ext.set_gemm_core(0)
    got, ref = _gemm_run(*case)
    _assert_same(got, ref, _case_id(case))
    assert ext.gemm_last_launch() == [0, 0 if case[1] % 128 == 0 else 1]


@gpu
@pytest.mark.parametrize("case", DMA_CASES, ids=_case_id)
def test_conv1x1_bn_lds_dma_core_exact(case):
    ext = _ext()
    ext.set_gemm_core(1)
    got, ref = _gemm_run(*case)
    _assert_same(got, ref, _case_id(case))
    assert ext.gemm_last_launch()[0] == 1


@gpu
@pytest.mark.parametrize("cfg", sorted(CFG_RUNS))
@pytest.mark.parametrize("case", CFG_CASES, ids=_case_id)
def test_conv1x1_bn_forced_config_runs_and_is_exact(case, cfg):
    """A forced LDS-DMA config the inference epilogues are instantiated for is the one that runs; config 4
    (not instantiated) runs the documented fallback, config 1 -- it does not fail."""
    ext = _ext()
    ext.set_gemm_core(1)
    ext.set_igemm_cfg(cfg)
    got, ref = _gemm_run(*case)
    _assert_same(got, ref, f"cfg{cfg} {_case_id(case)}")
    assert ext.gemm_last_launch() == [1, CFG_RUNS[cfg]]


@gpu
@pytest.mark.parametrize("case", C3_CASES, ids=str)
def test_conv3x3_bn_exact(case):
    got, ref = _conv3_run(*case)
    _assert_same(got, ref, str(case))
    assert _ext().gemm_last_launch()[0] == 1  # the implicit GEMM (the halo kernel does not have these epilogues)


@gpu
def test_conv3x3_bn_forced_configs_exact():
    ext = _ext()
    for cfg, runs in sorted(CFG_RUNS.items()):
        if cfg == 0:
            continue  # N = 128: the 256-wide tile does not divide it (falls back to the by-shape pick)
        ext.set_igemm_cfg(cfg)
        got, ref = _conv3_run(*C3_CASES[2])
        _assert_same(got, ref, f"cfg{cfg}")
        assert ext.gemm_last_launch() == [1, runs]


@gpu
def test_inference_calls_consume_and_refuse_pending_armings():
    """An arming left by a training call never leaks through an inference conv into the next training GEMM."""
    ext = _ext()
    case = (G_SMALL, 64, 128, EPI_BN_RELU, False)
    d, ref = _gemm_ref(*case)
    M, N, K = 45, 64, 128
    ws = _ws(N)
    A, W = _dev(d["A"]), _dev(d["W"])
    C = torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16)

    def call():
        ext.conv1x1_bn(A, W, C, M, N, K, 5, 9, 5, 9, 1, _coef(d), True, None)

    ext.bn_fin_arm(ws, None, N, M)
    with pytest.raises(RuntimeError, match="bn_fin_arm"):
        call()
    ext.bn_bwd_pro_arm(torch.zeros(M, K, device="cuda", dtype=torch.bfloat16), _ws(K), K, None)
    with pytest.raises(RuntimeError, match="pro_arm"):
        call()
    ext.conv3x3_aout_arm(torch.zeros(M, K, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="aout_arm"):
        call()
    call()  # every arming was consumed by the refused call
    _assert_same({"C": C}, ref, "after the refusals")
    # ... and none reaches a training GEMM: PLAIN with a pending finalize would be refused by the binding
    P = torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16)
    _gemm(A, W, P, M, N, K)
    assert not P.isnan().any()


# ================================================================ identity with the two-pass path (issue item 9)
def _float_case(M, N, K, rows_in, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(rows_in, K, generator=g).to(torch.bfloat16).cuda()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).cuda()
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).cuda()
    coef = torch.cat([torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.3]).cuda()
    return A, W, res, coef


def _two_pass(plain, coef, res, relu):
    M, N = plain.shape
    ws = _ws(N)
    _views(ws, N)["fcoef"].copy_(coef.view(2, N))
    y = torch.full_like(plain, NAN)
    _ext().bn_stage_fwd_apply(plain, ws, res, None, None, y, None, M, N, relu)
    return y


MODES = [(False, False), (True, False), (True, True)]  # (relu, res): res requires relu


@gpu
@pytest.mark.parametrize("core,case", [(0, c) for c in REG_CASES if c[3] == EPI_BN] +
                         [(1, c) for c in DMA_CASES if c[3] == EPI_BN],
                         ids=lambda v: _case_id(v) if isinstance(v, tuple) else f"core{v}")
def test_conv1x1_bn_equals_plain_gemm_then_bn_apply_bitwise(core, case):
    ext = _ext()
    ext.set_gemm_core(core)
    (nb, H, W), N, K, _, s2 = case
    M = nb * H * W
    Hin, Win = (2 * H - 1, 2 * W) if s2 else (H, W)
    A, Wt, res, coef = _float_case(M, N, K, nb * Hin * Win, 31 * M + N + K)
    plain = torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16)
    _gemm(A, Wt, plain, M, N, K, Hout=H, Wout=W, Hin=Hin, Win=Win, stride=2 if s2 else 1)
    for relu, with_res in MODES:
        if with_res and s2:
            continue
        r = res if with_res else None
        C = torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16)
        ext.conv1x1_bn(A, Wt, C, M, N, K, H, W, Hin, Win, 2 if s2 else 1, coef, relu, r)
        assert not C.isnan().any()
        assert _bits_equal(C, _two_pass(plain, coef, r, relu)), f"relu={relu} res={with_res}"


@gpu
@pytest.mark.parametrize("case", C3_CASES, ids=str)
def test_conv3x3_bn_equals_plain_conv_then_bn_apply_bitwise(case):
    ext = _ext()
    nb, H, W, Cin, Cout, stride = case
    ext.set_halo3x3(0)  # the halo geometry: both sides on the implicit GEMM (see the module docstring)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = nb * Ho * Wo
    A, Wt, _, coef = _float_case(M, Cout, 9 * Cin, nb * H * W, 7 * M + Cout)
    A = A[:, :Cin].contiguous()
    plain = torch.full((M, Cout), NAN, device="cuda", dtype=torch.bfloat16)
    ext.conv3x3_gemm(A, Wt, plain, nb, H, W, Cin, Cout, stride, None, 0, None, None, None, None, None)
    C = torch.full((M, Cout), NAN, device="cuda", dtype=torch.bfloat16)
    ext.conv3x3_bn(A, Wt, C, nb, H, W, Cin, Cout, stride, coef, True)
    assert not C.isnan().any()
    assert _bits_equal(C, _two_pass(plain, coef, None, True))


# ================================================================ bn_infer_coefs (issue item 10)
@gpu
def test_bn_infer_coefs_against_fp64():
    """With u = 2^-24 (fp32 unit roundoff), scale = fl(gamma fl(rsqrt(fl(var + eps)))): the rounding of
    var + eps (relative u) is halved by the root (u / 2), the reciprocal root is within 1 ulp (2u), the
    product rounds once (u): |scale - ref| <= 4u |ref| to first order.  shift = beta - mean scale, as two
    roundings or one fused: the product carries scale's 4u plus its own u, the subtraction one more u on the
    result, |result| <= |beta| + |mean scale|: |shift - ref| <= 5u (|beta| + |mean scale|) -- with one more u of
    headroom taken by neither: the bound is asserted as stated."""
    ext = _ext()
    u = 2.0 ** -24
    eps = 1e-5
    g = torch.Generator().manual_seed(5)
    Cs = [64, 256, 2048, 64, 512]
    pdt = [torch.float32, torch.bfloat16, torch.float32, torch.bfloat16, torch.bfloat16]
    layers = []
    for C, dt in zip(Cs, pdt):
        gamma = (torch.rand(C, generator=g) + 0.5).to(dt).cuda()
        beta = (torch.randn(C, generator=g) * 0.3).to(dt).cuda()
        mean = (torch.randn(C, generator=g) * 2).cuda()
        var = (10.0 ** (torch.rand(C, generator=g) * 9 - 6)).cuda()  # 1e-6 .. 1e3
        layers.append((gamma, beta, mean, var))
    layers[3] = (None, None) + layers[3][2:]  # a BN without affine parameters: gamma 1, beta 0
    table, n = ext.bn_infer_table(layers)
    offs = table[:, 5].tolist()
    assert all(o % 4 == 0 for o in offs) and n >= offs[-1] + 2 * Cs[-1]
    pad = 64
    buf = torch.full((n + pad,), NAN, device="cuda")
    ext.bn_infer_coefs(table, buf[:n], eps)
    written = torch.zeros(n + pad, dtype=torch.bool)
    for (gamma, beta, mean, var), C, off in zip(layers, Cs, offs):
        g64 = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device="cuda")
        b64 = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64, device="cuda")
        sc = g64 / torch.sqrt(var.double() + eps)
        sf = b64 - mean.double() * sc
        got_sc, got_sf = buf[off:off + C].double(), buf[off + C:off + 2 * C].double()
        r1 = ((got_sc - sc).abs() / (4 * u * sc.abs())).max().item()
        r2 = ((got_sf - sf).abs() / (5 * u * (b64.abs() + (mean.double() * sc).abs()))).max().item()
        print(f"C={C}: scale err / bound {r1:.3f}, shift err / bound {r2:.3f}")
        assert r1 <= 1.0 and r2 <= 1.0
        written[off:off + 2 * C] = True
    assert buf.cpu()[~written].isnan().all(), "bytes between the slices / past the end were written"
    assert not buf.cpu()[written].isnan().any()
    # a buffer too small for the last slice: that row writes nothing (no out-of-bounds store)
    small = torch.full((n,), NAN, device="cuda")
    ext.bn_infer_coefs(table, small[:offs[-1] + 8], eps)
    assert small[offs[-1]:].isnan().all() and not small[:offs[-1]].isnan().all()


# ================================================================ head_eval (issue item 11)
def _rank_rule(z, y):
    L = z.shape[1]
    ok = (y >= 0) & (y < L)
    out = []
    for n in range(z.shape[0]):
        if not ok[n]:
            out.append(L)
            continue
        yn = int(y[n])
        zy = z[n, yn]
        out.append(int((z[n] > zy).sum()) + int((z[n, :yn] == zy).sum()))
    return torch.tensor(out, dtype=torch.int32)


def _head_bufs(ext, Nb, C, L):
    s1, _ = ext.head_splits(Nb, C, L)
    return dict(feat=torch.empty(Nb, C, device="cuda", dtype=torch.bfloat16), part1=torch.empty(s1 * Nb * L, device="cuda"),
                lrow=torch.full((Nb,), NAN, device="cuda"), rank=torch.full((Nb,), -1, device="cuda", dtype=torch.int32),
                logits=torch.full((Nb, L), NAN, device="cuda"))


def _head_eval(ext, x, w, b, y, totals):
    Nb, C = x.shape[:2]
    o = _head_bufs(ext, Nb, C, w.shape[0])
    ext.head_eval(x, w, b, y, o["feat"], o["part1"], o["lrow"], o["rank"], o["logits"], totals)
    return o


@gpu
@pytest.mark.parametrize("Nb,C,L,HW", [(8, 2048, 1000, 49), (3, 512, 10, 16), (65, 64, 1000, 1)])
def test_head_eval_matches_head_forward_and_the_rank_rule(Nb, C, L, HW):
    ext = _ext()
    g = torch.Generator().manual_seed(Nb + C + L)
    hw = int(HW ** 0.5)
    Np = (Nb + 7) // 8 * 8  # head_forward's workspace rows (the Nb % 8 rule of its backward)
    xp = torch.randn(Np, hw, hw, C, generator=g).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)
    w = (torch.randn(L, C, generator=g) / C ** 0.5).to(torch.bfloat16).cuda()
    b = (torch.randn(L, generator=g) * 0.1).to(torch.bfloat16).cuda()
    yp = torch.randint(0, L, (Np,), generator=g).cuda()
    x, y = xp[:Nb], yp[:Nb].contiguous()
    totals = torch.zeros(4, dtype=torch.float64, device="cuda")
    o = _head_eval(ext, x, w, b, y, totals)
    o2 = _head_eval(ext, x, w, b, y, totals)
    torch.cuda.synchronize()
    for k in ("lrow", "rank", "logits"):
        assert _bits_equal(o[k], o2[k]) if o[k].dtype != torch.int32 else torch.equal(o[k], o2[k]), k
    # loss rows: bit-equal to the training head's
    s1, _ = ext.head_splits(Np, C, L)
    lrow = torch.empty(Np, device="cuda")
    ext.head_forward(xp, w, b, yp, torch.empty(Np, C, device="cuda", dtype=torch.bfloat16),
                     torch.empty(s1 * Np * L, device="cuda"), lrow,
                     torch.empty(Np, ext.head_lpad(L), device="cuda", dtype=torch.bfloat16),
                     torch.empty(L, Np, device="cuda", dtype=torch.bfloat16))
    assert _bits_equal(o["lrow"], lrow[:Nb])
    # logits: the existing head test's fp32 comparison
    feat = x.float().mean((2, 3))
    ref = feat @ w.float().t() + b.float()
    scale = ref.abs().max().item()
    torch.testing.assert_close(o["logits"], ref, atol=1e-2 * scale, rtol=2e-2)
    # the rank rule, applied to the kernel's own logits
    z = o["logits"].cpu()
    rank = _rank_rule(z, y.cpu())
    assert torch.equal(o["rank"].cpu(), rank)
    # totals after two calls
    t = totals.cpu()
    lsum = 2 * o["lrow"].cpu().double().sum().item()
    assert abs(t[0].item() - lsum) <= Nb * 2.0 ** -53 * abs(lsum)
    assert t[1].item() == 2 * int((rank < 1).sum()) and t[2].item() == 2 * int((rank < 5).sum())
    assert t[3].item() == 2 * Nb


@gpu
def test_head_eval_integer_ties_and_out_of_range_label():
    """Integer features and weights: the logits are exact small integers with many ties, so the top-1 / top-5
    counts are known exactly; one label is out of range (loss NaN, rank L, never a wild read)."""
    ext = _ext()
    Nb, C, L = 11, 64, 40
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-1, 2, (Nb, 1, 1, C), generator=g).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)
    w = torch.randint(-1, 2, (L, C), generator=g)
    w[1] = w[0]   # exact ties between classes 0, 1 and L - 1
    w[L - 1] = w[0]
    wd = w.to(torch.bfloat16).cuda()
    y = torch.randint(0, L, (Nb,), generator=g)
    y[0], y[1], y[2], y[3], y[4] = 0, 1, L - 1, L + 5, -100
    totals = torch.zeros(4, dtype=torch.float64, device="cuda")
    o = _head_eval(ext, x, wd, None, y.cuda(), totals)
    z = (x.float().cpu().reshape(Nb, C).long() @ w.t()).float()
    assert torch.equal(o["logits"].cpu(), z)
    rank = _rank_rule(z, y)
    assert torch.equal(o["rank"].cpu(), rank)
    assert rank[3] == L and rank[4] == L and o["lrow"][3].isnan() and o["lrow"][4].isnan()
    assert not o["lrow"].cpu()[[0, 1, 2] + list(range(5, Nb))].isnan().any()
    t = totals.cpu()
    assert t[1].item() == int((rank < 1).sum()) and t[2].item() == int((rank < 5).sum()) and t[3].item() == Nb
    assert t[0].isnan()  # the out-of-range labels turn the loss sum NaN, loudly
