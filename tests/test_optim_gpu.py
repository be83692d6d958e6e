"""The update path -- csrc/optim.hip (``sgd_chunk_kernel``, ``adam_chunk_kernel``, ``sumsq_chunk_kernel``,
``cast_copy_kernel``), ``pack_kernel`` of csrc/multi_tensor.hip and their drivers in kubedl_amd/ops/optim.py --
against fp64 references with derived bounds, and bit for bit wherever the result is exact.

* Bounded: ``|got - ref64| <= R * 2^-24 * A``.  ``ref64`` is the formula in fp64 on the kernel's own fp32 / bf16
  inputs (hyper-parameters rounded to fp32 first, as ``make_hyper`` does; ``bc1`` / ``bc2`` computed in double and
  then rounded, as ``adam_step`` does).  ``A`` is the same expression with every term replaced by its absolute
  value, and ``R`` counts the fp32 roundings of the unfused path to that output (``ref_sgd`` / ``ref_adam`` count
  them).  Fusing into ``fmaf`` only removes roundings.  Multi-step tests are teacher-forced: step k+1 of the
  reference starts from the kernel's own step-k buffers, so error does not accumulate and a failure names its step.
* Exact: the parameter store (``param == master.to(param.dtype)``, round-to-nearest-even for bf16), everything
  outside the chunk table, ``grad``, ``cast_copy`` and ``pack_kernel`` are compared bit for bit.
* CPU self-checks (no ``gpu`` marker, no extension): a plain unfused fp32 implementation stays inside the bounds
  on the very inputs the GPU tests use, mutants of the references leave them, and the chunk tables tile the slots.

The bound tests print their worst ``error / bound`` ratio (``pytest -rA`` shows them).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24  # one fp32 rounding, relative (half an ulp)

# R: fp32 roundings per output on the unfused path (counted in ref_sgd / ref_adam / _sumsq_bound)
R_SGD_MOM, R_SGD_W = 6, 11
R_ADAM_M1, R_ADAM_M2, R_ADAM_W = 6, 6, 18

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
DT = {"f32": F32, "bf16": BF16}

SGD_H = dict(lr=0.05, momentum=0.9, dampening=0.1, grad_scale=0.125,
             wd=[0.05, 0.0, 0.01, 0.002], lr_scale=[1.0, 0.5, 2.0, 0.25])
ADAM_H = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.125,
              wd=[0.1, 0.0, 0.01, 0.05], lr_scale=[1.0, 0.5, 2.0, 0.25])
ADAM_STEPS = [1, 2, 1000]


def _ext():
    from kubedl_amd.ops import _ext
    return _ext.load()


def _f32(x):
    return float(np.float32(x))


def _round_up(x, a):
    return (x + a - 1) // a * a


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _np64(t):
    return t.detach().cpu().double().numpy()


# ---------------------------------------------------------------- references
def ref_sgd(g, w, b, hyper, group_of_element, mutant=None):
    """``sgd_chunk_kernel`` in fp64 with ``torch.optim.SGD`` semantics: {"mom": (value, A), "master": (value, A)}.

    Roundings of the unfused fp32 path, per element (``1 - dampening`` and ``lr * lr_scale`` are per-launch scalars):
      gk  = g*grad_scale (1) + wd*w (2)                    -> add (3)
      bk  = momentum*b (4) + (1-dampening)*gk (5)          -> add (6)                 R_SGD_MOM = 6
      upd = gk + momentum*bk : mul (7), add (8)
      w'  = w - (lr*lr_scale)*upd : lr_eff (9), mul (10), sub (11)                    R_SGD_W  = 11
    No term of A passes through all of them (``momentum*|b|`` sees 2 of the 6), which leaves room for the rounding
    of the scalar ``1 - dampening`` itself.  ``momentum == 0`` skips the buffer and ignores dampening."""
    g, w, b = (np.asarray(t, np.float64) for t in (g, w, b))
    grp = np.asarray(group_of_element)
    lr, m, d, gs = (_f32(hyper[k]) for k in ("lr", "momentum", "dampening", "grad_scale"))
    wd = np.array([_f32(x) for x in hyper["wd"]])
    ls = np.array([_f32(x) for x in hyper["lr_scale"]])
    if mutant == "wd_neighbour":
        wd = np.roll(wd, -1)
    wde = wd[grp]
    lre = lr * ls[grp] if mutant != "lr_unscaled" else np.full(grp.shape, lr)
    if mutant == "scale_after_decay":
        gk, A_g = (g + wde * w) * gs, (np.abs(g) + wde * np.abs(w)) * gs
    else:
        gk, A_g = g * gs + wde * w, np.abs(g) * gs + wde * np.abs(w)
    damp = 1.0 if mutant == "no_dampening" else 1.0 - d
    if m == 0:
        bk, A_b, upd, A_upd = b, np.abs(b), gk, A_g
    else:
        if hyper["first_step"]:
            bk, A_b = gk, A_g
        else:
            bk, A_b = m * b + damp * gk, m * np.abs(b) + damp * A_g
        if hyper["nesterov"] and mutant != "no_nesterov":
            upd, A_upd = gk + m * bk, A_g + m * A_b
        else:
            upd, A_upd = bk, A_b
    return {"mom": (bk, A_b), "master": (w - lre * upd, np.abs(w) + lre * A_upd)}


def ref_adam(g, w, a, v, hyper, group_of_element, mutant=None):
    """``adam_chunk_kernel`` in fp64: {"m1": (value, A), "m2": (value, A), "master": (value, A)}.

    Roundings of the unfused fp32 path, per element (``1 - beta``, ``lr * lr_scale``, ``1 - lr*wd`` are scalars):
      gk = g*grad_scale (1) [L2: + wd*w (2) -> add (3)]        AdamW instead: w *= 1 - lr*wd (1 on the w path)
      a' = beta1*a (4) + (1-beta1)*gk (5) -> add (6)                                  R_ADAM_M1 = 6
      v' = beta2*v (4) + (1-beta2)*gk (5) *gk (6) -> add (7); 6 on the AdamW path, and ``wd*w`` is a side
           branch of the L2 path: the table value 6 is kept, the tighter of the two                R_ADAM_M2 = 6
      w' = w - (lr_eff/bc1) * a' / (sqrt(v') * rsqrt(bc2) + eps):
           a' (6), v' through the square root (6/2 = 3), sqrt (1), rsqrtf (2, it is not correctly rounded),
           mul (1), + eps (1), div (1), lr_eff/bc1 (1), mul (1), sub (1)                           R_ADAM_W = 18
    The quotient's magnitude is ``max(A_a, |a'| * A_v / v') / denom``: its relative error is that of ``a'`` or of
    ``v'``, whichever is conditioned worse (``A_v / v' > 1`` only where ``g*grad_scale`` and ``wd*w`` cancel)."""
    g, w, a, v = (np.asarray(t, np.float64) for t in (g, w, a, v))
    grp = np.asarray(group_of_element)
    lr, b1, b2, eps, gs = (_f32(hyper[k]) for k in ("lr", "beta1", "beta2", "eps", "grad_scale"))
    step = hyper["step"]
    bc1 = _f32(1.0 - float(hyper["beta1"]) ** step)
    bc2 = _f32(1.0 - float(hyper["beta2"]) ** (step + {"bc2_next": 1, "bc2_prev": -1}.get(mutant, 0)))
    wd = np.array([_f32(x) for x in hyper["wd"]])
    ls = np.array([_f32(x) for x in hyper["lr_scale"]])
    if mutant == "wd_neighbour":
        wd = np.roll(wd, -1)
    wde = wd[grp]
    lre = lr * ls[grp] if mutant != "lr_unscaled" else np.full(grp.shape, lr)
    adam_w = bool(hyper["adam_w"]) != (mutant == "swap_decay")
    gk, A_g = g * gs, np.abs(g) * gs
    if adam_w:
        wv, A_wv = w * (1.0 - lre * wde), np.abs(w) * (1.0 + lre * wde)
    elif mutant == "scale_after_decay":
        gk, A_g, wv, A_wv = (g + wde * w) * gs, (np.abs(g) + wde * np.abs(w)) * gs, w, np.abs(w)
    else:
        gk, A_g, wv, A_wv = gk + wde * w, A_g + wde * np.abs(w), w, np.abs(w)
    a1, A_a = b1 * a + (1.0 - b1) * gk, b1 * np.abs(a) + (1.0 - b1) * A_g
    v1, A_v = b2 * v + (1.0 - b2) * gk * gk, b2 * v + (1.0 - b2) * A_g * A_g
    if mutant == "eps_inside":
        denom = (np.sqrt(v1) + eps) / np.sqrt(bc2)
    else:
        denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    cond = np.divide(A_v, v1, out=np.ones_like(v1), where=v1 > 0)
    A_q = np.maximum(A_a, np.abs(a1) * cond) / denom
    s = lre / bc1
    return {"m1": (a1, A_a), "m2": (v1, A_v), "master": (wv - s * (a1 / denom), A_wv + s * A_q)}


# ---------------------------------------------------------------- plain unfused fp32 implementations
def f32_sgd(g, w, b, hyper, grp):
    f = np.float32
    g, w, b = (np.asarray(t, f) for t in (g, w, b))
    lr, m, d, gs = (f(hyper[k]) for k in ("lr", "momentum", "dampening", "grad_scale"))
    wd = np.array(hyper["wd"], f)[grp]
    lre = lr * np.array(hyper["lr_scale"], f)[grp]
    gk = g * gs + wd * w
    if m == 0:
        bk, upd = b, gk
    else:
        bk = gk if hyper["first_step"] else m * b + (f(1) - d) * gk
        upd = gk + m * bk if hyper["nesterov"] else bk
    out = {"mom": bk, "master": w - lre * upd}
    assert all(x.dtype == f for x in out.values())
    return out


def f32_adam(g, w, a, v, hyper, grp):
    f = np.float32
    g, w, a, v = (np.asarray(t, f) for t in (g, w, a, v))
    lr, b1, b2, eps, gs = (f(hyper[k]) for k in ("lr", "beta1", "beta2", "eps", "grad_scale"))
    bc1 = f(1.0 - float(hyper["beta1"]) ** hyper["step"])
    bc2 = f(1.0 - float(hyper["beta2"]) ** hyper["step"])
    wd = np.array(hyper["wd"], f)[grp]
    lre = lr * np.array(hyper["lr_scale"], f)[grp]
    gk = g * gs
    if hyper["adam_w"]:
        w = w * (f(1) - lre * wd)
    else:
        gk = gk + wd * w
    a1 = b1 * a + (f(1) - b1) * gk
    v1 = b2 * v + (f(1) - b2) * gk * gk
    denom = np.sqrt(v1) * (f(1) / np.sqrt(bc2)) + eps
    out = {"m1": a1, "m2": v1, "master": w - (lre / bc1) * (a1 / denom)}
    assert all(x.dtype == f for x in out.values())
    return out


# ---------------------------------------------------------------- bound check
def _check(tag, got, ref, A, R, mask=None):
    """Assert ``|got - ref| <= R * 2^-24 * A`` on ``mask`` and return the worst ``error / bound``."""
    got = np.asarray(got, np.float64)
    mask = np.ones(got.shape, bool) if mask is None else mask
    err, bnd = np.abs(got - ref)[mask], (R * U * A)[mask]
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    bad = np.flatnonzero(~(err <= bnd))
    if bad.size:
        i = np.flatnonzero(mask)[bad[0]]
        raise AssertionError(f"{tag}: {bad.size} of {err.size} elements outside R={R} bound, worst ratio {ratio:.3f}; "
                             f"first at {i}: got {got[i]!r} ref {ref[i]!r} bound {R * U * A[i]!r}")
    return ratio


def _caught(mut, ref, A, R, stratum):
    """Share of ``stratum`` on which a mutant's value lies outside the bound around the reference."""
    with np.errstate(invalid="ignore"):
        out = ~(np.abs(mut - ref) <= R * U * A)
    return float(out[stratum].mean())


# ---------------------------------------------------------------- hand-built chunk tables (sections 4 and 6)
# 8: one live thread; 2040: thread 255 idle; 2048: every thread once; 2056: the loop's second trip with a single
# live thread; 16384: eight trips (the production chunk); 16392: a ninth trip with a single live thread
LENS = (8, 2040, 2048, 2056, 16384, 16392, 2056, 2040)
GROUPS = (3, 0, 1, 2, 3, 0, 1, 2)
ORDER = (4, 0, 6, 2, 7, 5, 1, 3)  # table row r describes memory region ORDER[r]: blocks do not walk memory in order


@functools.lru_cache(maxsize=None)
def _layout():
    starts, cur = [], 0
    for j, ln in enumerate(LENS):
        cur = _round_up(cur, 64) + 8 * (1 + j % 7)  # a multiple of 8, never of 64
        starts.append(cur)
        cur += ln + 8                                # at least 8 unlisted elements before the next chunk
    n = _round_up(cur, 64) + 64
    rows = [(starts[j], LENS[j], GROUPS[j]) for j in ORDER]
    grp = np.full(n, -1)
    for s, ln, gi in rows:
        assert s % 8 == 0 and s % 64 != 0 and (grp[s:s + ln] == -1).all()
        grp[s:s + ln] = gi
    table = torch.tensor([(s, ln | (gi << 32)) for s, ln, gi in rows], dtype=torch.int64)
    return SimpleNamespace(n=n, rows=rows, table=table, grp=grp, covered=grp >= 0)


def _mixed(n, gen):
    """Per-element magnitudes 1e-3, 1 and 30."""
    scale = torch.tensor([1e-3, 1.0, 30.0])[torch.randint(0, 3, (n,), generator=gen)]
    return torch.randn(n, generator=gen) * scale


def _eps_values(n, gen):
    """|g| about 1e-9 with random signs."""
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    return sign * (0.5 + 1.5 * torch.rand(n, generator=gen)) * 1e-9


@functools.lru_cache(maxsize=None)
def _kernel_case(gname):
    """Inputs of the section 4 tests (CPU, never modified).  Listed elements: mixed magnitudes, and every fourth
    one eps-dominated (``|g|`` about 1e-9, ``w = a = v = 0``).  Unlisted elements: recognisable finite patterns."""
    L = _layout()
    gen = torch.Generator().manual_seed(20240 + len(gname))
    idx = torch.arange(L.n)
    cov = torch.from_numpy(L.covered)
    epsm = cov & (idx % 4 == 3)
    g, w, s1 = _mixed(L.n, gen), _mixed(L.n, gen), _mixed(L.n, gen)
    s2 = _mixed(L.n, gen).square()
    g[epsm] = _eps_values(int(epsm.sum()), gen)
    w[epsm], s1[epsm], s2[epsm] = 0.0, 0.0, 0.0
    pat = (idx % 13).float()
    return SimpleNamespace(
        g=g.to(DT[gname]), eps=epsm.numpy(),
        master=torch.where(cov, w, 1.5 + pat), s1=torch.where(cov, s1, -2.25 - pat),
        s2=torch.where(cov, s2, 0.75 + pat), param_fill=-3.0 - pat)  # the patterns are exact in bf16


def _sgd_hyper(nesterov, first_step):
    return dict(SGD_H, nesterov=nesterov, first_step=first_step)


def _adam_hyper(adam_w, step):
    return dict(ADAM_H, adam_w=adam_w, step=step)


# ---------------------------------------------------------------- section 3a: plain fp32 stays inside the bounds
@pytest.mark.parametrize("gname", ["f32", "bf16"])
def test_plain_fp32_sgd_is_inside_the_bounds(gname):
    L, c = _layout(), _kernel_case(gname)
    worst = {"mom": 0.0, "master": 0.0}
    for nesterov in (False, True):
        for first in (False, True):
            h = _sgd_hyper(nesterov, first)
            grp = np.where(L.covered, L.grp, 0)
            ref = ref_sgd(_np64(c.g), _np64(c.master), _np64(c.s1), h, grp)
            got = f32_sgd(c.g.float().numpy(), c.master.numpy(), c.s1.numpy(), h, grp)
            for k, R in (("mom", R_SGD_MOM), ("master", R_SGD_W)):
                worst[k] = max(worst[k], _check(f"sgd {k} nesterov={nesterov} first={first}", got[k], *ref[k], R,
                                                L.covered))
    print(f"plain fp32 sgd[{gname}] worst err/bound mom {worst['mom']:.3f} master {worst['master']:.3f}")
    assert max(worst.values()) <= 1


@pytest.mark.parametrize("gname", ["f32", "bf16"])
def test_plain_fp32_adam_is_inside_the_bounds(gname):
    L, c = _layout(), _kernel_case(gname)
    worst = {"m1": 0.0, "m2": 0.0, "master": 0.0}
    grp = np.where(L.covered, L.grp, 0)
    for adam_w in (False, True):
        for step in ADAM_STEPS:
            h = _adam_hyper(adam_w, step)
            ref = ref_adam(_np64(c.g), _np64(c.master), _np64(c.s1), _np64(c.s2), h, grp)
            got = f32_adam(c.g.float().numpy(), c.master.numpy(), c.s1.numpy(), c.s2.numpy(), h, grp)
            for k, R in (("m1", R_ADAM_M1), ("m2", R_ADAM_M2), ("master", R_ADAM_W)):
                worst[k] = max(worst[k], _check(f"adam {k} adam_w={adam_w} step={step}", got[k], *ref[k], R,
                                                L.covered))
    print(f"plain fp32 adam[{gname}] worst err/bound m1 {worst['m1']:.3f} m2 {worst['m2']:.3f} "
          f"master {worst['master']:.3f}")
    assert max(worst.values()) <= 1


# ---------------------------------------------------------------- section 3b: the bounds catch wrong formulas
MIN_CAUGHT = 0.10


def _sgd_mutant_share(mutant, output, stratum_of, nesterov=True, first=False, gname="bf16"):
    L, c = _layout(), _kernel_case(gname)
    grp = np.where(L.covered, L.grp, 0)
    h = _sgd_hyper(nesterov, first)
    args = (_np64(c.g), _np64(c.master), _np64(c.s1), h, grp)
    ref, mut = ref_sgd(*args), ref_sgd(*args, mutant=mutant)
    R = {"mom": R_SGD_MOM, "master": R_SGD_W}[output]
    return _caught(mut[output][0], *ref[output], R, stratum_of(L, c))


def _normal(L, c):
    return L.covered & ~c.eps


def _scaled_lr(L, c):
    return L.covered & (np.array(SGD_H["lr_scale"])[np.where(L.covered, L.grp, 0)] != 1)


@pytest.mark.parametrize("mutant,output,stratum_of", [
    ("no_dampening", "mom", _normal), ("no_dampening", "master", _normal),
    ("no_nesterov", "master", _normal),
    ("lr_unscaled", "master", _scaled_lr),
    ("wd_neighbour", "mom", _normal), ("wd_neighbour", "master", _normal),
    ("scale_after_decay", "mom", _normal), ("scale_after_decay", "master", _normal),
], ids=lambda x: x if isinstance(x, str) else x.__name__)
def test_sgd_mutants_leave_the_bounds(mutant, output, stratum_of):
    share = _sgd_mutant_share(mutant, output, stratum_of)
    print(f"sgd mutant {mutant} on {output}: outside the bound on {share:.1%} of {stratum_of.__name__}")
    assert share >= MIN_CAUGHT


def _adam_mutant_share(mutant, output, stratum_of, adam_w, step, gname="bf16"):
    L, c = _layout(), _kernel_case(gname)
    grp = np.where(L.covered, L.grp, 0)
    h = _adam_hyper(adam_w, step)
    args = (_np64(c.g), _np64(c.master), _np64(c.s1), _np64(c.s2), h, grp)
    ref, mut = ref_adam(*args), ref_adam(*args, mutant=mutant)
    R = {"m1": R_ADAM_M1, "m2": R_ADAM_M2, "master": R_ADAM_W}[output]
    return _caught(mut[output][0], *ref[output], R, stratum_of(L, c))


def _eps_stratum(L, c):
    return L.covered & c.eps


def _small_w(L, c):
    return L.covered & ~c.eps & (np.abs(c.master.numpy()) < 1e-2)


@pytest.mark.parametrize("mutant,output,stratum_of,adam_w,step", [
    ("lr_unscaled", "master", _scaled_lr, True, 2),
    ("wd_neighbour", "master", _normal, True, 2), ("wd_neighbour", "m1", _normal, False, 2),
    ("scale_after_decay", "m1", _normal, False, 2), ("scale_after_decay", "m2", _normal, False, 2),
    ("swap_decay", "master", _normal, True, 2), ("swap_decay", "master", _normal, False, 2),
    ("swap_decay", "m1", _normal, True, 2), ("swap_decay", "m1", _normal, False, 2),
    ("bc2_next", "master", _normal, True, 1), ("bc2_next", "master", _normal, True, 2),
    ("bc2_prev", "master", _normal, True, 2),
    ("bc2_next", "master", _small_w, True, 1000), ("bc2_prev", "master", _small_w, True, 1000),
    ("eps_inside", "master", _eps_stratum, True, 1), ("eps_inside", "master", _eps_stratum, True, 2),
    ("eps_inside", "master", _eps_stratum, False, 1), ("eps_inside", "master", _eps_stratum, False, 2),
], ids=lambda x: x if isinstance(x, str) else getattr(x, "__name__", str(x)))
def test_adam_mutants_leave_the_bounds(mutant, output, stratum_of, adam_w, step):
    share = _adam_mutant_share(mutant, output, stratum_of, adam_w, step)
    print(f"adam mutant {mutant} on {output} (adam_w={adam_w}, step {step}): outside the bound on {share:.1%} "
          f"of {stratum_of.__name__}")
    assert share >= MIN_CAUGHT


def test_eps_stratum_is_eps_dominated():
    """There ``sqrt(v') / sqrt(bc2) = |g*grad_scale|`` at step 1, far below ``eps``: the stratum exists."""
    c = _kernel_case("bf16")
    gk = np.abs(_np64(c.g))[c.eps] * ADAM_H["grad_scale"]
    assert c.eps.sum() > 1000 and gk.max() < ADAM_H["eps"] / 10 and gk.min() > 0


# ---------------------------------------------------------------- section 3c: table properties
PARAM_SHAPES = [(1,), (3,), (13, 1), (1001,), (32, 64), (8, 257), (5000,), (200, 200)]  # 2-D: decayed; 1-D: not
assert [int(np.prod(s)) for s in PARAM_SHAPES] == [1, 3, 13, 1001, 2048, 2056, 5000, 40000]


def _module(dtype, device):
    gen = torch.Generator().manual_seed(11)
    return torch.nn.ParameterList([torch.nn.Parameter(_mixed(int(np.prod(s)), gen).view(s).to(dtype).to(device))
                                   for s in PARAM_SHAPES])


def test_chunk_for_thresholds():
    from kubedl_amd.ops.optim import CHUNK, CHUNK_MIN_BLOCKS, chunk_for
    assert (CHUNK, CHUNK_MIN_BLOCKS) == (16384, 1024)
    for c in (16384, 8192, 4096):
        assert chunk_for(c * 1024) == c and chunk_for(c * 1024 - 1) == c // 2
    assert chunk_for(1) == chunk_for(2048 * 1024) == 2048 and chunk_for(1 << 40) == 16384


@pytest.mark.parametrize("chunk", [2048, 16384])
def test_chunk_tables_tile_the_slots(chunk):
    from kubedl_amd.ops.optim import ALIGN, FlatParamSpace, GradPacker
    sp = FlatParamSpace(_module(F32, "cpu"))
    assert sp.chunk == 2048 and {s.group for s in sp.slots} == {0, 1}
    assert all(s.offset % ALIGN == 0 and s.group == (1 if s.param.dim() <= 1 else 0) for s in sp.slots)
    want_cover, want_grp = np.zeros(sp.numel, int), np.full(sp.numel, -1)
    for s in sp.slots:
        assert (want_cover[s.offset:s.offset + _round_up(s.numel, 8)] == 0).all()
        want_cover[s.offset:s.offset + _round_up(s.numel, 8)] = 1
        want_grp[s.offset:s.offset + _round_up(s.numel, 8)] = s.group
    table = FlatParamSpace._chunk_table(SimpleNamespace(slots=sp.slots, chunk=chunk)).numpy()
    if chunk == sp.chunk:
        assert np.array_equal(table, sp.chunks_cpu.numpy())
    start, ln, grp = table[:, 0], table[:, 1] & 0xffffffff, table[:, 1] >> 32
    assert (start % 8 == 0).all() and (ln % 8 == 0).all() and (ln > 0).all() and (ln <= chunk).all()
    cover, got_grp = np.zeros(sp.numel, int), np.full(sp.numel, -1)
    for s0, l0, g0 in zip(start, ln, grp):
        cover[s0:s0 + l0] += 1
        got_grp[s0:s0 + l0] = g0
    assert np.array_equal(cover, want_cover)  # each slot's padded range exactly once, nothing else, no overlap
    assert np.array_equal(got_grp, want_grp)
    assert ln.max() == min(chunk, 40000)

    packer = GradPacker(SimpleNamespace(chunk=chunk, device=torch.device("cpu")), sp.slots)
    rows = packer.chunks.numpy()
    assert packer.nchunks == len(rows)
    tens, pl, src_off, dst_off = rows[:, 0] & 0xffffffff, rows[:, 0] >> 32, rows[:, 1], rows[:, 2]
    assert (pl > 0).all() and (pl <= chunk).all()
    for i, s in enumerate(sp.slots):
        seen = np.zeros(s.numel, int)
        for l0, so, do in zip(pl[tens == i], src_off[tens == i], dst_off[tens == i]):
            assert do == s.offset + so
            seen[so:so + l0] += 1
        assert (seen == 1).all()
    assert pl.sum() == sum(s.numel for s in sp.slots)


# ---------------------------------------------------------------- section 4: the optimizer kernels, hand-built tables
def _run_sgd(c, pdtype, h, mom0):
    L = _layout()
    master, mom, grad = c.master.cuda(), mom0.cuda(), c.g.cuda()
    param = c.param_fill.to(pdtype).cuda()
    _ext().sgd_step(L.table.cuda(), master, mom, grad, param, h["lr"], h["momentum"], h["dampening"],
                    h["grad_scale"], h["nesterov"], h["first_step"], h["wd"], h["lr_scale"])
    torch.cuda.synchronize()
    return SimpleNamespace(master=master.cpu(), mom=mom.cpu(), grad=grad.cpu(), param=param.cpu())


def _check_exact_parts(tag, c, L, pdtype, out, states):
    cov = torch.from_numpy(L.covered)
    want = torch.where(cov, out.master.to(pdtype), c.param_fill.to(pdtype))
    assert _bits_equal(out.param, want), f"{tag}: param is not the rounded master inside / the pattern outside"
    assert _bits_equal(out.grad, c.g), f"{tag}: grad changed"
    for name, got, before in [("master", out.master, c.master)] + states:
        assert _bits_equal(got[~cov], before[~cov]), f"{tag}: {name} changed outside the chunk table"


@gpu
@pytest.mark.parametrize("first_step", [False, True])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("pname", ["f32", "bf16"])
@pytest.mark.parametrize("gname", ["f32", "bf16"])
def test_sgd_kernel(gname, pname, nesterov, first_step):
    L, c, pd = _layout(), _kernel_case(gname), DT[pname]
    tag = f"sgd[g {gname} p {pname} nesterov={nesterov} first={first_step}]"
    h = _sgd_hyper(nesterov, first_step)
    out = _run_sgd(c, pd, h, c.s1)
    grp = np.where(L.covered, L.grp, 0)
    ref = ref_sgd(_np64(c.g), _np64(c.master), _np64(c.s1), h, grp)
    r_m = _check(tag + " mom", out.mom.numpy(), *ref["mom"], R_SGD_MOM, L.covered)
    r_w = _check(tag + " master", out.master.numpy(), *ref["master"], R_SGD_W, L.covered)
    print(f"{tag} worst err/bound mom {r_m:.3f} master {r_w:.3f}")
    _check_exact_parts(tag, c, L, pd, out, [("mom", out.mom, c.s1)])
    again = _run_sgd(c, pd, h, c.s1)
    for k in ("master", "mom", "param"):
        assert _bits_equal(getattr(out, k), getattr(again, k)), f"{tag}: {k} differs between two identical calls"
    if first_step:  # the momentum buffer is not read: huge finite contents and zeros give the same bits
        cov = torch.from_numpy(L.covered)
        huge = _run_sgd(c, pd, h, torch.where(cov, torch.full_like(c.s1, 3e38), c.s1))
        zero = _run_sgd(c, pd, h, torch.where(cov, torch.zeros_like(c.s1), c.s1))
        for k in ("master", "mom", "param"):
            assert _bits_equal(getattr(huge, k), getattr(zero, k)), f"{tag}: {k} depends on the stale momentum"
            assert _bits_equal(getattr(huge, k), getattr(out, k))


def _run_adam(c, pdtype, h):
    L = _layout()
    master, m1, m2, grad = c.master.cuda(), c.s1.cuda(), c.s2.cuda(), c.g.cuda()
    param = c.param_fill.to(pdtype).cuda()
    _ext().adam_step(L.table.cuda(), master, m1, m2, grad, param, h["lr"], h["beta1"], h["beta2"], h["eps"],
                     h["step"], h["grad_scale"], h["adam_w"], h["wd"], h["lr_scale"])
    torch.cuda.synchronize()
    return SimpleNamespace(master=master.cpu(), m1=m1.cpu(), m2=m2.cpu(), grad=grad.cpu(), param=param.cpu())


@gpu
@pytest.mark.parametrize("step", ADAM_STEPS)
@pytest.mark.parametrize("adam_w", [False, True])
@pytest.mark.parametrize("pname", ["f32", "bf16"])
@pytest.mark.parametrize("gname", ["f32", "bf16"])
def test_adam_kernel(gname, pname, adam_w, step):
    L, c, pd = _layout(), _kernel_case(gname), DT[pname]
    tag = f"adam[g {gname} p {pname} adam_w={adam_w} step {step}]"
    h = _adam_hyper(adam_w, step)
    out = _run_adam(c, pd, h)
    grp = np.where(L.covered, L.grp, 0)
    ref = ref_adam(_np64(c.g), _np64(c.master), _np64(c.s1), _np64(c.s2), h, grp)
    r_a = _check(tag + " m1", out.m1.numpy(), *ref["m1"], R_ADAM_M1, L.covered)
    r_v = _check(tag + " m2", out.m2.numpy(), *ref["m2"], R_ADAM_M2, L.covered)
    r_w = _check(tag + " master", out.master.numpy(), *ref["master"], R_ADAM_W, L.covered)
    r_e = _check(tag + " master, eps stratum", out.master.numpy(), *ref["master"], R_ADAM_W, L.covered & c.eps)
    print(f"{tag} worst err/bound m1 {r_a:.3f} m2 {r_v:.3f} master {r_w:.3f} (eps stratum {r_e:.3f})")
    _check_exact_parts(tag, c, L, pd, out, [("m1", out.m1, c.s1), ("m2", out.m2, c.s2)])
    again = _run_adam(c, pd, h)
    for k in ("master", "m1", "m2", "param"):
        assert _bits_equal(getattr(out, k), getattr(again, k)), f"{tag}: {k} differs between two identical calls"


# ---------------------------------------------------------------- section 5: through the Python classes
CLS_WD, CLS_GRAD_SCALE, CLS_STEPS = 0.01, 0.5, 3


def _space_masks(sp):
    """group per element (0 in the gaps), the elements the kernels process, the elements that are parameters."""
    grp, proc, real = np.zeros(sp.numel, int), np.zeros(sp.numel, bool), np.zeros(sp.numel, bool)
    for s in sp.slots:
        grp[s.offset:s.offset + _round_up(s.numel, 8)] = s.group
        proc[s.offset:s.offset + _round_up(s.numel, 8)] = True
        real[s.offset:s.offset + s.numel] = True
    return grp, proc, real


def _class_grads(sp, real, dtype):
    """One flat gradient per step (CPU, model dtype), zero outside the parameters."""
    gen = torch.Generator().manual_seed(5)
    return [(_mixed(sp.numel, gen) * torch.from_numpy(real)).to(dtype) for _ in range(CLS_STEPS)]


def _check_space_after_step(tag, sp, proc):
    master = sp.master.cpu()
    assert _bits_equal(sp.param.cpu(), master.to(sp.dtype)), f"{tag}: flat param is not the rounded master"
    for s in sp.slots:
        assert s.param.data_ptr() == sp.param.data_ptr() + s.offset * sp.param.element_size()
        assert _bits_equal(s.param.data.reshape(-1), master[s.offset:s.offset + s.numel].to(sp.dtype)), \
            f"{tag}: parameter {s.name} is not the rounded master"
    gap = torch.from_numpy(~proc)
    assert torch.count_nonzero(master[gap]) == 0 and torch.count_nonzero(sp.param.cpu()[gap].float()) == 0, \
        f"{tag}: alignment gaps are no longer zero"
    return master


@gpu
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_fused_sgd_steps(dtype, nesterov):
    from kubedl_amd.ops.optim import FlatParamSpace, FusedSGD
    sp = FlatParamSpace(_module(dtype, "cuda"))
    assert sp.grad_mode == "pack" and sp.dtype == dtype
    opt = FusedSGD(sp, lr=SGD_H["lr"], momentum=0.9, dampening=0.1, weight_decay=CLS_WD, nesterov=nesterov)
    opt.grad_scale = CLS_GRAD_SCALE
    grp, proc, real = _space_masks(sp)
    worst = {"mom": 0.0, "master": 0.0}
    for k, g in enumerate(_class_grads(sp, real, dtype)):
        tag = f"FusedSGD[{dtype} nesterov={nesterov}] step {k + 1}"
        h = dict(lr=opt.lr, momentum=0.9, dampening=0.1, grad_scale=CLS_GRAD_SCALE, nesterov=nesterov,
                 first_step=k == 0, wd=[CLS_WD, 0.0, 0.0, 0.0], lr_scale=[1.0] * 4)
        w0, b0 = _np64(sp.master), _np64(opt.mom)
        sp.grad.copy_(g)
        opt.step()
        torch.cuda.synchronize()
        master = _check_space_after_step(tag, sp, proc)
        assert _bits_equal(sp.grad, g), f"{tag}: grad changed"
        ref = ref_sgd(_np64(g), w0, b0, h, grp)
        worst["mom"] = max(worst["mom"], _check(tag + " mom", opt.mom.cpu().numpy(), *ref["mom"], R_SGD_MOM, proc))
        worst["master"] = max(worst["master"], _check(tag + " master", master.numpy(), *ref["master"], R_SGD_W, proc))
        plain = ref_sgd(_np64(g), w0, b0, dict(h, wd=[0.0] * 4), grp)  # the no-decay group received no decay
        _check(tag + " master, no-decay group", master.numpy(), *plain["master"], R_SGD_W, proc & (grp == 1))
    print(f"FusedSGD[{dtype} nesterov={nesterov}] worst err/bound mom {worst['mom']:.3f} "
          f"master {worst['master']:.3f}")


@gpu
@pytest.mark.parametrize("adam_w", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_fused_adam_steps(dtype, adam_w):
    from kubedl_amd.ops.optim import FlatParamSpace, FusedAdam
    sp = FlatParamSpace(_module(dtype, "cuda"))
    opt = FusedAdam(sp, lr=ADAM_H["lr"], weight_decay=CLS_WD, adam_w=adam_w)
    opt.grad_scale = CLS_GRAD_SCALE
    grp, proc, real = _space_masks(sp)
    worst = {"m1": 0.0, "m2": 0.0, "master": 0.0}
    for k, g in enumerate(_class_grads(sp, real, dtype)):
        tag = f"FusedAdam[{dtype} adam_w={adam_w}] step {k + 1}"
        h = dict(lr=opt.lr, beta1=opt.betas[0], beta2=opt.betas[1], eps=opt.eps, grad_scale=CLS_GRAD_SCALE,
                 adam_w=adam_w, step=k + 1, wd=[CLS_WD, 0.0, 0.0, 0.0], lr_scale=[1.0] * 4)
        w0, a0, v0 = _np64(sp.master), _np64(opt.m1), _np64(opt.m2)
        sp.grad.copy_(g)
        opt.step()
        torch.cuda.synchronize()
        master = _check_space_after_step(tag, sp, proc)
        assert _bits_equal(sp.grad, g), f"{tag}: grad changed"
        ref = ref_adam(_np64(g), w0, a0, v0, h, grp)
        got = {"m1": opt.m1.cpu().numpy(), "m2": opt.m2.cpu().numpy(), "master": master.numpy()}
        for name, R in (("m1", R_ADAM_M1), ("m2", R_ADAM_M2), ("master", R_ADAM_W)):
            worst[name] = max(worst[name], _check(f"{tag} {name}", got[name], *ref[name], R, proc))
        plain = ref_adam(_np64(g), w0, a0, v0, dict(h, wd=[0.0] * 4), grp)  # the no-decay group received no decay
        _check(tag + " master, no-decay group", got["master"], *plain["master"], R_ADAM_W, proc & (grp == 1))
    print(f"FusedAdam[{dtype} adam_w={adam_w}] worst err/bound m1 {worst['m1']:.3f} m2 {worst['m2']:.3f} "
          f"master {worst['master']:.3f}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_fused_sgd_without_momentum_ignores_dampening(dtype):
    """``torch.optim.SGD`` applies dampening only inside the momentum buffer update: with ``momentum == 0`` the
    update is ``lr * (g*grad_scale + wd*w)`` whatever ``dampening`` is, on the HIP path as on the CPU path."""
    from kubedl_amd.ops.optim import FlatParamSpace, FusedSGD
    sp, sp_cpu = FlatParamSpace(_module(dtype, "cuda")), FlatParamSpace(_module(dtype, "cpu"))
    opts = [FusedSGD(s, lr=SGD_H["lr"], momentum=0.0, dampening=0.1, weight_decay=CLS_WD) for s in (sp, sp_cpu)]
    for o in opts:
        o.grad_scale = CLS_GRAD_SCALE
    grp, proc, real = _space_masks(sp)
    worst = worst_cpu = 0.0
    for k, g in enumerate(_class_grads(sp, real, dtype)):
        tag = f"FusedSGD[{dtype} momentum=0 dampening=0.1] step {k + 1}"
        h = dict(lr=SGD_H["lr"], momentum=0.0, dampening=0.1, grad_scale=CLS_GRAD_SCALE, nesterov=False,
                 first_step=k == 0, wd=[CLS_WD, 0.0, 0.0, 0.0], lr_scale=[1.0] * 4)
        w0 = sp.master.cpu()
        sp_cpu.master.copy_(w0)  # teacher-forced: both paths start the step from the HIP path's master
        sp.grad.copy_(g)
        sp_cpu.grad.copy_(g)
        for o in opts:
            o.step()
        torch.cuda.synchronize()
        master = _check_space_after_step(tag, sp, proc)
        ref, A = ref_sgd(_np64(g), _np64(w0), np.zeros(sp.numel), h, grp)["master"]
        worst = max(worst, _check(tag + " master", master.numpy(), ref, A, R_SGD_W, proc))
        # the CPU path is an fp32 evaluation of the same formula: each side is within R roundings of the reference
        worst_cpu = max(worst_cpu, _check(tag + " master vs the CPU path", master.numpy(),
                                          _np64(sp_cpu.master), A, 2 * R_SGD_W, proc))
    print(f"FusedSGD[{dtype} momentum=0] worst err/bound vs fp64 {worst:.3f}, vs the CPU path {worst_cpu:.3f}")


# ---------------------------------------------------------------- section 6: chunk_sumsq
def _sumsq_bound(ln):
    """Relative bound of one chunk's fp32 sum of squares: ``(len/8/256 + 14) * 2^-24``.  All terms are non-negative,
    so every rounding is relative to at most the sum itself.  A thread makes ``len/8/256`` trips of 8 ``fmaf``; then
    come the 6 ``wave_sum`` shuffle adds and the 3 adds of the four wave sums; squaring the rounded ``x*scale`` costs
    2.  The worst case of that chain is ``8 * trips + 2 + 6 + 3``, reached only if every rounding of a thread's
    accumulator falls the same way on a sum as large as the thread's total.  Asserted is the tighter count of one
    rounding per trip plus the 8 of one trip, the 6 and the 3 (the square's 2 go into the trip's 8: ``x*scale`` is
    exact for the power-of-two scales used): ``trips + 14 <= 8 * trips + 11`` for every length.
    ``test_plain_fp32_sumsq_is_inside_the_bound`` evaluates the kernel's order of summation in unfused fp32
    against it."""
    return (ln / 8 / 256 + 14) * U


@functools.lru_cache(maxsize=None)
def _sumsq_case(name, integers):
    L = _layout()
    gen = torch.Generator().manual_seed(77 + integers)
    x = torch.randint(-8, 9, (L.n,), generator=gen).float() if integers else _mixed(L.n, gen)
    s, ln, _ = L.rows[3]  # one chunk is all zeros
    x[s:s + ln] = 0.0
    return x.to(DT[name])


def _sumsq_ref(x, scale):
    xs = _np64(x) * _f32(scale)
    return np.array([np.sum(xs[s:s + ln] ** 2) for s, ln, _ in _layout().rows])


def _sumsq_plain_fp32(x, scale):
    """The kernel's order of summation in unfused fp32: per thread over trips and lanes, butterfly, four waves."""
    f = np.float32
    out = []
    for s, ln, _ in _layout().rows:
        trips = -(-ln // 2048)
        seg = np.zeros(trips * 2048, f)
        seg[:ln] = x[s:s + ln].float().numpy()
        seg = seg.reshape(trips, 256, 8)
        acc = np.zeros(256, f)
        for t in range(trips):
            for k in range(8):
                sv = seg[t, :, k] * f(scale)
                acc = sv * sv + acc
        acc = acc.reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, np.arange(64) ^ o]
        out.append(((acc[0, 0] + acc[1, 0]) + acc[2, 0]) + acc[3, 0])
    return np.array(out, np.float64)


def _check_sumsq(tag, got, ref):
    bound = np.array([_sumsq_bound(ln) for _, ln, _ in _layout().rows]) * ref
    err = np.abs(got - ref)
    assert (err <= bound).all(), f"{tag}: {got} vs {ref}, bounds {bound}"
    return float((err[bound > 0] / bound[bound > 0]).max())


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_plain_fp32_sumsq_is_inside_the_bound(name, scale):
    x = _sumsq_case(name, False)
    ratio = _check_sumsq(f"plain fp32 sumsq[{name} scale {scale}]", _sumsq_plain_fp32(x, scale), _sumsq_ref(x, scale))
    print(f"plain fp32 sumsq[{name} scale {scale}] worst err/bound {ratio:.3f}")
    xi = _sumsq_case(name, True)
    assert np.array_equal(_sumsq_plain_fp32(xi, scale), _sumsq_ref(xi, scale))


@gpu
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_chunk_sumsq(name, scale):
    L = _layout()
    table = L.table.cuda()
    tag = f"chunk_sumsq[{name} scale {scale}]"
    x = _sumsq_case(name, False)
    ref = _sumsq_ref(x, scale)
    assert len(set(ref.tolist())) == len(ref) and ref[3] == 0  # distinct sums: a permuted output cannot pass
    out = _ext().chunk_sumsq(table, x.cuda(), scale)
    assert out.dtype == F32 and out.shape == (len(L.rows),)
    got = out.cpu().double().numpy()
    ratio = _check_sumsq(tag, got, ref)
    assert got[3] == 0
    print(f"{tag} worst err/bound {ratio:.3f}")
    xi = _sumsq_case(name, True)  # small integers, power-of-two scale: every partial sum is exact in fp32
    ref_i = _sumsq_ref(xi, scale)
    assert ref_i.max() < 2 ** 24 and len(set(ref_i.tolist())) == len(ref_i)
    got_i = _ext().chunk_sumsq(table, xi.cuda(), scale).cpu().double().numpy()
    assert np.array_equal(got_i, ref_i), f"{tag}: integer sums {got_i} vs {ref_i}"


# ---------------------------------------------------------------- section 7: cast_copy
CAST_GRID = 2048 * 256 * 8  # elements one trip of the full grid moves
CAST_SIZES = [8, 2048 * 8 - 8, CAST_GRID + 8 * 1000]  # the last: a second trip for 1000 threads only


def _special(dtype):
    if dtype == F32:
        vals = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, float("inf"), float("-inf"),
                1.00390625, 1.01171875, -1.00390625, -1.01171875, 3.4028234663852886e38, -3.4028234663852886e38,
                float("nan"), 3.3895313892515355e38, 1.0, -2.5, 65504.0, 1e-3, 0.1, 1 / 3, 3e38]
    else:
        vals = [0.0, -0.0, 9.183549615799121e-41, -9.183549615799121e-41, 1e-39, -1e-39, float("inf"),
                float("-inf"), float("nan"), 3.3895313892515355e38, -3.3895313892515355e38, 1.0, 1.0078125,
                -2.5, 1e-3, 0.1]
    return torch.tensor(vals, dtype=torch.float32).to(dtype)


@functools.lru_cache(maxsize=None)
def _cast_src(sname, n):
    gen = torch.Generator().manual_seed(n % 1000 + len(sname))
    src = _mixed(n, gen).to(DT[sname])
    sp = _special(DT[sname])
    k = min(n, len(sp))
    src[:k] = sp[:k]
    if n > 2 * len(sp):
        src[n - len(sp):] = sp  # the specials also sit in the tail (the partial second trip of the largest size)
    return src


def test_cast_reference_rounds_ties_to_even():
    """What ``src.to(bfloat16)`` on the CPU gives for the values the GPU test is about."""
    got = _bits(torch.tensor([1.00390625, 1.01171875, 3.4028234663852886e38]).to(BF16)).tolist()
    assert [x & 0xffff for x in got] == [0x3F80, 0x3F82, 0x7F80]


@gpu
@pytest.mark.parametrize("n", CAST_SIZES)
@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("sname", ["f32", "bf16"])
def test_cast_copy(sname, dname, n):
    src = _cast_src(sname, n)
    want = src.to(DT[dname])
    tail = 64
    fill = torch.full((n + tail,), -7.0, dtype=DT[dname])
    dst = fill.cuda()
    src_dev = src.cuda()
    _ext().cast_copy(src_dev, dst[:n])
    torch.cuda.synchronize()
    got = dst.cpu()
    assert _bits_equal(got[n:], fill[n:]), "cast_copy wrote past n"
    assert _bits_equal(src_dev, src), "cast_copy changed its source"
    nan = torch.isnan(want.float())
    has_all = n >= len(_special(DT[sname]))  # the smallest size holds the first eight special values only
    assert nan.sum() >= has_all and torch.equal(torch.isnan(got[:n].float()), nan)
    gb, wb = _bits(got[:n])[~nan], _bits(want)[~nan]
    if not torch.equal(gb, wb):
        i = int(torch.nonzero(gb != wb)[0])
        j = int(torch.nonzero(~nan).reshape(-1)[i])
        raise AssertionError(f"cast_copy {sname}->{dname} n={n}: {int((gb != wb).sum())} elements differ, first at "
                             f"{j}: src {src[j].item()!r} got bits {int(gb[i]) & 0xffffffff:#x} "
                             f"want {int(wb[i]) & 0xffffffff:#x}")
    if sname == "f32" and dname == "bf16" and has_all:  # ties to even and overflow to inf, spelled out
        assert [x & 0xffff for x in _bits(got[9:11]).tolist()] == [0x3F80, 0x3F82]
        assert _bits(got[13:14]).item() & 0xffff == 0x7F80


# ---------------------------------------------------------------- section 8: pack_kernel
PACK_NUMELS = [1, 7, 8, 9, 2047, 2048, 2049, 5000, 2049, 2055, 100, 3000]
PACK_NONE, PACK_UNALIGNED, PACK_SKIPPED = 8, 9, (10, 11)  # indices into PACK_NUMELS


def _pack_sources(dtype, seed):
    """CPU gradients per parameter: None for one, a view one element into its storage for another."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(PACK_NUMELS):
        if i == PACK_NONE:
            out.append(None)
        elif i == PACK_UNALIGNED:
            out.append(_mixed(n + 1, gen).to(dtype)[1:])
        else:
            out.append(_mixed(n, gen).to(dtype))
    return out


def _pack_want(fill, slots_by_index, sources, scale, dtype):
    want = fill.clone()
    for i, src in enumerate(sources):
        s = slots_by_index[i]
        if i in PACK_SKIPPED:
            continue
        if src is None:
            want[s.offset:s.offset + s.numel] = 0
        elif scale == 1.0:
            want[s.offset:s.offset + s.numel] = src
        else:  # one fp32 multiply and one rounding to the buffer's dtype: exact
            want[s.offset:s.offset + s.numel] = (src.float() * torch.tensor(scale, dtype=F32)).to(dtype)
    return want


@gpu
@pytest.mark.parametrize("scale", [1.0, 0.5, 1 / 3], ids=["1", "0.5", "third"])
@pytest.mark.parametrize("mode", ["ptrs", "table"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_pack_kernel(dtype, mode, scale):
    from kubedl_amd.ops.optim import FlatParamSpace
    ext = _ext()
    params = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n, dtype=dtype, device="cuda"))
                                     for n in PACK_NUMELS])
    sp = FlatParamSpace(params, grad_mode="pack")
    assert sp.chunk == 2048 and len(PACK_NUMELS) <= ext.pack_arg_ptrs
    by_index = {int(s.name): s for s in sp.slots}
    packer = sp.packer([s for s in sp.slots if int(s.name) not in PACK_SKIPPED])
    assert packer.nchunks == sum(-(-PACK_NUMELS[int(s.name)] // 2048) for s in packer.slots)
    table_before = packer.chunks.clone()
    fill = (4.0 + (torch.arange(sp.numel) % 7).float()).to(dtype)
    for seed in (1, 2):  # twice: the second call reuses the table
        sources = _pack_sources(dtype, seed)
        dev = []
        for i, src in enumerate(sources):
            if src is None:
                dev.append(None)
            elif i == PACK_UNALIGNED:
                store = torch.zeros(src.numel() + 1, dtype=dtype, device="cuda")
                store[1:] = src.cuda()
                dev.append(store[1:])
                assert dev[-1].data_ptr() % 16 != 0 and dev[-1].is_contiguous()
            else:
                dev.append(src.cuda())
                assert dev[-1].data_ptr() % 16 == 0
            by_index[i].param.grad = dev[-1]
        sp.grad.copy_(fill)
        if mode == "ptrs":
            packer.pack(scale)
        else:
            ptrs = torch.tensor([0 if s.param.grad is None else s.param.grad.data_ptr() for s in packer.slots],
                                dtype=torch.int64, device="cuda")
            ext.pack_grads(packer.chunks, ptrs, sp.grad, scale)
        torch.cuda.synchronize()
        want = _pack_want(fill, by_index, sources, scale, dtype)
        got = sp.grad.cpu()
        if not _bits_equal(got, want):
            i = int(torch.nonzero(_bits(got) != _bits(want))[0])
            raise AssertionError(f"pack {dtype} {mode} scale {scale} call {seed}: first difference at flat element {i}: "
                                 f"got {got[i].item()!r} want {want[i].item()!r}")
        for i, src in enumerate(sources):  # the sources are read only
            if src is not None:
                assert _bits_equal(dev[i], src)
        assert torch.equal(packer.chunks, table_before)
