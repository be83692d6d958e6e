"""``FusedLARS`` (csrc/optim.hip ``lars_norms_kernel`` / ``lars_update_kernel``) and the label-smoothed head
(csrc/head.hip ``head_ce_kernel<true>``) against fp64 references computed from the very tensors the kernels read.

Bounds as in tests/test_optim_gpu.py: ``|got - ref64| <= R * 2^-24 * A``, ``A`` the reference with every term replaced
by its absolute value, ``R`` the fp32 roundings of the kernel's own operation sequence.  A 2,048-element chunk's sum of
squares: 8 ``fmaf`` per lane, 6 ``wave_sum`` adds, 3 adds over the waves = 17, relative to at most the sum; the fp64
tensor sum adds nothing and the square root halves it: 8.5 per norm.  trust = eta*wn / (gn + wd*wn + eps): 8.5 + 8.5
(a sum of positive terms) + the rounding to fp32, R_TRUST = 18.  v' = momentum*v + (lr*trust)*u: rate (18 + 1),
u = g*grad_scale (1) + wd*w (1), add (1), rate*u (1), the final add (1), R_MOM = 24; w' = w - v', R_W = 25.  With
``trust`` taken as stored (the update's ``fmaf`` chain alone): R_MOM_UPD = 6, R_W_UPD = 7."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
U = 2.0 ** -24
R_TRUST, R_MOM, R_W, R_MOM_UPD, R_W_UPD = 18, 24, 25, 6, 7
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# a padded group-1 slot, one partial chunk, three chunks (the last: 5 live elements), a zero gradient, a zero weight
SHAPES = {"b5": (5,), "w8": (8, 8), "w3": (3, 1367), "gzero": (6, 50), "wzero": (9, 33)}
H = dict(lr=0.7, momentum=0.9, weight_decay=0.05, eta=0.02, eps=1e-9)


def _mixed(n, gen):
    return torch.randn(n, generator=gen) * torch.tensor([1e-3, 1.0, 30.0])[torch.randint(0, 3, (n,), generator=gen)]


def _space(device):
    from kubedl_amd.ops.optim import FlatParamSpace
    mod = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.zeros(s)) for k, s in SHAPES.items()})
    return FlatParamSpace(mod.to(device), grad_mode="view")


@functools.lru_cache(maxsize=None)
def _inputs():
    """CPU fp32 flat buffers (never modified): values in the slots, zeros in their padding to 8, patterns between."""
    sp, gen = _space("cpu"), torch.Generator().manual_seed(4)
    assert sp.chunk == 2048 and {s.name: s.group for s in sp.slots} == {k: int(k == "b5") for k in SHAPES}
    pat = (torch.arange(sp.numel) % 13).float()
    w, g, v = 1.5 + pat, 0.5 + pat, -2.25 - pat
    for s in sp.slots:
        for buf, zero in ((w, s.name == "wzero"), (g, s.name == "gzero"), (v, False)):
            buf[s.offset:s.offset + (s.numel + 7) // 8 * 8] = 0
            if not zero:
                buf[s.offset:s.offset + s.numel] = _mixed(s.numel, gen)
    return sp.slots, w, g, v, -3.0 - pat


def _ref(slots, g, w, v, gs, first, trust=None):
    """The class docstring's definition in fp64 on the fp32 / bf16 inputs: trust, (v', A), (w', A), processed mask."""
    g, w, v = (t.double().numpy() for t in (g, w, v))
    lr, m, wd, eta, eps = (float(np.float32(H[k])) for k in ("lr", "momentum", "weight_decay", "eta", "eps"))
    tr, proc, v1, Av = np.ones(len(slots)), np.zeros(len(w), bool), np.zeros_like(w), np.zeros_like(w)
    for t, s in enumerate(slots):
        sl = slice(s.offset, s.offset + (s.numel + 7) // 8 * 8)
        proc[sl] = True
        gk, wk, wdk = g[sl] * float(np.float32(gs)), w[sl], wd if s.group == 0 else 0.0
        wn, gn = np.sqrt(np.sum(wk * wk)), np.sqrt(np.sum(gk * gk))
        if s.group == 0 and wn > 0 and gn > 0:
            tr[t] = eta * wn / (gn + wd * wn + eps)
        rate = lr * (tr[t] if trust is None else trust[t])
        mv = 0.0 if first else m * v[sl]
        v1[sl], Av[sl] = mv + rate * (gk + wdk * wk), np.abs(mv) + rate * (np.abs(gk) + wdk * np.abs(wk))
    return tr, (v1, Av), (np.where(proc, w - v1, w), np.abs(w) + Av), proc


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _step(device, gname, pname, first, gs):
    from kubedl_amd.ops.optim import FusedLARS
    _, w, g, v, fill = _inputs()
    sp = _space(device)
    sp.master.copy_(w)
    sp.grad, sp.param = g.to(device, DT[gname], copy=True), fill.to(device, DT[pname], copy=True)  # dtypes of their own
    opt = FusedLARS(sp, **H)
    opt.mom.copy_(v)
    opt.step_count, opt.grad_scale = (0 if first else 1), gs
    opt.step()
    return sp, opt


def _check(tag, got, ref, A, R, mask):
    err, bnd = np.abs(got.double().cpu().numpy() - ref)[mask], (R * U * A)[mask]
    assert (err <= bnd).all(), f"{tag}: worst error / bound {np.max(err / np.maximum(bnd, 1e-300)):.3f} (R = {R})"


@gpu
@pytest.mark.parametrize("gs", [1.0, 0.125])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("pname", ["f32", "bf16"])
@pytest.mark.parametrize("gname", ["f32", "bf16"])
def test_lars_kernels(gname, pname, first, gs):
    tag = f"lars[g {gname} p {pname} first={first} grad_scale {gs}]"
    slots, w, g, v, fill = _inputs()
    sp, opt = _step("cuda", gname, pname, first, gs)
    tr, (v1, Av), (w1, Aw), proc = _ref(slots, g.to(DT[gname]), w, v, gs, first)
    got = opt.trust.double().cpu().numpy()
    assert (np.abs(got - tr) <= R_TRUST * U * tr).all(), f"{tag}: trust {got} vs {tr}"
    assert all((got[t] != 1) == (s.name in ("w8", "w3")) for t, s in enumerate(slots)), f"{tag}: trust {got}"
    _check(tag + " mom", opt.mom, v1, Av, R_MOM, proc)
    _check(tag + " master", sp.master, w1, Aw, R_W, proc)
    keep = torch.from_numpy(~proc)  # outside the chunk table nothing is written; grad is read only
    want = torch.where(keep, fill.to(DT[pname]), sp.master.cpu().to(DT[pname]))
    assert torch.equal(_bits(sp.param), _bits(want)), f"{tag}: param is not the rounded master / the pattern outside"
    assert torch.equal(_bits(sp.master)[keep], _bits(w)[keep]) and torch.equal(_bits(opt.mom)[keep], _bits(v)[keep])
    assert torch.equal(_bits(sp.grad), _bits(g.to(DT[gname])))
    sp2, opt2 = _step("cuda", gname, pname, first, gs)
    for a, b in ((sp.master, sp2.master), (opt.mom, opt2.mom), (sp.param, sp2.param), (opt.trust, opt2.trust)):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: two calls from equal state differ"


@gpu
def test_lars_blocks_of_a_tensor_share_one_ratio():
    """Every chunk of the three-chunk tensor, recomputed in fp64 from the stored ``trust[t]``, lies inside the update's
    own bound: no block formed a ratio of its own."""
    sp, opt = _step("cuda", "bf16", "bf16", False, 0.125)
    slots, w, g, v, _ = _inputs()
    _, (v1, Av), (w1, Aw), _ = _ref(slots, g.bfloat16(), w, v, 0.125, False, trust=opt.trust.double().cpu().numpy())
    s = next(s for s in slots if s.name == "w3")
    mask = np.zeros(len(w1), bool)
    mask[s.offset:s.offset + s.numel] = True
    _check("w3 mom from the stored ratio", opt.mom, v1, Av, R_MOM_UPD, mask)
    _check("w3 master from the stored ratio", sp.master, w1, Aw, R_W_UPD, mask)


def test_lars_cpu_path_three_steps():
    """The torch-op path of ``FusedLARS.step`` (norms in fp64, the update in fp32), teacher-forced as in test_optim_gpu."""
    from kubedl_amd.ops.optim import FusedLARS
    slots, w, g, _, _ = _inputs()
    sp = _space("cpu")
    sp.master.copy_(w)
    opt = FusedLARS(sp, **H)
    opt.grad_scale = 0.125
    for k in range(3):
        w0, v0 = sp.master.clone(), opt.mom.clone()
        sp.grad.copy_(g * (k + 1))
        opt.step()
        tr, (v1, Av), (w1, Aw), proc = _ref(slots, sp.grad, w0, v0, 0.125, k == 0)
        assert np.allclose(opt.trust.numpy(), tr, rtol=R_TRUST * U, atol=0)
        _check(f"cpu step {k + 1} mom", opt.mom, v1, Av, R_MOM, proc)  # (a slot's zero padding stays zero)
        _check(f"cpu step {k + 1} master", sp.master, w1, Aw, R_W, proc)
        assert torch.equal(sp.param, sp.master) and opt.step_count == k + 1


@gpu
@pytest.mark.parametrize("L", [10, 300])
def test_smoothed_head(L, n=8, c=64, hw=2, eps=0.1):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(n, hw, hw, c, device="cuda", generator=g).relu().bfloat16().permute(0, 3, 1, 2)
    w = (torch.randn(L, c, device="cuda", generator=g) * 0.05).bfloat16()
    b = (torch.randn(L, device="cuda", generator=g) * 0.1).bfloat16()
    y = torch.randint(0, L, (n,), device="cuda", generator=g)
    s1, s2 = ext.head_splits(n, c, L)
    bf = dict(dtype=torch.bfloat16, device="cuda")

    def run(*smooth):
        o = dict(feat=torch.empty(n, c, **bf), lrow=torch.empty(n, device="cuda"), dl=torch.empty(n, ext.head_lpad(L), **bf),
                 dlT=torch.empty(L, n, **bf), loss=torch.empty(1, device="cuda"), dfeat=torch.empty(n, c, **bf),
                 dw=torch.empty(L, c, **bf), db=torch.empty(L, **bf))
        ext.head_forward(x, w, b, y, o["feat"], torch.empty(s1 * n * L, device="cuda"), o["lrow"], o["dl"], o["dlT"], *smooth)
        ext.head_backward(o["feat"], w, o["dl"], o["dlT"], torch.empty(s2 * n * c, device="cuda"), o["dfeat"], o["dw"],
                          o["db"], o["lrow"], o["loss"])
        torch.cuda.synchronize()
        return o

    plain, zero, sm = run(), run(0.0), run(eps)
    assert all(torch.equal(_bits(plain[k]), _bits(zero[k])) for k in plain)  # eps = 0: today's launch, bit for bit
    z = sm["feat"].double() @ w.double().t() + b.double()  # fp64 from the bf16 features the kernel made and used
    lse, zy = torch.logsumexp(z, 1), z.gather(1, y[:, None])[:, 0]
    lrow = lse - (1 - eps) * zy - eps / L * z.sum(1)
    dl = (torch.softmax(z, 1) - (1 - eps) * torch.nn.functional.one_hot(y, L) - eps / L) / n
    # tests/test_head_gpu.py's tolerances for the loss and for a bf16 gradient, widened by the smoothing's counted extra
    # fp32 roundings only: one more block sum (1 + 6 + 3 adds) and two more multiplies, 12 * 2^-24 of the terms' size
    extra = 12 * U * (lse.abs() + zy.abs() + eps / L * z.abs().sum(1)).max().item()
    torch.testing.assert_close(sm["lrow"].double(), lrow, atol=2e-3 + extra, rtol=2e-3)
    torch.testing.assert_close(sm["dl"][:, :L].double(), dl, atol=1e-2 * dl.abs().max().item() + 12 * U / n, rtol=2e-2)
    assert torch.equal(sm["dl"][:, :L].t(), sm["dlT"]) and not sm["dl"][:, L:].any()
