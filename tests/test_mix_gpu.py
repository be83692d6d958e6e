"""Mixup / CutMix on the MI355X: ``augment_mix_batch`` bit-equal to ``augment_mix_reference`` (run on the CPU) with
guard bytes around every output, its identities with ``augment_batch``, the two-label head against fp64, the bindings'
refusals, and ShardInput / the fused trainer on the mixed path."""
import numpy as np
import pytest
import torch

from kubedl_amd.data import plan as P
from kubedl_amd.data.augment import augment_batch, augment_mix_batch, augment_mix_reference, norm_coeffs
from kubedl_amd.data.shards import IMAGENET_MEAN as MEAN, IMAGENET_STD as STD
from test_augment_gpu import PAD, SENT, _bits, _info  # x's guard elements and their value, int16 views, a world-1 rank

pytestmark = pytest.mark.gpu
A, BC = norm_coeffs(MEAN, STD)
G = np.random.default_rng(11)
IMG = torch.from_numpy(G.integers(0, 256, (6, 37, 53, 3), dtype=np.uint8))
LAB = torch.from_numpy(G.integers(0, 1000, 6, dtype=np.int64))
# eight rows: distinct boxes and mixed flips inside every pair (b, B-1-b), a repeated src
ROWS = torch.tensor([[5, 0, 0, 37, 53, 0, 0, 0], [0, 3, 7, 20, 31, 1, 0, 0], [2, 36, 0, 1, 53, 1, 0, 0],
                     [4, 5, 50, 30, 3, 0, 0, 0], [1, 10, 10, 24, 40, 1, 0, 0], [3, 0, 52, 37, 1, 0, 0, 0],
                     [5, 17, 2, 9, 49, 0, 0, 0], [2, 1, 1, 35, 51, 1, 0, 0]], dtype=torch.int32)
NOBOX = (0, 0, 0, 0)


def _mix(B, OH, OW, kind, lam16=65536, box=NOBOX, plain=False, rows=ROWS):
    """One launch into guarded buffers: (x NHWC bits, y_a, y_b) on the CPU (y_b untouched for augment_batch)."""
    n = B * OH * OW * 3
    buf = torch.full((PAD + n + PAD,), SENT, dtype=torch.bfloat16, device="cuda")
    x = buf[PAD:PAD + n].view(B, OH, OW, 3).permute(0, 3, 1, 2)
    yy = torch.full((2, B + 2), -7, dtype=torch.int64, device="cuda")
    args = (IMG.cuda(), LAB.cuda(), rows.cuda(), 0, B, OH, OW, A, BC)
    if plain:
        augment_batch(*args, x, yy[0, 1:B + 1])
    else:
        augment_mix_batch(*args, kind, lam16, box, x, yy[0, 1:B + 1], yy[1, 1:B + 1])
    torch.cuda.synchronize()
    assert (buf[:PAD] == SENT).all() and (buf[PAD + n:] == SENT).all(), "wrote outside x"
    assert (yy[:, 0] == -7).all() and (yy[:, -1] == -7).all(), "wrote outside y_a / y_b"
    return _bits(buf[PAD:PAD + n].view(B, OH, OW, 3)).cpu(), yy[0, 1:B + 1].cpu(), yy[1, 1:B + 1].cpu()


# 24x40: whole groups only; 61x35: two row tiles per image (59 + 2 rows), OW and OH * OW no multiple of 8, so the
# tile seam and every image end cut a group and the two streams of a pair start at different offsets in a group
@pytest.mark.parametrize("OH,OW", [(24, 40), (61, 35)])
@pytest.mark.parametrize("B", [1, 2, 5, 8])
def test_mix_kernel_bit_equal_to_the_reference(B, OH, OW):
    # CutMix boxes: empty, full, one pixel, each corner / border, and one whose edges fall inside 8-pixel store
    # groups and across the row-tile seam; Mixup at the ends and the middle of lam16; kind none
    boxes = [NOBOX, (0, 0, OH, OW), (OH // 2, OW // 2, 1, 1), (0, 0, 5, 7), (OH - 5, OW - 7, 5, 7),
             (0, OW - 3, OH // 2, 3), (OH - 2, 0, 2, OW // 2), (OH - 4, 3, 3, 9)]
    cases = [(1, l, NOBOX) for l in (0, 1, 32768, 65535, 65536)] + [(0, 65536, NOBOX)] + [(2, 65536, b) for b in boxes]
    for kind, lam16, box in cases:
        x, ya, yb = _mix(B, OH, OW, kind, lam16, box)
        xr, yar, ybr, _ = augment_mix_reference(IMG, LAB, ROWS[:B], OH, OW, MEAN, STD, kind, lam16, box)
        bad = x != _bits(xr.permute(0, 2, 3, 1))
        assert not bad.any(), (kind, lam16, box, int(bad.sum()), bad.nonzero()[0].tolist())
        assert torch.equal(ya, yar) and torch.equal(yb, ybr), (kind, lam16, box)
        again = _mix(B, OH, OW, kind, lam16, box)
        assert torch.equal(again[0], x) and torch.equal(again[1], ya) and torch.equal(again[2], yb)


@pytest.mark.parametrize("B", [5, 8])
def test_identities_with_augment_batch(B, OH=61, OW=35):
    x0, y0, _ = _mix(B, OH, OW, 0, plain=True)
    for kind in (1, 2):  # Mixup at lam16 = 65536; CutMix with the empty box
        x, ya, yb = _mix(B, OH, OW, kind, 65536, NOBOX)
        assert torch.equal(x, x0) and torch.equal(ya, y0) and torch.equal(yb, y0.flip(0))
    xr, yr, _ = _mix(B, OH, OW, 0, plain=True, rows=ROWS[:B].flip(0))  # the batch order reversed
    x, ya, yb = _mix(B, OH, OW, 2, 65536, (0, 0, OH, OW))              # the full box
    assert torch.equal(x, xr) and torch.equal(ya, y0) and torch.equal(yb, yr)


def test_mix_binding_refusals():
    i64 = dict(dtype=torch.int64, device="cuda")
    ok = dict(images=IMG.cuda(), labels=LAB.cuda(), plan=ROWS.cuda(), B=4, kind=2, lam16=65536, box=(1, 2, 7, 6),
              x=torch.empty(4, 8, 8, 3, dtype=torch.bfloat16, device="cuda").permute(0, 3, 1, 2),
              y_a=torch.empty(4, **i64), y_b=torch.empty(4, **i64))

    def call(**kw):
        a = {**ok, **kw}
        augment_mix_batch(a["images"], a["labels"], a["plan"], 0, a["B"], 8, 8, A, BC, a["kind"], a["lam16"], a["box"],
                          a["x"], a["y_a"], a["y_b"])
    call()
    for kw in [dict(images=ok["images"].to(torch.int8)), dict(labels=ok["labels"].int()), dict(plan=ok["plan"].long()),
               dict(x=ok["x"].float()), dict(y_b=ok["y_b"].int()), dict(y_a=ok["y_a"][:3]), dict(B=9), dict(kind=3),
               dict(lam16=-1), dict(lam16=65537), dict(box=(1, 2, 8, 6)), dict(box=(0, 3, 1, 6)),
               dict(box=(-1, 0, 2, 2)), dict(box=(0, 0, 2, -1)), dict(box=(9, 0, 0, 0)), dict(box=(0, 0, 8))]:
        with pytest.raises(RuntimeError, match="augment_mix_batch"):
            call(**kw)


def _head(L, eps, y, y_b=None, lam=1.0, n=8, c=64, hw=2):
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(n, hw, hw, c, device="cuda", generator=g).relu().bfloat16().permute(0, 3, 1, 2)
    w = (torch.randn(L, c, device="cuda", generator=g) * 0.05).bfloat16()
    b = (torch.randn(L, device="cuda", generator=g) * 0.1).bfloat16()
    bf = dict(dtype=torch.bfloat16, device="cuda")
    o = dict(feat=torch.empty(n, c, **bf), lrow=torch.empty(n, device="cuda"), dl=torch.empty(n, ext.head_lpad(L), **bf),
             dlT=torch.empty(L, n, **bf))
    ext.head_forward(x, w, b, y, o["feat"], torch.empty(ext.head_splits(n, c, L)[0] * n * L, device="cuda"), o["lrow"],
                     o["dl"], o["dlT"], eps, *(() if y_b is None else (y_b, lam)))
    torch.cuda.synchronize()
    return o, o["feat"].double() @ w.double().t() + b.double()  # fp64 logits of the bf16 features the kernel used


@pytest.mark.parametrize("L", [10, 1000])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_two_label_head_against_fp64(L, eps, lam, n=8, U=2.0 ** -24):
    g = torch.Generator(device="cuda").manual_seed(3)
    ya, yb = torch.randint(0, L, (n,), device="cuda", generator=g), torch.randint(0, L, (n,), device="cuda", generator=g)
    yb[0] = ya[0]  # one image whose two labels agree
    o, z = _head(L, eps, ya, yb, lam)
    lf, oh = float(np.float32(lam)), torch.nn.functional.one_hot
    lse, zy = torch.logsumexp(z, 1), lf * z.gather(1, ya[:, None])[:, 0] + (1 - lf) * z.gather(1, yb[:, None])[:, 0]
    lrow = lse - (1 - eps) * zy - eps / L * z.sum(1)
    dl = (torch.softmax(z, 1) - (1 - eps) * (lf * oh(ya, L) + (1 - lf) * oh(yb, L)) - eps / L) / n
    # the tolerances of tests/test_lars_gpu.py::test_smoothed_head, its expressions unchanged
    extra = 12 * U * (lse.abs() + zy.abs() + eps / L * z.abs().sum(1)).max().item()
    torch.testing.assert_close(o["lrow"].double(), lrow, atol=2e-3 + extra, rtol=2e-3)
    torch.testing.assert_close(o["dl"][:, :L].double(), dl, atol=1e-2 * dl.abs().max().item() + 12 * U / n, rtol=2e-2)
    assert torch.equal(o["dl"][:, :L].t(), o["dlT"]) and not o["dl"][:, L:].any()
    if lam == 1.0:  # bit-equal to the one-label launch on y_a
        one, _ = _head(L, eps, ya)
        assert all(torch.equal(_bits(one[k]), _bits(o[k])) for k in one)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_two_label_head_equal_labels_and_bad_labels(eps, L=10, n=8):
    y = torch.arange(n, device="cuda") % L
    one, _ = _head(L, eps, y)
    for lam in (0.5, 0.75, 0.625):  # lam + (1 - lam) == 1 exactly in fp32
        o, _ = _head(L, eps, y, y.clone(), lam)
        assert all(torch.equal(_bits(one[k]), _bits(o[k])) for k in one), lam
    ya, yb = y.clone(), y.flip(0).clone()
    ya[1], yb[2] = -100, L
    o, _ = _head(L, eps, ya, yb, 0.3)
    assert o["lrow"].isnan().tolist() == [i in (1, 2) for i in range(n)]
    assert not o["dl"][1:3].any() and not o["dlT"][:, 1:3].any() and o["dl"][0].any() and o["dl"][3:].any(1).all()
    for bad, msg in (((y.clone(), 1.5), "mix_lam"), ((y.int(), 0.5), "y_b")):
        with pytest.raises(RuntimeError, match=msg):
            _head(L, eps, y, *bad)


def test_shard_input_and_trainer_on_the_mixed_path(tmp_path):
    from kubedl_amd.data.input import ShardInput
    from kubedl_amd.data.shards import ImageShards, synthetic_images, write_shards
    from kubedl_amd.workers.resnet50 import ResNetTrainer
    info = _info()
    img, lab = synthetic_images(32, 10, 256, 0)
    write_shards(str(tmp_path), img, lab, 20, 10)
    sh, cfg = ImageShards.open(str(tmp_path)), P.MixConfig(0.2, 1.0, prob=0.8)
    pl = P.InputPlan(32, 256, 256, 1, 0, 8, seed=1, mix=cfg)
    assert {pl.mix_draw(s, 224, 224).kind for s in range(6)} == {0, 1, 2}  # seed 1's first six steps draw every kind
    res, stm = (ShardInput(sh, info, 8, 224, seed=1, mode=m, mix=cfg) for m in ("resident", "stream"))
    tr = ResNetTrainer(info, batch=8, image=224, num_classes=10, bn_backend="hip", train_input=res, label_smoothing=0.1)
    for step in range(6):
        d = pl.mix_draw(step, 224, 224)
        loss = float(tr.step())
        assert tr.engine_kind == "fused" and loss == loss and abs(loss) != float("inf")
        xr, ya, yb, ll = augment_mix_reference(torch.from_numpy(img), torch.from_numpy(lab),
                                               torch.from_numpy(pl.batch_rows(step)), 224, 224, sh.mean, sh.std,
                                               d.kind, d.lam16, d.box)
        xs, yas, ybs, lls = stm.next(step)
        for x in (tr.x, xs):
            assert torch.equal(_bits(x.permute(0, 2, 3, 1)).cpu(), _bits(xr.permute(0, 2, 3, 1))), step
        assert torch.equal(tr.y.cpu(), ya) and torch.equal(yas.cpu(), ya) and lls == ll
        assert d.kind == P.MIX_NONE or torch.equal(ybs.cpu(), yb)
    res.close()
    stm.close()
