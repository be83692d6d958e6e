"""csrc/augment.hip on the MI355X: the kernel's x must be bit-equal to
``augment_reference`` (kubedl_amd/data/augment.py, run on the CPU) and y equal,
for every geometry, box and store path; plus the binding's checks, ShardInput's
two modes on the GPU and the trainer reading its batches from an input.

Every launch writes into a view inside a larger sentinel-filled buffer and the
bytes around the view are checked afterwards.
"""
import numpy as np
import pytest
import torch

from kubedl_amd.data import plan as P
from kubedl_amd.data.augment import augment_batch, augment_reference, norm_coeffs
from kubedl_amd.data.shards import IMAGENET_MEAN as MEAN, IMAGENET_STD as STD

pytestmark = pytest.mark.gpu

PAD = 64          # sentinel elements on each side of x (a multiple of 8: x stays 16-byte aligned)
SENT = 12352.0    # exactly representable in bf16, far from any normalised pixel


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(img_d, lab_d, rows, OH, OW, row0=0, B=None, mean=MEAN, std=STD):
    """Run the kernel into a guarded view; returns (x, y) on the CPU after checking the guards."""
    dev = img_d.device
    rows_d = torch.as_tensor(np.asarray(rows, np.int32)).to(dev)
    B = rows_d.size(0) - row0 if B is None else B
    A, Bc = norm_coeffs(mean, std)
    n = B * OH * OW * 3
    buf = torch.full((PAD + n + PAD,), SENT, dtype=torch.bfloat16, device=dev)
    x = buf[PAD:PAD + n].view(B, OH, OW, 3).permute(0, 3, 1, 2)
    ybuf = torch.full((B + 2,), -7, dtype=torch.int64, device=dev)
    augment_batch(img_d, lab_d, rows_d, row0, B, OH, OW, A, Bc, x, ybuf[1:B + 1])
    torch.cuda.synchronize()
    sent = _bits(torch.tensor([SENT], dtype=torch.bfloat16))[0].item()
    assert (_bits(buf[:PAD]) == sent).all() and (_bits(buf[PAD + n:]) == sent).all(), "wrote outside x"
    assert ybuf[0].item() == -7 and ybuf[-1].item() == -7, "wrote outside y"
    return x.cpu(), ybuf[1:B + 1].cpu()


def _check(img, lab, rows, OH, OW, row0=0, B=None, **kw):
    dev = _dev()
    rows = np.asarray(rows, np.int32)
    P.EpochPlan(rows, img.shape[0], img.shape[1], img.shape[2]).validate()
    x, y = _launch(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), rows, OH, OW, row0, B, **kw)
    hi = len(rows) if B is None else row0 + B
    xr, yr = augment_reference(torch.from_numpy(img), torch.from_numpy(lab), torch.from_numpy(rows[row0:hi]),
                               OH, OW, kw.get("mean", MEAN), kw.get("std", STD))
    assert torch.equal(y, yr)
    bad = (_bits(x.permute(0, 2, 3, 1)) != _bits(xr.permute(0, 2, 3, 1)))
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} values differ, first at {bad.nonzero()[0].tolist()}"


def _set(n, H, W, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, H, W, 3), dtype=np.uint8), g.integers(0, 1000, n, dtype=np.int64)


def _boxes(n, H, W, OH, OW):
    """Boxes touching each border and corner, the full image, the identity box
    (where it fits), 1x1, h = 1 with w > 1 and w = 1 with h > 1; flips mixed;
    src repeated and descending."""
    h2, w2 = max(H // 2, 1), max(W // 2, 1)
    b = [(0, 0, h2, w2), (0, W - w2, h2, w2), (H - h2, 0, h2, w2), (H - h2, W - w2, h2, w2),   # corners
         (0, 1, h2, W - 2), (H - h2, 1, h2, W - 2), (1, 0, H - 2, w2), (1, W - w2, H - 2, w2),  # one border each
         (0, 0, H, W), (H - 1, W - 1, 1, 1), (0, 0, 1, 1), (H // 3, 0, 1, W), (0, W // 3, H, 1),
         (1, 1, H - 2, W - 2)]
    if OH <= H and OW <= W:
        b += [(H - OH, W - OW, OH, OW), ((H - OH) // 2, (W - OW) // 2, OH, OW)]  # identity boxes
    rows = []
    for i, (y0, x0, h, w) in enumerate(b):
        rows.append([(len(b) - 1 - i) // 2 % n, y0, x0, h, w, (i // 2 + i) % 2, 0, 0])  # src descending, in pairs
    return rows


@pytest.mark.parametrize("H,W,OH,OW", [(9, 11, 8, 8), (9, 11, 7, 13), (40, 36, 16, 16), (9, 11, 1, 1), (5, 4, 37, 3),
                                       (12, 16, 3, 512), (16, 12, 512, 5), (16, 12, 120, 37)])
def test_small_geometries_bit_equal(H, W, OH, OW):
    # 7x13, 37x3, 512x5: OW (and OH * OW) no multiple of 8 -- 8-pixel groups cut by the
    # image's ends; 120x37: two row tiles per image (111 + 9 rows), the group at their seam
    # shared between two blocks; 3x512, 512x5: the largest tables
    img, lab = _set(5, H, W, H * 1000 + W)
    _check(img, lab, _boxes(5, H, W, OH, OW), OH, OW)


def test_stored_256_to_224_batch_3():
    img, lab = _set(4, 256, 256, 1)
    rows = [[3, 17, 40, 180, 139, 1, 0, 0], [1, 16, 16, 224, 224, 0, 0, 0], [3, 0, 0, 256, 256, 1, 0, 0]]
    _check(img, lab, rows, 224, 224)


def test_row0_into_a_longer_table_and_batch_sizes():
    img, lab = _set(6, 40, 36, 2)
    rows = _boxes(6, 40, 36, 20, 18)
    _check(img, lab, rows, 20, 18, row0=5, B=4)
    _check(img, lab, rows, 20, 18, row0=len(rows) - 1, B=1)   # B = 1, the table's last row
    _check(img, lab, rows[:1], 20, 18)                        # B = 1, a one-row table
    five = [[4, 0, 0, 40, 36, 0, 0, 0], [4, 3, 5, 30, 7, 1, 0, 0], [0, 39, 0, 1, 36, 1, 0, 0],
            [2, 10, 10, 20, 18, 0, 0, 0], [1, 0, 35, 40, 1, 0, 0, 0]]
    _check(img, lab, five, 20, 18)                            # B = 5, five different boxes
    _check(img, lab, five, 20, 18, mean=[10.5, 0, 200], std=[1, 255, 3.25])  # other statistics


def test_offsets_beyond_2_31_and_2_32_bytes():
    dev = _dev()
    n, need = 22000, 22000 * 256 * 256 * 3
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need + (1 << 30):
        pytest.skip(f"needs {need / 2**30:.1f} GiB of device memory for the image array, {free / 2**30:.1f} GiB free")
    pick = [0, 10999, 21999]  # byte offsets 0, 2.16e9 (> 2^31) and 4.33e9 (> 2^32)
    small, _ = _set(3, 256, 256, 9)
    lab = np.arange(n, dtype=np.int64) % 1000
    big = torch.zeros(n, 256, 256, 3, dtype=torch.uint8, device=dev)
    for k, i in enumerate(pick):
        big[i].copy_(torch.from_numpy(small[k]))
    rows = np.asarray([[21999, 5, 9, 200, 170, 1, 0, 0], [10999, 16, 16, 224, 224, 0, 0, 0],
                       [0, 0, 0, 256, 256, 0, 0, 0], [21999, 255, 255, 1, 1, 0, 0, 0]], np.int32)
    x, y = _launch(big, torch.from_numpy(lab).to(dev), rows, 224, 224)
    del big
    local = rows.copy()
    local[:, 0] = [2, 1, 0, 2]
    xr, yr = augment_reference(torch.from_numpy(small), torch.from_numpy(lab[pick]), torch.from_numpy(local),
                               224, 224, MEAN, STD)
    assert torch.equal(y, yr) and torch.equal(_bits(x.permute(0, 2, 3, 1)), _bits(xr.permute(0, 2, 3, 1)))


def test_binding_rejects_bad_arguments():
    dev = _dev()
    img, lab = _set(3, 12, 12, 4)
    img_d, lab_d = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    rows = torch.tensor([[0, 0, 0, 12, 12, 0, 0, 0]] * 4, dtype=torch.int32, device=dev)
    A, Bc = norm_coeffs(MEAN, STD)

    def x_cl(B=2, OH=8, OW=8, device=dev):
        return torch.empty(B, OH, OW, 3, dtype=torch.bfloat16, device=device).permute(0, 3, 1, 2)

    def call(images=img_d, labels=lab_d, plan=rows, row0=0, B=2, x=None, y=None):
        x = x_cl() if x is None else x
        y = torch.empty(B, dtype=torch.int64, device=dev) if y is None else y
        augment_batch(images, labels, plan, row0, B, 8, 8, A, Bc, x, y)
    call()  # the well-formed call passes
    bad = [dict(images=img_d.to(torch.int8)), dict(images=img_d.float()), dict(labels=lab_d.int()),
           dict(plan=rows.long()), dict(x=x_cl().float()),
           dict(images=img_d.transpose(1, 2)),                                       # non-contiguous images
           dict(x=torch.empty(2, 3, 8, 8, dtype=torch.bfloat16, device=dev)),        # NCHW-contiguous x
           dict(x=torch.empty(2 * 8 * 8 * 3 + 8, dtype=torch.bfloat16, device=dev)[1:-7].view(2, 8, 8, 3)
                .permute(0, 3, 1, 2)),                                               # x not 16-byte aligned
           dict(row0=3), dict(row0=-1), dict(row0=4, B=1, x=x_cl(1)), dict(B=0, x=x_cl(0)),  # row0 + B > rows
           dict(x=x_cl(3)), dict(y=torch.empty(3, dtype=torch.int64, device=dev)),
           dict(x=x_cl(device="cpu")), dict(labels=lab_d.cpu()), dict(plan=rows.cpu()), dict(images=img_d.cpu())]
    if torch.cuda.device_count() > 1:
        bad.append(dict(x=x_cl(device=torch.device("cuda", 1))))  # two GPUs: mixed devices
    for kw in bad:
        with pytest.raises(RuntimeError, match="augment_batch"):
            call(**kw)
    with pytest.raises(RuntimeError, match="augment_batch"):
        augment_batch(img_d, lab_d, rows, 0, 2, 513, 8, A, Bc, x_cl(2, 513, 8), torch.empty(2, dtype=torch.int64,
                                                                                             device=dev))
    torch.cuda.synchronize()


# ================================================================ ShardInput and the trainer
def _info():
    from kubedl_amd.parallel.dist import DistInfo
    return DistInfo(rank=0, world_size=1, local_rank=0, device=_dev(), backend="nccl")


def _bits_eq(a, b):
    return torch.equal(_bits(a.permute(0, 2, 3, 1).cpu()), _bits(b.permute(0, 2, 3, 1).cpu()))


def test_shard_input_resident_equals_stream_and_reference(tmp_path):
    from kubedl_amd.data.input import ShardInput
    from kubedl_amd.data.shards import ImageShards, write_shards
    img, lab = _set(40, 36, 44, 6)
    lab %= 7
    write_shards(str(tmp_path), img, lab, 16, 7)
    sh = ImageShards.open(str(tmp_path))
    res = ShardInput(sh, _info(), 8, 24, seed=3, mode="resident")
    stm = ShardInput(sh, _info(), 8, 24, seed=3, mode="stream", workers=2)
    pl = P.InputPlan(40, 36, 44, 1, 0, 8, seed=3)
    assert res.steps_per_epoch == 5 and res.images.dtype == torch.uint8 and res.images.device.type == "cuda"
    prev = None
    for step in range(10):  # two epochs
        xa, ya = res.next(step)
        xb, yb = stm.next(step)
        xr, yr = augment_reference(torch.from_numpy(img), torch.from_numpy(lab),
                                   torch.from_numpy(pl.batch_rows(step)), 24, 24, sh.mean, sh.std)
        assert _bits_eq(xa, xr) and _bits_eq(xb, xr), step
        assert torch.equal(ya.cpu(), yr) and torch.equal(yb.cpu(), yr)
        assert res.plan_uploads == step // 5 + 1  # the epoch boundary re-uploads the plan, a step does not
        assert prev is None or prev.data_ptr() != xa.data_ptr()  # two x buffers alternate
        prev = xa
    ev = ShardInput(sh, _info(), 8, 24, train=False, mode="stream")
    got = [(x.clone(), y.clone()) for x, y in ev]
    assert len(got) == 5 and ev.dropped == 0
    rows = P.InputPlan(40, 36, 44, 1, 0, 8, train=False).epoch(0).rows
    xr, yr = augment_reference(torch.from_numpy(img), torch.from_numpy(lab), torch.from_numpy(rows), 24, 24,
                               sh.mean, sh.std)
    assert _bits_eq(torch.cat([x for x, _ in got]), xr) and torch.equal(torch.cat([y for _, y in got]).cpu(), yr)
    for i in (res, stm, ev):
        i.close()


@pytest.fixture(scope="module")
def shards32(tmp_path_factory):
    from kubedl_amd.data.shards import ImageShards, synthetic_images, write_shards
    d = tmp_path_factory.mktemp("s32")
    img, lab = synthetic_images(32, 10, 256, 0)
    write_shards(str(d), img, lab, 20, 10)
    return ImageShards.open(str(d)), img, lab


def _trainer(**kw):
    from kubedl_amd.workers.resnet50 import ResNetTrainer
    return ResNetTrainer(_info(), batch=8, image=224, num_classes=10, bn_backend="hip", **kw)  # smoke()'s geometry


def test_trainer_reads_its_batches_from_the_input(shards32):
    from kubedl_amd.data.input import ShardInput
    sh, img, lab = shards32
    inp = ShardInput(sh, _info(), 8, 224, seed=1, mode="resident")
    tr = _trainer(train_input=inp)
    assert tr.engine_kind == "fused" and tr.input is inp
    pl = P.InputPlan(32, 256, 256, 1, 0, 8, seed=1)
    for step in range(3):
        loss = float(tr.step())
        torch.cuda.synchronize()
        assert loss == loss and abs(loss) != float("inf")
        xr, yr = augment_reference(torch.from_numpy(img), torch.from_numpy(lab),
                                   torch.from_numpy(pl.batch_rows(step)), 224, 224, sh.mean, sh.std)
        assert _bits_eq(tr.x, xr) and torch.equal(tr.y.cpu(), yr), step
    assert tr.steps_done == 3
    ev = ShardInput(sh, _info(), 8, 224, train=False, mode="resident")
    out = tr.evaluate(ev)
    assert out["eval_images"] == 32 and out["eval_loss"] == out["eval_loss"]
    inp.close()
    ev.close()


def test_trainer_without_an_input_is_the_default_path():
    """Two no-input trainers from one seed: the same synthetic batch bit for bit and
    the same first-step loss (to the 1e-3 that tests/test_ddp_world1_gpu.py allows
    two runs of one step: the BN sums are fp32 atomics, their order varies)."""
    a, b = _trainer(seed=0), _trainer(seed=0)
    assert a.input is None and b.input is None
    assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y)
    xa = a.x.clone()
    la, lb = float(a.step()), float(b.step())
    torch.cuda.synchronize()
    assert torch.equal(a.x, xa)  # the step leaves the synthetic batch alone
    assert la == la and abs(la - lb) <= 1e-3 + 1e-3 * abs(lb), (la, lb)
