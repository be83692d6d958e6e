"""Image input on the CPU: shard sets, the host-side plan, the resample rule's
reference, the two ShardInput modes and the ResNet worker end to end
(kubedl_amd/data, workers/resnet50.py --data).
"""
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from kubedl_amd.data import plan as P
from kubedl_amd.data.augment import augment_reference, norm_coeffs, normalize_q, resample_q
from kubedl_amd.data.input import ShardInput
from kubedl_amd.data.shards import IMAGENET_MEAN, IMAGENET_STD, ImageShards, synthetic_images, write_shards
from kubedl_amd.parallel.dist import DistInfo

PY = sys.executable
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = IMAGENET_MEAN, IMAGENET_STD


def _rand_set(n, H=12, W=10, classes=5, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, H, W, 3), dtype=np.uint8), g.integers(0, classes, n, dtype=np.int64)


def _info(rank=0, world=1):
    return DistInfo(rank, world, 0, torch.device("cpu"), "gloo")


# ================================================================ 1. shard sets
def test_write_open_round_trip_ragged(tmp_path):
    img, lab = _rand_set(25)
    meta = write_shards(str(tmp_path), img, lab, 10, 5, mean=[1, 2, 3], std=[4, 5, 6])
    assert [s["count"] for s in meta["shards"]] == [10, 10, 5]
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]
    sh = ImageShards.open(str(tmp_path))
    assert (sh.count, sh.height, sh.width, sh.classes) == (25, 12, 10, 5)
    assert sh.mean == (1.0, 2.0, 3.0) and sh.std == (4.0, 5.0, 6.0)
    assert np.array_equal(np.concatenate(sh.images), img) and np.array_equal(np.concatenate(sh.labels), lab)
    assert isinstance(sh.images[0], np.memmap)
    idx = [24, 0, 9, 10, 19, 20]
    assert np.array_equal(sh.gather(idx), img[idx]) and np.array_equal(sh.gather_labels(idx), lab[idx])
    # the defaults: the ImageNet statistics in 0..255 units
    write_shards(str(tmp_path / "d"), img, lab, 25, 5)
    assert ImageShards.open(str(tmp_path / "d")).mean == pytest.approx((123.675, 116.28, 103.53))


def _set(tmp_path):
    img, lab = _rand_set(25)
    write_shards(str(tmp_path), img, lab, 10, 5)
    return img, lab


def _edit_meta(tmp_path, **kw):
    m = json.load(open(tmp_path / "meta.json"))
    m.update(kw)
    json.dump(m, open(tmp_path / "meta.json", "w"))


def test_open_names_the_file_bad_dtype(tmp_path):
    img, _ = _set(tmp_path)
    np.save(tmp_path / "images-00001.npy", img[10:20].astype(np.int16))
    with pytest.raises(ValueError, match=r"images-00001\.npy.*dtype int16"):
        ImageShards.open(str(tmp_path))
    np.save(tmp_path / "images-00001.npy", img[10:20])
    np.save(tmp_path / "labels-00002.npy", np.zeros(5, np.int32))
    with pytest.raises(ValueError, match=r"labels-00002\.npy.*dtype int32"):
        ImageShards.open(str(tmp_path))


def test_open_names_the_file_count_mismatch(tmp_path):
    img, _ = _set(tmp_path)
    _edit_meta(tmp_path, count=26)
    with pytest.raises(ValueError, match=r"meta\.json.*sum to 25.*26"):
        ImageShards.open(str(tmp_path))
    _edit_meta(tmp_path, count=25)
    np.save(tmp_path / "images-00002.npy", img[20:24])  # a shard shorter than its count
    with pytest.raises(ValueError, match=r"images-00002\.npy.*shape"):
        ImageShards.open(str(tmp_path))


def test_open_names_the_file_label_out_of_range(tmp_path):
    _set(tmp_path)
    np.save(tmp_path / "labels-00001.npy", np.full(10, 5, np.int64))
    with pytest.raises(ValueError, match=r"labels-00001\.npy.*outside \[0, 5\)"):
        ImageShards.open(str(tmp_path))


def test_open_names_the_file_newer_version(tmp_path):
    _set(tmp_path)
    _edit_meta(tmp_path, version=2)
    with pytest.raises(ValueError, match=r"meta\.json.*version 2"):
        ImageShards.open(str(tmp_path))


# ================================================================ 2. the plan
def test_epoch_covers_owned_images_once_and_ranks_are_disjoint():
    N, batch = 103, 8
    for world in (2, 3):
        seen = []
        spe = {P.InputPlan(N, 20, 24, world, r, batch).steps_per_epoch for r in range(world)}
        assert spe == {(N // world) // batch}  # equal across ranks with a ragged N, no collective
        for r in range(world):
            pl = P.InputPlan(N, 20, 24, world, r, batch, seed=3)
            assert pl.n_own == len(range(r, N, world))
            ep = pl.epoch(0)
            src = ep.rows[:, 0]
            assert len(src) == pl.steps_per_epoch * batch and len(set(src.tolist())) == len(src)
            assert pl.dropped == pl.n_own - len(src)
            g = pl.global_index(src)
            assert (g % world == r).all() and g.max() < N
            seen.append(set(g.tolist()))
        for a in range(world):
            for b in range(a + 1, world):
                assert not (seen[a] & seen[b])


def test_plan_of_a_step_is_a_pure_function_and_epochs_differ():
    pl = P.InputPlan(70, 20, 24, 2, 1, 4, seed=5)
    spe = pl.steps_per_epoch
    assert spe == 8
    full = [pl.epoch(e).rows for e in range(3)]
    for step in (0, 3, spe - 1, spe, spe + 5, 2 * spe + 7):  # from any resume point: a fresh object
        fresh = P.InputPlan(70, 20, 24, 2, 1, 4, seed=5)
        e, r0 = fresh.locate(step)
        assert (e, r0) == (step // spe, (step % spe) * 4)
        assert np.array_equal(fresh.batch_rows(step), full[e][r0:r0 + 4])
    assert not np.array_equal(full[0], full[1]) and not np.array_equal(full[1], full[2])
    assert not np.array_equal(full[0][:, 0], full[1][:, 0])  # the order too, not only the boxes
    assert not np.array_equal(P.InputPlan(70, 20, 24, 2, 1, 4, seed=6).epoch(0).rows, full[0])


@pytest.mark.parametrize("H,W", [(256, 256), (40, 36), (9, 11), (30, 200)])
def test_boxes_inside_and_within_scale_and_ratio_or_fallback(H, W):
    n = 4000
    b = P.random_boxes(np.random.Generator(np.random.PCG64([1, 2, 3])), n, H, W)
    y0, x0, h, w = (b[:, i].astype(np.float64) for i in range(4))
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= H).all() and (x0 + w <= W).all()
    fb = (b == np.array(P.fallback_box(H, W))).all(axis=1)
    # h and w are the real-valued sides rounded to integers: each is within 0.5 of
    # a pair whose area / (H W) lies in SCALE and whose ratio lies in RATIO
    area_ok = ((w - .5) * (h - .5) <= P.SCALE[1] * H * W) & ((w + .5) * (h + .5) >= P.SCALE[0] * H * W)
    ratio_ok = ((w - .5) / (h + .5) <= P.RATIO[1]) & ((w + .5) / np.maximum(h - .5, 1e-9) >= P.RATIO[0])
    assert (fb | (area_ok & ratio_ok)).all()
    if (H, W) == (256, 256):
        assert fb.mean() < 0.01 and len(np.unique(b, axis=0)) > n // 2
    if (H, W) == (30, 200):  # ratio 6.67: the fallback is the central 30 x 40 crop
        assert P.fallback_box(H, W) == (0, 80, 30, 40)


def test_flip_is_about_half():
    rows = P.InputPlan(4096, 32, 32, 1, 0, 4096, seed=11).epoch(0).rows
    k, n = int(rows[:, 5].sum()), 4096
    assert set(np.unique(rows[:, 5])) == {0, 1}
    assert abs(k - n / 2) < 5 * math.sqrt(n / 4)  # 5 sigma of Binomial(4096, 0.5): 160


def test_eval_plan_is_natural_order_central_box_no_flip():
    pl = P.InputPlan(45, 256, 256, 2, 1, 8, train=False)
    assert pl.n_own == 22 and pl.steps_per_epoch == 2 and pl.dropped == 6
    rows = pl.epoch(0).rows
    assert rows[:, 0].tolist() == list(range(16)) and (rows[:, 5] == 0).all()
    assert (rows[:, 1:5] == [16, 16, 224, 224]).all()  # 256 stored, 224 out: an exact copy
    assert P.eval_box(40, 36) == (2, 2, 35, 32)  # round-half-even of 31.5


@pytest.mark.parametrize("col,val,msg", [(0, -1, "src"), (0, 7, "src"), (1, -1, "outside"), (2, 8, "outside"),
                                         (3, 0, "empty"), (4, 0, "empty"), (3, 12, "outside"), (4, 11, "outside"),
                                         (5, 2, "flip"), (5, -1, "flip")])
def test_validate_rejects_each_kind_of_bad_row(col, val, msg):
    rows = np.zeros((3, 8), np.int32)
    rows[:, 3], rows[:, 4] = 5, 4
    rows[:, 0] = [0, 6, 3]
    ep = P.EpochPlan(rows, 7, 10, 9)
    assert ep.validate() is ep
    rows[1, col] = val
    with pytest.raises(ValueError, match=rf"plan row 1 .*{msg}"):
        ep.validate()
    with pytest.raises(ValueError, match="int32"):
        P.EpochPlan(rows.astype(np.int64), 7, 10, 9).validate()


# ================================================================ 3. the resample rule's reference
def _row(src, y0, x0, h, w, flip=0):
    return [src, y0, x0, h, w, flip, 0, 0]


def _bilinear64(img, y0, x0, h, w, OH, OW):
    """Independent fp64 bilinear sample of the box (half-pixel centres, edge clamp)."""
    box = img[y0:y0 + h, x0:x0 + w].astype(np.float64)
    sy = np.clip((np.arange(OH) + 0.5) * h / OH - 0.5, 0, h - 1)
    sx = np.clip((np.arange(OW) + 0.5) * w / OW - 0.5, 0, w - 1)
    yl, xl = np.floor(sy).astype(int), np.floor(sx).astype(int)
    yh, xr = np.minimum(yl + 1, h - 1), np.minimum(xl + 1, w - 1)
    fy, fx = (sy - yl)[:, None, None], (sx - xl)[None, :, None]
    top = box[yl][:, xl] * (1 - fx) + box[yl][:, xr] * fx
    bot = box[yh][:, xl] * (1 - fx) + box[yh][:, xr] * fx
    return top * (1 - fy) + bot * fy


def test_identity_box_is_the_slice_and_flip_is_torch_flip():
    img, lab = _rand_set(4, 20, 24)
    ti, tl = torch.from_numpy(img), torch.from_numpy(lab)
    rows = torch.tensor([_row(2, 3, 5, 8, 13), _row(2, 3, 5, 8, 13, 1), _row(0, 0, 0, 20, 24), _row(3, 1, 2, 11, 6, 1)])
    q = resample_q(ti, rows[:2], 8, 13)
    assert q.min() >= 0 and q.max() <= 255
    assert torch.equal(q[0], ti[2, 3:11, 5:18].long())          # h == OH, w == OW: every weight is 0
    assert torch.equal(q[1], torch.flip(q[0], dims=[1]))
    x, y = augment_reference(ti, tl, rows, 7, 9, MEAN, STD)
    assert x.shape == (4, 3, 7, 9) and x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, tl[[2, 2, 0, 3]])
    assert torch.equal(x[1], torch.flip(x[0], dims=[2]))
    unfl = augment_reference(ti, tl, torch.tensor([_row(3, 1, 2, 11, 6, 0)]), 7, 9, MEAN, STD)[0]
    assert torch.equal(x[3], torch.flip(unfl[0], dims=[2]))


def test_one_by_one_box_is_constant():
    img, lab = _rand_set(2, 9, 11)
    q = resample_q(torch.from_numpy(img), torch.tensor([_row(1, 4, 7, 1, 1), _row(1, 4, 7, 1, 1, 1)]), 6, 5)
    assert torch.equal(q, torch.from_numpy(img[1, 4, 7]).long().expand(2, 6, 5, 3))


@pytest.mark.parametrize("H,W,OH,OW", [(3, 3, 16, 16), (31, 31, 8, 8), (7, 13, 13, 7), (40, 36, 16, 16), (13, 7, 5, 9)])
def test_q_is_within_one_and_a_half_levels_of_exact_bilinear(H, W, OH, OW):
    g = np.random.default_rng(H * 100 + W)
    img = g.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    rows = [_row(0, 0, 0, H, W)]
    for _ in range(40):
        h, w = int(g.integers(1, H + 1)), int(g.integers(1, W + 1))
        rows.append(_row(int(g.integers(0, 3)), int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1)), h, w))
    q = resample_q(torch.from_numpy(img), torch.tensor(rows), OH, OW).numpy()
    worst = 0.0
    for i, (s, y0, x0, h, w, *_) in enumerate(rows):
        worst = max(worst, float(np.abs(q[i] - _bilinear64(img[s], y0, x0, h, w, OH, OW)).max()))
    # 2^-9 * 255 per axis from the 8-bit weights + 0.5 from the final rounding
    assert worst < 1.5, worst


def test_normalise_equals_fp64_expression_for_all_768_inputs():
    q = torch.arange(256)[:, None].expand(256, 3)
    got = normalize_q(q, MEAN, STD)
    A, B = norm_coeffs(MEAN, STD)
    assert A.dtype == np.float32 and B.dtype == np.float32
    for c in range(3):
        a, b = float(A[c]), float(B[c])
        assert a == np.float32(1.0 / STD[c]) and b == np.float32(-MEAN[c] / STD[c])
        want = torch.tensor([v * a + b for v in range(256)], dtype=torch.float64).float().bfloat16()
        assert torch.equal(got[:, c], want)
        # the fp64 value is the exact real one, so rounding it once is what an fp32 fma does
        from fractions import Fraction
        assert all(Fraction(v) * Fraction(a) + Fraction(b) == Fraction(v * a + b) for v in range(256))


# ================================================================ 4. ShardInput on the CPU
def _unique_set(tmp_path, n, H=12, W=10, classes=5):
    """Image i is filled with the bytes of i: what a batch shows says which images it read."""
    img = np.zeros((n, H, W, 3), np.uint8)
    img += np.arange(n, dtype=np.uint8)[:, None, None, None]
    lab = (np.arange(n) % classes).astype(np.int64)
    write_shards(str(tmp_path), img, lab, 16, classes, mean=[0, 0, 0], std=[1, 1, 1])
    return ImageShards.open(str(tmp_path))


def test_stream_equals_resident_for_two_epochs(tmp_path):
    img, lab = _rand_set(50, 14, 12)
    write_shards(str(tmp_path), img, lab, 16, 5)
    sh = ImageShards.open(str(tmp_path))
    before = threading.active_count()
    a = ShardInput(sh, _info(), 8, 10, seed=2, mode="resident")
    b = ShardInput(sh, _info(), 8, 10, seed=2, mode="stream", workers=2)
    assert (a.mode, b.mode, a.steps_per_epoch, a.dropped) == ("resident", "stream", 6, 2)
    ref_rows = P.InputPlan(50, 14, 12, 1, 0, 8, seed=2)
    for step in range(12):
        xa, ya = a.next(step)
        xb, yb = b.next(step)
        assert torch.equal(xa, xb) and torch.equal(ya, yb), step
        xr, yr = augment_reference(torch.from_numpy(img), torch.from_numpy(lab),
                                   torch.from_numpy(ref_rows.batch_rows(step)), 10, 10, sh.mean, sh.std)
        assert torch.equal(xa, xr) and torch.equal(ya, yr)
    assert b.data_wait_ms > 0
    xj, _ = b.next(3)  # a jump (a resume point) restarts the loader at that step
    assert torch.equal(xj, a.next(3)[0])
    a.close()
    b.close()
    assert threading.active_count() == before
    assert not [t for t in threading.enumerate() if t.name.startswith("kdl-")]
    assert ShardInput(sh, _info(), 8, 10, mode="auto").mode == "resident"
    assert ShardInput(sh, _info(), 8, 10, mode="auto", resident_gb=1e-9).mode == "stream"


def test_loader_exception_surfaces_in_next(tmp_path):
    sh = _unique_set(tmp_path, 40)
    inp = ShardInput(sh, _info(), 8, 6, mode="stream")
    inp.next(0)

    def boom(idx, out=None):
        raise OSError("shard went away")
    sh.gather = boom
    with pytest.raises(OSError, match="shard went away"):
        for s in range(1, 6):  # the ring holds at most three batches gathered before the failure
            inp.next(s)
    inp.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("kdl-")]


def test_eval_input_is_an_iterable_and_ranks_read_disjoint_images(tmp_path):
    sh = _unique_set(tmp_path, 45)
    seen = []
    for r in range(2):
        tr_in = ShardInput(sh, _info(r, 2), 4, 6, seed=1, mode="stream" if r else "resident")
        ids = set()
        for s in range(tr_in.steps_per_epoch):
            x, y = tr_in.next(s)
            v = x.float()[:, 0, 0, 0].long()  # mean 0, std 1: the value is the image's index
            assert torch.equal(v % 5, y)
            ids |= set(v.tolist())
        assert len(ids) == tr_in.steps_per_epoch * 4 and all(i % 2 == r for i in ids)
        seen.append(ids)
        tr_in.close()
    assert not (seen[0] & seen[1])
    ev = ShardInput(sh, _info(1, 2), 4, 6, train=False, max_batches=3)
    assert ev.steps_per_epoch == 5 and ev.dropped == 2 and len(ev) == 3
    got = [x.float()[:, 0, 0, 0].long().tolist() for x, _ in ev]
    assert got == [[1, 3, 5, 7], [9, 11, 13, 15], [17, 19, 21, 23]]
    assert len(list(ev)) == 3  # a second pass starts over


def test_trainer_checks_classes_and_geometry(tmp_path):
    from kubedl_amd.workers.resnet50 import ResNetTrainer
    sh = _unique_set(tmp_path, 16, 40, 40, classes=12)
    tr = ResNetTrainer(_info(), batch=4, image=32, tiny=True, num_classes=10, bn_backend="torch", engine="autograd")
    with pytest.raises(ValueError, match="12 classes"):
        tr.set_input(ShardInput(sh, _info(), 4, 32))
    with pytest.raises(ValueError, match="batch 2"):
        tr.set_input(ShardInput(sh, _info(), 2, 32))


# ================================================================ 5. the worker end to end
@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("sets")
    for name, n, seed in (("train", 64, 1), ("eval", 37, 2)):
        img, lab = synthetic_images(n, 4, 40, seed)
        write_shards(str(d / name), img, lab, 30, 4)
    return d


def _worker(args, env=None, check=True):
    e = dict(os.environ, OMP_NUM_THREADS="2", **(env or {}))
    for k in ("KDL_CKPT_DIR", "KDL_CKPT_EVERY", "KDL_FAULT", "RANK", "WORLD_SIZE", "MASTER_PORT"):
        if k not in (env or {}):
            e.pop(k, None)
    r = subprocess.run([PY, "-m", "kubedl_amd.workers.resnet50", "--tiny", "--cpu", "--batch", "8", "--image", "32",
                        "--warmup", "0"] + args, cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def _json(r):
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_worker_trains_two_epochs_and_evaluates(sets, tmp_path):
    steplog = tmp_path / "steps.jsonl"
    res = _json(_worker(["--data", str(sets / "train"), "--data-eval", str(sets / "eval"), "--epochs", "2"],
                        env={"KDL_STEP_LOG": str(steplog)}))
    assert res["data_mode"] == "resident" and res["steps_per_epoch"] == 8 and res["epochs_done"] == 2
    assert res["images_seen"] == 128 and res["data_wait_ms"] == 0.0 and res["steps"] == 16
    assert res["eval_dropped"] == 5 and res["eval_images"] == 32  # 0 --eval-batches with --data-eval: the whole set
    losses = [json.loads(ln)["loss"] for ln in steplog.read_text().splitlines()]
    assert len(losses) == 16 and all(math.isfinite(v) for v in losses)
    assert math.isfinite(res["loss"]) and res["loss"] < losses[0] and losses[-1] == pytest.approx(res["loss"])
    assert math.isfinite(res["eval_loss"])
    capped = _json(_worker(["--data", str(sets / "train"), "--data-eval", str(sets / "eval"), "--steps", "2",
                            "--eval-batches", "3", "--data-mode", "stream", "--data-workers", "2"]))
    assert capped["eval_images"] == 24 and capped["data_mode"] == "stream" and capped["data_wait_ms"] > 0


def test_worker_refuses_steps_with_epochs(sets):
    r = _worker(["--data", str(sets / "train"), "--epochs", "1", "--steps", "3"], check=False)
    assert r.returncode == 2 and "--epochs and --steps" in r.stderr
    r = _worker(["--epochs", "1"], check=False)
    assert r.returncode == 2 and "--epochs needs --data" in r.stderr


def test_worker_resume_is_bit_equal_and_eval_only_scores_the_set(sets, tmp_path):
    args = ["--data", str(sets / "train"), "--epochs", "2", "--data-seed", "4"]
    ck_a, ck_b = tmp_path / "a", tmp_path / "b"
    _worker(args, env={"KDL_CKPT_DIR": str(ck_a), "KDL_CKPT_EVERY": "1"})
    env_b = {"KDL_CKPT_DIR": str(ck_b), "KDL_CKPT_EVERY": "1"}
    r = _worker(args, env={**env_b, "KDL_FAULT": "0:9:137"}, check=False)  # dies inside the second epoch
    assert r.returncode == 137
    assert json.load(open(ck_b / "latest.json"))["step"] == 10
    res = _json(_worker(args, env=env_b))
    assert res["resumed_from_step"] == 10 and res["epochs_done"] == 2 and res["images_seen"] == 128
    a = torch.load(ck_a / "step-00000016.pt", weights_only=True)
    b = torch.load(ck_b / "step-00000016.pt", weights_only=True)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    ev = _json(_worker(["--data-eval", str(sets / "eval"), "--eval-only"], env={"KDL_CKPT_DIR": str(ck_a)}))
    assert ev["eval_images"] == 32 and ev["eval_dropped"] == 5 and ev["steps"] == 0 and ev["data_mode"] == "resident"


def test_worker_two_gloo_ranks(sets):
    from kubedl_amd.workers.common import free_port
    port = str(free_port())
    args = [PY, "-m", "kubedl_amd.workers.resnet50", "--tiny", "--cpu", "--batch", "8", "--image", "32", "--warmup",
            "0", "--data", str(sets / "train"), "--data-eval", str(sets / "eval"), "--epochs", "1"]
    procs = []
    for rank in range(2):
        env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="2",
                   RANK=str(rank), KDL_PG_TIMEOUT_S="120")
        procs.append(subprocess.Popen(args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs[0][1][-1500:] + outs[1][1][-1500:]
    res = json.loads([ln for ln in outs[0][0].splitlines() if ln.startswith("{")][-1])
    # 64 images over 2 ranks: 32 owned, 4 steps of 8; the eval set's 37: 19 / 18 owned, 2 batches each
    assert res["world_size"] == 2 and res["steps_per_epoch"] == 4 and res["images_seen"] == 64
    assert res["eval_images"] == 32 and math.isfinite(res["loss"])
