"""Mixup / CutMix on the CPU: the plan's per-step draws, the reference rule of data/augment.py against
independent evaluations, the worker end to end (tests/test_mix_gpu.py holds the kernels to this reference)."""
import json
import math

import numpy as np
import pytest
import torch

from kubedl_amd.data import plan as P
from kubedl_amd.data.augment import augment_mix_reference, augment_reference, norm_coeffs, resample_q
from kubedl_amd.data.shards import IMAGENET_MEAN as MEAN, IMAGENET_STD as STD, synthetic_images, write_shards
from test_image_shards import _json, _worker  # the tiny CPU worker (batch 8, 32 px, no timing warm-up) in a subprocess

CFG = P.MixConfig(mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.8, switch_prob=0.3)
MIX = ["--mixup-alpha", "0.2", "--cutmix-alpha", "1.0"]  # the worker's flags


def _draws(n, rank=0, seed=5, first=0, mix=CFG):
    pl = P.InputPlan(400, 40, 40, 2, rank, 8, seed=seed, mix=mix)
    return [pl.mix_draw(s, 32, 24) for s in range(first, n)]


def test_draws_are_a_pure_function_of_seed_step_rank():
    a = _draws(40)
    assert _draws(40, first=25) == a[25:]  # a plan re-created at step 25, as on resume
    assert _draws(40, rank=1) != a and _draws(40, seed=6) != a and {d.kind for d in a} == {0, 1, 2}
    for d in a:
        cy0, cx0, ch, cw = d.box
        assert 0 <= cy0 and 0 <= cx0 and cy0 + ch <= 32 and cx0 + cw <= 24 and 0 <= d.lam16 <= 65536
        assert d.kind == P.MIX_CUTMIX or (ch, cw) == (0, 0)
    assert _draws(4, mix=None) == [P.MixDraw()] * 4
    assert P.InputPlan(400, 40, 40, 1, 0, 8, train=False, mix=CFG).mix is None  # evaluation is never mixed


def test_kind_frequencies_and_mean_lam(n=4000):
    """Seed 5: each kind's count within 4 binomial standard deviations of n p, each kind's mean lam within
    4 standard errors of 1/2 (Beta(a, a): variance 1 / (4 (2 a + 1)))."""
    d = _draws(n)
    for kind, p in ((P.MIX_NONE, 0.2), (P.MIX_CUTMIX, 0.8 * 0.3), (P.MIX_MIXUP, 0.8 * 0.7)):
        got = sum(x.kind == kind for x in d)
        assert abs(got - n * p) <= 4 * math.sqrt(n * p * (1 - p)), (kind, got, n * p)
    for kind, alpha in ((P.MIX_MIXUP, 0.2), (P.MIX_CUTMIX, 1.0)):
        lam = np.array([x.lam for x in d if x.kind == kind])
        assert abs(lam.mean() - 0.5) <= 4 * math.sqrt(1 / (4 * (2 * alpha + 1)) / len(lam)), (kind, lam.mean())


G = np.random.default_rng(1)
IMG = torch.from_numpy(G.integers(0, 256, (5, 20, 22, 3), dtype=np.uint8))
LAB = torch.from_numpy(G.integers(0, 10, 5, dtype=np.int64))
ROWS = torch.tensor([[2, 0, 0, 20, 22, 0, 0, 0], [0, 3, 1, 9, 17, 1, 0, 0], [4, 5, 5, 15, 6, 1, 0, 0],
                     [1, 19, 0, 1, 22, 0, 0, 0], [3, 0, 2, 20, 20, 0, 0, 0]], dtype=torch.int32)


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.61803, 1.0])
def test_mixup_reference_against_a_float_evaluation(lam):
    """x is lam * x_i + (1 - lam) * x_j of the unrounded normalised images to one bf16 ulp (the output's
    rounding) plus 2^-17 |x_i - x_j| (lam's 16-bit quantisation)."""
    x, ya, yb, ll = augment_mix_reference(IMG, LAB, ROWS, 12, 13, MEAN, STD, 1, P.lam_to_16(lam))
    A, B = norm_coeffs(MEAN, STD)
    xf = resample_q(IMG, ROWS, 12, 13).double() * torch.from_numpy(A).double() + torch.from_numpy(B).double()
    want = lam * xf + (1 - lam) * xf.flip(0)
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -100))) - 7)
    err = (x.permute(0, 2, 3, 1).double() - want).abs()
    assert (err <= ulp + 2.0 ** -17 * (xf - xf.flip(0)).abs()).all(), float((err / ulp).max())
    assert torch.equal(ya, LAB[ROWS[:, 0].long()]) and torch.equal(yb, ya.flip(0))
    assert ll == P.lam_to_16(lam) / 65536 and abs(ll - lam) <= 2.0 ** -17


@pytest.mark.parametrize("box", [(0, 0, 0, 0), (0, 0, 12, 13), (3, 4, 1, 1), (0, 5, 7, 8), (6, 0, 6, 2)])
def test_cutmix_reference_selects_pixels_of_the_unmixed_images(box):
    x, ya, yb, ll = augment_mix_reference(IMG, LAB, ROWS, 12, 13, MEAN, STD, 2, 65536, box)
    xr, yr = augment_reference(IMG, LAB, ROWS, 12, 13, MEAN, STD)
    inside = torch.zeros(12, 13, dtype=torch.bool)
    inside[box[0]:box[0] + box[2], box[1]:box[1] + box[3]] = True
    assert torch.equal(x.view(torch.int16), torch.where(inside, xr.flip(0), xr).view(torch.int16))
    assert torch.equal(ya, yr) and torch.equal(yb, yr.flip(0))
    assert ll == float(np.float32(1 - box[2] * box[3] / (12 * 13)))
    none = augment_mix_reference(IMG, LAB, ROWS, 12, 13, MEAN, STD, 0)
    assert torch.equal(none[0].view(torch.int16), xr.view(torch.int16)) and none[3] == 1.0
    with pytest.raises(ValueError, match="box"):
        augment_mix_reference(IMG, LAB, ROWS, 12, 13, MEAN, STD, 2, 65536, (6, 0, 7, 2))


def test_worker_trains_mixed_and_resumes_bit_equal(tmp_path):
    """A mixed step's loss has a floor that moves with its lam, so besides tests/test_image_shards.py's "the last
    step's loss is below the first's" the unmixed loss over the training images must end below chance level, ln 4."""
    img, lab = synthetic_images(64, 4, 40, 1)
    write_shards(str(tmp_path / "set"), img, lab, 30, 4)
    args = ["--data", str(tmp_path / "set"), "--data-eval", str(tmp_path / "set"), "--epochs", "2", "--data-seed", "4",
            "--lr", "0.02"] + MIX
    ck_a, ck_b, steplog = tmp_path / "a", tmp_path / "b", tmp_path / "steps.jsonl"
    res = _json(_worker(args, env={"KDL_CKPT_DIR": str(ck_a), "KDL_CKPT_EVERY": "1", "KDL_STEP_LOG": str(steplog)}))
    losses = [json.loads(ln)["loss"] for ln in steplog.read_text().splitlines()]
    assert res["steps"] == 16 and len(losses) == 16 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0] and res["eval_loss"] < math.log(4)
    env_b = {"KDL_CKPT_DIR": str(ck_b), "KDL_CKPT_EVERY": "1"}
    assert _worker(args, env={**env_b, "KDL_FAULT": "0:9:137"}, check=False).returncode == 137  # killed in epoch 2
    _worker(args, env=env_b)
    a = torch.load(ck_a / "step-00000016.pt", weights_only=True)
    b = torch.load(ck_b / "step-00000016.pt", weights_only=True)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


@pytest.mark.parametrize("flags,msg", [(MIX, "need --data"), (["--cutmix-alpha", "1"], "need --data"),
                                       (["--mixup-alpha", "-1"], "--mixup-alpha")])
def test_worker_refuses_bad_mix_flags(flags, msg):
    r = _worker(flags, check=False)
    assert r.returncode == 2 and msg in r.stderr
