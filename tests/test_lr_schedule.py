"""The learning-rate schedule (kubedl_amd/ops/lr_schedule.py), the trainer that follows it across a checkpoint resume,
and the worker's large-batch recipe flags (LARS + warm-up + poly decay + label smoothing) on the tiny CPU model."""
import json
import math

import pytest
import torch

from kubedl_amd.ops.lr_schedule import lr_at

PEAK, END, WARM, TOTAL = 0.8, 0.05, 4, 20   # 16 decay steps: step 4 (f = 0) .. step 19 (f = 15/16)
DECAY = {"constant": lambda f: PEAK,
         "poly": lambda f: END + (PEAK - END) * (1 - f) ** 2,
         "cosine": lambda f: END + (PEAK - END) * (1 + math.cos(math.pi * f)) / 2}


@pytest.mark.parametrize("kind", ["constant", "poly", "cosine"])
def test_lr_at_warmup_and_decay_ends(kind):
    kw = dict(peak=PEAK, kind=kind, warmup_steps=WARM, total_steps=TOTAL, end_lr=END)
    assert lr_at(0, **kw) == pytest.approx(PEAK / WARM, rel=1e-15)
    assert lr_at(WARM - 1, **kw) == PEAK                                   # the last warm-up step
    assert lr_at(WARM, **kw) == pytest.approx(PEAK, rel=1e-15)             # the first decay step: f = 0
    assert lr_at(TOTAL - 1, **kw) == pytest.approx(DECAY[kind](15 / 16), rel=1e-12)
    assert lr_at(TOTAL, **kw) == lr_at(TOTAL + 7, **kw) == pytest.approx(DECAY[kind](1.0), rel=1e-15)  # clamped
    assert all(lr_at(s, peak=PEAK, kind="constant") == PEAK for s in (0, 1, 1000))
    with pytest.raises(ValueError):
        lr_at(0, peak=PEAK, kind="step")


def _trainer(**kw):
    from kubedl_amd.parallel.dist import DistInfo
    from kubedl_amd.workers.resnet50 import ResNetTrainer
    info = DistInfo(0, 1, 0, torch.device("cpu"), "gloo")
    return ResNetTrainer(info, batch=2, image=32, tiny=True, num_classes=10, bn_backend="torch", engine="autograd", **kw)


def test_trainer_follows_the_schedule_across_a_resume(tmp_path):
    from kubedl_amd.utils.checkpoint import Checkpointer
    kw = dict(lr=0.5, optimizer="lars", label_smoothing=0.1, lr_schedule="poly", lr_warmup_steps=2, lr_total_steps=6,
              lr_end=0.01)
    want = [lr_at(s, peak=0.5, kind="poly", warmup_steps=2, total_steps=6, end_lr=0.01) for s in range(5)]
    ref, a, b = _trainer(**kw), _trainer(**kw), _trainer(**kw)
    for s in range(5):
        ref.step()
        assert ref.steps_done == s + 1 and ref.opt.lr == want[s]
    for _ in range(3):
        a.step()
    Checkpointer(str(tmp_path), every=1).save(3, a.state_dict())
    b.steps_done, st = Checkpointer(str(tmp_path)).load_latest()
    b.load_state_dict(st)
    for s in (3, 4):
        b.step()
        assert b.opt.lr == want[s]
    assert torch.equal(b.space.master, ref.space.master) and torch.equal(b.opt.mom, ref.opt.mom)
    plain = _trainer(lr=0.25)  # constant, no warm-up: the optimizer's rate is left alone
    plain.opt.lr = 0.125
    plain.step()
    assert plain.opt.lr == 0.125 and type(plain.opt).__name__ == "FusedSGD"


def test_worker_large_batch_recipe_on_cpu(capsys, monkeypatch, tmp_path):
    from kubedl_amd.workers.resnet50 import main
    monkeypatch.delenv("MASTER_PORT", raising=False)
    monkeypatch.delenv("KDL_CKPT_DIR", raising=False)
    monkeypatch.setenv("KDL_STEP_LOG", str(tmp_path / "steps.jsonl"))
    assert main(["--tiny", "--cpu", "--steps", "7", "--warmup", "1", "--batch", "4", "--image", "32", "--optimizer", "lars",
                 "--lr-schedule", "poly", "--lr-warmup-steps", "2", "--label-smoothing", "0.1"]) == 0
    res = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    loss = [json.loads(l)["loss"] for l in (tmp_path / "steps.jsonl").read_text().splitlines()]
    assert len(loss) == 8 and res["total_steps"] == 8 and all(math.isfinite(x) for x in loss)
    assert loss[-1] < loss[0] and res["loss"] == loss[-1]  # the one synthetic batch is being fitted
