"""ResNet evaluation: the engine's inference forward, the evaluation head and the worker's ``--eval-*`` flags.

CPU: the TorchKernels backend (the HIP path's data flow and rounding points in torch ops) against the autograd
module in ``eval()``; the rank / top-k tie rule; evaluation leaves every piece of training state bit-equal; the
worker end to end (schedule, unchanged default output, ``--eval-only``, two gloo ranks); the example specs;
the new kernels' descriptors.  GPU: the HipKernels backend on real networks against the fp32 ``eval()`` truth.

The running statistics are never the 0 / 1 defaults here (a wrong coefficient table would hide behind them):
one training-mode forward of the fp32 copy at BN momentum 1.0 populates them, and every model under test gets
a copy.
"""
import copy
import json
import os
import re
import shutil
import socket
import subprocess
from pathlib import Path

import pytest
import torch

import kubedl_amd.models.resnet_engine as RE
from kubedl_amd.models.resnet import BNAct, ResNet
from kubedl_amd.models.resnet_engine import ResNetEngine, label_rank, torch_head_eval

gpu = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------- models with populated statistics
def _models(layers, width, dev, image, batch, classes=10, seed=0):
    """(fp32 truth in eval(), bf16 model for the engine, bf16 autograd reference in eval(), x bf16, y)."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    truth = ResNet(layers, num_classes=classes, width=width)
    with torch.no_grad():
        for m in truth.modules():
            if isinstance(m, BNAct):
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.uniform_(-0.2, 0.2, generator=g)
    truth.set_bn_backend("torch")
    x = torch.randn(batch, 3, image, image, generator=g).to(torch.bfloat16)
    x2 = torch.randn(batch, 3, image, image, generator=g).to(torch.bfloat16)
    y = torch.randint(0, classes, (batch,), generator=g)
    # the statistics of a second batch become the running statistics (momentum 1.0)
    bns = [m for m in truth.modules() if isinstance(m, BNAct)]
    for m in bns:
        m.momentum = 1.0
    truth.train()
    with torch.no_grad():
        truth(x2.float())
    for m in bns:
        m.momentum = 0.1
    truth.eval()
    truth = truth.to(dev)
    model = copy.deepcopy(truth)
    if dev == "cuda":
        model = model.to(memory_format=torch.channels_last)
    for p in model.parameters():
        p.data = p.data.to(torch.bfloat16)
    ref = copy.deepcopy(model)
    model.train()  # the engine does not look at the flag: evaluation must not depend on it
    x = x.to(dev).contiguous(memory_format=torch.channels_last)
    return truth, model, ref, x, y.to(dev)


def _rel(a, t):
    return ((a.float() - t.float()).norm() / (t.float().norm() + 1e-12)).item()


def _engine_logits(eng, x, y, classes):
    totals = torch.zeros(4, dtype=torch.float64, device=x.device)
    logits = torch.full((x.shape[0], classes), float("nan"), device=x.device)
    loss_row, rank_row = eng.evaluate(x, y, totals, logits)
    return logits, loss_row, rank_row, totals


def _check_totals(logits, y, loss_row, rank_row, totals, calls=1):
    rank = label_rank(logits, y)
    assert torch.equal(rank_row.cpu(), rank.cpu())
    t = totals.cpu()
    assert t[1].item() == calls * int((rank < 1).sum()) and t[2].item() == calls * int((rank < 5).sum())
    assert t[3].item() == calls * logits.shape[0]
    ls = calls * loss_row.double().sum().item()
    assert abs(t[0].item() - ls) <= 1e-12 * abs(ls)


# ================================================================ 1. torch backend vs the autograd module
@pytest.mark.parametrize("layers,width", [((2, 1, 1, 2), 8), ((1, 1, 1, 1), 64)])
def test_infer_torch_backend_fp32_matches_eval_module(layers, width, monkeypatch):
    """fp32 storage (no rounding points): the folded scale | shift data flow is exactly eval()."""
    monkeypatch.setattr(RE, "_bfr", lambda t: t.float())
    truth, _, _, x, y = _models(layers, width, "cpu", 64, 4)
    model = copy.deepcopy(truth)
    with torch.no_grad():
        want = truth(x.float())
    logits, loss_row, rank_row, totals = _engine_logits(ResNetEngine(model, backend="torch"), x.float(), y, 10)
    torch.testing.assert_close(logits, want, atol=1e-5, rtol=1e-5)
    _check_totals(logits, y, loss_row, rank_row, totals)
    torch.testing.assert_close(loss_row, torch.nn.functional.cross_entropy(want, y, reduction="none"), atol=1e-5,
                               rtol=1e-5)


@pytest.mark.parametrize("layers,width", [((2, 1, 1, 2), 8), ((1, 1, 1, 1), 64)])
def test_infer_torch_backend_bf16_close_to_fp32_truth(layers, width):
    """bf16 storage: the engine's error against the fp32 truth is within the project's slack
    (1.5 x + 0.01, tests/test_resnet_engine.py _vs_truth_strict) of the bf16 eval() module's own."""
    truth, model, ref, x, y = _models(layers, width, "cpu", 64, 4)
    with torch.no_grad():
        want = truth(x.float())
        got_ref = ref(x).float()
    logits, *_ = _engine_logits(ResNetEngine(model, backend="torch"), x, y, 10)
    ee, er = _rel(logits, want), _rel(got_ref, want)
    print(f"rel-L2 engine {ee:.5f} autograd bf16 {er:.5f}")
    assert ee <= 1.5 * er + 0.01


# ================================================================ 2. the rank / top-k rule
def test_rank_rule_on_hand_made_logits_and_totals_over_two_calls():
    z = torch.tensor([[3., 1., 3., 0., 3., -1.],    # label 2: ties before (0) and after (4) -> rank 1
                      [3., 1., 3., 0., 3., -1.],    # label 0: first of the tied maxima -> rank 0
                      [3., 1., 3., 0., 3., -1.],    # label 4: last of them -> rank 2
                      [0., 0., 0., 0., 0., 0.],     # all tied, label L - 1 -> rank 5: not in the top 5
                      [0., 0., 0., 0., 0., 0.],     # all tied, label 0 -> rank 0
                      [5., 4., 3., 2., 1., 0.],     # label 5 at L - 1, strictly last -> rank 5
                      [1., 2., 3., 4., 5., 6.],     # out-of-range label -> rank L, loss NaN
                      [1., 2., 3., 4., 5., 6.]])    # negative label likewise
    y = torch.tensor([2, 0, 4, 5, 0, 5, 6, -100])
    assert label_rank(z, y).tolist() == [1, 0, 2, 5, 0, 5, 6, 6]
    # through the head: identity fc, one pixel -> the logits are z
    fmap = z.view(8, 6, 1, 1)
    totals = torch.zeros(4, dtype=torch.float64)
    out = torch.empty(8, 6)
    loss_row, rank_row = torch_head_eval(fmap[:6], torch.eye(6), None, y[:6], totals, out[:6])
    assert torch.equal(out[:6], z[:6]) and rank_row.tolist() == [1, 0, 2, 5, 0, 5]
    first = totals.clone()
    assert first.tolist()[1:] == [2.0, 4.0, 6.0]
    assert abs(first[0].item() - loss_row.double().sum().item()) < 1e-12
    loss2, rank2 = torch_head_eval(fmap[:3], torch.eye(6), None, y[:3], totals)
    assert totals.tolist()[1:] == [3.0, 7.0, 9.0]
    assert abs(totals[0].item() - (first[0].item() + loss2.double().sum().item())) < 1e-12
    # an out-of-range label: NaN loss, never in a top k, counted as an image
    t3 = torch.zeros(4, dtype=torch.float64)
    loss3, rank3 = torch_head_eval(fmap[6:], torch.eye(6), None, y[6:], t3)
    assert loss3.isnan().all() and rank3.tolist() == [6, 6] and t3[0].isnan() and t3.tolist()[1:] == [0.0, 0.0, 2.0]


# ================================================================ 3. evaluation leaves training state alone
def _trainer(dev="cpu", **kw):
    from kubedl_amd.parallel.dist import DistInfo
    from kubedl_amd.workers.resnet50 import ResNetTrainer
    info = DistInfo(0, 1, 0, torch.device(dev), "gloo" if dev == "cpu" else "nccl")
    args = dict(batch=4, image=32, num_classes=10, tiny=True, engine="fused", seed=3)
    args.update(kw)
    return ResNetTrainer(info, **args)


def _state(tr):
    """Every tensor of the training state, cloned: parameters, master weights, momentum, gradient buffer,
    buffers, every BNState tensor (workspace, saved statistics, torch-backend sums and coefficients)."""
    st = {"param": tr.space.param, "master": tr.space.master, "mom": tr.opt.mom, "grad": tr.space.grad}
    for n, b in tr.model.named_buffers():
        st["buf." + n] = b
    for i, bs in enumerate(tr.engine.bn.values()):
        for k in ("save_mean", "save_invstd", "ws", "xam"):
            if torch.is_tensor(getattr(bs, k)):
                st[f"bn{i}.{k}"] = getattr(bs, k)
        for k in ("fsum", "fcoef", "bsum", "bcoef"):
            for j, t in enumerate(getattr(bs, k) or ()):
                st[f"bn{i}.{k}{j}"] = t
        st[f"bn{i}.flags"] = torch.tensor([bs.fin_done, bs.bfin_done])
    for i, t in enumerate(tr.engine._wt_buf.values()):
        st[f"wt{i}"] = t
    return {k: v.detach().clone() for k, v in st.items()}


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8) if t.dtype != torch.bool else t.contiguous().view(-1)


def _assert_state_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(_bytes(a[k]), _bytes(b[k])), f"{k} changed"


def test_evaluation_leaves_training_state_bit_equal_and_the_next_step_unchanged():
    tr = _trainer()
    tr.step()
    before = _state(tr)
    saved_id = id(tr.engine._saved)
    ev = tr.evaluate(tr.eval_batches(2))
    assert ev["eval_images"] == 8 and ev["eval_loss"] == ev["eval_loss"]
    _assert_state_equal(before, _state(tr))
    assert id(tr.engine._saved) == saved_id and tr.model.training
    loss2 = tr.step().clone()
    other = _trainer()
    other.step()
    want2 = other.step()
    assert torch.equal(loss2, want2)
    _assert_state_equal(_state(tr), _state(other))


def test_autograd_trainer_evaluates_in_eval_mode_and_restores_training_mode():
    tr = _trainer(engine="autograd", bn_backend="torch")
    tr.step()
    bufs = {n: b.clone() for n, b in tr.model.named_buffers()}
    ev = tr.evaluate(tr.eval_batches(3))
    assert ev["eval_images"] == 12 and 0 <= ev["eval_top1"] <= ev["eval_top5"] <= 1
    assert tr.model.training
    for n, b in tr.model.named_buffers():
        assert torch.equal(b, bufs[n]), n
    # the same totals as the engine path's torch composition on the same weights
    x, y = tr.eval_batches(1)[0]
    tr.model.eval()
    with torch.no_grad():
        z = tr.model(x).float()
    tr.model.train()
    one = tr.evaluate([(x, y)])
    assert one["eval_top1"] == float((label_rank(z, y) < 1).sum()) / 4


# ================================================================ 4. the worker
# the parent commit's output keys: the default run (--eval-batches 0) must print exactly these
PARENT_KEYS = {"rank", "world_size", "steps", "seconds", "ms_per_step", "steps_per_sec", "images_per_sec", "loss",
               "startup_s", "resumed_from_step", "total_steps"}
TINY = ["--cpu", "--tiny", "--steps", "4", "--warmup", "1", "--batch", "4", "--image", "32"]


def _worker(argv, capsys, monkeypatch, rc=0):
    from kubedl_amd.workers.resnet50 import main
    monkeypatch.delenv("MASTER_PORT", raising=False)
    capsys.readouterr()
    assert main(argv) == rc
    cap = capsys.readouterr()
    lines = [l for l in cap.out.splitlines() if l.startswith("{")]
    return (json.loads(lines[-1]) if lines else None), cap.err


def test_worker_evaluates_on_schedule_and_default_output_is_unchanged(capsys, monkeypatch):
    monkeypatch.delenv("KDL_CKPT_DIR", raising=False)
    off, _ = _worker(TINY + ["--eval-batches", "0"], capsys, monkeypatch)
    assert set(off) == PARENT_KEYS
    on, _ = _worker(TINY + ["--eval-batches", "2", "--eval-every", "2"], capsys, monkeypatch)
    assert set(on) == PARENT_KEYS | {"eval_loss", "eval_top1", "eval_top5", "eval_images", "eval_images_per_sec",
                                     "eval_history"}
    assert on["eval_images"] == 2 * 4
    assert [h["step"] for h in on["eval_history"]] == [2, 4] and len(on["eval_history"]) == 2
    assert on["eval_loss"] == on["eval_loss"] and abs(on["eval_loss"]) != float("inf")
    assert 0 <= on["eval_top1"] <= on["eval_top5"] <= 1
    assert on["loss"] == off["loss"]  # the training random stream is the same with and without evaluation
    once, _ = _worker(TINY + ["--eval-batches", "2"], capsys, monkeypatch)
    assert "eval_history" not in once and once["eval_loss"] == on["eval_loss"]


def test_worker_eval_only_needs_a_checkpoint_and_reproduces_the_final_evaluation(capsys, monkeypatch, tmp_path):
    monkeypatch.setenv("KDL_CKPT_DIR", str(tmp_path))
    monkeypatch.delenv("KDL_CKPT_EVERY", raising=False)
    res, err = _worker(["--cpu", "--tiny", "--batch", "4", "--image", "32", "--eval-only"], capsys, monkeypatch, rc=2)
    assert res is None and "no checkpoint" in err
    assert not list(tmp_path.iterdir())  # it never trains, so it never saves
    monkeypatch.setenv("KDL_CKPT_EVERY", "5")
    trained, _ = _worker(TINY + ["--eval-batches", "2"], capsys, monkeypatch)
    monkeypatch.delenv("KDL_CKPT_EVERY")
    ev, _ = _worker(["--cpu", "--tiny", "--batch", "4", "--image", "32", "--eval-only", "--eval-batches", "2"], capsys,
                    monkeypatch)
    assert ev["steps"] == 0 and ev["resumed_from_step"] == 5 and "loss" not in ev
    for k in ("eval_loss", "eval_top1", "eval_top5", "eval_images"):
        assert ev[k] == trained[k], k


def _rank_main(rank, world, port, out, argv):
    import contextlib
    import io
    from kubedl_amd.workers.resnet50 import ResNetTrainer
    import torch.distributed as dist
    from kubedl_amd.parallel.dist import DistInfo
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    info = DistInfo(rank, world, rank, torch.device("cpu"), "gloo")
    tr = ResNetTrainer(info, batch=2, image=32, num_classes=10, tiny=True, engine="fused", bucket_cap_mb=0.05, seed=0)
    tr.step()
    out[f"ev{rank}"] = tr.evaluate(tr.eval_batches(3))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_merge_their_totals():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out, None)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    assert out["ev0"]["eval_images"] == 2 * 3 * 2
    assert out["ev0"] == out["ev1"]


# ================================================================ 5. the example specs
@pytest.mark.parametrize("name,flags", [("resnet50_train_eval.yaml", {"eval_batches": 4, "eval_every": 50}),
                                        ("resnet50_eval.yaml", {"eval_batches": 4, "eval_only": True})])
def test_example_specs_load_and_their_flags_parse(name, flags):
    from kubedl_amd.api import codec
    from kubedl_amd.runtime import images
    from kubedl_amd.workers.resnet50 import build_parser
    (obj,) = codec.load_file(str(ROOT / "examples" / "pytorch" / name))
    assert obj["kind"] == "PyTorchJob"
    (ct,) = obj["spec"]["pytorchReplicaSpecs"]["Master"]["template"]["spec"]["containers"]
    assert ct["image"] == "kubedl-amd/resnet50" and "kubedl-amd/resnet50" in open(images.__file__).read()
    args = build_parser().parse_args(ct["args"])
    for k, v in flags.items():
        assert getattr(args, k) == v
    assert any(a.startswith("--eval-") for a in ct["args"])
    env = {e["name"]: e["value"] for e in ct["env"]}
    assert env["KDL_CKPT_DIR"] == "/tmp/kdl-ckpt/resnet50"  # the pair shares one checkpoint directory


# ================================================================ 6. kernel descriptors
def _descriptors(src, tmp_path):
    out = tmp_path / (src.stem + ".s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-S",
                        f"-I{ROOT / 'csrc'}", str(src), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        sz = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        meta[m.group(1)] = int(sz.group(1)) if sz else 0
    return meta


@pytest.mark.skipif(not Path(HIPCC).exists() or shutil.which("python3") is None, reason="no hipcc")
def test_inference_epilogue_kernels_exist_and_use_no_scratch(tmp_path):
    """igemm_kernel<BM, BN, WM, WN, GATHER, EPI, MINB, STAGES> / gemm1x1_kernel<BM, BN, MINB, PRO, GATHER, EPI,
    KBK>, looked up by their mangled template arguments: G_DENSE (0) with EPI 7, 8, 9; G_STRIDED (1) with 7, 8;
    G_CONV3 (2) with 8 -- on the four two-stage LDS-DMA tiles and the two 128-row register-staged tiles."""
    import concurrent.futures as cf
    want = [(0, 7), (0, 8), (0, 9), (1, 7), (1, 8), (2, 8)]
    with cf.ThreadPoolExecutor(2) as ex:  # the two compiles side by side
        both = [ex.submit(_descriptors, ROOT / "csrc" / f, tmp_path) for f in ("igemm.hip", "conv1x1.hip")]
        meta, meta1 = (f.result() for f in both)
    for tile in ("Li256ELi256ELi2ELi4E", "Li256ELi128ELi4ELi2E", "Li128ELi128ELi2ELi2E", "Li256ELi64ELi4ELi1E"):
        for gather, epi in want:
            frag = f"igemm_kernelI{tile}Li{gather}ELi{epi}ELi"
            hits = {k: v for k, v in meta.items() if frag in k and k.split(frag)[1].split("E")[1] == "Li2"}
            assert len(hits) == 1, f"{frag}: {list(hits)}"
            for k, v in hits.items():
                assert v == 0, f"{k}: {v} B of scratch"
    new = {k: v for k, v in meta.items() if re.search(r"igemm_kernelI(Li\d+E){5}Li[789]E", k)}
    assert len(new) == 24 and not any(new.values())
    meta = meta1
    for tile in ("Li128ELi128ELi2E", "Li128ELi64ELi2E"):
        for gather, epi in want:
            frag = f"gemm1x1_kernelI{tile}Li0ELi{gather}ELi{epi}ELi64E"
            hits = [k for k in meta if frag in k]
            assert len(hits) == 1, f"{frag}: {hits}"
            assert meta[hits[0]] == 0, f"{hits[0]}: {meta[hits[0]]} B of scratch"


# ================================================================ GPU: the HIP backend (issue items 12, 13)
def _snapshot(eng):
    st = {}
    for n, p in eng.model.named_parameters():
        st["p." + n] = p
    for n, b in eng.model.named_buffers():
        st["b." + n] = b
    for i, bs in enumerate(eng.bn.values()):
        st[f"bn{i}.ws"], st[f"bn{i}.save_mean"], st[f"bn{i}.save_invstd"] = bs.ws, bs.save_mean, bs.save_invstd
    return {k: v.detach().clone() for k, v in st.items()}


@gpu
@pytest.mark.parametrize("layers,image,batch,classes", [((1, 1, 1, 1), 64, 8, 10), ((2, 2, 2, 2), 96, 4, 10),
                                                        ((3, 4, 6, 3), 224, 8, 1000)])
def test_engine_hip_evaluate_matches_fp32_eval_truth(layers, image, batch, classes):
    from test_resnet_engine import _ref_step, _truth_of, _vs_truth
    truth, model, ref, x, y = _models(layers, 64, "cuda", image, batch, classes=classes)
    with torch.no_grad():
        want = truth(x.float())
        got_ref = ref(x).float()
    eng = ResNetEngine(model, backend="hip")
    before = _snapshot(eng)
    logits, loss_row, rank_row, totals = _engine_logits(eng, x, y, classes)
    torch.cuda.synchronize()
    ee, er = _rel(logits, want), _rel(got_ref, want)
    print(f"rel-L2 engine {ee:.5f} autograd bf16 {er:.5f}")
    assert not logits.isnan().any()
    assert ee <= 1.5 * er + 0.01
    _check_totals(logits, y, loss_row, rank_row, totals)
    after = _snapshot(eng)
    _assert_state_equal(before, after)
    assert not hasattr(eng, "_saved") and not eng._wt_buf
    # a following training step is still right: no arming or workspace leak
    ref.train()
    model.train()
    tt, tloss = _truth_of(ref, x, y)
    loss = eng.forward_backward(x, y)
    _ref_step(ref, x, y)
    torch.cuda.synchronize()
    torch.testing.assert_close(loss, tloss, atol=2e-2, rtol=2e-2)
    _vs_truth(model, ref, tt)


@gpu
def test_engine_hip_evaluate_batch_1_and_3_row_tails():
    """Any batch size: image 0 of a batch of 1 and of 3 gives, bit for bit, the logits it gives inside a batch
    of 8 (the row tiles' tails, the head without the training head's Nb % 8 rule)."""
    truth, model, ref, x, y = _models((1, 1, 1, 1), 64, "cuda", 224, 8)
    eng = ResNetEngine(model, backend="hip")
    full, *_ = _engine_logits(eng, x, y, 10)
    for nb in (1, 3):
        part, loss_row, rank_row, totals = _engine_logits(eng, x[:nb].contiguous(memory_format=torch.channels_last),
                                                          y[:nb].contiguous(), 10)
        torch.cuda.synchronize()
        assert not part.isnan().any()
        assert torch.equal(part.view(torch.int32), full[:nb].view(torch.int32)), f"batch {nb}"
        _check_totals(part, y[:nb], loss_row, rank_row, totals)
