"""XDLJob evaluation: the streaming AUC (kubedl_amd/ops/auc.py, csrc/ctr_eval.hip),
the forward-only tower, pull-only exchange rounds and the worker's --eval-* flags.
Every AUC comparison is between integers."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from kubedl_amd.models.ctr import CTRModel, DenseTower, ShardedEmbedding
from kubedl_amd.ops.auc import BUCKETS, StreamingAUC, bucket_keys

SPECIAL = [0.0, -0.0, float("inf"), float("-inf"), 1e-45, -1e-45, 3e38, -3e38, float("nan"), 1.0, 1.0, 1.00390625,
           65.0, -65.0, 2.0 ** -20]
# 0 / -0 and the two 1.0 carry opposite labels: ties across the classes
SPECIAL_Y = [1, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1]


def _special():
    return torch.tensor(SPECIAL, dtype=torch.float32), torch.tensor(SPECIAL_Y, dtype=torch.float32)


def _random(n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale, (torch.rand(n, generator=g) < 0.4).float()


def _np_keys(logit):
    """The issue's key definition on numpy uint32 words (independent of ops/auc.py)."""
    x = logit.numpy().astype(np.float32).copy()
    x[x == 0] = 0.0  # -0 -> +0
    b = x.view(np.uint32)
    m = np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000))
    return (m >> 16).astype(np.int64)


def _brute_u2(sp, sn):
    """2 * #(pos > neg) + #(pos == neg) over all P x N pairs."""
    sp, sn = sp[:, None], sn[None, :]
    return 2 * int((sp > sn).sum()) + int((sp == sn).sum())


def _ref_state(logit, y):
    """(hist [2, 65536] numpy int64, invalid, U2, P, N) by brute force on bucketed keys."""
    ok = ~np.isnan(logit.numpy())
    keys, pos = _np_keys(logit)[ok], (y.numpy() > 0.5)[ok]
    hist = np.zeros((2, BUCKETS), dtype=np.int64)
    np.add.at(hist, (pos.astype(np.int64), keys), 1)
    kp, kn = keys[pos], keys[~pos]
    return hist, int((~ok).sum()), _brute_u2(kp, kn), int(kp.size), int(kn.size)


def _cpu_auc(logit, y):
    a = StreamingAUC("cpu")
    a.update(logit, y)
    return a


def _py_u2(hist):
    """(U2, P, N) in Python integers."""
    neg, pos = hist[0].tolist(), hist[1].tolist()
    above = u2 = 0
    for b in range(BUCKETS - 1, -1, -1):
        u2 += neg[b] * (2 * above + pos[b])
        above += pos[b]
    return u2, sum(pos), sum(neg)


# ------------------------------------------------------------------ CPU
def test_bucket_key_definition():
    assert int(bucket_keys(torch.tensor([1.0]))) == 49024
    x, _ = _special()
    k = bucket_keys(x)
    assert int(k[0]) == int(k[1]) == 0x8000  # 0 and -0 tie
    fin = x[~torch.isnan(x)]
    order = torch.argsort(fin)
    ks = bucket_keys(fin)[order]
    assert bool((ks[1:] >= ks[:-1]).all())  # non-decreasing in the logit
    assert np.array_equal(_np_keys(fin), bucket_keys(fin).numpy())


@pytest.mark.parametrize("case", [1, 2, 65, 4099, "special"])
def test_fallback_matches_brute_force(case):
    """The torch composition's (hist, invalid, U2, P, N) equal a brute-force pair
    count over the bucketed keys."""
    if case == "special":
        logit, y = _special()
    else:
        logit, y = _random(case, 3.0, case)
        if case == 2:
            y = torch.tensor([1.0, 0.0])
    hist, invalid, u2, p, n = _ref_state(logit, y)
    a = _cpu_auc(logit, y)
    assert np.array_equal(a.hist.numpy(), hist)
    assert int(a.invalid) == invalid
    assert a.counts() == (u2, p, n)
    assert a.counts() == _py_u2(a.hist)
    res = a.compute()
    assert (res["pos"], res["neg"], res["invalid"]) == (p, n, invalid)
    if p and n:
        assert res["auc"] == u2 / (2 * p * n)
    else:
        assert res["auc"] != res["auc"]
    if case == "special":
        assert invalid == 1 and p + n == len(SPECIAL) - 1
        # 0 and the denormal 1e-45 (positives) share bucket 0x8000 with -0 (negative); -1e-45 is one below
        assert hist[:, 0x8000].tolist() == [1, 2] and hist[:, 0x7fff].tolist() == [1, 0]
        assert hist[:, 49024].tolist() == [2, 1]                # 1.0, 1.0 and 1 + 2^-8


@pytest.mark.parametrize("scale", [3.0, 0.05, 1e-3])
def test_bucketed_u2_within_the_exact_bound(scale):
    """Against the exact AUC of the fp32 logits |dU2| <= sum_b pos[b] neg[b] (the
    bound from the reference histogram): only pairs sharing a bucket differ."""
    logit, y = _random(4099, scale, 11)
    hist, _, _, p, n = _ref_state(logit, y)
    pos = y.numpy() > 0.5
    exact = _brute_u2(logit.numpy()[pos], logit.numpy()[~pos])
    bound = int((hist[0] * hist[1]).sum())
    u2, p2, n2 = _cpu_auc(logit, y).counts()
    assert (p2, n2) == (p, n)
    assert abs(u2 - exact) <= bound
    assert bound < p * n // 50  # the buckets resolve these scales: the bound is not vacuous


def test_degenerate_and_oversized():
    x, _ = _random(65, 3.0, 3)
    for label in (0.0, 1.0):
        res = _cpu_auc(x, torch.full((65,), label)).compute()
        assert res["auc"] != res["auc"]
        assert res["pos"] + res["neg"] == 65
    assert StreamingAUC("cpu").compute()["auc"] != StreamingAUC("cpu").compute()["auc"]
    for row in (0, 1):
        a = StreamingAUC("cpu")
        a.hist[row, 100] = 1 << 31
        a.hist[1 - row, 7] = 1
        with pytest.raises(OverflowError):
            a.compute()
    a = StreamingAUC("cpu")
    a.hist[1, 100] = (1 << 31) - 1
    a.hist[0, 7] = (1 << 31) - 1
    assert a.compute()["auc"] == 1.0
    assert a.counts()[0] == 2 * ((1 << 31) - 1) ** 2


def test_update_takes_any_layout_and_label_dtype():
    logit, y = _random(130, 3.0, 5)
    ref = _cpu_auc(logit, y)
    a = StreamingAUC("cpu")
    wide = torch.stack([logit, logit], 1)
    a.update(wide[:, 0], y.to(torch.int64))       # strided logits, integer labels
    assert torch.equal(a.hist, ref.hist)
    a.update(logit.double()[:0], y[:0])            # empty
    assert torch.equal(a.hist, ref.hist)
    a.reset()
    assert int(a.hist.sum()) == 0 and int(a.invalid) == 0
    with pytest.raises(ValueError):
        a.update(logit, y[:3])


def test_state_dict_round_trip():
    logit, y = _special()
    a = _cpu_auc(logit, y)
    state = a.state_dict()
    a.update(*_random(65, 3.0, 1))  # the saved state is a copy
    b = StreamingAUC("cpu")
    b.load_state_dict(state)
    ref = _cpu_auc(logit, y)
    assert torch.equal(b.hist, ref.hist) and torch.equal(b.invalid, ref.invalid)
    assert b.compute() == ref.compute()
    with pytest.raises(ValueError):
        b.load_state_dict({"hist": torch.zeros(2, 8, dtype=torch.int64), "invalid": torch.zeros(1)})


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, world, *args):
    port = _port()
    out = mp.Manager().dict()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=fn, args=(r, world, port, out) + args) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    return dict(out)


def _merge_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    logit, y = _random(1000, 3.0, 21)
    logit[5] = float("nan")
    logit[900] = float("nan")
    lo, hi = (0, 377) if rank == 0 else (377, 1000)
    a = StreamingAUC("cpu")
    a.update(logit[lo:hi], y[lo:hi])
    a.merge()
    out[f"hist{rank}"], out[f"invalid{rank}"] = a.hist.clone(), a.invalid.clone()
    dist.destroy_process_group()


def test_merge_two_gloo_ranks_equals_one_process():
    got = _spawn(_merge_worker, 2)
    logit, y = _random(1000, 3.0, 21)
    logit[5] = float("nan")
    logit[900] = float("nan")
    ref = _cpu_auc(logit, y)
    for r in (0, 1):
        assert torch.equal(got[f"hist{r}"], ref.hist)
        assert torch.equal(got[f"invalid{r}"], ref.invalid) and int(ref.invalid) == 2


def test_tower_logits_equal_loss_logits_cpu():
    torch.manual_seed(0)
    tower = DenseTower(64, (32, 16))
    x, y = torch.randn(37, 64), (torch.rand(37) < 0.5).float()
    loss, logit = tower.loss(x, y)
    got, got_loss = tower.logits(x, y)
    assert torch.equal(got, logit) and torch.equal(got_loss, loss.detach())
    assert not got.requires_grad and not got_loss.requires_grad
    got2, none = tower.logits(x)
    assert none is None and torch.equal(got2, logit)


def _ps_eval_run(rank, world, dev, do_eval):
    """tests/test_ctr.py's _ps_worker_ctr (1 PS + 1 worker on the fixed exchange, or
    the one-rank rehearsal) with an evaluation of two held-out batches between
    training steps 2 and 3."""
    B, F, V, D = 16, 6, 50, 8
    emb = ShardedEmbedding(F * V, D, [0], rank, world, dev, lr=0.1, max_ids=B * F, force_fixed=True, rows_bf16=True)
    if world == 2 and rank == 0:
        for step in range(3):
            if step == 2 and do_eval:
                emb.participate_pull()
                emb.participate_pull()
            emb.participate(scale=0.5)
        emb.finalize()
        return {"table": emb.table.cpu().clone(), "accum": emb.accum.cpu().clone()}
    torch.manual_seed(0)
    model = CTRModel(F, V, D, 5, (64, 32), emb, dev, dtype=torch.float32 if dev == "cpu" else torch.bfloat16)

    def batch(g):
        ids = torch.randint(0, V, (B, F), generator=g)
        ids[:, 0] = 3
        dense, y = torch.randn(B, 5, generator=g), torch.randint(0, 2, (B,), generator=g).float()
        return ids.to(dev), dense.to(dev), y.to(dev)

    g, ge = torch.Generator().manual_seed(10), torch.Generator().manual_seed(77)
    held_out = [batch(ge) for _ in range(2)]
    auc = StreamingAUC(dev)
    res = {"losses": [], "eval_losses": []}
    for step in range(3):
        if step == 2 and do_eval:
            for ids, dense, y in held_out:
                res["eval_losses"].append(float(model.evaluate(ids, dense, y, auc)))
            if world == 1:  # a stray push after the pull-only rounds
                try:
                    emb.push(torch.zeros(1, D, device=dev), 0.5)
                    res["push_raised"] = False
                except RuntimeError:
                    res["push_raised"] = True
        ids, dense, y = batch(g)
        x, inv, U = model.build_input(ids, dense)
        if dev != "cpu" and model.tower.fused_ok(x):
            loss, xgrad = model.tower.train_step(x, y)
        else:
            x.requires_grad_(True)
            loss, _ = model.tower.loss(x, y)
            loss.backward()
            xgrad = x.grad
        model.push_grads(xgrad, inv, U, scale=0.5)
        res["losses"].append(float(loss.detach()))
    emb.finalize()
    res["hist"] = auc.hist.cpu().clone()
    if world == 1:
        res["table"], res["accum"] = emb.table.cpu().clone(), emb.accum.cpu().clone()
    return res


def _ps_worker_eval(rank, world, port, out, dev):
    """world 1: the rehearsal with and without the evaluation, one after the other;
    world 2: rank 0 the PS, rank 1 the worker, with the evaluation."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if world == 1:
        out["ref"] = _ps_eval_run(0, 1, dev, True)
        out["plain"] = _ps_eval_run(0, 1, dev, False)
    else:
        out[f"rank{rank}"] = _ps_eval_run(rank, world, dev, True)
    dist.destroy_process_group()


def _check_ps_eval(dev):
    out = mp.Manager().dict()
    ctx = mp.get_context("spawn")
    p1, p2 = _port(), _port()
    procs = [ctx.Process(target=_ps_worker_eval, args=(0, 1, p1, out, dev))] + \
        [ctx.Process(target=_ps_worker_eval, args=(r, 2, p2, out, dev)) for r in range(2)]
    for p in procs:  # the rehearsal and the PS + worker pair side by side
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    ref, plain, ps, got = out["ref"], out["plain"], out["rank0"], out["rank1"]
    # 1 PS + 1 worker == the one-rank rehearsal: losses, table, Adagrad state, histogram
    assert got["losses"] == ref["losses"] and got["eval_losses"] == ref["eval_losses"]
    assert torch.equal(ps["table"], ref["table"]) and torch.equal(ps["accum"], ref["accum"])
    assert torch.equal(got["hist"], ref["hist"])
    assert int(ref["hist"].sum()) == 32 and len(ref["eval_losses"]) == 2
    # the evaluation touched no row and no Adagrad state
    assert plain["losses"] == ref["losses"]
    assert torch.equal(plain["table"], ref["table"]) and torch.equal(plain["accum"], ref["accum"])
    assert int(plain["hist"].sum()) == 0
    assert ref["push_raised"] is True
    assert not torch.equal(ref["table"], ShardedEmbedding(6 * 50, 8, [0], 0, 1, "cpu").table)  # it trained


def test_ps_plus_worker_evaluation_is_pull_only():
    _check_ps_eval("cpu")


def test_push_after_discard_pull_raises():
    emb = ShardedEmbedding(40, 4, [0], 0, 1, "cpu")
    before = emb.table.clone()
    rows, _inv = emb.pull(torch.tensor([1, 5, 5]))
    emb.discard_pull()
    with pytest.raises(RuntimeError):
        emb.push(torch.ones_like(rows))
    emb.participate_pull()
    with pytest.raises(RuntimeError):
        emb.push(torch.ones_like(rows))
    assert torch.equal(emb.table, before)


CPU_ARGS = ["--cpu", "--steps", "60", "--warmup", "0", "--batch", "256", "--fields", "8", "--vocab", "200", "--dim",
            "8", "--hidden", "64,32"]


def _worker_json(argv, capsys):
    from kubedl_amd.workers.xdl_ctr import main
    capsys.readouterr()
    assert main(argv) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def test_worker_end_to_end_reports_auc(capsys):
    """60 CPU steps, then 8 held-out batches: the worker printed eval_auc
    0.7393579344781391 (eval_logloss 0.5998561158776283, 875 positives of 2048
    rows) on one host and 0.7394076239191328 on another (their bf16 CPU GEMMs
    round differently); an untrained fp32 emulation of the same settings gives
    0.440, so the bound 0.6 separates a trained model from a broken evaluation."""
    res = _worker_json(CPU_ARGS + ["--eval-batches", "8"], capsys)
    print(res)
    assert res["eval_rows"] == 2048
    assert res["eval_auc"] > 0.6
    assert res["eval_invalid"] == 0 and 0 < res["eval_pos"] < 2048
    assert 0 < res["eval_logloss"] < 0.69
    assert "eval_history" not in res


def test_worker_eval_off_is_unchanged_and_eval_every_reports_history(capsys):
    off = _worker_json(CPU_ARGS + ["--eval-batches", "0"], capsys)
    assert not [k for k in off if k.startswith("eval")]
    on8 = _worker_json(CPU_ARGS + ["--eval-batches", "8"], capsys)
    assert on8["loss_last"] == off["loss_last"] and on8["loss_first"] == off["loss_first"]
    on = _worker_json(CPU_ARGS + ["--eval-batches", "2", "--eval-every", "25"], capsys)
    assert on["loss_last"] == off["loss_last"] and on["loss_first"] == off["loss_first"]
    assert [h["step"] for h in on["eval_history"]] == [25, 50, 60]
    assert on["eval_history"][-1]["auc"] == on["eval_auc"] and on["eval_rows"] == 512


def test_eval_schedule_is_a_function_of_the_arguments():
    from kubedl_amd.workers.xdl_ctr import eval_steps
    assert eval_steps(60, 0, 10) == frozenset() and eval_steps(60, 4, 0) == frozenset()
    assert sorted(eval_steps(60, 4, 25)) == [25, 50]
    assert sorted(eval_steps(20, 1, 10)) == [10]  # the last step's evaluation is the final one


def _job_rank(rank, world, port, out, argv):
    """One replica of a 1 PS + (world - 1) workers job: the worker's ``main`` under
    the runtime's rank env, its JSON line captured."""
    import contextlib
    import io
    from kubedl_amd.workers.xdl_ctr import main
    os.environ.update(KDL_RANK=str(rank), KDL_WORLD_SIZE=str(world), KDL_NUM_PS="1",
                      KDL_RDZV_ENDPOINT=f"127.0.0.1:{port}", TASK_NAME="ps" if rank == 0 else "worker")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = main(argv)
    out[f"rc{rank}"], out[f"stdout{rank}"] = rc, buf.getvalue()


def test_example_job_one_ps_two_workers_evaluates():
    """examples/xdl/ctr_train_eval.yaml: 1 PS + 2 workers, every replica with the same
    arguments.  Its replicas run here (CPU / gloo, plumbing sizes) to the end: the
    PS's pull-only rounds follow the workers' schedule -- or the job would hang --
    and the first worker reports the AUC merged over both workers."""
    from kubedl_amd.api import codec
    from kubedl_amd.runtime import images
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    (obj,) = codec.load_file(os.path.join(root, "examples", "xdl", "ctr_train_eval.yaml"))
    specs = obj["spec"]["xdlReplicaSpecs"]
    assert specs["PS"]["replicas"] == 1 and specs["Worker"]["replicas"] == 2
    ctrs = [s["template"]["spec"]["containers"][0] for s in specs.values()]
    assert ctrs[0]["args"] == ctrs[1]["args"]  # one schedule for every replica
    assert all(ct["image"] == "kubedl-amd/xdl-ctr" for ct in ctrs)
    assert "kubedl-amd/xdl-ctr" in open(images.__file__).read()
    flags = [a for a in ctrs[0]["args"] if a.startswith("--eval-")]
    assert sorted(flags) == ["--eval-batches=8", "--eval-every=20"]
    argv = ["--cpu", "--steps=20", "--warmup=1", "--batch=64", "--fields=4", "--vocab=100", "--dim=8",
            "--hidden=32,16"] + flags
    got = _spawn(_job_rank, 3, argv)
    assert [got[f"rc{r}"] for r in range(3)] == [0, 0, 0]
    assert got["stdout0"].strip() == "" and got["stdout2"].strip() == ""  # the first worker reports
    res = json.loads([l for l in got["stdout1"].splitlines() if l.startswith("{")][-1])
    assert (res["ps"], res["workers"], res["eval_rows"]) == (1, 2, 2 * 8 * 64)
    assert [h["step"] for h in res["eval_history"]] == [20, 21]
    assert 0 < res["eval_auc"] < 1 and res["eval_invalid"] == 0


def test_eval_launchers_issue_kernels_only():
    """csrc/ctr.hip's convention (tests/test_ctr.py::test_ctr_launchers_issue_kernels_only)
    holds for the evaluation kernels."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "csrc", "ctr_eval.hip")).read()
    for call in ("hipMemsetAsync", "hipMemcpyAsync", "hipMemset(", "hipMemcpy("):
        assert call not in src


# ------------------------------------------------------------------ GPU
def _gpu_auc(logit, y, a=None):
    a = a or StreamingAUC("cuda")
    assert a.use_kernel
    a.update(logit.cuda(), y.cuda())
    return a


def _same_state(a, ref):
    assert torch.equal(a.hist.cpu(), ref.hist)
    assert torch.equal(a.invalid.cpu(), ref.invalid)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 4099, 70001])
def test_auc_accumulate_matches_fallback(n):
    logit, y = _random(n, 3.0, n)
    ref = _cpu_auc(logit, y)
    a = _gpu_auc(logit, y)
    _same_state(a, ref)
    assert a.counts() == ref.counts()


@pytest.mark.gpu
def test_auc_accumulate_special_values_and_empty():
    logit, y = _special()
    a = _gpu_auc(logit, y)
    _same_state(a, _cpu_auc(logit, y))
    assert int(a.invalid) == 1
    a.update(torch.empty(0, device="cuda"), torch.empty(0, device="cuda"))  # n = 0: no launch
    _same_state(a, _cpu_auc(logit, y))
    # rows far outside the LDS windows only (the direct path), many of them
    big = torch.cat([logit[~torch.isnan(logit)][[0, 1, 2, 3, 4, 5, 6, 7, 11, 12]]] * 500)
    by = (torch.arange(big.numel()) % 3 == 0).float()
    _same_state(_gpu_auc(big, by), _cpu_auc(big, by))


@pytest.mark.gpu
def test_auc_accumulate_one_bucket_past_16_bits():
    """70,001 rows in ONE bucket (logit 1.0, alternating labels): more than a 16-bit
    LDS counter holds; a block counts at most auc_rows_per_block(n) < 65536 rows."""
    from kubedl_amd.ops import _ext
    n = 70001
    assert 0 < _ext.load().auc_rows_per_block(n) < 65536
    assert 0 < _ext.load().auc_rows_per_block(1 << 30) < 65536
    logit, y = torch.ones(n), (torch.arange(n) % 2).float()
    a = _gpu_auc(logit, y)
    assert a.hist[:, 49024].tolist() == [35001, 35000]
    assert int(a.hist.sum()) == n
    assert a.counts() == (35001 * 35000, 35000, 35001)


@pytest.mark.gpu
def test_auc_accumulate_successive_updates_and_unaligned_views():
    l1, y1 = _random(4099, 3.0, 1)
    l2, y2 = _random(1025, 0.05, 2)
    ref = _cpu_auc(torch.cat([l1, l2[1:]]), torch.cat([y1, y2[1:]]))
    a = _gpu_auc(l1, y1)
    a.update(l2.cuda()[1:], y2.cuda()[1:])  # 4-byte-aligned views: the scalar-load path
    _same_state(a, ref)
    b = StreamingAUC("cuda", use_kernel=False)  # the torch composition on the device: the same integers
    b.update(l1.cuda(), y1.cuda())
    b.update(l2.cuda()[1:], y2.cuda()[1:])
    _same_state(b, ref)
    assert a.compute() == ref.compute()


@pytest.mark.gpu
def test_auc_finalize_matches_python_integers():
    from kubedl_amd.ops import _ext
    ext = _ext.load()
    g = torch.Generator().manual_seed(4)
    dense = torch.randint(0, 1 << 14, (2, BUCKETS), generator=g)              # P, N < 2^30
    sparse = torch.randint(0, 1 << 20, (2, BUCKETS), generator=g) * (torch.rand(2, BUCKETS, generator=g) < 0.01)
    far = torch.zeros(2, BUCKETS, dtype=torch.int64)
    far[1, 100], far[0, 50000] = 1 << 30, 1 << 30                             # every negative above every positive
    edge = torch.zeros(2, BUCKETS, dtype=torch.int64)
    edge[1, 65535], edge[0, 0], edge[1, 0], edge[0, 65535] = 3, 5, 7, 11
    for hist in (dense, sparse, far, far.flip(0), edge, torch.zeros(2, BUCKETS, dtype=torch.int64)):
        got = tuple(ext.auc_finalize(hist.cuda()).tolist())
        assert got == _py_u2(hist)
    assert tuple(ext.auc_finalize(far.cuda()).tolist()) == (0, 1 << 30, 1 << 30)
    assert tuple(ext.auc_finalize(far.flip(0).contiguous().cuda()).tolist()) == (1 << 61, 1 << 30, 1 << 30)


@pytest.mark.gpu
def test_fused_tower_logits_bit_identical_to_training_forward():
    torch.manual_seed(0)
    tower = DenseTower(128, (128, 64)).cuda().to(torch.bfloat16)
    x = torch.randn(300, 128, device="cuda").to(torch.bfloat16)
    y = (torch.rand(300, device="cuda") < 0.5).float()
    assert tower.fused_ok(x)
    loss, logit = tower.loss(x, y)
    step_loss, _dx = tower.train_step(x, y)
    got, got_loss = tower.logits(x, y)
    assert got.dtype == torch.float32 and got.shape == (300,)
    assert torch.equal(got, logit)
    assert torch.equal(got_loss, loss.detach()) and torch.equal(got_loss, step_loss)
    got2, none = tower.logits(x)
    assert none is None and torch.equal(got2, logit)


@pytest.mark.gpu
def test_evaluate_world1_sync_free_and_side_effect_free():
    torch.manual_seed(0)
    emb = ShardedEmbedding(26 * 1000, 64, [0], 0, 1, "cuda", lr=0.05)
    model = CTRModel(26, 1000, 64, 13, (256, 128), emb, "cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    batches = [(torch.randint(0, 1000, (512, 26), device="cuda", generator=g),
                torch.randn(512, 13, device="cuda", generator=g),
                torch.randint(0, 2, (512,), device="cuda", generator=g).float()) for _ in range(3)]
    # one training step first, so the Adagrad state is not all zeros
    x, inv, U = model.build_input(*batches[0][:2])
    _loss, xgrad = model.tower.train_step(x, batches[0][2])
    model.push_grads(xgrad, inv, U, scale=1.0)
    table, accum = emb.table.clone(), emb.accum.clone()
    params = [p.detach().clone() for p in model.tower.parameters()]
    auc = StreamingAUC("cuda")
    losses = []
    for i, (ids, dense, y) in enumerate(batches):
        if i > 0:  # first call: workspace allocation / kernel loading
            torch.cuda.set_sync_debug_mode("error")
        try:
            losses.append(model.evaluate(ids, dense, y, auc))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(emb.table, table) and torch.equal(emb.accum, accum)
    assert all(torch.equal(p, q) for p, q in zip(model.tower.parameters(), params))
    assert emb._ctx is None
    res = auc.compute()
    assert res["pos"] + res["neg"] == 3 * 512 and res["invalid"] == 0
    # the state equals the torch composition over the same logits
    ref = StreamingAUC("cpu")
    for ids, dense, y in batches:
        x, _, _ = model.build_input(ids, dense)
        emb.discard_pull()
        ref.update(model.tower.logits(x)[0].cpu(), y.cpu())
    _same_state(auc, ref)
    assert all(bool(torch.isfinite(l)) for l in losses)


@pytest.mark.gpu
def test_ps_plus_worker_evaluation_on_gpu():
    _check_ps_eval("cuda")


@pytest.mark.gpu
def test_ctr_worker_trains_and_evaluates_on_gpu(capsys):
    res = _worker_json(["--steps", "20", "--warmup", "2", "--batch", "1024", "--fields", "8", "--vocab", "5000",
                        "--dim", "32", "--hidden", "256,128", "--eval-batches", "4", "--eval-every", "10"], capsys)
    print(res)
    assert res["eval_rows"] == 4096
    assert 0 < res["eval_auc"] < 1
    assert res["hip_kernels"] is True
    assert [h["step"] for h in res["eval_history"]] == [10, 20, 22]
