"""Checkpoint and resume of the device parameter server (parallel/async_ps.py, csrc/async_ps.hip): a job
saved at a quiesce point and resumed in fresh processes / trainers ends exactly where an uninterrupted one does
(reference: save on every applied gradient, resume from the last version, re-dispatch what is incomplete --
/root/reference/src/server/asynchronousSGD_server.ts:95-108, models.ts:98-111,140-150, dataset.ts:47-67)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from mp_util import free_port as _port
from mp_util import init_rank, real_devices

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {"lenet5-fused": ("lenet5", None), "keras_cnn-excl": ("keras_cnn", None),
         "keras_cnn-generic": ("keras_cnn", "ps_excl_fused=0")}
_REF = {}  # (path, graph) -> the uninterrupted run, computed once


def _trainer(model, seed, graph, data, labels, perm, epochs, B=256, **kw):
    from distriflow_amd.models.zoo import build_model
    from distriflow_amd.parallel.async_ps import AsyncPSTrainer

    net = build_model(model, device=data.device, seed=seed)
    kw.setdefault("max_staleness", 0)
    tr = AsyncPSTrainer(net, lr=0.05, graph=graph, **kw)
    tr.bind_dataset(data, labels, B, scale=1.0 / 255.0)
    tr.bind_schedule(perm, epochs=epochs)
    return tr


def _steps(tr, n, graph):
    if graph == "full":
        tr.prepare_run(4)
        tr.run(n)
    else:
        for _ in range(n):
            tr.step()
    torch.cuda.synchronize()


def _end_state(tr):
    st = tr.ps_stats()
    assert st["error"] == 0, st
    return ({k: st[k] for k in ("version", "duplicates", "redispatched", "completed", "noop_steps", "epoch")},
            tr.done_epochs(), tr.pull_master(torch.empty_like(tr.net.store.master)).clone())


def _world1_problem():
    from distriflow_amd.data.synthetic import synthetic_mnist
    from distriflow_amd.parallel.data_parallel import epoch_permutations

    dev = torch.device("cuda", 0)
    nb = 8
    data, labels = synthetic_mnist(nb * 256, seed=3, device=dev)
    return dev, nb, data, labels, epoch_permutations(nb * 256, 256, nb, dev, seed=1)


# ------------------------------------------------------------------------------------------ a. world 1
@pytest.mark.parametrize("k", [5, 8], ids=["mid-epoch", "epoch-boundary"])
@pytest.mark.parametrize("graph", ["none", "full"])
@pytest.mark.parametrize("path", list(PATHS))
def test_resumed_equals_uninterrupted(path, graph, k, monkeypatch, tmp_path):
    """Run A: nb * epochs + 3 steps.  Run B: k steps, save, a fresh net of ANOTHER seed and a fresh trainer, load,
    the remaining steps.  Same kernels, same inputs, same order (the bf16 copies and conv fragments are
    functions of the fp32 master alone): the end states and the final masters are bit-equal."""
    from distriflow_amd.checkpoint.ps_state import open_store

    model, diag = PATHS[path]
    if diag:
        monkeypatch.setenv("DISTRIFLOW_DIAG", diag)
    dev, nb, data, labels, perm = _world1_problem()
    epochs, total = 2, nb * 2 + 3
    if (path, graph) not in _REF:
        ta = _trainer(model, 0, graph, data, labels, perm, epochs)
        assert (ta.fused_ps, ta.excl_fused) == {"lenet5-fused": (True, False), "keras_cnn-excl": (False, True),
                                                "keras_cnn-generic": (False, False)}[path]
        _steps(ta, total, graph)
        _REF[(path, graph)] = _end_state(ta)
        del ta
    ref_st, ref_done, ref_master = _REF[(path, graph)]
    assert ref_st["version"] == nb * epochs and ref_st["duplicates"] == 0 and ref_done == [epochs] * nb, ref_st

    store = open_store(str(tmp_path / "ckpt"))
    tb = _trainer(model, 0, graph, data, labels, perm, epochs)
    assert tb.ps_stats()["resumed_from_version"] is None
    _steps(tb, k, graph)
    assert tb.save_checkpoint(store) == store.current()
    saved_master = tb._ckpt_master.clone()
    rec = store.read_resume()
    has_inflight = path != "keras_cnn-generic"
    assert rec["version"] == rec["ps"]["version"] == rec["ps"]["applied"] == k and rec["engine_step"] >= 0
    if has_inflight:  # one claimed, untrained batch; at the epoch boundary it already belongs to epoch 1
        assert rec["inflight"][0] is not None and rec["inflight"][0] >> 32 == (1 if k == nb else 0), rec["inflight"]
    else:
        assert rec["inflight"] == [None]
    del tb

    tc = _trainer(model, 7, graph, data, labels, perm, epochs)  # different initial weights
    assert not torch.equal(tc.net.store.master, saved_master)
    got = tc.load_checkpoint(store)
    assert got["store_version"] == rec["store_version"]
    assert torch.equal(tc.pull_master(torch.empty_like(saved_master)), saved_master)
    st = tc.ps_stats()
    assert (st["version"], st["epoch"], st["cursor"], st["applied"]) == \
        (rec["ps"]["version"], rec["ps"]["epoch"], rec["ps"]["cursor"], rec["ps"]["applied"]), st
    assert st["resumed_from_version"] == k and tc.done_epochs() == rec["ps"]["done_epoch"]
    assert int(tc.net.step_dev.item()) == rec["engine_step"]
    if has_inflight:  # the first trained microbatch is the recorded one, not a fresh claim
        tc._prime()
        assert tc.ps.inflight_bid() == rec["inflight"][0]
        assert tc.ps_stats()["cursor"] == rec["ps"]["cursor"]  # no cursor add
        with pytest.raises(RuntimeError, match="before the first step"):
            tc.load_checkpoint(store)
    _steps(tc, total - k, graph)
    end_st, end_done, end_master = _end_state(tc)
    assert end_st == ref_st, (end_st, ref_st)
    assert end_done == ref_done
    assert torch.equal(end_master, ref_master)


# ------------------------------------------------------------------------------------------ b. no perturbation
def test_saving_does_not_perturb_training(tmp_path):
    from distriflow_amd.checkpoint.ps_state import open_store

    dev, nb, data, labels, perm = _world1_problem()
    res = []
    for save in (False, True):
        tr = _trainer("lenet5", 0, "full", data, labels, perm, 2)
        store = open_store(str(tmp_path / "s"))
        for i in range(nb * 2 + 3):
            tr.step()
            if save and i % 3 == 2:
                tr.save_checkpoint(store)
        torch.cuda.synchronize()
        res.append(_end_state(tr))
        if save:
            assert len(store.list()) == 2 and store.read_resume()["store_version"] == store.current()
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert torch.equal(res[0][2], res[1][2])


def test_joinable_trainer_refuses_checkpoints(tmp_path):
    from distriflow_amd.checkpoint.ps_state import open_store

    dev, nb, data, labels, perm = _world1_problem()
    tr = _trainer("lenet5", 0, "none", data, labels, perm, 2, joinable=True)
    store = open_store(str(tmp_path / "s"))
    with pytest.raises(RuntimeError, match="joinable"):
        tr.save_checkpoint(store)
    with pytest.raises(RuntimeError, match="joinable"):
        tr.load_checkpoint(store)
    assert store.list() == []


# ------------------------------------------------------------------------------------------ c. native round trip
def _open_ps(rank, world, n, timeout_s=20.0, owner_ring=0):
    import torch.distributed as dist

    from distriflow_amd import native

    ps = native.require().PSComm(rank, world, 0, n, timeout_s)
    ctrl = [ps.handle() if rank == 0 else b""]
    shard = ps.shard_handle()
    shards = [shard] * world
    dist.broadcast_object_list(ctrl, src=0)
    dist.all_gather_object(shards, shard)
    ps.open(ctrl[0], shards)
    if owner_ring:
        oh = ps.owner_init(owner_ring)
        ohs = [oh] * world
        dist.all_gather_object(ohs, oh)
        ps.owner_open(ohs)
    return ps


NATIVE_N, NATIVE_NB, NATIVE_LR, NATIVE_STALE = 4096, 16, 0.5, 2


def _native_phase(rank, world, port, out_dir, owner, phase, steps):
    """Phase 1: constant gradients g = rank + 1 on a zero master, quiesce, export.  Phase 2 (new processes):
    seed the shards from the saved master, import, read back, apply more."""
    import torch.distributed as dist

    dev = init_rank(rank, world, port)
    n = NATIVE_N
    ps = _open_ps(rank, world, n, owner_ring=NATIVE_STALE + 2 if owner else 0)
    ps.set_schedule(NATIVE_NB, 0)
    res = {}
    if phase == 1:
        ps.init_master(torch.zeros(n, device=dev))
        dist.barrier()
    else:
        saved = torch.load(os.path.join(out_dir, "p1_r0.pt"), weights_only=True)
        ps.init_master(saved["master"].to(dev))
        dist.barrier()
        if rank == 0:
            refused = 0
            for bad in (dict(saved["state"], applied=saved["state"]["applied"] - 1),
                        dict(saved["state"], completed_in_epoch=saved["state"]["completed_in_epoch"] + 1),
                        dict(saved["state"], done_epoch=saved["state"]["done_epoch"] + [0]),
                        dict(saved["state"], owner_prefix=[saved["state"]["version"] + 1])):
                try:
                    ps.import_state(bad)
                except RuntimeError:
                    refused += 1
            res["refused"] = refused
            res["untouched"] = ps.export_state()["version"] == 0  # a refused import writes nothing
            ps.import_state(saved["state"])
        else:
            try:
                ps.import_state(saved["state"])
                res["nonserver_refused"] = False
            except RuntimeError:
                res["nonserver_refused"] = True
        dist.barrier()
        res["readback"] = ps.export_state()
        res["done_epochs"] = list(ps.done_epochs())
        dist.barrier()
    w = torch.empty(n, device=dev)
    g = torch.full((n,), float(rank + 1), device=dev)
    for _ in range(steps):
        ps.fetch_pull(w)
        ps.apply(g, NATIVE_LR, NATIVE_STALE)
    torch.cuda.synchronize()
    dist.barrier()
    if owner:
        ps.drain(w, quiesced=True)
        torch.cuda.synchronize()
        dist.barrier()
    st = ps.stats()
    res.update(accepted=st[0], rejected=st[1], err=st[5], herr=ps.host_error(), state=ps.export_state(),
               inflight=ps.inflight_bid())
    m = torch.empty(n, device=dev)
    ps.copy_master(m)
    torch.cuda.synchronize()
    res["master"] = m.cpu()
    torch.save(res, os.path.join(out_dir, f"p{phase}_r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("owner", [False, True], ids=["cas", "owner-applies"])
def test_native_state_round_trip_exact(owner):
    """Integers in fp32 (lr a power of two, g = rank + 1): the resumed server's master is exactly
    saved - lr * sum(accepted_r * (r + 1)) and its version the saved one plus the admissions after it."""
    world = 2
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_native_phase, args=(world, _port(), d, owner, 1, 6), nprocs=world, join=True)
        p1 = [torch.load(os.path.join(d, f"p1_r{r}.pt"), weights_only=True) for r in range(world)]
        mp.spawn(_native_phase, args=(world, _port(), d, owner, 2, 5), nprocs=world, join=True)
        p2 = [torch.load(os.path.join(d, f"p2_r{r}.pt"), weights_only=True) for r in range(world)]
    s1 = p1[0]["state"]
    assert all(x["err"] == 0 and x["herr"] == 0 for x in p1 + p2)
    assert p1[1]["state"] == s1  # any rank may export: every rank maps the control buffer
    acc1 = sum(x["accepted"] for x in p1)
    assert s1["version"] == s1["applied"] == acc1 >= 6
    assert s1["owner_prefix"] == ([acc1] * world if owner else [])
    assert len(s1["done_epoch"]) == len(s1["claimed_epoch"]) == NATIVE_NB
    assert s1["completed_in_epoch"] == sum(1 for v in s1["done_epoch"] if v == s1["epoch"] + 1)
    exp1 = -NATIVE_LR * sum(x["accepted"] * (r + 1) for r, x in enumerate(p1))
    assert torch.equal(p1[0]["master"], torch.full((NATIVE_N,), exp1)) and torch.equal(p1[0]["master"], p1[1]["master"])
    # the quiesced drain claimed nothing: every rank still holds the id of its last pull
    assert all(x["inflight"] >= 0 for x in p1)
    # phase 2: the words read back equal, on both ranks
    assert p2[0]["refused"] == 4 and p2[0]["untouched"] and p2[1]["nonserver_refused"]
    for x in p2:
        assert x["readback"] == s1 and x["done_epochs"] == s1["done_epoch"]
    acc2 = sum(x["accepted"] for x in p2)
    s2 = p2[0]["state"]
    assert acc2 >= 5 and s2["version"] == s2["applied"] == s1["version"] + acc2
    exp2 = exp1 - NATIVE_LR * sum(x["accepted"] * (r + 1) for r, x in enumerate(p2))
    assert torch.equal(p2[0]["master"], torch.full((NATIVE_N,), exp2))
    assert s2["sched_ctr"][0] + s2["sched_ctr"][3] == s2["version"]  # completed + duplicates: every admission counted


# ------------------------------------------------------------------------------------------ d. world 2, trainer
T_NB, T_B, T_EPOCHS = 16, 64, 2


def _w2_problem(dev):
    from distriflow_amd.data.synthetic import synthetic_mnist
    from distriflow_amd.parallel.data_parallel import epoch_permutations

    data, labels = synthetic_mnist(T_NB * T_B, seed=3, device=dev)
    return data, labels, epoch_permutations(T_NB * T_B, T_B, T_NB, dev, seed=1)


def _run_to_end(tr, world):
    """Log the id about to be trained before each step; step until every rank is finished."""
    from distriflow_amd.parallel.p2p import _agree

    tr.prepare_run(1)  # (graph "none": the eager prologue alone -- the first id is now claimed or taken)
    log = []
    for _ in range(8 * T_NB * T_EPOCHS):
        log.append(int(tr.ps.inflight_bid()))
        tr.step()
        torch.cuda.synchronize()
        fin = tr.finished()
        if world > 1:
            fin = _agree(fin, None, tr.net.device)
        if fin:
            break
    return log


def _w2_worker(rank, world, port, ckpt_dir, out_dir, owner, phase):
    import torch.distributed as dist

    from distriflow_amd.checkpoint.ps_state import open_store

    dev = init_rank(rank, world, port)
    data, labels, perm = _w2_problem(dev)
    tr = _trainer("lenet5", rank if phase == 1 else 10 + rank, "none", data, labels, perm, T_EPOCHS, B=T_B,
                  max_staleness=4, owner_apply=owner, timeout_s=20.0)
    assert tr.fused_ps and tr.owner_apply == owner
    store = open_store(ckpt_dir)
    res = {}
    if phase == 1:
        for _ in range(5):
            tr.step()
        tr.save_checkpoint(store)
        res["bid"] = int(tr.ps.inflight_bid())
    else:
        tr.load_checkpoint(store)
        res["log"] = _run_to_end(tr, world)
        torch.cuda.synchronize()
        dist.barrier()
        res.update(stats=tr.ps_stats(), done=tr.done_epochs())
    torch.save(res, os.path.join(out_dir, f"p{phase}_r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _check_resumed_logs(rec, logs):
    e0, done0 = rec["ps"]["epoch"], rec["ps"]["done_epoch"]
    seen = set()
    for log in logs:
        for bid in log:
            if bid >= 0 and bid >> 32 == e0:
                b = bid & 0xFFFFFFFF
                assert done0[b] != e0 + 1, f"batch {b} was complete in epoch {e0} before the snapshot, trained again"
                seen.add(b)
    assert {b for b in range(T_NB) if done0[b] != e0 + 1} <= seen


@pytest.mark.timeout(300)
@pytest.mark.parametrize("owner", [False, True], ids=["cas", "owner-applies"])
def test_world2_resume_and_changed_rank_count(owner):
    from distriflow_amd.checkpoint.ps_state import open_store

    world = 2
    with tempfile.TemporaryDirectory() as d:
        ck = os.path.join(d, "ckpt")
        mp.spawn(_w2_worker, args=(world, _port(), ck, d, owner, 1), nprocs=world, join=True)
        rec = open_store(ck).read_resume()
        p1 = [torch.load(os.path.join(d, f"p1_r{r}.pt"), weights_only=True) for r in range(world)]
        assert rec["version"] == rec["ps"]["version"] == rec["ps"]["applied"] and rec["world"] == 2
        assert rec["ps"]["owner_prefix"] == ([rec["version"]] * world if owner else [])
        assert rec["inflight"] == [x["bid"] for x in p1] and all(b is not None for b in rec["inflight"])
        mp.spawn(_w2_worker, args=(world, _port(), ck, d, owner, 2), nprocs=world, join=True)
        p2 = [torch.load(os.path.join(d, f"p2_r{r}.pt"), weights_only=True) for r in range(world)]
        for r, x in enumerate(p2):
            assert x["log"][0] == rec["inflight"][r], (r, x["log"][:3], rec["inflight"])
            assert x["stats"]["error"] == 0 and x["stats"]["resumed_from_version"] == rec["version"]
        _check_resumed_logs(rec, [x["log"] for x in p2])
        assert p2[0]["done"] == [T_EPOCHS] * T_NB and p2[0]["stats"]["completed"] == T_NB * T_EPOCHS, p2[0]["stats"]
        # the same checkpoint at world 1: rank 1's in-flight id is dropped and comes round again on the cursor
        dev = torch.device("cuda", 0)
        data, labels, perm = _w2_problem(dev)
        tr = _trainer("lenet5", 20, "none", data, labels, perm, T_EPOCHS, B=T_B, max_staleness=4)
        assert tr.world == 1
        tr.load_checkpoint(open_store(ck))
        log = _run_to_end(tr, 1)
        torch.cuda.synchronize()
        assert log[0] == rec["inflight"][0]
        _check_resumed_logs(rec, [log])
        st = tr.ps_stats()
        assert tr.done_epochs() == [T_EPOCHS] * T_NB and st["completed"] == T_NB * T_EPOCHS and st["error"] == 0, st


# ------------------------------------------------------------------------------------------ e. launcher
def _launch(args, timeout=170):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    if not real_devices(2):  # the ranks share cuda:0 with gloo as the control plane (mp_util.init_rank does the same)
        env["DISTRIFLOW_BACKEND"] = "gloo"
    return subprocess.run([sys.executable, "-m", "distriflow_amd.launch"] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def _last_json(out):
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


@pytest.mark.timeout(400)
def test_launcher_async_save_and_resume(tmp_path):
    d = str(tmp_path / "ckpt")
    nb, epochs = 16, 2
    common = ["--nproc", "2", "async", "--model", "lenet5", "--num-examples", str(nb * 256), "--batch", "256",
              "--epochs", str(epochs), "--max-staleness", "4", "--save-dir", d]
    p = _launch(common + ["--steps", "8"])
    assert p.returncode == 0, p.stderr[-3000:]
    first = _last_json(p.stdout)
    assert first["steps_per_rank"] == 8 and first["checkpoints"] == 1 and first["resumed_from_version"] is None, first
    assert first["checkpoint_ms_mean"] > 0 and first["checkpoint_ms_max"] >= first["checkpoint_ms_mean"]
    assert not first["finished"] and 0 < first["version"] <= 16
    assert json.load(open(os.path.join(d, "resume.json")))["version"] == first["version"]
    p = _launch(common + ["--resume"])
    assert p.returncode == 0, p.stderr[-3000:]
    out = _last_json(p.stdout)
    assert out["resumed_from_version"] == first["version"], out
    assert out["epoch"] == epochs and out["finished"] and out["completed"] == nb * epochs and out["error"] == 0, out
    assert out["checkpoints"] >= 1


def test_launcher_save_dir_with_store_port_is_a_usage_error(tmp_path):
    p = _launch(["async", "--save-dir", str(tmp_path / "x"), "--store-port", "29611"], timeout=60)
    assert p.returncode == 2 and "--store-port" in p.stderr
    assert not os.path.exists(tmp_path / "x")
