"""Checkpoint / resume of the device parameter-server engines, host side (no GPU): the on-disk record
(checkpoint/ps_state.py), the launcher's restart argv, and the FedAvg device engine resumed on CPU."""
import copy
import json
import os
import subprocess
import sys

import pytest

from distriflow_amd.checkpoint import ps_state
from distriflow_amd.checkpoint.store import VersionedStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, B, NPARAMS = 8, 256, 4096
TABLE = bytes(range(256)) * 4


def _ps(version=5, epoch=0, done=None):
    done = [1, 1, 1, 1, 1, 0, 0, 0] if done is None else done
    return {"version": version, "applied": version, "cursor": 6, "epoch": epoch,
            "completed_in_epoch": sum(1 for d in done if d == epoch + 1), "sched_ctr": [version, 0, 0, 0],
            "done_epoch": list(done), "claimed_epoch": [1, 1, 1, 1, 1, 1, 0, 0], "owner_prefix": []}


def _record(**kw):
    ps = kw.pop("ps", None) or _ps()
    return ps_state.make_record(ps, kw.pop("inflight", [5]), world=1, n_params=NPARAMS, nbatches=NB, batch=B, epochs=2,
                                schedule_hash=ps_state.schedule_sha256(TABLE), engine_step=5, lr=0.05, max_staleness=4)


def _fake_model(tag):
    def save(d):
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "model.json"), "w") as f:
            json.dump({"tag": tag}, f)
    return save


def _read(store, **kw):
    want = dict(n_params=NPARAMS, nbatches=NB, batch=B, schedule_hash=ps_state.schedule_sha256(TABLE))
    want.update(kw)
    return ps_state.read_checkpoint(store, **want)


def test_record_round_trip(tmp_path):
    store = ps_state.open_store(str(tmp_path / "c"))
    assert _read(store) is None  # nothing saved yet
    rec = _record(inflight=[(0 << 32) | 5, -1, None])
    v = ps_state.write_checkpoint(store, _fake_model("a"), rec)
    got = _read(store)
    assert got["store_version"] == v == store.current()
    assert got["model_json"] == os.path.join(store.path(v), "model.json")
    assert got["inflight"] == [5, None, None]  # a negative id (schedule finished) is no in-flight batch
    for k in ("engine", "version", "ps", "world", "n_params", "nbatches", "batch", "epochs", "schedule_sha256",
              "engine_step", "lr", "max_staleness"):
        assert got[k] == rec[k], k
    assert got["engine"] == "async_ps" and got["version"] == 5
    # resume.json is written whole (atomic replace): no temporary file is left
    assert sorted(os.listdir(store.save_dir)) == sorted([v, "current", "resume.json"])


def test_version_directory_newer_than_record_is_ignored(tmp_path):
    store = ps_state.open_store(str(tmp_path / "c"))
    v = ps_state.write_checkpoint(store, _fake_model("good"), _record())
    torn = store.new_version()  # a save that died after its model directory, before the record
    _fake_model("torn")(store.path(torn))
    assert store.last() == torn != v
    got = _read(store)
    assert got["store_version"] == v
    assert json.load(open(got["model_json"]))["tag"] == "good"


@pytest.mark.parametrize("kw", [dict(schedule_hash=ps_state.schedule_sha256(TABLE + b"x")), dict(batch=B // 2),
                                dict(nbatches=NB + 1), dict(n_params=NPARAMS + 4)],
                         ids=["schedule", "batch", "nbatches", "n_params"])
def test_reader_raises_on_job_mismatch(tmp_path, kw):
    store = ps_state.open_store(str(tmp_path / "c"))
    ps_state.write_checkpoint(store, _fake_model("a"), _record())
    with pytest.raises(ValueError, match="mismatch|schedule"):
        _read(store, **kw)


def _corrupt_unquiesced(rec):
    rec["ps"]["applied"] -= 1


def _corrupt_count(rec):
    rec["ps"]["completed_in_epoch"] += 1


def _corrupt_prefix(rec):
    rec["ps"]["owner_prefix"] = [rec["ps"]["version"], rec["ps"]["version"] - 1]


def _corrupt_len(rec):
    rec["ps"]["done_epoch"].append(0)


@pytest.mark.parametrize("corrupt", [_corrupt_unquiesced, _corrupt_count, _corrupt_prefix, _corrupt_len])
def test_reader_and_writer_refuse_inconsistent_record(tmp_path, corrupt):
    store = ps_state.open_store(str(tmp_path / "c"))
    ps_state.write_checkpoint(store, _fake_model("a"), _record())
    bad = copy.deepcopy(store.read_resume())
    corrupt(bad)
    store.write_resume(bad)
    with pytest.raises(ValueError, match="inconsistent"):
        _read(store)
    fresh = _record()
    corrupt(fresh)
    n_before = len(store.list())
    with pytest.raises(ValueError, match="inconsistent"):
        ps_state.write_checkpoint(store, _fake_model("b"), fresh)
    assert len(store.list()) == n_before  # nothing was written


def test_keep_last_never_deletes_the_recorded_version(tmp_path):
    store = ps_state.open_store(str(tmp_path / "c"), keep_last=1)
    for i in range(4):
        v = ps_state.write_checkpoint(store, _fake_model(str(i)), _record(ps=_ps(version=5 + i, done=[1] * 5 + [0] * 3)))
        assert store.list() == [v] and store.read_resume()["store_version"] == v
    # torn saves newer than the record pile up behind it: pruning to keep_last must still keep the recorded one
    for _ in range(3):
        _fake_model("torn")(store.path(store.new_version()))
    ps_state.prune(store, v)
    assert v in store.list() and len(store.list()) == 2
    assert json.load(open(_read(store, )["model_json"]))["tag"] == "3"
    # bounded over many saves
    store2 = ps_state.open_store(str(tmp_path / "d"))
    for i in range(6):
        v2 = ps_state.write_checkpoint(store2, _fake_model(str(i)), _record())
    assert len(store2.list()) == ps_state.KEEP_LAST and v2 in store2.list()


def test_restart_argv():
    from distriflow_amd.launch import restart_argv

    kill = ["--fault-kill-rank", "0", "--fault-kill-step=25"]
    sync = ["sync", "--model", "mlp_mnist", "--save-dir", "d"]
    assert restart_argv(sync + kill) == sync + ["--resume"]
    assert restart_argv(sync + ["--resume"] + kill) == sync + ["--resume"]  # not added twice
    assert restart_argv(["sync", "--model", "mlp_mnist"] + kill) == ["sync", "--model", "mlp_mnist", "--resume"]
    for mode in ("async", "fedavg"):
        base = [mode, "--model", "lenet5"]
        assert restart_argv(base + kill) == base  # no checkpoint to resume from; the fault is stripped
        assert restart_argv(base + ["--resume"] + kill) == base
        assert restart_argv(base + ["--save-dir", "d"] + kill) == base + ["--save-dir", "d", "--resume"]
        assert restart_argv(base + ["--save-dir=d"] + kill) == base + ["--save-dir=d", "--resume"]
    assert restart_argv(["fedsgd", "--save-dir", "d"] + kill) == ["fedsgd", "--save-dir", "d"]
    # the delay flags are no injected failure: they stay
    assert restart_argv(["async", "--fault-delay-rank", "1", "--fault-delay-ms", "5"]) == \
        ["async", "--fault-delay-rank", "1", "--fault-delay-ms", "5"]


def test_async_save_dir_usage_errors():
    from distriflow_amd.launch import build_parser, check_args

    ap = build_parser()
    for argv in (["async", "--save-dir", "d", "--store-port", "29600"], ["async", "--resume"],
                 ["async", "--engine", "roles", "--save-dir", "d"], ["fedavg", "--resume"],
                 ["fedavg", "--engine", "roles", "--save-dir", "d"]):
        with pytest.raises(SystemExit) as e:
            check_args(ap, ap.parse_args(argv))
        assert e.value.code == 2, argv
    a = ap.parse_args(["async", "--save-dir", "d"])
    check_args(ap, a)
    assert a.save_every == 1024 and a.steps == 0 and not a.resume


def _launch(args, timeout=280):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "-m", "distriflow_amd.launch"] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


@pytest.mark.timeout(600)
def test_fedavg_device_resumed_job_matches_uninterrupted_job(tmp_path):
    """4 rounds in one job against 2 rounds, then --resume for the rest: the stream is rebuilt from the original
    seed and the resumed job skips the rounds already run, so both save bit-identical weights."""
    common = ["fedavg", "--engine", "device", "--device", "cpu", "--model", "mlp_mnist", "--num-examples", "2048",
              "--batch", "32", "--local-steps", "5", "--lr", "0.1"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    p = _launch(["--nproc", "2"] + common + ["--rounds", "4", "--save-dir", a])
    assert p.returncode == 0, p.stderr[-3000:]
    p = _launch(["--nproc", "2"] + common + ["--rounds", "2", "--save-dir", b])
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.load(open(os.path.join(b, "resume.json")))["round"] == 2
    w2 = open(os.path.join(b, "current", "weights.bin"), "rb").read()
    p = _launch(["--nproc", "2"] + common + ["--rounds", "4", "--save-dir", b, "--resume"])
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.load(open(os.path.join(b, "resume.json")))["round"] == 4
    wa = open(os.path.join(a, "current", "weights.bin"), "rb").read()
    wb = open(os.path.join(b, "current", "weights.bin"), "rb").read()
    assert len(wa) > 0 and wa == wb and wb != w2
    assert len(VersionedStore(b).list()) <= ps_state.KEEP_LAST
