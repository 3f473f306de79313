"""On-disk record of a device parameter-server job (parallel/async_ps.py): what a resumed job needs besides
the weights.  Pure Python, no GPU.

Reference behaviour: the asynchronous server saves the model on every applied gradient and a restarted
server loads the last version and re-dispatches what was incomplete
(/root/reference/src/server/asynchronousSGD_server.ts:95-108, models.ts:98-111,140-150,
dataset.ts:47-67).  The device engine keeps that state in HBM: the version and applied words, the FCFS
cursor, the dataset epoch and its completion arrays (``PSComm.export_state``), the microbatch every rank had
claimed but not yet trained, and the dropout step counter.

Layout, over a :class:`VersionedStore`::

    <dir>/<v>/model.json, weights.bin    the tf.js model (save_layers_model)
    <dir>/resume.json                    the record below (atomic replace)
    <dir>/current -> <v>

    {engine: "async_ps", version, ps: <export_state>, inflight: [bid or null per rank], world, n_params,
     nbatches, batch, epochs, schedule_sha256, engine_step, lr, max_staleness, store_version: v}

Write order: the model directory, then ``resume.json``, then ``current``.  A crash between the first two
leaves a model directory newer than the record: a torn save.  The reader therefore trusts
``resume.json["store_version"]`` and never ``store.last()``; the writer never prunes the version the record
names.
"""
from __future__ import annotations

import hashlib
import os
import shutil
from typing import Callable, Optional

from .store import VersionedStore

ENGINE = "async_ps"
KEEP_LAST = 2
_PS_KEYS = ("version", "applied", "cursor", "epoch", "completed_in_epoch", "sched_ctr", "done_epoch", "claimed_epoch")
_REC_KEYS = ("engine", "version", "ps", "inflight", "world", "n_params", "nbatches", "batch", "epochs",
             "schedule_sha256", "engine_step", "lr", "max_staleness", "store_version")


def schedule_sha256(table_bytes: bytes) -> str:
    """Hash of the microbatch table's bytes (int64, row major): a resumed job must dispatch the same rows."""
    return hashlib.sha256(table_bytes).hexdigest()


def check_ps_state(ps: dict, nbatches: Optional[int] = None):
    """The invariants of a quiesced parameter server (the same ``PSComm.import_state`` enforces)."""
    for k in _PS_KEYS:
        if k not in ps:
            raise ValueError(f"parameter-server state lacks {k!r}")
    if int(ps["version"]) != int(ps["applied"]):
        raise ValueError(f"inconsistent record: version {ps['version']} != applied {ps['applied']} "
                         "(the job was not quiesced)")
    for p in ps.get("owner_prefix") or []:
        if int(p) != int(ps["version"]):
            raise ValueError(f"inconsistent record: an owner prefix ({p}) differs from the version {ps['version']}")
    done, claimed = ps["done_epoch"], ps["claimed_epoch"]
    if len(done) != len(claimed) or (nbatches is not None and len(done) != int(nbatches)):
        raise ValueError(f"inconsistent record: completion arrays of {len(done)} / {len(claimed)} entries"
                         + (f", schedule has {nbatches}" if nbatches is not None else ""))
    cnt = sum(1 for d in done if int(d) == int(ps["epoch"]) + 1)
    if cnt != int(ps["completed_in_epoch"]):
        raise ValueError(f"inconsistent record: completed_in_epoch {ps['completed_in_epoch']} but {cnt} batches "
                         f"are done in epoch {ps['epoch']}")
    if len(ps["sched_ctr"]) != 4:
        raise ValueError("inconsistent record: four schedule counters expected")


def make_record(ps: dict, inflight: list, *, world: int, n_params: int, nbatches: int, batch: int, epochs: int,
                schedule_hash: str, engine_step: int, lr: float, max_staleness: int) -> dict:
    return {"engine": ENGINE, "version": int(ps["version"]), "ps": ps,
            "inflight": [None if b is None or int(b) < 0 else int(b) for b in inflight], "world": int(world),
            "n_params": int(n_params), "nbatches": int(nbatches), "batch": int(batch), "epochs": int(epochs),
            "schedule_sha256": schedule_hash, "engine_step": int(engine_step), "lr": float(lr),
            "max_staleness": int(max_staleness), "store_version": None}


def open_store(save_dir: str, keep_last: int = KEEP_LAST) -> VersionedStore:
    store = VersionedStore(save_dir, keep_last=keep_last)
    store.setup()
    return store


def prune(store: VersionedStore, recorded: str):
    """Drop all but the newest ``keep_last`` version directories -- never the one the record names."""
    if not store.keep_last:
        return
    vs = store.list()
    for v in vs[: max(0, len(vs) - store.keep_last)]:
        if v != recorded and v != store.current():
            shutil.rmtree(store.path(v), ignore_errors=True)


def write_checkpoint(store: VersionedStore, save_model: Callable[[str], object], record: dict) -> str:
    """``save_model(directory)`` writes the tf.js model; then the record, then ``current``.  Returns the store
    version.  The record is validated first: an inconsistent state is never written."""
    check_ps_state(record["ps"], record["nbatches"])
    store.setup()
    v = store.new_version()
    save_model(store.path(v))
    rec = dict(record, store_version=v)
    store.write_resume(rec)
    store.mark_current(v)
    prune(store, v)
    return v


def read_checkpoint(store: VersionedStore, *, n_params: Optional[int] = None, nbatches: Optional[int] = None,
                    batch: Optional[int] = None, schedule_hash: Optional[str] = None) -> Optional[dict]:
    """The validated record (``record["model_json"]`` is the model to load), or None when nothing was saved.
    Raises ValueError when the record is inconsistent or does not belong to this job's model / schedule."""
    rec = store.read_resume()
    if rec is None:
        return None
    if rec.get("engine") != ENGINE:
        raise ValueError(f"resume record of engine {rec.get('engine')!r}, expected {ENGINE!r}")
    for k in _REC_KEYS:
        if k not in rec:
            raise ValueError(f"resume record lacks {k!r}")
    for name, want in (("n_params", n_params), ("nbatches", nbatches), ("batch", batch)):
        if want is not None and int(rec[name]) != int(want):
            raise ValueError(f"checkpoint mismatch: {name} is {rec[name]} in the record, {want} in this job")
    if schedule_hash is not None and rec["schedule_sha256"] != schedule_hash:
        raise ValueError("checkpoint mismatch: the microbatch schedule differs from the saved job's "
                         "(schedule_sha256; same data size, batch and seed are required)")
    check_ps_state(rec["ps"], rec["nbatches"])
    if int(rec["version"]) != int(rec["ps"]["version"]):
        raise ValueError(f"inconsistent record: version {rec['version']} != ps.version {rec['ps']['version']}")
    for b in rec["inflight"]:
        if b is not None and not (0 <= (int(b) & 0xFFFFFFFF) < int(rec["nbatches"])):
            raise ValueError(f"inconsistent record: in-flight id {b} outside the schedule")
    # the version the record names -- a newer directory is a torn save and is ignored
    model_json = os.path.join(store.path(str(rec["store_version"])), "model.json")
    if not os.path.exists(model_json):
        raise ValueError(f"checkpoint {store.save_dir}: the recorded version {rec['store_version']} has no model.json")
    return dict(rec, model_json=model_json)
