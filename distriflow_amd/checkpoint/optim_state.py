"""Optimizer state beside the weights of a checkpoint version.

``<version>/optimizer/`` holds the store's optimizer tensors in the flat-variable format
(:mod:`.flatvars`: ``meta.json`` + ``data.bin``) and ``optimizer.json`` = ``{"config": {...}, "tensors":
[names in file order]}``: SGD's momentum buffer, or Adam's first and second moments and its step state
(``ParamStore.optimizer_state``).  A resumed job then continues bit for bit; without this a momentum job
restarts from zero momentum and an Adam job from zero moments and bias-correction step 0.
"""
from __future__ import annotations

import json
import os
from typing import Optional

from .flatvars import load_flat, save_flat

SUBDIR = "optimizer"


def save_optimizer_state(store, directory: str) -> dict:
    """Write ``store``'s optimizer state under ``directory``; returns the optimizer's config record."""
    d = os.path.join(directory, SUBDIR)
    state = store.optimizer_state()
    names = list(state)
    save_flat(d, [state[k] for k in names])
    cfg = store.optimizer_config()
    tmp = os.path.join(d, "optimizer.json.tmp")
    with open(tmp, "w") as f:
        json.dump({"config": cfg, "tensors": names}, f)
    os.replace(tmp, os.path.join(d, "optimizer.json"))
    return cfg


def saved_optimizer(directory: str) -> Optional[dict]:
    """The ``optimizer.json`` record of a checkpoint version, or None for one written without it."""
    p = os.path.join(directory, SUBDIR, "optimizer.json")
    if not os.path.exists(p):
        return None
    with open(p) as f:
        return json.load(f)


def load_optimizer_state(store, directory: str) -> bool:
    """Restore ``store``'s optimizer state from ``directory`` (the store's optimizer is already chosen).
    False for a checkpoint without optimizer state; ValueError when it was saved by another optimizer."""
    rec = saved_optimizer(directory)
    if rec is None:
        return False
    saved = rec["config"].get("name")
    if saved != store.optimizer:
        raise ValueError(f"the checkpoint holds {saved!r} optimizer state; refusing to resume it under "
                         f"{store.optimizer!r} (pass the same --optimizer, or start without --resume)")
    tensors = load_flat(os.path.join(directory, SUBDIR), device=store.device)
    store.load_optimizer_state(dict(zip(rec["tensors"], tensors)))
    return True
