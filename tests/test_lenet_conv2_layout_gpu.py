"""Fused LeNet-5 train kernel, the LDS layout of the conv2 output gradient (csrc/lenet_fused.hip): dC2 rows on
a bank diagonal (phase D stores through ``place``), phase E reading the physical rows in order with its pixels
from the row-to-pixel table, phase F gathering placed rows and class-matched rows of the zero block.

What can go wrong is a position stored at one row and read at another (any of the three phases disagreeing
about ``place``), a padding or zero-block row that is not zero or is counted, a pixel paired with the wrong
dC2 row in phase E, a "no tap" lane of phase F reading live data, or the trimmed kernel's trip counts no longer
covering the rows of its live images.  The shapes are the smallest that reach every case: every default and
forced ``lenet_ipw``, last workgroups of 1, 3, 5 and 7 images, exactly 3 and 9 workgroups.

``lenet_ipw`` reads DISTRIFLOW_DIAG once per process, so every forced setting runs in one fresh child
process (this file as a script) that reports one verdict per case; the tests below read the verdicts."""
import functools
import inspect
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# forced lenet_ipw (0: the default policy, one image per workgroup at these sizes) -> batch sizes
GRAD_CASES = {0: (5, 8), 2: (6,), 4: (12,), 8: (9, 11, 13, 15, 24, 72)}
CONV1 = ("conv2d_1/kernel", "conv2d_1/bias")
FR_C2, FR_DG = 15, 22  # conv2 forward fragments of the fragment buffer (csrc/lenet_frag.h), 1 KB each


# ------------------------------------------------------------------------------------------------ child
def _tols(base):
    p = inspect.signature(base._check).parameters
    return p["tol_rel"].default, p["min_cos"].default


def _close(base, tag, name, gg, gc):
    """One tensor under base._check's own measure and tolerances, figures printed first."""
    tol_rel, min_cos = _tols(base)
    gg, gc = gg.double().flatten(), gc.double().flatten()
    cos = float((gg @ gc) / (gg.norm() * gc.norm() + 1e-30))
    rel = float((gg - gc).abs().max() / (gc.abs().max() + 1e-12))
    print(f"{tag}: {name:<18} cos {cos:.6f} max-rel {rel:.5f}")
    assert cos > min_cos and rel < tol_rel, f"{name}: cos {cos:.5f} max-rel {rel:.4f}"


def _grads_vs_cpu(base, ipw, B):
    """The recipe and tolerances of test_lenet_frag_stage_gpu: every tensor and the stats."""
    import torch

    from distriflow_amd import ops

    assert ops.lenet_blocks(B) == -(-B // ipw), f"lenet_ipw is not {ipw} at B = {B}"
    g, c = base._nets(B)
    x, y = base._batch(B)
    sg = g.compute_gradients(x.cuda(), y.cuda()).clone()
    sc = c.compute_gradients(x, y)
    torch.cuda.synchronize()
    for s in g.store.specs:
        _close(base, f"grads{B}", s.name, g.store.gradient(s.name).detach().cpu(), c.store.gradient(s.name))
    print(f"grads{B}: stats gpu {sg.tolist()} cpu {sc.tolist()}")
    base._check(g, {s.name: c.store.gradient(s.name) for s in c.store.specs}, sc, sg)


def _repeatable(base, B, n=10):
    import torch

    g, _ = base._nets(B)
    x, y = base._batch(B, seed=1)
    x, y = x.cuda(), y.cuda()
    s0 = g.compute_gradients(x, y).clone()
    g0 = g.store.grad.clone()
    assert torch.isfinite(g0).all()
    assert float(g.store.gradient(CONV1[0]).abs().max()) > 0
    for k in range(1, n):
        s = g.compute_gradients(x, y).clone()
        assert torch.equal(s, s0), f"stats differ in run {k}"
        assert torch.equal(g.store.grad, g0), f"gradients differ in run {k}"


def _border(base, ipw, B):
    """0 / 255 uint8 images read through the index vector: the conv1 kernel and bias gradients come from dP1,
    every element of which sums the "no tap" lanes of phase F (zero-block rows) with the live ones."""
    import torch

    from distriflow_amd import ops
    from distriflow_amd.data.synthetic import synthetic_mnist

    assert ops.lenet_blocks(B) == -(-B // ipw), f"lenet_ipw is not {ipw} at B = {B}"
    g, c = base._nets(B)
    names = [s.name for s in g.store.specs]
    assert all(n in names for n in CONV1), names
    data, labels = synthetic_mnist(4 * B, seed=7, device="cuda")
    data = ((data > 127).to(data.dtype) * 255).contiguous()
    assert set(data.unique().tolist()) == {0, 255}
    idx = torch.randperm(4 * B, device="cuda")[:B].to(torch.int64)
    scale = 1.0 / 255.0
    g.compute_gradients(ops.GatherRef(data, idx, scale, (28, 28, 1)), ops.LabelRef(labels, idx))
    xc = (data.index_select(0, idx).float() * scale).to(torch.bfloat16).float().cpu()
    assert set(xc.unique().tolist()) == {0.0, 1.0}
    c.compute_gradients(xc, labels.index_select(0, idx).cpu().to(torch.int32))
    torch.cuda.synchronize()
    for n in CONV1:
        assert float(c.store.gradient(n).abs().max()) > 0
        _close(base, f"border{B}", n, g.store.gradient(n).detach().cpu(), c.store.gradient(n))


def _update_paths(base, B, lr=0.5):
    """Two fused-update steps, then two steps whose update is the optimizer launch: after every step the
    conv2 forward fragments the next step will stage equal, bitwise, those the prep launch builds from the
    same master."""
    import torch

    from distriflow_amd import ops

    g, _ = base._nets(B)
    h, _ = base._nets(B)
    h.store.lenet_frag = None
    for s in (g.store, h.store):
        s.set_hyper(lr)
    assert g.store.lenet_frag is not None
    _, _, scratch = ops.lenet_tables(torch.device("cuda", torch.cuda.current_device()))
    lo, hi = FR_C2 * 1024, FR_DG * 1024
    seen = []
    for step in range(4):
        x, y = base._batch(B, seed=20 + step)
        if step < 2:
            g.compute_gradients_and_update(x.cuda().to(torch.bfloat16), y.cuda())
        else:
            g.compute_gradients(x.cuda(), y.cuda())
            g.store.sgd_step()
        torch.cuda.synchronize()
        mine = g.store.lenet_frag[0][lo:hi].clone()
        h.store.set_flat(g.store.master.clone())
        h.store.lenet_frag = None
        h.compute_gradients(x.cuda(), y.cuda())  # prep launch: fragments of g's master into the scratch buffer
        torch.cuda.synchronize()
        assert torch.equal(mine, scratch[lo:hi]), f"step {step}: conv2 forward fragments differ from the prep launch's"
        assert all(not torch.equal(mine, m) for m in seen), f"step {step}: the fragments did not move"
        seen.append(mine)


def _child(forced):
    sys.path.insert(0, HERE)
    import test_lenet_fused_gpu as base
    import torch

    out = {}

    def run(name, fn, *args):
        # the recipe's biases come from the global generator: seeded here, a case's weights do not depend
        # on the cases that ran before it in this process
        torch.manual_seed(0)
        try:
            fn(base, *args)
            out[name] = "ok"
        except AssertionError as e:
            out[name] = f"FAILED: {e}"

    for B in GRAD_CASES[forced]:
        run(f"grads{B}", _grads_vs_cpu, forced or 1, B)
    if forced in (0, 8):
        run("border8", _border, forced or 1, 8)
    if forced == 8:
        run("repeat13", _repeatable, 13)
        run("update24", _update_paths, 24)
    print("VERDICTS " + json.dumps(out))


# ------------------------------------------------------------------------------------------------ tests
@functools.lru_cache(maxsize=None)
def _verdicts(forced):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("DISTRIFLOW_DIAG", None)
    if forced:
        env["DISTRIFLOW_DIAG"] = f"lenet_ipw={forced}"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(forced)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child (lenet_ipw={forced}) failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    line = [l for l in r.stdout.splitlines() if l.startswith("VERDICTS ")]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][len("VERDICTS "):]), r.stdout


def _verdict(forced, name):
    verdicts, log = _verdicts(forced)
    print("\n".join(l for l in log.splitlines() if l.startswith(name)))  # the figures the child asserted on
    return verdicts[name]


@pytest.mark.parametrize("forced,B", [(f, B) for f, bs in GRAD_CASES.items() for B in bs])
def test_gradients_match_cpu_reference(forced, B):
    """Default policy at B = 5, 8 (one image per workgroup); forced 2 at B = 6 and 4 at B = 12 (the trimmed
    kernel with several images); forced 8 (the benchmarked TRIM = false kernel): B = 9, 11, 13, 15 a last
    workgroup of 1, 3, 5, 7 images, 24 exactly three workgroups, 72 nine (8 XCD-grouped plus a tail)."""
    assert _verdict(forced, f"grads{B}") == "ok"


def test_gradients_repeatable():
    """10 calls on one batch (forced lenet_ipw = 8, B = 13): gradients and stats bitwise equal every time."""
    assert _verdict(8, "repeat13") == "ok"


@pytest.mark.parametrize("forced", [8, 0])
def test_conv1_gradients_on_binary_images(forced):
    """0 / 255 images at B = 8 (one 8-image workgroup; eight 1-image workgroups): the zero codes of phase F."""
    assert _verdict(forced, "border8") == "ok"


def test_conv2_forward_fragments_follow_every_update_path():
    """Two fused-update steps, then two optimizer-launch steps (forced lenet_ipw = 8, B = 24)."""
    assert _verdict(8, "update24") == "ok"


if __name__ == "__main__":
    _child(int(sys.argv[1]))
