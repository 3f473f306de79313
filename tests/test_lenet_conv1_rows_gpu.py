"""Fused LeNet-5 train kernel, conv1 forward with two kernel rows per MFMA step (csrc/lenet_fused.hip phase A):
rows (image, y), four x tiles of 8 columns, the horizontal pool partner in the neighbouring lane, nine banded B
fragments placed by ``lenet_conv1_frag_pos`` (csrc/lenet_frag.h), and phase 0 without the first shifted copy.

What can go wrong is a pool window assembled from the wrong lane or row (the x-tile seams at x = 8, 16, 24, the
4-row group seams, an M-tile that holds the end of one image and the start of the next), the wrapped piece of
the last x tile or the clamped sixth K slot meeting a weight, the trimmed kernel's trip count not covering its
live images, a phase-C reader meeting bytes of the fragment image that now stay where the shifted copy used to
be written, or the three users of the position rule (prep launch, fused update, optimizer launch) disagreeing.
The shapes are the smallest that reach every case.

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
GRAD_CASES = {0: (5, 8), 2: (6,), 4: (12,), 8: (9, 13, 15, 24, 72)}
# one pixel of 255 per image: the corners, the x-tile seams and the 4-row group seams
ONE_HOT = ((0, 0), (0, 27), (27, 0), (27, 27), (3, 7), (4, 8), (15, 23), (16, 24))
FR_C1_USED, FR_C2 = 9, 15  # conv1 fragments in use / allocated (csrc/lenet_frag.h), 1 KB = 512 bf16 each


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


def _compare(base, tag, g, c, sg, sc):
    for s in g.store.specs:
        _close(base, tag, s.name, g.store.gradient(s.name).detach().cpu(), c.store.gradient(s.name))
    print(f"{tag}: stats gpu {sg.tolist()} cpu {sc.tolist()}")
    base._check(g, {s.name: c.store.gradient(s.name) for s in c.store.specs}, sc, sg)


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
    _compare(base, f"grads{B}", g, c, sg, sc)


def _one_hot(base, ipw, B=8):
    """uint8 images, zero except one pixel of 255, read through the index vector."""
    import torch

    from distriflow_amd import ops

    assert ops.lenet_blocks(B) == -(-B // ipw), f"lenet_ipw is not {ipw} at B = {B}"
    assert B == len(ONE_HOT)
    g, c = base._nets(B)
    data = torch.zeros((2 * B, 28, 28, 1), dtype=torch.uint8)
    for k, (y, x) in enumerate(ONE_HOT):
        data[2 * k + 1, y, x, 0] = 255  # the even rows of the pool stay zero images and are not drawn
    labels = (torch.arange(2 * B) % 10).to(torch.int32)
    data, labels = data.cuda(), labels.cuda()
    idx = (2 * torch.randperm(B, device="cuda") + 1).to(torch.int64)
    scale = 1.0 / 255.0
    sg = g.compute_gradients(ops.GatherRef(data, idx, scale, (28, 28, 1)), ops.LabelRef(labels, idx)).clone()
    xc = (data.index_select(0, idx).float() * scale).to(torch.bfloat16).float().cpu()
    assert float(xc.sum()) == B and sorted(xc.flatten(1).argmax(1).tolist()) == sorted(y * 28 + x for y, x in ONE_HOT)
    sc = c.compute_gradients(xc, labels.index_select(0, idx).cpu().to(torch.int32))
    torch.cuda.synchronize()
    assert float(c.store.gradient("conv2d_1/kernel").abs().max()) > 0
    _compare(base, f"onehot{B}", g, c, sg, sc)


def _repeatable(base, B, n=10):
    import torch

    g, _ = base._nets(B)
    x, y = base._batch(B, seed=1)
    x, y = x.cuda(), y.cuda()
    s0 = g.compute_gradients(x, y).clone()
    g0 = g.store.grad.clone()
    assert torch.isfinite(g0).all()
    assert float(g.store.gradient("conv2d_1/kernel").abs().max()) > 0
    for k in range(1, n):
        s = g.compute_gradients(x, y).clone()
        assert torch.equal(s, s0), f"stats differ in run {k}"
        assert torch.equal(g.store.grad, g0), f"gradients differ in run {k}"


def _fragments(base, B, lr=0.5):
    """After the prep launch, after each of two fused-update steps and after each of two optimizer-launch
    steps: conv1 fragments 0 .. 8 equal, bit for bit, the band built on the host from the master through
    ``lenet_conv1_frag_map``; fragments 9 .. 14 are zero."""
    import torch

    from distriflow_amd import native, ops

    fmap = native.require().lenet_conv1_frag_map().to(torch.int64).cuda()
    g, _ = base._nets(B)
    h, _ = base._nets(B)
    assert g.store.lenet_frag is not None
    o1 = int(g.store.lenet_frag[1])
    h.store.lenet_frag = None
    for s in (g.store, h.store):
        s.set_hyper(lr)
    _, _, scratch = ops.lenet_tables(torch.device("cuda", torch.cuda.current_device()))

    def band(master):
        z = torch.zeros(FR_C2 * 512, dtype=torch.bfloat16, device="cuda")
        z[fmap.reshape(-1)] = master[o1:o1 + 150].to(torch.bfloat16).repeat_interleave(8)
        return z.view(torch.int16)

    def conv1(buf):
        return buf[:FR_C2 * 1024].clone().view(torch.int16)

    def check(tag, got, master):
        want = band(master)
        assert int((want != 0).sum()) > 1000, "the band is (nearly) empty"
        assert not got[FR_C1_USED * 512:].any(), f"{tag}: fragments 9 .. 14 are not zero"
        bad = int((got != want).sum())
        print(f"fragments{B}: {tag}: {bad} of {want.numel()} elements differ")
        assert bad == 0, f"{tag}: {bad} conv1 fragment elements differ from the host's band"

    seen = []
    for step in range(-1, 4):
        x, y = base._batch(B, seed=20 + step)
        if step == -1:  # g's first step builds its own buffer with the prep launch
            g.compute_gradients(x.cuda(), y.cuda())
        elif step < 2:
            g.compute_gradients_and_update(x.cuda().to(torch.bfloat16), y.cuda())
        else:
            g.compute_gradients(x.cuda(), y.cuda())
            g.store.sgd_step()
        torch.cuda.synchronize()
        mine = conv1(g.store.lenet_frag[0])
        check(["prep launch", "fused update 1", "fused update 2", "optimizer launch 1", "optimizer launch 2"][step + 1],
              mine, g.store.master)
        h.store.set_flat(g.store.master.clone())
        h.store.lenet_frag = None
        h.compute_gradients(x.cuda(), y.cuda())  # prep launch: fragments of g's master into the scratch buffer
        torch.cuda.synchronize()
        check(f"prep launch of step {step}'s master", conv1(scratch), g.store.master)
        if step >= 0:
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
        run("onehot8", _one_hot, forced or 1)
    if forced == 8:
        run("repeat13", _repeatable, 13)
        run("fragments24", _fragments, 24)
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
    """Default policy at B = 5, 8 (the trimmed kernel, one image per workgroup: 2 M-tiles for 28 rows); forced 2
    at B = 6 (an M-tile across the image boundary); forced 4 at B = 12 (exactly 7 M-tiles); forced 8 (the
    benchmarked TRIM = false kernel): B = 9, 13, 15 a last workgroup of 1, 5, 7 images, 24 exactly three
    workgroups, 72 nine (8 XCD-grouped plus a tail)."""
    assert _verdict(forced, f"grads{B}") == "ok"


@pytest.mark.parametrize("forced", [8, 0])
def test_gradients_on_one_hot_images(forced):
    """B = 8, one pixel of 255 per image (one 8-image workgroup; eight 1-image workgroups)."""
    assert _verdict(forced, "onehot8") == "ok"


def test_gradients_repeatable():
    """10 calls on one batch (forced lenet_ipw = 8, B = 13): gradients and stats bitwise equal every time."""
    assert _verdict(8, "repeat13") == "ok"


def test_conv1_fragments_follow_the_map_on_every_update_path():
    """Prep launch, two fused-update steps, two optimizer-launch steps (forced lenet_ipw = 8, B = 24)."""
    assert _verdict(8, "fragments24") == "ok"


if __name__ == "__main__":
    _child(int(sys.argv[1]))
