"""Fused LeNet-5 train kernel: the conv1 / conv2 weight fragments are loaded once per workgroup and
handed to the waves through LDS scratch that later phases overwrite (csrc/lenet_fused.hip, phase 0).

What can go wrong is a wave reading a scratch range after it was overwritten (or zero-filled), or the
staged image missing the conv weights of the previous update.  The shapes are the smallest that reach
every path: full workgroups, a partly filled last workgroup, the XCD-grouped workgroup order plus a tail,
and the trimmed (TRIM) kernel with 1, 2 and 4 images per workgroup.

``lenet_ipw`` reads DISTRIFLOW_DIAG once per process, so every forced setting runs in one fresh child
process (this file as a script) that reports one verdict per case; the tests below read the verdicts."""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# forced lenet_ipw (0: the default policy, one image per workgroup at these sizes) -> batch sizes
GRAD_CASES = {8: (24, 13, 72), 0: (5, 8), 2: (6,), 4: (12,)}


# ------------------------------------------------------------------------------------------------ child
def _check(base, tag, gnet, cnet, ref_stats, stats):
    """base._check with its tolerances, after printing every figure it asserts on."""
    for spec in gnet.store.specs:
        gg = gnet.store.gradient(spec.name).detach().cpu().double().flatten()
        gc = cnet.store.gradient(spec.name).double().flatten()
        cos = float((gg @ gc) / (gg.norm() * gc.norm() + 1e-30))
        rel = float((gg - gc).abs().max() / (gc.abs().max() + 1e-12))
        print(f"{tag}: {spec.name:<18} cos {cos:.6f} max-rel {rel:.5f}")
    print(f"{tag}: stats gpu {stats.tolist()} cpu {ref_stats.tolist()}")
    base._check(gnet, {s.name: cnet.store.gradient(s.name) for s in cnet.store.specs}, ref_stats, stats)


def _grads_vs_cpu(base, ipw, B):
    """As test_fused_lenet_matches_cpu_reference: same weights recipe, same tolerances."""
    import torch

    from distriflow_amd import ops

    assert ops.lenet_blocks(B) == -(-B // ipw), f"lenet_ipw is not {ipw} at B = {B}"
    g, c = base._nets(B)
    x, y = base._batch(B)
    sg = g.compute_gradients(x.cuda(), y.cuda()).clone()
    sc = c.compute_gradients(x, y)
    torch.cuda.synchronize()
    _check(base, f"grads{B}", g, c, sc, sg)


def _repeatable(base, B, n=10):
    import torch

    g, _ = base._nets(B)
    x, y = base._batch(B, seed=1)
    x, y = x.cuda(), y.cuda()
    s0 = g.compute_gradients(x, y).clone()
    g0 = g.store.grad.clone()
    assert torch.isfinite(g0).all()
    for k in range(1, n):
        s = g.compute_gradients(x, y).clone()
        assert torch.equal(s, s0), f"stats differ in run {k}"
        assert torch.equal(g.store.grad, g0), f"gradients differ in run {k}"


def _two_update_steps(base, B, lr=0.5):
    """Two fused-update steps: the reduce launch of step 1 scatters the new conv weights into the
    fragments that step 2 stages.  Step 2 against two CPU steps (existing tolerances) and, bitwise,
    against a net whose fragments the prep launch rebuilds from the master before every step."""
    import torch

    g, c = base._nets(B)
    h, _ = base._nets(B)
    h.store.set_flat(g.store.master.clone())
    h.store.lenet_frag = None
    for s in (g.store, h.store, c.store):
        s.set_hyper(lr)
    convs = [s.name for s in g.store.specs if len(s.shape) == 4]
    assert len(convs) == 2
    w0 = {n: g.store[n].to(torch.bfloat16).clone() for n in convs}
    for step in range(2):
        x, y = base._batch(B, seed=10 + step)
        sg = g.compute_gradients_and_update(x.cuda().to(torch.bfloat16), y.cuda()).clone()
        sh = h.compute_gradients(x.cuda(), y.cuda()).clone()
        sc = c.compute_gradients(x, y)
        torch.cuda.synchronize()
        _check(base, f"update{B} step {step}", g, c, sc, sg)
        assert torch.equal(sg, sh), f"step {step}: stats differ from the prep-built fragments' step"
        assert torch.equal(g.store.grad, h.store.grad), f"step {step}: stale or damaged fragment image"
        h.store.sgd_step()
        c.store.sgd_step()
        # the GPU multiplies with the bf16 copy of its updated kernels (biases stay fp32), the CPU engine
        # with its master as it is: the recipe's rounding (base._nets) again, on the CPU's own new kernels
        for s in c.store.specs:
            if not s.name.endswith("/bias"):
                c.store[s.name].copy_(c.store[s.name].to(torch.bfloat16).float())
        torch.cuda.synchronize()
        assert torch.equal(g.store.master, h.store.master)
        # the update moved most bf16 conv weights, so a stale image would have been a different step
        for n in convs:
            moved = float((g.store[n].to(torch.bfloat16) != w0[n]).float().mean())
            assert moved > 0.5, f"step {step}: only {moved:.2f} of {n} changed"


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
    if forced == 8:
        run("repeat24", _repeatable, 24)
        run("update24", _two_update_steps, 24)
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
def test_staged_fragments_match_cpu_reference(forced, B):
    """forced 8 (the benchmarked TRIM = false kernel): B = 24 three full workgroups, 13 a 5-image last
    workgroup, 72 the 8 XCD-grouped workgroups plus a tail; default policy at B = 5, 8 (one image per
    workgroup); forced 2 at B = 6 and 4 at B = 12 (TRIM with several images)."""
    assert _verdict(forced, f"grads{B}") == "ok"


def test_staged_fragments_repeatable():
    """10 calls on one batch (forced lenet_ipw = 8, B = 24): gradients and stats bitwise equal every time."""
    assert _verdict(8, "repeat24") == "ok"


def test_staged_fragments_follow_fused_update():
    """Two consecutive fused-update steps (forced lenet_ipw = 8, B = 24)."""
    assert _verdict(8, "update24") == "ok"


if __name__ == "__main__":
    _child(int(sys.argv[1]))
