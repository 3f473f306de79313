"""Fused LeNet-5 train kernel, conv2 weight gradient (csrc/lenet_fused.hip, phase E): the 8 waves run as
2 K-halves x 4 column groups and the halves meet in one fp32 add through LDS.

What can go wrong is a row of the padded GEMM landing in both halves or in neither (the 13-step halves
of the 26-step loop, the odd tail step, the trimmed trip counts), a column tile summed from the wrong
slot of the exchange buffer, or the exchange racing with the reads of P1 around it.  The shapes are the
smallest that reach every trip-count case: every ``rows`` of a partly filled 8-image workgroup (a half
that holds only zero rows, a half that holds a partial image), full workgroups, the XCD-grouped order
plus a tail, and the trimmed kernel with 1, 2 and 4 images per workgroup.

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

# forced lenet_ipw (0: the default policy, one image per workgroup at these sizes) -> batch sizes.
# forced 8: B = 9, 11, 13, 15 leave rows = 1, 3, 5, 7 in the last workgroup; 24 is exactly 3 workgroups,
# 72 the 8 XCD-grouped workgroups plus a tail
GRAD_CASES = {8: (13, 24, 72, 9, 11, 15), 0: (5, 8), 2: (6,), 4: (12,)}
CONV2 = ("conv2d_2/kernel", "conv2d_2/bias")


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
    """The recipe of test_lenet_frag_stage_gpu: the conv2 tensors first, then every tensor and the stats
    under base._check."""
    import torch

    from distriflow_amd import ops

    assert ops.lenet_blocks(B) == -(-B // ipw), f"lenet_ipw is not {ipw} at B = {B}"
    g, c = base._nets(B)
    names = [s.name for s in g.store.specs]
    assert all(n in names for n in CONV2), names
    x, y = base._batch(B)
    sg = g.compute_gradients(x.cuda(), y.cuda()).clone()
    sc = c.compute_gradients(x, y)
    torch.cuda.synchronize()
    for n in CONV2:
        _close(base, f"grads{B}", n, g.store.gradient(n).detach().cpu(), c.store.gradient(n))
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
    assert float(g.store.gradient(CONV2[0]).abs().max()) > 0
    for k in range(1, n):
        s = g.compute_gradients(x, y).clone()
        assert torch.equal(s, s0), f"stats differ in run {k}"
        assert torch.equal(g.store.grad, g0), f"gradients differ in run {k}"


def _bias_is_sum_of_dc2(base, ipw, B):
    """0 / 255 uint8 images read through the index vector: the conv2 bias gradient is the ones column of
    phase E's GEMM, so it must equal the sum of dC2 over positions and images -- taken here from what the
    CPU engine hands its conv2 weight gradient (the pool gradient and the argmax / relu' codes of a fused
    conv + pool layer, or dC2 itself)."""
    import torch

    from distriflow_amd import ops
    from distriflow_amd.data.synthetic import synthetic_mnist

    assert ops.lenet_blocks(B) == -(-B // ipw), f"lenet_ipw is not {ipw} at B = {B}"
    g, c = base._nets(B)
    data, labels = synthetic_mnist(4 * B, seed=7, device="cuda")
    data = ((data > 127).to(data.dtype) * 255).contiguous()
    assert set(data.unique().tolist()) == {0, 255}
    idx = torch.randperm(4 * B, device="cuda")[:B].to(torch.int64)
    scale = 1.0 / 255.0
    g.compute_gradients(ops.GatherRef(data, idx, scale, (28, 28, 1)), ops.LabelRef(labels, idx))
    xc = (data.index_select(0, idx).float() * scale).to(torch.bfloat16).float().cpu()
    assert set(xc.unique().tolist()) == {0.0, 1.0}
    yc = labels.index_select(0, idx).cpu().to(torch.int32)

    layer = [l for l in c.exec_layers if l.name == "conv2d_2"]
    assert len(layer) == 1, [l.name for l in c.exec_layers]
    layer = layer[0]
    seen = {}
    inner = layer.backward_weights

    def spy(dy, *args, **kw):
        seen["dy"] = dy.detach().clone()
        return inner(dy, *args, **kw)

    layer.backward_weights = spy
    c.compute_gradients(xc, yc)
    torch.cuda.synchronize()
    dy = seen["dy"].double()
    if hasattr(layer, "code"):  # fused conv + pool: code bit 2 = the window's maximum is positive
        dy = dy.reshape(layer.code.shape) * ((layer.code & 4) > 0).double()
    ref = dy.reshape(-1, dy.shape[-1]).sum(0)
    assert ref.numel() == 16 and float(ref.abs().max()) > 0
    _close(base, f"bias{B}", "sum of dC2", g.store.gradient(CONV2[1]).detach().cpu(), ref)
    # and the CPU engine's own bias gradient is that sum
    _close(base, f"bias{B}", "cpu bias vs sum", c.store.gradient(CONV2[1]), ref)


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
        run("bias8", _bias_is_sum_of_dc2, forced or 1, 8)
    if forced == 8:
        run("repeat13", _repeatable, 13)
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
def test_conv2_gradient_matches_cpu_reference(forced, B):
    """forced 8 (the benchmarked TRIM = false kernel, 13 + 13 steps): B = 24 three full workgroups, 72 nine,
    B = 9, 11, 13, 15 a last workgroup of 1, 3, 5, 7 images; default policy at B = 5, 8 (one image per
    workgroup: 2 + 2 steps); forced 2 at B = 6 (4 + 3) and 4 at B = 12 (7 + 6)."""
    assert _verdict(forced, f"grads{B}") == "ok"


def test_conv2_gradient_repeatable():
    """10 calls on one batch (forced lenet_ipw = 8, B = 13): gradients and stats bitwise equal every time."""
    assert _verdict(8, "repeat13") == "ok"


@pytest.mark.parametrize("forced", [8, 0])
def test_conv2_bias_gradient_is_sum_of_dc2(forced):
    """0 / 255 images at B = 8 (one 8-image workgroup; eight 1-image workgroups): no half drops or
    double-counts the padding or zero rows."""
    assert _verdict(forced, "bias8") == "ok"


if __name__ == "__main__":
    _child(int(sys.argv[1]))
