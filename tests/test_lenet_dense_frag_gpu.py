"""Fused LeNet-5 step: the dense weights are read as lane-linear MFMA fragments (csrc/lenet_frag.h) kept
next to the conv fragments, written by every path that leaves the fragments "fresh": the prep launch, the
reduce launch's fused update and the optimizer launch.

What can go wrong: a writer that misses the dense ranges (the train kernel then multiplies with stale
weights), a wrong position (forward against transposed, tile / k-step order), padding that is not zero,
and the train kernel's tile / k-step addressing at partial tiles.  The fragment ranges are un-permuted
through the position maps and compared bitwise with the bf16 compute copies (``wbf``), which the same
launches write and the per-layer kernels read; the gradients are compared with the CPU fp32 engine as
tests/test_lenet_frag_stage_gpu.py does, one fresh child process per forced ``lenet_ipw``.

The transposed dense activations and output gradients the train kernel hands to the reduce launch use the
same operand form (blocks of 16 rows x 32 batch columns); they are read back through their position map."""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CONV_ELEMS = 37 * 64 * 8
# forced lenet_ipw (0: the default policy, one image per workgroup at these sizes) -> batch sizes:
# B = 5, 6 at 1 and 2 images per workgroup; 12 at 4; 13 and 24 at 8 with a partial / full last group; 33 two
# k-steps of the reduce with the second almost empty; 72 more than one 32-column block
GRAD_CASES = {0: (5, 6), 2: (5, 6), 4: (12,), 8: (13, 24, 33, 72)}
REPEAT_B = 33
# transposed activation buffers: one image per workgroup (element stores) and eight (vector stores, a
# partial last group)
ACT_FORCED, ACT_CASES = (0, 8), (13, 33)


# ------------------------------------------------------------------------------------- fragments == wbf
def _assert_dense_fragments_match_wbf(net, what):
    import torch

    from distriflow_amd import native

    m = native.require()
    st = net.store
    torch.cuda.synchronize()
    frag = st.lenet_frag[0].view(torch.bfloat16).cpu()
    live = torch.zeros(frag.numel(), dtype=torch.bool)
    for l, d in enumerate(net.exec_layers[2:5]):
        fwd, tr = m.lenet_dense_frag_map(l)
        N, K = fwd.shape
        name = f"{d.name}/kernel"
        w = st.weight(name).cpu()
        wt = st.weight_t(name).cpu()
        assert torch.equal(w[:N, :K], st[name].view(N, K).to(torch.bfloat16).cpu()), f"{what}: wbf of {name}"
        assert torch.equal(frag[fwd], w[:N, :K]), f"{what}: forward fragments of {name}"
        assert torch.equal(frag[tr], wt[:K, :N]), f"{what}: transposed fragments of {name}"
        live[fwd.reshape(-1)] = True
        live[tr.reshape(-1)] = True
    pad = frag[CONV_ELEMS:][~live[CONV_ELEMS:]]
    assert pad.numel() == frag.numel() - CONV_ELEMS - 2 * (120 * 400 + 84 * 120 + 10 * 84)
    assert bool((pad.view(torch.int16) == 0).all()), f"{what}: padding of the dense fragments is not zero"


def _net(B):
    sys.path.insert(0, HERE)
    import test_lenet_fused_gpu as base

    g, _ = base._nets(B)
    x, y = base._batch(B, seed=2)
    return g, x.cuda(), y.cuda()


def test_dense_fragments_after_prep_launch():
    """The buffer filled with ones, state stale: the prep launch must rebuild every element, padding
    included (the conv fragments are covered by tests/test_lenet_fused_gpu.py)."""
    g, x, y = _net(24)
    _assert_dense_fragments_match_wbf(g, "construction (optimizer launch, no update)")
    g.store.lenet_frag[0].fill_(0x3F)
    g.store.lenet_state = "stale"
    g.compute_gradients(x, y)
    _assert_dense_fragments_match_wbf(g, "prep launch")


def test_dense_fragments_after_fused_update_steps():
    import torch

    g, x, y = _net(24)
    g.store.set_hyper(0.5)
    w0 = g.store.wbf.clone()
    for step in range(2):
        g.compute_gradients_and_update(x.to(torch.bfloat16), y)
        assert g.store.lenet_state == "fresh"
        _assert_dense_fragments_match_wbf(g, f"fused update step {step}")
    assert float((g.store.wbf != w0).float().mean()) > 0.1, "the update did not move the weights"


def test_dense_fragments_after_optimizer_launch_steps():
    g, x, y = _net(24)
    g.store.set_hyper(0.5, momentum=0.9)
    w0 = g.store.wbf.clone()
    for step in range(2):
        g.compute_gradients(x, y)
        g.store.sgd_step()
        assert g.store.lenet_state == "fresh"
        _assert_dense_fragments_match_wbf(g, f"optimizer launch step {step}")
    assert float((g.store.wbf != w0).float().mean()) > 0.1, "the update did not move the weights"


def test_dense_fragments_after_adam_step():
    """Adam leaves the fragments stale; the next step's prep launch rebuilds them from the new master."""
    g, x, y = _net(24)
    g.store.set_hyper(0.01)
    g.store.set_optimizer("adam")
    w0 = g.store.wbf.clone()
    g.compute_gradients(x, y)
    g.store.step()
    assert g.store.lenet_state == "stale"
    g.compute_gradients(x, y)
    _assert_dense_fragments_match_wbf(g, "Adam step + prep launch")
    assert float((g.store.wbf != w0).float().mean()) > 0.1, "the update did not move the weights"


def test_dense_fragments_after_set_flat():
    import torch

    g, x, y = _net(24)
    torch.manual_seed(5)
    g.store.set_flat((torch.randn(g.store.total) * 0.1).cuda())
    assert g.store.lenet_state == "fresh"
    _assert_dense_fragments_match_wbf(g, "set_flat")


# ------------------------------------------------------------------- transposed activations (block layout)
def _acts_vs_cpu(base, B):
    """After one step: H0^T, H1^T, H2^T, dZ1^T, dZ2^T, dZ3^T read back through the position map against the
    CPU engine's dense inputs / output gradients of the same step (same bf16 weights and inputs), with the
    gradient tolerances of tests/test_lenet_fused_gpu.py (cos > 0.999, max error < 3 % of the largest
    value); everything outside the live [rows][B] region -- the padding rows and batch columns the reduce
    launch reads -- must be zero."""
    import torch

    from distriflow_amd import native
    from distriflow_amd.models.layers import Dense

    m = native.require()
    g, c = base._nets(B)
    x, y = base._batch(B)
    g.compute_gradients(x.cuda(), y.cuda())
    c.compute_gradients(x, y)
    torch.cuda.synchronize()
    d1, d2, d3 = [l for l in c._all_leaf_layers() if isinstance(l, Dense)]
    ref = {"h0T": d1.x.reshape(B, -1), "h1T": d2.x.reshape(B, -1), "h2T": d3.x.reshape(B, -1),
           "dz1T": d2.dx.reshape(B, -1), "dz2T": d3.dx.reshape(B, -1), "dz3T": c.dlogits.reshape(B, -1)}
    got = {"h0T": g.head_xT, "h1T": g.head_hT[0], "h2T": g.head_hT[1],
           "dz1T": g.head_dzT[0], "dz2T": g.head_dzT[1], "dz3T": g.head_dzT[2]}
    for name, buf in got.items():
        want = ref[name].detach().double().t()  # [N][B]
        N = want.shape[0]
        rows, ldt = buf.shape
        assert rows == (N + 15) // 16 * 16 and ldt % 32 == 0 and ldt >= (B + 31) // 32 * 32
        full = buf.cpu().reshape(-1)[m.lenet_act_map(rows, ldt)].double()  # [rows][ldt], un-permuted
        live = full[:N, :B]
        cos = float((live.flatten() @ want.flatten()) / (live.norm() * want.norm() + 1e-30))
        rel = float((live - want).abs().max() / (want.abs().max() + 1e-12))
        print(f"acts{B}: {name:<5} cos {cos:.6f} max-rel {rel:.5f}")
        assert cos > 0.999 and rel < 0.03, f"{name}: cos {cos:.5f} max-rel {rel:.4f}"
        outside = full.clone()
        outside[:N, :B] = 0
        assert int((outside != 0).sum()) == 0, f"{name}: non-zero padding"


# ------------------------------------------------------------------------------------------------ child
def _child(forced):
    sys.path.insert(0, HERE)
    import test_lenet_frag_stage_gpu as stage
    import test_lenet_fused_gpu as base
    import torch

    out = {}

    def run(name, fn, *args):
        torch.manual_seed(0)  # the recipe's biases come from the global generator
        try:
            fn(base, *args)
            out[name] = "ok"
        except AssertionError as e:
            out[name] = f"FAILED: {e}"

    for B in GRAD_CASES[forced]:
        run(f"grads{B}", stage._grads_vs_cpu, forced or 1, B)
    if forced == 8:
        run(f"repeat{REPEAT_B}", stage._repeatable, REPEAT_B)
    if forced in ACT_FORCED:
        for B in ACT_CASES:
            run(f"acts{B}", _acts_vs_cpu, B)
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
def test_dense_fragment_step_matches_cpu_reference(forced, B):
    """Gradients and stats against the CPU fp32 engine, tolerances of tests/test_lenet_fused_gpu.py."""
    assert _verdict(forced, f"grads{B}") == "ok"


def test_dense_fragment_step_repeatable():
    """10 calls on one batch (forced lenet_ipw = 8, B = 33): gradients and stats bitwise equal every time."""
    assert _verdict(8, f"repeat{REPEAT_B}") == "ok"


@pytest.mark.parametrize("forced,B", [(f, B) for f in ACT_FORCED for B in ACT_CASES])
def test_transposed_activations_block_layout(forced, B):
    assert _verdict(forced, f"acts{B}") == "ok"


if __name__ == "__main__":
    _child(int(sys.argv[1]))
