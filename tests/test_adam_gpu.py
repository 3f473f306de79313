"""Adam / AdamW on the GPU: the fused adam_multi launch (csrc/adam.hip) against a float64 oracle, its bf16
compute copies, the device-resident step state under graph replay, the LeNet-5 fragment rebuild and
two data-parallel ranks."""
import os
import subprocess
import sys

import pytest
import torch

from adam_util import BETAS, EPS, LR, STEPS, fixed_grads, rel_err, torch_adam
from mp_util import free_port

pytestmark = pytest.mark.gpu

MODELS = ["mlp_mnist", "lenet5", "keras_cnn"]
DEV = "cuda:0"


def _net(name, seed=0):
    from distriflow_amd.models.zoo import build_model

    return build_model(name, device=DEV, seed=seed)


def _pads(store):
    """(bf_off, pad_) of every descriptor (ParamDesc, csrc/kernels.h) from the host copy of the table."""
    d = store._descs_host.view(-1, 6)
    return [(int(r[1]), int(r[5]) >> 32) for r in d]


def _layout_classes(store):
    out = set()
    for bf_off, pad in _pads(store):
        if bf_off < 0:
            out.add("vector")
            continue
        if (pad >> 28) & 1:
            out.add("tile")
        if (pad & 0xffff) and not (pad >> 30) & 1:
            out.add("row-segment")
        if (pad >> 30) & 1:
            out.add("row-pair")
        if (pad >> 29) & 1:
            out.add("dgrad-pair")
        if pad == 0:
            out.add("plain")
    return out


def test_models_cover_every_copy_layout():
    """The three models together hit every layout class ParamStore._build_compute_copies can emit, and a
    parameter whose numel is no multiple of 4 or of 1024."""
    seen, numels = set(), []
    for name in MODELS:
        st = _net(name).store
        seen |= _layout_classes(st)
        numels += [s.numel for s in st.specs]
    assert seen == {"vector", "tile", "row-segment", "row-pair", "dgrad-pair", "plain"}
    assert any(n % 4 and n % 1024 for n in numels) and any(n > 1024 and n % 1024 for n in numels)


# worst case of the moments' own arithmetic, relative to the operands' magnitude: per step three roundings
# (beta * m, (1 - beta) * g [* g], the sum) and the fp32 representation of beta and 1 - beta, each at most
# 2^-24 -> 5 * 2^-24 per step, summed over the steps
MOMENT_BOUND = STEPS * 5 * 2.0 ** -24


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("opt,wd", [("adam", 0.0), ("adam", 1e-2), ("adamw", 1e-2)])
def test_kernel_against_float64_oracle(name, opt, wd):
    """5 adam_multi launches on fixed random gradients (with g == 0 and |g| ~ 1e-20 elements, grad_scale
    0.25) against torch.optim.Adam / AdamW in float64 on the same fp32 inputs.  The weights may be off by
    4x the fp32 floor = the error (adam_util.rel_err) of fp32 CPU torch.optim against that oracle; the
    moments by MOMENT_BOUND."""
    st = _net(name).store
    grads = fixed_grads(st)
    ref = torch_adam(st.master, grads, opt, wd, 0.25, torch.float64)
    f32 = torch_adam(st.master, grads, opt, wd, 0.25, torch.float32)
    floor = rel_err(f32["w"][-1], ref["w"])
    st.set_optimizer(opt, *BETAS, EPS)
    st.set_hyper(LR, 0.0, wd, grad_scale=0.25)
    for g in grads:
        st.grad.copy_(g.to(DEV))
        st.step()
    torch.cuda.synchronize()
    err = {k: rel_err(t, ref[k]) for k, t in (("w", st.master), ("m", st.adam_m), ("v", st.adam_v))}
    print(f"adam {name} {opt} wd={wd}: fp32 floor {floor:.3e}, kernel w {err['w']:.3e} m {err['m']:.3e} "
          f"v {err['v']:.3e} (torch fp32 m {rel_err(f32['m'][-1], ref['m']):.3e} "
          f"v {rel_err(f32['v'][-1], ref['v']):.3e})")
    assert st.adam_t == STEPS
    assert floor > 0 and err["w"] <= 4 * floor
    assert err["m"] <= MOMENT_BOUND and err["v"] <= MOMENT_BOUND
    if not (opt == "adam" and wd):  # (L2 weight decay gives a g == 0 element the gradient wd * w)
        zero_g = grads[0] == 0
        assert torch.equal(st.adam_m.cpu()[zero_g], torch.zeros(int(zero_g.sum())))


@pytest.mark.parametrize("name", MODELS)
def test_compute_copies_match_refresh(name):
    """After Adam updates the bf16 compute copies are bit for bit what refresh_compute() writes from the
    new master."""
    st = _net(name).store
    st.set_optimizer("adam", *BETAS, EPS)
    st.set_hyper(0.05, 0.0, 1e-2)  # large steps: most bf16 values change
    before = st.wbf.clone()
    for g in fixed_grads(st, steps=2):
        st.grad.copy_(g.to(DEV))
        st.step()
    got = st.wbf.clone()
    assert not torch.equal(got, before)
    st.wbf.zero_()
    st.refresh_compute()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), st.wbf.view(torch.int16))


def _mlp_trainer(graph, rows, data, labels):
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer

    net = _net("mlp_mnist")
    tr = DataParallelTrainer(net, lr=LR, optimizer="adam", betas=BETAS, eps=EPS, graph=graph)
    tr.bind_dataset(data, labels, 32, scale=1.0 / 255.0)
    tr.bind_index_stream(rows.to(DEV))
    return net, tr


def _state(net):
    torch.cuda.synchronize()
    st = net.store
    return {"w": st.master.clone(), "m": st.adam_m.clone(), "v": st.adam_v.clone(), "state": st.adam_state.clone()}


def test_graph_replay_advances_the_step_state():
    """6 single-step replays == one 6-step prepare_run graph == 6 eager steps, bit for bit in master, m and
    v, each ending at step count 6 (not 9: the capture warm-up is undone, step state included); set_lr
    between replays takes effect without a re-capture."""
    from distriflow_amd.data.synthetic import synthetic_mnist

    data, labels = synthetic_mnist(1024, seed=3, device=DEV)
    g = torch.Generator().manual_seed(5)
    rows = torch.stack([torch.randperm(1024, generator=g)[:32] for _ in range(8)])
    na, ta = _mlp_trainer("full", rows, data, labels)
    for _ in range(6):
        ta.step()
    nb, tb = _mlp_trainer("full", rows, data, labels)
    tb.prepare_run(6)
    assert tb._multi_u == 6
    tb.run(6)
    nc, tc = _mlp_trainer("none", rows, data, labels)
    for _ in range(6):
        tc.step()
    a, b, c = _state(na), _state(nb), _state(nc)
    assert ta.graph_mode == "full" and tb.graph_mode == "full" and ta._graph is not None
    for n in (na, nb, nc):
        assert n.store.adam_t == 6
    for k in a:
        assert torch.equal(a[k], b[k]), f"multi-step graph: {k}"
        assert torch.equal(a[k], c[k]), f"eager: {k}"
    # a new learning rate reaches the captured launch through device memory
    graph = ta._graph
    ta.set_lr(10 * LR)
    tc.set_lr(10 * LR)
    ta.step()
    tc.step()
    assert ta._graph is graph
    a2, c2 = _state(na), _state(nc)
    for k in a2:
        assert torch.equal(a2[k], c2[k]), f"after set_lr: {k}"
    # Adam's first steps move a weight by about lr: the 7th step's largest move is ~10x the 6th's lr
    assert float((a2["w"] - a["w"]).abs().max()) > 3 * LR
    assert na.store.adam_t == 7


def test_lenet_fragments_rebuild_under_adam():
    """Under Adam the fused LeNet-5 step is off and the conv-weight fragments are rebuilt by the next train
    launch: step 2's gradient equals, bit for bit, the gradient a fresh Net computes from the master after
    step 1 on the same batch."""
    from distriflow_amd.data.synthetic import synthetic_mnist
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer

    data, labels = synthetic_mnist(1024, seed=3, device=DEV)
    g = torch.Generator().manual_seed(5)
    rows = torch.stack([torch.randperm(1024, generator=g)[:64] for _ in range(2)]).to(DEV)
    net = _net("lenet5")
    tr = DataParallelTrainer(net, lr=LR, optimizer="adam", graph="none")
    tr.bind_dataset(data, labels, 64, scale=1.0 / 255.0)
    tr.bind_index_stream(rows)
    assert not tr._fused_step_ok() and tr.step_launches == "compute+adam"
    tr.step()
    torch.cuda.synchronize()
    w1 = net.store.master.clone()
    if net.store.lenet_frag is not None:
        assert net.store.lenet_state == "stale"
    tr.step()
    torch.cuda.synchronize()
    g2 = net.store.grad.clone()
    assert net.store.adam_t == 2 and not torch.equal(net.store.master, w1)

    fresh = _net("lenet5", seed=9)
    tf = DataParallelTrainer(fresh, lr=0.05, graph="none")
    tf.bind_dataset(data, labels, 64, scale=1.0 / 255.0)
    tf.bind_index_stream(rows[1:])
    fresh.store.set_flat(w1)
    tf._gather()
    fresh.compute_gradients(tf.xb, tf.yb)
    torch.cuda.synchronize()
    assert torch.equal(fresh.store.grad, g2)
    # back under SGD the same net takes the fused step again (its first train launch rebuilds the fragments)
    ts = DataParallelTrainer(net, lr=0.05, graph="none")
    ts.bind_dataset(data, labels, 64, scale=1.0 / 255.0)
    ts.bind_index_stream(rows)
    assert net.store.optimizer == "sgd" and ts._fused_step_ok()
    w2 = net.store.master.clone()
    ts.step()
    torch.cuda.synchronize()
    assert net.store.adam_t == 2 and not torch.equal(net.store.master, w2)


def test_adam_rejects_the_parameter_server_gate():
    st = _net("mlp_mnist").store
    st.set_optimizer("adam")
    st.set_hyper(LR)
    with pytest.raises(ValueError, match="SGD only"):
        st.step(ps_gate=8, ps_mirror=8)
    from distriflow_amd import native

    with pytest.raises(RuntimeError, match="SGD only"):
        native.require().adam_multi(st._descs, st._ndesc, st._sgd_blocks, st.master, st.grad, st.adam_m, st.adam_v,
                                    st.wbf, st.adam_hyper, st.adam_state, st._adam_tickets, gate=8, mirror=8)
    assert st.adam_t == 0


@pytest.mark.timeout(300)
def test_two_ranks_apply_the_same_adam_update(tmp_path):
    """2 processes (a GPU each when the node has two, else sharing cuda:0), mlp_mnist, 3 Adam steps: both
    ranks end with bit-identical master, m and v.  Each rank runs under its own time limit, and nothing
    further is started after a failure."""
    world, port = 2, free_port()
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adam_dp_worker.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, worker, str(r), str(world), str(port),
                               str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate()[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, f"rank exited {p.returncode}:\n{o[-2000:]}"
    r = [torch.load(os.path.join(tmp_path, f"r{i}.pt"), weights_only=True) for i in range(world)]
    for x in r:
        assert x["t"] == 3 and x["launches"] == "compute+allreduce+adam"
        assert not torch.equal(x["w"], x["w0"])
    for k in ("w", "m", "v"):
        assert torch.equal(r[0][k], r[1][k]), k
