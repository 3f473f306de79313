"""Training a lossesMap loss through the engine on the GPU (``Net(loss=...)``, the general loss path): gradients
against the CPU engine, the fused plans that the normalisation rule keeps, a dataset-bound step with a dense target
table captured into a hipGraph, and convergence of a regression onto a linear teacher."""
import pytest
import torch

from distriflow_amd.models.layers import Dense
from distriflow_amd.models.net import Net
from distriflow_amd.models.zoo import lenet5_layers

pytestmark = pytest.mark.gpu


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def _mlp(act, loss, device, seed=4, dtype=None):
    return Net([Dense(32, "relu", name="l0"), Dense(8, act, name="l1")], (24,), device=device, seed=seed, loss=loss,
               compute_dtype=dtype)


def _pair(make):
    """The same model on the GPU and on the CPU engine with bf16 buffers and bf16-representable weights (the
    recipe of test_model_gradients_match_cpu)."""
    g, c = make("cuda", None), make("cpu", torch.bfloat16)
    c.store.master.copy_(c.store.master.to(torch.bfloat16).float())
    g.store.set_flat(c.store.master.cuda())
    assert torch.equal(g.store.master.cpu(), c.store.master)
    return g, c


def _compare(g, c, x, y):
    sg = g.compute_gradients(x.cuda(), y.cuda())
    sc = c.compute_gradients(x, y)
    torch.cuda.synchronize()
    print("loss sum gpu", float(sg[0]), "cpu", float(sc[0]))
    assert abs(float(sg[0]) - float(sc[0])) <= 0.02 * abs(float(sc[0])) + 0.05
    coss = {s.name: _cos(g.store.gradient(s.name).cpu(), c.store.gradient(s.name)) for s in g.store.specs
            if c.store.gradient(s.name).norm() >= 1e-6}
    print({k: round(v, 4) for k, v in coss.items()})
    assert coss and all(v > 0.99 for v in coss.values()), coss


@pytest.mark.parametrize("loss,act", [("meanSquaredError", "linear"), ("huberLoss", "sigmoid"), ("logLoss", "sigmoid")])
def test_general_loss_gradients_match_cpu(loss, act):
    g, c = _pair(lambda dev, dt: _mlp(act, loss, dev, dtype=dt))
    assert g.loss == loss and g.head_start is None and not g.lenet_fused
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(64, 24, generator=gen).to(torch.bfloat16).float()
    t = torch.rand(64, 8, generator=gen)
    _compare(g, c, x, t)


def test_lenet5_plans_follow_the_loss():
    def make(loss):
        return lambda dev, dt: Net(*lenet5_layers(), device=dev, seed=3, loss=loss, compute_dtype=dt)

    gen = torch.Generator().manual_seed(1)
    x = torch.rand(128, 28, 28, 1, generator=gen).to(torch.bfloat16).float()
    y = torch.randint(0, 10, (128,), generator=gen, dtype=torch.int32)
    # a cross-entropy on the softmax output is what the fused step trains: the plan and the numbers are kept
    a = make(None)("cuda", None)
    b = make("softmaxCrossEntropy")("cuda", None)
    assert a.lenet_fused and b.lenet_fused and b.loss is None
    sa = a.compute_gradients(x.cuda(), y.cuda()).clone()
    sb = b.compute_gradients(x.cuda(), y.cuda()).clone()
    torch.cuda.synchronize()
    assert torch.equal(a.store.grad, b.store.grad) and torch.equal(sa, sb)
    # any other loss: the per-layer kernels and the loss kernel, still the CPU engine's gradients
    g, c = _pair(make("meanSquaredError"))
    assert g.loss == "meanSquaredError" and not g.lenet_fused and g.head_start is None and not g.khead
    _compare(g, c, x, y)


def test_dense_target_table_step_captures_and_matches_eager():
    """bind_dataset with a uint8 data table and a float target table: the loss kernel reads the targets through the
    step's index vector, the step captures into a hipGraph, and three replays leave the master that three eager
    steps from the same state leave (same kernels in the same order; dlogits is a pure function of its row)."""
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer

    gen = torch.Generator().manual_seed(5)
    data = torch.randint(0, 256, (512, 24), generator=gen, dtype=torch.uint8).cuda()
    table = torch.rand(512, 8, generator=gen).cuda()
    idxs = [torch.randint(0, 512, (64,), generator=gen).cuda() for _ in range(3)]
    outs = []
    for graph in ("full", "none"):
        net = _mlp("linear", "meanSquaredError", "cuda")
        tr = DataParallelTrainer(net, lr=0.05, graph=graph)
        tr.bind_dataset(data, table, 64, scale=1 / 255)
        for idx in idxs:
            tr.step_indices(idx)
        torch.cuda.synchronize()
        assert tr.graph_mode == graph and (tr._graph is not None) == (graph == "full"), tr.capture_error
        outs.append(net.store.master.clone())
    assert not torch.equal(outs[0], _mlp("linear", "meanSquaredError", "cuda").store.master)
    assert torch.equal(outs[0], outs[1])


def _regress(device, dtype=None, lr=0.1, steps=200):
    """SGD on the 24 -> 32 -> 8 MLP, meanSquaredError on a linear output, onto a fixed random linear teacher;
    -> (initial, final) mean loss over the 256 examples."""
    net = _mlp("linear", "meanSquaredError", device, dtype=dtype)
    gen = torch.Generator().manual_seed(9)
    X = torch.randn(256, 24, generator=gen).to(torch.bfloat16).float()
    Y = X @ (torch.randn(24, 8, generator=gen) / 24 ** 0.5)
    Xd, Yd = X.to(device), Y.to(device)
    net.store.set_hyper(lr)
    first = net.evaluate(X, Y)[0]
    for s in range(steps):
        b = (s % 4) * 64
        net.compute_gradients(Xd[b:b + 64], Yd[b:b + 64])
        net.store.sgd_step()
    return first, net.evaluate(X, Y)[0]


def test_regression_converges():
    """lr 0.1 and 200 steps were chosen on the CPU engine, which ends at 0.062 x its initial loss (bound 0.1); the
    GPU engine (bf16 compute) from the same weights and data must end within 0.2 x its own initial loss."""
    c0, c1 = _regress("cpu")
    g0, g1 = _regress("cuda")
    print(f"meanSquaredError cpu {c0:.4f} -> {c1:.4f} ({c1 / c0:.4f} x), gpu {g0:.4f} -> {g1:.4f} ({g1 / g0:.4f} x)")
    assert c1 <= 0.1 * c0
    assert g1 <= 0.2 * g0


def test_engine_model_trains_the_compile_loss_with_both_target_forms():
    from distriflow_amd.models.distri_model import EngineModel

    cfg = {"loss": "meanSquaredError", "learningRate": 0.1, "metrics": ["accuracy"]}
    m = EngineModel(_mlp("linear", "meanSquaredError", "cuda"), cfg, train_compile_loss=True)
    gen = torch.Generator().manual_seed(7)
    X = torch.randn(64, 24, generator=gen).to(torch.bfloat16).float()
    Y = torch.randn(64, 8, generator=gen)
    yi = Y.argmax(1)
    dense0, acc = m.evaluate(X, Y)
    want = float(((m.predict(X).float().cpu() - Y) ** 2).mean())
    assert abs(dense0 - want) <= 1e-3 * want + 1e-3
    onehot0, acc_i = m.evaluate(X, yi)  # class indices: the same loss against the one-hot rows
    p = m.predict(X).float().cpu()
    want = float(((p - torch.nn.functional.one_hot(yi, 8).float()) ** 2).mean())
    assert abs(onehot0 - want) <= 1e-3 * want + 1e-3 and acc_i == acc == float((p.argmax(1) == yi).float().mean())
    for _ in range(20):
        m.update(m.fit(X, Y))
    m.update_flat(m.fit_flat(X, Y))
    m.accumulate(X, yi)
    assert m.evaluate(X, Y)[0] < dense0


def test_float_table_without_a_net_loss_is_refused():
    from distriflow_amd.parallel.async_ps import AsyncPSTrainer
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer
    from distriflow_amd.parallel.fedavg import FedAvgTrainer
    from distriflow_amd.parallel.fedsgd_ps import FedSGDDeviceTrainer

    data = torch.zeros(128, 24, dtype=torch.uint8, device="cuda")
    table = torch.rand(128, 8, device="cuda")
    with pytest.raises(ValueError):
        DataParallelTrainer(_mlp("linear", None, "cuda"), graph="none").bind_dataset(data, table, 64)
    net = _mlp("linear", "meanSquaredError", "cuda")
    for cls in (AsyncPSTrainer, FedSGDDeviceTrainer, FedAvgTrainer):
        with pytest.raises(NotImplementedError):
            cls(net)
