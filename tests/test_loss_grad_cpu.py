"""Training any lossesMap loss (CPU): ``ops.loss_grad`` against the fp64 autograd oracle of tests/loss_oracle.py,
``Net(loss=...)`` parameter gradients against autograd, the normalisation rule that keeps the default path,
``EngineModel(train_compile_loss=True)``, the Keras loss mapping and the launcher's ``--loss``."""
import os
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

import loss_oracle as lo
from distriflow_amd import losses, ops
from distriflow_amd.models.distri_model import EngineModel
from distriflow_amd.models.keras import loss_from_keras
from distriflow_amd.models.layers import Dense
from distriflow_amd.models.net import Net
from distriflow_amd.models.zoo import lenet5_layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", lo.KINDS)
def test_fp64_restatements_match_losses_py(kind):
    g = torch.Generator().manual_seed(1)
    for C in (1, 7):
        t = torch.rand(9, C, generator=g)
        p = torch.rand(9, C, generator=g) * 0.9 + 0.05
        torch.testing.assert_close(lo.loss64(kind, t.double(), p.double()).float(), losses.get_loss(kind)(t, p),
                                   rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("form", lo.FORMS)
@pytest.mark.parametrize("act", lo.ACTS)
@pytest.mark.parametrize("kind", lo.KINDS)
def test_loss_grad_cpu_matches_oracle(kind, act, form):
    gs = 0.37
    for B, C in lo.SHAPES:
        if act == "softmax" and C == 1:
            continue  # p == 1 and every gradient is 0: test_softmax_single_class_is_zero
        c = lo.Case(kind, act, form, B, C)
        dl = torch.full((B, C), 7.0)
        st = torch.zeros(2)
        ops.loss_grad(c.z, c.table, kind, act, dl, st, gs, idx=c.idx)
        lo.check(kind, act, c, dl, st, gs, what=f"{kind}/{act}/{form} B={B} C={C}")


@pytest.mark.parametrize("kind", lo.KINDS)
def test_softmax_single_class_is_zero(kind):
    z = torch.tensor([[0.3], [-2.0], [4.0]])
    for target in (torch.zeros(3, dtype=torch.int32), torch.rand(3, 1)):
        dl = torch.full((3, 1), 7.0)
        ops.loss_grad(z, target, kind, "softmax", dl, None, 1.0)
        assert torch.equal(dl, torch.zeros(3, 1))


def test_loss_grad_cpu_label_clamp_and_optional_outputs():
    c = lo.Case("huberLoss", "sigmoid", "labels", 9, 5, out_of_range_labels=True)
    assert int(c.table.max()) > 4 and int(c.table.min()) < 0
    dl, st = torch.zeros(9, 5), torch.zeros(2)
    ops.loss_grad(c.z, c.table, "huberLoss", "sigmoid", dl, st, 1.0)
    lo.check("huberLoss", "sigmoid", c, dl, st, 1.0)
    ops.loss_grad(c.z, c.table, "huberLoss", "sigmoid", dl, None, 1.0)
    st2 = torch.zeros(2)
    ops.loss_grad(c.z, c.table, "huberLoss", "sigmoid", None, st2, 1.0)
    assert torch.equal(st, st2)
    with pytest.raises(KeyError):
        ops.loss_grad(c.z, c.table, "noSuchLoss", "sigmoid", dl, st, 1.0)


def _mlp(act, loss, device="cpu", seed=5):
    return Net([Dense(16, "tanh", name="l0"), Dense(4, act, name="l1")], (6,), device=device, seed=seed, loss=loss)


@pytest.mark.parametrize("loss,act", [("meanSquaredError", "linear"), ("huberLoss", "sigmoid"),
                                      ("absoluteDifference", "softmax")])
def test_net_general_loss_gradients_match_autograd(loss, act):
    net = _mlp(act, loss)
    assert net.loss == loss and net.final_act == act
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 6, generator=g)
    t = torch.rand(8, 4, generator=g)
    st = net.compute_gradients(x, t)
    P = {s.name: net.store[s.name].detach().clone().requires_grad_(True) for s in net.store.specs}
    z = F.linear(torch.tanh(F.linear(x, P["l0/kernel"], P["l0/bias"])), P["l1/kernel"], P["l1/bias"])
    p = torch.softmax(z, 1) if act == "softmax" else (torch.sigmoid(z) if act == "sigmoid" else z)
    L = losses.get_loss(loss)(t, p).mean()
    L.backward()
    assert abs(float(st[0]) / 8 - L.item()) < 1e-4
    assert float(st[1]) == float((z.argmax(1) == t.argmax(1)).sum())
    for s in net.store.specs:
        torch.testing.assert_close(net.store.gradient(s.name), P[s.name].grad, rtol=1e-4, atol=1e-5)
    # the same step through a TargetRef, and evaluate() reports [mean loss, accuracy] of that loss
    g0 = net.store.grad.clone()
    tab = torch.cat([torch.rand(3, 4), t])
    net.compute_gradients(x, ops.TargetRef(tab, torch.arange(3, 11)))
    assert torch.equal(net.store.grad, g0)
    ev = net.evaluate(x, t)
    assert abs(ev[0] - L.item()) < 1e-4


def test_loss_normalisation_keeps_the_default_path():
    layers, shape = lenet5_layers()
    a = Net(layers, shape, device="cpu", seed=2)
    layers, shape = lenet5_layers()
    b = Net(layers, shape, device="cpu", seed=2, loss="softmaxCrossEntropy")
    assert a.loss is None and b.loss is None
    x = torch.rand(4, 28, 28, 1)
    y = torch.randint(0, 10, (4,), dtype=torch.int32)
    a.compute_gradients(x, y)
    b.compute_gradients(x, y)
    assert torch.equal(a.store.grad, b.store.grad)
    for loss in ("softmaxCrossEntropy", "categorical_crossentropy", "categoricalCrossentropy"):
        for act in ("linear", "softmax"):
            assert _mlp(act, loss).loss is None
        assert _mlp("sigmoid", loss).loss == loss
    assert _mlp("sigmoid", "sigmoidCrossEntropy").loss is None
    assert _mlp("linear", "sigmoidCrossEntropy").loss == "sigmoidCrossEntropy"
    assert _mlp("softmax", "meanSquaredError").loss == "meanSquaredError"
    with pytest.raises(KeyError):
        _mlp("linear", "noSuchLoss")
    with pytest.raises(ValueError):  # dense targets need the general loss path
        _mlp("linear", None).compute_gradients(torch.randn(2, 6), torch.rand(2, 4))


def test_engine_model_trains_the_compile_loss():
    cfg = {"loss": "meanSquaredError", "learningRate": 0.1, "metrics": ["accuracy"]}
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no "metrics only" warning
        m = EngineModel(_mlp("linear", "meanSquaredError"), cfg, train_compile_loss=True)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(32, 6, generator=g)
    Y = torch.randn(32, 4, generator=g)
    xx, yy = m._prep(X, Y)
    assert yy.dtype == torch.float32 and torch.equal(yy, Y)  # a 2-D float y is used as it stands
    _, yi = m._prep(X, torch.randint(0, 4, (32,)))
    assert yi.dtype == torch.int32 and yi.dim() == 1
    l0 = m.evaluate(X, Y)[0]
    assert abs(l0 - float(((m.predict(X) - Y) ** 2).mean())) < 1e-5
    for _ in range(50):
        m.update(m.fit(X, Y))
    l1 = m.evaluate(X, Y)[0]
    print(f"meanSquaredError before {l0:.4f}, after 50 SGD steps {l1:.4f}")
    assert l1 < l0
    m.update_flat(m.fit_flat(X, Y))
    m.accumulate(X, Y)
    # a Net that does not carry the compile loss is refused; a zoo name is built with it
    with pytest.raises(ValueError):
        EngineModel(_mlp("linear", None), cfg, train_compile_loss=True)
    z = EngineModel("mlp_mnist", cfg, device="cpu", train_compile_loss=True)
    assert z.fetch_initial().loss == "meanSquaredError"
    # without the flag nothing changes: the one-hot convention, class indices
    plain = EngineModel(_mlp("linear", None), {"loss": "softmaxCrossEntropy"})
    assert plain._prep(X, Y)[1].dtype == torch.int32


def _topo(loss):
    return {"training_config": {"loss": loss}}


def test_loss_from_keras():
    want = {"mean_squared_error": "meanSquaredError", "mse": "meanSquaredError",
            "mean_absolute_error": "absoluteDifference", "mae": "absoluteDifference", "hinge": "hingeLoss",
            "huber": "huberLoss", "huber_loss": "huberLoss", "binary_crossentropy": "logLoss",
            "categorical_crossentropy": "categorical_crossentropy"}
    for k, v in want.items():
        assert loss_from_keras(_topo(k)) == v
        assert v in ops.METRIC_KINDS and v in losses.LOSSES
    assert loss_from_keras({}) is None and loss_from_keras(None) is None
    assert loss_from_keras({"training_config": {}}) is None
    for bad in ("kullback_leibler_divergence", {"out": "mse"}, ["mse", "mae"]):
        with pytest.raises(NotImplementedError):
            loss_from_keras(_topo(bad))


def test_ps_trainers_refuse_a_general_loss_net():
    from distriflow_amd.parallel.async_ps import AsyncPSTrainer
    from distriflow_amd.parallel.fedavg import FedAvgTrainer
    from distriflow_amd.parallel.fedsgd_ps import FedSGDDeviceTrainer

    net = _mlp("linear", "meanSquaredError")
    for cls in (AsyncPSTrainer, FedSGDDeviceTrainer, FedAvgTrainer):
        with pytest.raises(NotImplementedError):
            cls(net)


def test_trainer_takes_dense_targets_on_the_general_path_only():
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer

    g = torch.Generator().manual_seed(11)
    data, tab = torch.randn(32, 6, generator=g), torch.rand(32, 4, generator=g)
    tr = DataParallelTrainer(_mlp("linear", "meanSquaredError"), lr=0.1, graph="none")
    first = float(tr.train_step(data[:8], tab[:8])[0])
    for _ in range(30):
        last = float(tr.train_step(data[:8], tab[:8])[0])
    assert last < first
    tr.bind_dataset(data, tab, 8)
    tr.step_indices(torch.arange(8))
    with pytest.raises(NotImplementedError):
        tr.add_preprocess_callback(lambda b: b)
    plain = DataParallelTrainer(_mlp("linear", None), lr=0.1, graph="none")
    with pytest.raises(ValueError):
        plain.bind_dataset(data, tab, 8)


def test_launcher_loss_argument():
    from types import SimpleNamespace

    from distriflow_amd.launch import sync_loss

    assert sync_loss(SimpleNamespace(model="lenet5", loss=None)) is None
    assert sync_loss(SimpleNamespace(model="lenet5", loss="huberLoss")) == "huberLoss"
    # the bundled Keras CNN was compiled with categorical_crossentropy, which its softmax output normalises away
    assert sync_loss(SimpleNamespace(model="keras_cnn", loss="model")) == "categorical_crossentropy"
    for bad in (SimpleNamespace(model="lenet5", loss="model"), SimpleNamespace(model="lenet5", loss="noSuchLoss")):
        with pytest.raises(SystemExit):
            sync_loss(bad)


@pytest.mark.timeout(300)
def test_launch_sync_with_a_loss():
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", "distriflow_amd.launch", "--nproc", "1", "sync", "--model", "mlp_mnist",
                        "--device", "cpu", "--loss", "meanSquaredError", "--num-examples", "256", "--batch", "64",
                        "--epochs", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
