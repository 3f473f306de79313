"""Training a model whose output is an image (CPU): ``ops.image_loss_grad`` against the fp64 autograd oracle of
tests/loss_oracle.py on the [B, E] view of the output map, a conv autoencoder ``Net`` against torch autograd,
the errors an image output raises, the zoo's autoencoder through Keras JSON, the trainer's ``labels="input"``,
EngineModel and the launcher's ``--target input``."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import loss_oracle as lo
from distriflow_amd import ops
from distriflow_amd.models.keras import keras_config_from_layers, layers_from_keras, loss_from_keras
from distriflow_amd.models.layers import Conv2D, Conv2DTranspose, Dense, Flatten
from distriflow_amd.models.net import Net
from distriflow_amd.models.zoo import (MODELS, build_model, conv_autoencoder_mnist_layers,
                                       conv_autoencoder_mnist_topology)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = lo.KINDS[:6]  # the mean kinds
ACTS = ["linear", "sigmoid"]
FORMS = ["f32", "f32_idx", "u8_idx"]
SHAPES = [(1, 1), (3, 27), (2, 128), (5, 200)]


def _margin(kind, t, p):
    return (p - t).abs() if kind == "absoluteDifference" else (1.0 - (2.0 * t - 1.0) * p).abs()


class _Case:
    """fp32 outputs ``z`` [B][E], a target table (fp32, or uint8 with scale 1/255) read directly or through ``idx``
    with repeats, and the float64 rows ``t`` the call sees; z is moved off the kinks of absoluteDifference and
    hingeLoss (towards zero, which also leaves the flat ends of a sigmoid) and the margin is asserted."""

    def __init__(self, kind, act, form, B, E):
        g = torch.Generator().manual_seed(97 * B + E + 13 * KINDS.index(kind))
        unit = kind == "logLoss" and act == "linear"
        z = torch.rand(B, E, generator=g) * 0.9 + 0.05 if unit else (1.5 * torch.randn(B, E, generator=g)).clamp(-4, 4)
        N = B if form == "f32" else B + 3
        self.idx, self.scale = None, 1.0
        if form != "f32":
            self.idx = torch.randint(0, N, (B,), generator=g)
            if B > 1:
                self.idx[-1] = self.idx[0]
        if form == "u8_idx":
            self.table = torch.randint(0, 256, (N, E), generator=g, dtype=torch.uint8)
            self.scale = 1.0 / 255.0
            full = (self.table.float() * torch.tensor(self.scale, dtype=torch.float32)).double()
        else:
            self.table = torch.rand(N, E, generator=g)
            full = self.table.double()
        self.t = full[self.idx] if self.idx is not None else full
        if kind in ("absoluteDifference", "hingeLoss"):
            for _ in range(64):
                bad = _margin(kind, self.t, lo.act64(z.double(), act)) < 2 * lo.MARGIN
                if not bool(bad.any()):
                    break
                z = torch.where(bad, z + torch.where(z > 0, -2.0 ** -5, 2.0 ** -5), z)
            m = float(_margin(kind, self.t, lo.act64(z.double(), act)).min())
            assert m >= lo.MARGIN, f"an element is {m:.2e} from a kink of {kind}"
        self.z = z.float()


def _oracle(kind, act, c, gs):
    zz = c.z.double().clone().requires_grad_(True)
    L = lo.loss64(kind, c.t, lo.act64(zz, act))
    (g,) = torch.autograd.grad(L.sum(), zz)
    return gs * g, float(L.detach().sum())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", KINDS)
def test_image_loss_cpu_matches_oracle(kind, act, form):
    """The tolerances of loss_oracle.check, the gradient's on dz * E (per-element gradients of order 1)."""
    gs = 0.37
    for B, E in SHAPES:
        c = _Case(kind, act, form, B, E)
        dz = torch.full((B, E), 7.0)
        st = torch.zeros(2)
        ops.image_loss_grad(c.z, c.table, kind, act, dz, st, gs, idx=c.idx, target_scale=c.scale)
        ed, el = _oracle(kind, act, c, gs)
        torch.testing.assert_close(dz.double() * E, ed * E, rtol=1e-2, atol=1e-4,
                                   msg=lambda m: f"{kind}/{act}/{form} B={B} E={E} dz: {m}")
        assert abs(float(st[0]) - el) <= 1e-3 * abs(el) + 1e-3 and float(st[1]) == 0.0


def test_image_loss_cpu_shapes_and_optional_outputs():
    c = _Case("huberLoss", "sigmoid", "f32_idx", 3, 27)
    z4, tab4 = c.z.reshape(3, 3, 3, 3), c.table.reshape(-1, 3, 3, 3)
    dz, st = torch.zeros(3, 3, 3, 3), torch.zeros(2)
    ops.image_loss_grad(z4, tab4, "huberLoss", "sigmoid", dz, st, 1.0, idx=c.idx)
    ed, el = _oracle("huberLoss", "sigmoid", c, 1.0)
    torch.testing.assert_close(dz.reshape(3, 27).double() * 27, ed * 27, rtol=1e-2, atol=1e-4)
    st2 = torch.zeros(2)
    ops.image_loss_grad(z4, tab4, "huberLoss", "sigmoid", None, st2, 1.0, idx=c.idx)
    assert torch.equal(st, st2)
    ops.image_loss_grad(z4, tab4, "huberLoss", "sigmoid", dz, None, 1.0, idx=c.idx)
    # indices outside the table are clamped
    a, b = torch.zeros(3, 27), torch.zeros(3, 27)
    ops.image_loss_grad(c.z, c.table, "mse", "linear", a, None, 1.0, idx=torch.tensor([-4, 15, 2]))
    ops.image_loss_grad(c.z, c.table, "mse", "linear", b, None, 1.0, idx=torch.tensor([0, 5, 2]))
    assert torch.equal(a, b)
    # a fused-ReLU output: relu' of the output multiplies the gradient
    zr = torch.relu(c.z)
    ops.image_loss_grad(zr, c.table, "mse", "linear", a, None, 1.0, idx=c.idx)
    ops.image_loss_grad(zr, c.table, "mse", "linear", b, None, 1.0, idx=c.idx, out_relu=True)
    assert torch.equal(b, a * (zr > 0)) and bool((zr == 0).any())


def test_image_loss_errors():
    z, t = torch.zeros(4, 8), torch.zeros(4, 8)
    for loss, act in (("mse", "softmax"), ("softmaxCrossEntropy", "linear"), ("categorical_crossentropy", "linear")):
        with pytest.raises(NotImplementedError, match="per-pixel softmax"):
            ops.image_loss_grad(z, t, loss, act)
    with pytest.raises(KeyError):
        ops.image_loss_grad(z, t, "noSuchLoss", "linear")
    for bad in (torch.zeros(4, 7), torch.zeros(3, 8), torch.zeros(4, 8, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.image_loss_grad(z, bad, "mse", "linear")
    with pytest.raises(ValueError):
        ops.image_loss_grad(z, t, "mse", "linear", dz=torch.zeros(4, 9))
    ops.image_loss_grad(z, t[:1], "mse", "linear", idx=torch.zeros(4, dtype=torch.int64))  # one row through idx


def test_target_ref_keeps_its_dense_form_and_carries_a_scale():
    idx = torch.arange(5)
    r = ops.TargetRef(torch.zeros(9, 4), idx)
    assert r.shape == (5, 4) and r.scale == 1.0 and r.targets.shape == (9, 4) and r.idx is idx
    r = ops.TargetRef(torch.zeros(9, 6, 6, 1, dtype=torch.uint8), idx, 1.0 / 255.0)
    assert r.shape == (5, 6, 6, 1) and r.scale == 1.0 / 255.0


# ---------------------------------------------------------------------------------------------- Net
def _autoencoder(loss="logLoss", act="sigmoid", seed=3, relu_out=False):
    return Net([Conv2D(4, 3, 2, "same", "relu", name="enc"),
                Conv2DTranspose(4, 3, 2, "same", "relu", name="up"),
                Conv2D(1, 3, 1, "same", "relu" if relu_out else act, name="out")], (8, 8, 1), device="cpu", seed=seed,
               loss=loss)


def _conv_tf(h, w, b, strides=(1, 1)):
    """NHWC conv with the engine kernel OHWI and TensorFlow 'same' padding (tests/test_decoder_cpu.py)."""
    B, H, W, C = h.shape
    kh, kw = w.shape[1], w.shape[2]
    th = max((-(-H // strides[0]) - 1) * strides[0] + kh - H, 0)
    tw = max((-(-W // strides[1]) - 1) * strides[1] + kw - W, 0)
    hp = F.pad(h.permute(0, 3, 1, 2), (tw // 2, tw - tw // 2, th // 2, th - th // 2))
    return F.conv2d(hp, w.permute(0, 3, 1, 2), b, stride=strides).permute(0, 2, 3, 1)


def _deconv_same_s2(x, w, b):
    """Keras Conv2DTranspose 3x3, stride 2, 'same' with the engine kernel [Cin][KH][KW][F] (tests/test_decoder_cpu.py)."""
    B, H, W, C = x.shape
    full = F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, stride=2)
    full = F.pad(full, (0, max(2 * W - full.shape[3], 0), 0, max(2 * H - full.shape[2], 0)))
    return full[:, :, :2 * H, :2 * W].permute(0, 2, 3, 1) + b


def _torch_forward(P, x):
    h = F.relu(_conv_tf(x, P["enc/kernel"], P["enc/bias"], (2, 2)))
    h = F.relu(_deconv_same_s2(h, P["up/kernel"], P["up/bias"]))
    return _conv_tf(h, P["out/kernel"], P["out/bias"])


@pytest.mark.parametrize("loss,act,relu_out", [("logLoss", "sigmoid", False), ("meanSquaredError", "linear", False),
                                               ("huberLoss", "linear", True), ("sigmoidCrossEntropy", "sigmoid", False)])
def test_autoencoder_gradients_match_autograd(loss, act, relu_out):
    net = _autoencoder(loss, act, relu_out=relu_out)
    assert net.image_output and net.loss == loss and net.final_act == act and tuple(net.output_shape) == (8, 8, 1)
    assert net.exec_layers[-1].relu == relu_out and net.head_start is None and not net.lenet_fused
    g = torch.Generator().manual_seed(2)
    B = 5
    x = torch.rand(B, 8, 8, 1, generator=g)
    tgt = torch.rand(B, 8, 8, 1, generator=g)
    with torch.no_grad():  # biases start at zero: make them count
        for s in net.store.specs:
            if s.name.endswith("/bias"):
                net.store[s.name].copy_(torch.randn(s.shape, generator=g) * 0.1)
    P = {s.name: net.store[s.name].detach().clone().requires_grad_(True) for s in net.store.specs}
    z = _torch_forward(P, x)
    z = F.relu(z) if relu_out else z
    p = torch.sigmoid(z) if act == "sigmoid" else z
    want = lo.loss64(loss, tgt.reshape(B, -1).double(), p.reshape(B, -1).double()).mean()
    want.backward()
    st = net.compute_gradients(x, tgt)
    assert abs(float(st[0]) / B - float(want.detach())) < 1e-4 and float(st[1]) == 0.0
    for s in net.store.specs:
        torch.testing.assert_close(net.store.gradient(s.name), P[s.name].grad, rtol=1e-4, atol=1e-5,
                                   msg=lambda m, n=s.name: f"{n}: {m}")
    # the other target forms give the same gradients: flat [B, E], a float table and the uint8 input through idx
    g0 = net.store.grad.clone()
    net.compute_gradients(x, tgt.reshape(B, 64))
    assert torch.equal(net.store.grad, g0)
    idx = torch.tensor([4, 3, 2, 1, 0])
    net.compute_gradients(x, ops.TargetRef(tgt.flip(0).contiguous(), idx))
    assert torch.equal(net.store.grad, g0)
    # evaluate reports the same objective and no accuracy; predict applies the output activation
    lv, acc = net.evaluate(x, tgt)
    assert acc == 0.0 and abs(lv - float(want.detach())) < 1e-4
    torch.testing.assert_close(net.predict(x), p.detach().float(), rtol=1e-4, atol=1e-5)


def test_autoencoder_trains_on_its_own_uint8_input():
    """The eager "the input itself" target (an ops.GatherRef as x and as target) and a few SGD steps."""
    g = torch.Generator().manual_seed(8)
    data = (torch.rand(16, 8, 1, generator=g) * torch.rand(16, 1, 8, generator=g) * 255).to(torch.uint8).reshape(16, 64)
    net = _autoencoder()
    net.store.set_hyper(0.5)
    idx = torch.arange(16)
    ref = ops.GatherRef(data, idx, 1.0 / 255.0, (8, 8, 1))
    losses = []
    for _ in range(12):
        losses.append(float(net.compute_gradients(ref, ref)[0]) / 16)
        net.store.sgd_step()
    x = data.float().reshape(16, 8, 8, 1) / 255.0
    assert abs(net.evaluate(x, data.reshape(16, 8, 8, 1))[0] - net.evaluate(x, x)[0]) < 1e-6  # uint8 maps: u8 / 255
    assert losses[-1] < losses[0], losses
    dense = _autoencoder()
    first = float(dense.compute_gradients(x, x)[0]) / 16
    assert abs(first - losses[0]) < 1e-5


def test_image_output_errors_say_why():
    conv = lambda act="sigmoid": [Conv2D(2, 3, 1, "same", "relu", name="a"), Conv2D(1, 3, 1, "same", act, name="b")]  # noqa: E731
    with pytest.raises(ValueError, match="no default loss"):
        Net(conv(), (6, 6, 1), device="cpu")
    for cat in ("softmaxCrossEntropy", "categorical_crossentropy"):
        with pytest.raises(NotImplementedError, match="per-pixel softmax"):
            Net(conv(), (6, 6, 1), device="cpu", loss=cat)
    from distriflow_amd.models.layers import Activation
    with pytest.raises(NotImplementedError, match="per-pixel softmax"):
        Net(conv("linear") + [Activation("softmax", name="sm")], (6, 6, 1), device="cpu", loss="mse")
    with pytest.raises(NotImplementedError):
        conv("softmax")  # (a conv layer itself never takes a softmax)
    with pytest.raises(KeyError):
        Net(conv(), (6, 6, 1), device="cpu", loss="noSuchLoss")
    from distriflow_amd.models.layers import MaxPooling2D
    with pytest.raises(NotImplementedError, match="last executed layer"):
        Net(conv() + [MaxPooling2D(2, name="p")], (6, 6, 1), device="cpu", loss="mse")
    net = Net(conv(), (6, 6, 1), device="cpu", loss="mse")
    x = torch.rand(4, 6, 6, 1)
    for bad in (torch.rand(4, 5, 5, 1), torch.rand(4, 35), torch.rand(3, 6, 6, 1), torch.zeros(4, dtype=torch.int64),
                torch.zeros(4, 6, 6, 1, dtype=torch.int32), ops.TargetRef(torch.rand(9, 10), torch.arange(4)),
                ops.LabelRef(torch.zeros(9, dtype=torch.int32), torch.arange(4))):
        with pytest.raises(ValueError):
            net.compute_gradients(x, bad)
    # nets that end in Dense are untouched
    d = Net([Flatten(name="f"), Dense(3, "softmax", name="d")], (6, 6, 1), device="cpu")
    assert not d.image_output and d.loss is None and tuple(d.dlogits.shape if d._bound_B else (0,)) == (0,)


def test_parameter_server_and_fedavg_trainers_refuse_an_image_output():
    from distriflow_amd.parallel.async_ps import AsyncPSTrainer
    from distriflow_amd.parallel.fedavg import FedAvgTrainer
    from distriflow_amd.parallel.fedsgd_ps import FedSGDDeviceTrainer

    net = _autoencoder()
    for cls in (AsyncPSTrainer, FedSGDDeviceTrainer, FedAvgTrainer):
        with pytest.raises(NotImplementedError, match="output is an image"):
            cls(net)


def test_trainer_binds_image_targets():
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer

    g = torch.Generator().manual_seed(8)
    data = (torch.rand(32, 8, 1, generator=g) * torch.rand(32, 1, 8, generator=g) * 255).to(torch.uint8).reshape(32, 64)
    x = data.float().reshape(32, 8, 8, 1) / 255.0

    def after(labels, **kw):
        tr = DataParallelTrainer(_autoencoder(), lr=0.5, graph="none")
        tr.bind_dataset(data, labels, 8, scale=1.0 / 255.0, **kw)
        for s in range(3):
            tr.step_indices(torch.arange(8) + 8 * s)
        return tr.net.store.master.clone()

    w = after("input")
    assert torch.equal(w, after(data.reshape(32, 8, 8, 1), target_scale=1.0 / 255.0))  # a uint8 table of its own
    torch.testing.assert_close(w, after(x), rtol=1e-5, atol=1e-6)                       # a float table
    tr = DataParallelTrainer(_autoencoder(), lr=0.5, graph="none")
    first = float(tr.train_step(x[:8], x[:8])[0])  # dense map targets on an explicit batch
    for _ in range(10):
        last = float(tr.train_step(x[:8], x[:8])[0])
    assert last < first
    with pytest.raises(ValueError, match="target table"):
        tr.bind_dataset(data, torch.zeros(32, 10), 8)
    with pytest.raises(ValueError, match="target_scale"):
        tr.bind_dataset(data, data, 8)
    with pytest.raises(ValueError, match="uint8"):
        tr.bind_dataset(x, "input", 8)
    with pytest.raises(ValueError):
        tr.bind_dataset(data, "output", 8)
    with pytest.raises(ValueError):
        tr.bind_dataset(data, torch.zeros(32, dtype=torch.int32), 8)
    plain = DataParallelTrainer(Net([Flatten(name="f"), Dense(3, name="d")], (8, 8, 1), device="cpu"), graph="none")
    with pytest.raises(ValueError, match="image"):
        plain.bind_dataset(data, "input", 8)


def test_engine_model_trains_the_compile_loss_on_maps():
    from distriflow_amd.models.distri_model import EngineModel

    g = torch.Generator().manual_seed(8)
    x = (torch.rand(16, 8, 1, generator=g) * torch.rand(16, 1, 8, generator=g)).reshape(16, 8, 8, 1)
    m = EngineModel(_autoencoder(), {"loss": "logLoss", "learningRate": 0.5}, train_compile_loss=True)
    first = m.evaluate(x, x)
    for _ in range(10):
        m.update(m.fit(x, x.reshape(16, 64)))  # [B, E] targets as well
    last = m.evaluate(x, x)
    assert first[1] == 0.0 and last[1] == 0.0 and last[0] < first[0]
    assert m.output_shape == [8, 8, 1] and tuple(m.predict(x).shape) == (16, 8, 8, 1)
    with pytest.raises(ValueError, match="train_compile_loss"):
        EngineModel(_autoencoder(), {"loss": "logLoss"})
    with pytest.raises(ValueError):
        EngineModel(_autoencoder(), {"loss": "meanSquaredError"}, train_compile_loss=True)  # the Net trains logLoss
    z = EngineModel("conv_autoencoder_mnist", {"loss": "logLoss"}, device="cpu", train_compile_loss=True)
    assert z.fetch_initial().image_output and z.net.loss == "logLoss"


# ---------------------------------------------------------------------------------------------- zoo / Keras / launcher
def test_zoo_autoencoder_round_trips_through_keras_json():
    assert "conv_autoencoder_mnist" in MODELS
    layers, shape = conv_autoencoder_mnist_layers()
    topo = json.loads(json.dumps(conv_autoencoder_mnist_topology()))
    assert topo["model_config"] == json.loads(json.dumps(keras_config_from_layers(layers, shape,
                                                                                  name="conv_autoencoder_mnist")))
    assert topo["training_config"]["loss"] == "binary_crossentropy" and loss_from_keras(topo) == "logLoss"
    again, shape2 = layers_from_keras(topo)
    assert shape2 == shape == (28, 28, 1)
    assert [(type(l).__name__, l.name, l.config()) for l in again] == \
        [(type(l).__name__, l.name, l.config()) for l in layers]
    a = build_model("conv_autoencoder_mnist", device="cpu", seed=4, loss=loss_from_keras(topo))
    b = Net(again, shape2, device="cpu", seed=4, loss="logLoss", name="conv_autoencoder_mnist")
    assert a.summary() == b.summary() and torch.equal(a.store.master, b.store.master)
    assert a.image_output and a.final_act == "sigmoid" and tuple(a.output_shape) == (28, 28, 1)
    assert [l.out_shape for l in a.exec_layers] == [(14, 14, 16), (7, 7, 32), (14, 14, 16), (28, 28, 1)]
    assert a.num_params() == 160 + 4640 + 4624 + 145
    with pytest.raises(ValueError, match="no default loss"):
        build_model("conv_autoencoder_mnist", device="cpu")


def test_launcher_target_argument():
    from types import SimpleNamespace

    from distriflow_amd.launch import build_parser, sync_loss

    assert sync_loss(SimpleNamespace(model="conv_autoencoder_mnist", loss="model")) == "logLoss"
    assert sync_loss(SimpleNamespace(model="keras_cnn", loss="model")) == "categorical_crossentropy"
    p = build_parser()
    assert p.parse_args(["sync", "--model", "lenet5"]).target is None
    assert p.parse_args(["sync", "--model", "conv_autoencoder_mnist", "--target", "input"]).target == "input"


def _launch(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", "distriflow_amd.launch", "--nproc", "1", "sync", "--device", "cpu",
                           "--num-examples", "128", "--batch", "32", "--epochs", "1", *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=280)


@pytest.mark.timeout(300)
def test_launch_sync_trains_the_autoencoder_on_its_input():
    p = _launch("--model", "conv_autoencoder_mnist", "--loss", "model", "--target", "input", "--lr", "0.5")
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["steps"] == 4 and 0.0 < out["loss"] < 1.0, out  # (logLoss of an untrained sigmoid map: ln 2)
    # an image output without --target (or without a loss), and --target on a classifier, are refused with a reason
    p = _launch("--model", "conv_autoencoder_mnist", "--loss", "logLoss")
    assert p.returncode != 0 and "--target input" in p.stderr
    p = _launch("--model", "conv_autoencoder_mnist", "--target", "input")
    assert p.returncode != 0 and "no default loss" in p.stderr
    p = _launch("--model", "mlp_mnist", "--target", "input")
    assert p.returncode != 0 and "--target input" in p.stderr
