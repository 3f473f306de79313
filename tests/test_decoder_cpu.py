"""Conv2DTranspose and UpSampling2D of Keras / tf.js LayersModels (autoencoders, U-Net-style skip networks): the
CPU fp32 engine against an independent torch formulation (F.conv_transpose2d builds the full output, which is
then padded or cropped as TensorFlow does; F.interpolate / repeat_interleave), the Keras topology and tf.js
checkpoint round trips, whole-model gradients against autograd, and a build-level guard on csrc/upsample.hip.
The GPU kernels are checked against the same fp32 reference in tests/test_decoder_gpu.py."""
import json
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from distriflow_amd import ops
from distriflow_amd.models.graph import GraphLayer
from distriflow_amd.models.keras import keras_config_from_layers, layers_from_keras
from distriflow_amd.models.layers import Conv2D, Conv2DTranspose, UpSampling2D
from distriflow_amd.models.net import Net
from distriflow_amd.models.params import ParamStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (B, H, W, Cin, F, kernel, strides, padding)
GEOMETRIES = [
    (2, 5, 5, 3, 4, (3, 3), (2, 2), "same"),    # asymmetric crop (total 1: bottom / right)
    (2, 4, 6, 3, 5, (3, 3), (2, 2), "valid"),
    (2, 4, 4, 4, 2, (4, 4), (2, 2), "same"),    # symmetric crop
    (1, 3, 3, 2, 3, (2, 2), (3, 3), "same"),    # kernel smaller than the stride: bias-only pixels
    (1, 3, 2, 2, 3, (2, 2), (3, 3), "valid"),
    (2, 1, 1, 3, 4, (3, 3), (1, 1), "same"),    # 1x1 input
    (2, 5, 4, 2, 3, (5, 3), (1, 2), "same"),    # non-square kernel, per-axis strides
    (2, 3, 4, 2, 2, (2, 4), (3, 1), "valid"),   # ... with one axis' kernel smaller than its stride
    (2, 4, 5, 3, 2, (3, 3), (1, 1), "valid"),   # 'valid', stride 1
    (1, 6, 6, 2, 1, (5, 5), (3, 3), "same"),    # one filter, wide kernel
]
GEOM_IDS = [f"{c[0]}x{c[1]}x{c[2]}x{c[3]}f{c[4]}_k{c[5][0]}{c[5][1]}_s{c[6][0]}{c[6][1]}_{c[7]}" for c in GEOMETRIES]


def deconv_torch(x, w, b, kernel, strides, padding):
    """Keras Conv2DTranspose on NHWC ``x`` with the engine kernel [Cin][KH][KW][F]: the full transposed conv
    ((H - 1) * s + K rows), zero-extended at the bottom / right where the kernel is smaller than the stride,
    then ('same') cropped to H * s rows from TensorFlow's top / left pad of the matching conv."""
    (kh, kw), (sh, sw) = kernel, strides
    B, H, W, C = x.shape
    full = F.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, stride=(sh, sw))
    if padding == "same":
        OH, OW = H * sh, W * sw
        pt, pl = max(kh - sh, 0) // 2, max(kw - sw, 0) // 2
    else:
        OH, OW = H * sh + max(kh - sh, 0), W * sw + max(kw - sw, 0)
        pt = pl = 0
    full = F.pad(full, (0, max(pl + OW - full.shape[3], 0), 0, max(pt + OH - full.shape[2], 0)))
    y = full[:, :, pt:pt + OH, pl:pl + OW].permute(0, 2, 3, 1)
    return y + b if b is not None else y


def _standalone(layer, in_shape, B, seed):
    """A layer outside a Net: built, bound to its own CPU parameter store, buffers allocated."""
    layer.build(in_shape)
    store = ParamStore(layer.specs(), "cpu", False, seed=seed)
    layer.store = store
    layer.alloc(B, torch.device("cpu"), torch.float32, SimpleNamespace(wgrad=None))
    return store


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", GEOMETRIES, ids=GEOM_IDS)
def test_conv2d_transpose_layer_matches_conv_transpose2d(case, relu):
    B, H, W, Cin, Fo, k, s, pad = case
    l = Conv2DTranspose(Fo, k, s, pad, "relu" if relu else "linear", True, name="d")
    l.in_relu = relu  # the relu' mask of the input gradient, on the same cases
    store = _standalone(l, (H, W, Cin), B, seed=GEOMETRIES.index(case))
    assert store.spec("d/kernel").shape == (Cin, k[0], k[1], Fo)
    assert store.spec("d/kernel").mat == (Cin, k[0] * k[1], Fo) and store.spec("d/kernel").needs_dgrad
    assert store.spec("d/kernel").fan == (k[0] * k[1] * Fo, k[0] * k[1] * Cin)
    g = torch.Generator().manual_seed(50 + GEOMETRIES.index(case))
    with torch.no_grad():
        store["d/bias"].copy_(torch.randn(Fo, generator=g))
    x = torch.randn(B, H, W, Cin, generator=g)
    xr = x.clone().requires_grad_(True)
    w = store["d/kernel"].detach().clone().requires_grad_(True)
    b = store["d/bias"].detach().clone().requires_grad_(True)
    want = deconv_torch(torch.relu(xr) if relu else xr, w, b, k, s, pad)
    want = torch.relu(want) if relu else want
    xin = torch.relu(x) if relu else x
    y = l.forward(xin, True)
    assert tuple(y.shape) == tuple(want.shape) == (B,) + l.out_shape
    torch.testing.assert_close(y, want.detach())
    dy = torch.randn(want.shape, generator=g)
    if relu:
        dy = dy * (y > 0)  # the consumer of a fused-ReLU output hands down an already masked gradient
    want.backward(dy)
    dx = l.backward(dy)
    torch.testing.assert_close(dx, xr.grad)
    torch.testing.assert_close(store.gradient("d/kernel"), w.grad)
    torch.testing.assert_close(store.gradient("d/bias"), b.grad)


def test_conv2d_transpose_bias_only_pixels_and_no_bias():
    """A 2x2 kernel at stride 3: every third row and column of the output is reached by no tap."""
    l = Conv2DTranspose(3, (2, 2), (3, 3), "same", use_bias=True, name="d")
    store = _standalone(l, (3, 3, 2), 1, seed=1)
    with torch.no_grad():
        store["d/bias"].copy_(torch.tensor([1.0, -2.0, 3.0]))
    y = l.forward(torch.ones(1, 3, 3, 2), True)
    assert y.shape == (1, 9, 9, 3)
    assert torch.equal(y[0, 2::3, :, :], store["d/bias"].expand(3, 9, 3))
    assert torch.equal(y[0, :, 2::3, :], store["d/bias"].expand(9, 3, 3))
    nb = Conv2DTranspose(3, (2, 2), (3, 3), "same", use_bias=False, name="n")
    st2 = _standalone(nb, (3, 3, 2), 1, seed=1)
    assert st2.names() == ["n/kernel"]
    assert not nb.need_dx or nb.forward(torch.ones(1, 3, 3, 2), True)[0, 2::3].abs().max() == 0


def test_conv2d_transpose_is_not_a_conv2d():
    assert not issubclass(Conv2DTranspose, Conv2D)
    assert Conv2DTranspose(4).can_fuse_relu() and Conv2DTranspose.has_params and not UpSampling2D.has_params


UP_SIZES = [(3, 5, 7, 8, (2, 2)), (2, 4, 4, 3, (3, 2)), (1, 1, 1, 16, (2, 2)), (2, 6, 5, 4, (4, 1))]


@pytest.mark.parametrize("in_relu", [False, True])
@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("case", UP_SIZES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}_s{c[4][0]}{c[4][1]}" for c in UP_SIZES])
def test_upsampling2d_layer_matches_torch(case, interp, in_relu):
    B, H, W, C, size = case
    l = UpSampling2D(size, interp, name="u")
    l.in_relu = in_relu
    _standalone(l, (H, W, C), B, seed=0)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, C, generator=g)
    xr = x.clone().requires_grad_(True)
    xin = torch.relu(xr) if in_relu else xr
    if interp == "nearest":
        want = xin.repeat_interleave(size[0], 1).repeat_interleave(size[1], 2)
    else:
        want = F.interpolate(xin.permute(0, 3, 1, 2), scale_factor=tuple(float(v) for v in size), mode="bilinear",
                             align_corners=False).permute(0, 2, 3, 1)
    y = l.forward(xin.detach(), True)
    assert tuple(y.shape) == (B, H * size[0], W * size[1], C)
    if interp == "nearest":
        assert torch.equal(y, want.detach())
    else:
        torch.testing.assert_close(y, want.detach())
    dy = torch.randn(want.shape, generator=g)
    want.backward(dy)
    torch.testing.assert_close(l.backward(dy), xr.grad)


def test_upsampling2d_legacy_convention_on_a_ramp():
    """half_pixel_centers=False (tf.js' resizeBilinear): src = dst / s, so a linear ramp maps to
    min(d / s, n - 1) exactly where d / s is exact; the default convention gives another result."""
    n, s = 5, 4
    ramp = torch.arange(float(n))
    l = UpSampling2D((s, 1), "bilinear", half_pixel_centers=False, name="u")
    _standalone(l, (n, 1, 1), 1, seed=0)
    y = l.forward(ramp.reshape(1, n, 1, 1), True).flatten()
    want = torch.clamp(torch.arange(float(n * s)) / s, max=n - 1.0)
    assert torch.equal(y, want)
    # along the other axis too, and its backward is the transpose of its forward
    l2 = UpSampling2D((1, s), "bilinear", half_pixel_centers=False, name="v")
    _standalone(l2, (1, n, 1), 1, seed=0)
    assert torch.equal(l2.forward(ramp.reshape(1, 1, n, 1), True).flatten(), want)
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(1, 1, n * s, 1, generator=g)
    x = torch.randn(1, 1, n, 1, generator=g)
    lhs = float((l2.forward(x, True) * dy).sum())
    rhs = float((l2.backward(dy) * x).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0)
    k = UpSampling2D((s, 1), "bilinear", name="k")
    _standalone(k, (n, 1, 1), 1, seed=0)
    assert not torch.equal(k.forward(ramp.reshape(1, n, 1, 1), True).flatten(), want)


# ------------------------------------------------------------------------------------------- topologies
def _seq(layers, input_shape):
    out = []
    for i, (cls, cfg) in enumerate(layers):
        c = dict(cfg, name=cfg.get("name", f"l{i}"))
        if i == 0:
            c["batch_input_shape"] = [None, *input_shape]
        out.append({"class_name": cls, "config": c})
    return {"class_name": "Sequential", "config": {"name": "m", "layers": out}}


def _functional(layers, input_shape, output):
    out = [{"class_name": "InputLayer", "name": "inp",
            "config": {"name": "inp", "batch_input_shape": [None, *input_shape], "dtype": "float32"},
            "inbound_nodes": []}]
    for cls, name, cfg, ins in layers:
        out.append({"class_name": cls, "name": name, "config": dict(cfg, name=name),
                    "inbound_nodes": [[[i, 0, 0, {}] for i in ins]]})
    return {"class_name": "Model", "config": {"name": "g", "layers": out, "input_layers": [["inp", 0, 0]],
                                              "output_layers": [[output, 0, 0]]}}


def sequential_decoder():
    return _seq([
        ("Conv2D", {"filters": 6, "kernel_size": [3, 3], "strides": [2, 2], "padding": "same", "activation": "relu"}),
        ("Conv2DTranspose", {"filters": 5, "kernel_size": [3, 3], "strides": [2, 2], "padding": "same",
                             "activation": "relu"}),
        ("UpSampling2D", {"size": [2, 2], "interpolation": "nearest"}),
        ("Conv2D", {"filters": 4, "kernel_size": [3, 3], "padding": "same", "activation": "relu"}),
        ("GlobalAveragePooling2D", {}),
        ("Dense", {"units": 3, "activation": "softmax"}),
    ], (8, 8, 2))


def unet_style(input_shape=(12, 12, 2)):
    """enc (input resolution) -> Conv2D stride 2 -> Conv2DTranspose stride 2 -> Concatenate with enc ->
    UpSampling2D (bilinear) -> Conv2D -> GlobalAveragePooling2D -> Dense softmax."""
    return _functional([
        ("Conv2D", "enc", {"filters": 8, "kernel_size": [3, 3], "padding": "same", "activation": "relu"}, ["inp"]),
        ("Conv2D", "down", {"filters": 8, "kernel_size": [3, 3], "strides": [2, 2], "padding": "same",
                            "activation": "relu"}, ["enc"]),
        ("Conv2DTranspose", "up", {"filters": 8, "kernel_size": [3, 3], "strides": [2, 2], "padding": "same",
                                   "activation": "relu"}, ["down"]),
        ("Concatenate", "cat", {"axis": -1}, ["enc", "up"]),
        ("UpSampling2D", "ups", {"size": [2, 2], "interpolation": "bilinear"}, ["cat"]),
        ("Conv2D", "dec", {"filters": 8, "kernel_size": [3, 3], "padding": "same", "activation": "relu"}, ["ups"]),
        ("GlobalAveragePooling2D", "gap", {}, ["dec"]),
        ("Dense", "out", {"units": 5, "activation": "softmax"}, ["gap"]),
    ], input_shape, "out")


def _conv_tf(h, w, b, strides=(1, 1)):
    """NHWC conv with the engine kernel OHWI and TensorFlow 'same' padding (the odd pixel bottom / right)."""
    B, H, W, C = h.shape
    kh, kw = w.shape[1], w.shape[2]
    th = max((-(-H // strides[0]) - 1) * strides[0] + kh - H, 0)
    tw = max((-(-W // strides[1]) - 1) * strides[1] + kw - W, 0)
    hp = F.pad(h.permute(0, 3, 1, 2), (tw // 2, tw - tw // 2, th // 2, th - th // 2))
    return F.conv2d(hp, w.permute(0, 3, 1, 2), b, stride=strides).permute(0, 2, 3, 1)


def _bilinear2(h):
    return F.interpolate(h.permute(0, 3, 1, 2), scale_factor=2.0, mode="bilinear",
                         align_corners=False).permute(0, 2, 3, 1)


def _params(net):
    return {s.name: net.store[s.name].detach().clone().requires_grad_(True) for s in net.store.specs}


def _check_grads(net, P, st, loss, B):
    assert abs(float(st[0]) / B - loss.item()) < 1e-4
    for s in net.store.specs:
        torch.testing.assert_close(net.store.gradient(s.name), P[s.name].grad, rtol=1e-4, atol=1e-5,
                                   msg=lambda m, n=s.name: f"{n}: {m}")


def test_both_topologies_load():
    layers, shape = layers_from_keras(sequential_decoder())
    assert [type(l).__name__ for l in layers] == ["Conv2D", "Conv2DTranspose", "UpSampling2D", "Conv2D",
                                                  "GlobalAveragePooling2D", "Dense"]
    net = Net(layers, shape, device="cpu", seed=0)
    assert [l.out_shape for l in net.exec_layers[:4]] == [(4, 4, 6), (8, 8, 5), (16, 16, 5), (16, 16, 4)]
    assert net.exec_layers[1].in_relu and net.exec_layers[2].in_relu and net.exec_layers[1].relu
    assert net.exec_layers[1] in net.wgrad_layers() and net.flops_per_example() > 0
    layers, shape = layers_from_keras(json.loads(json.dumps(unet_style())))
    graph = [l for l in layers if isinstance(l, GraphLayer)]
    assert len(graph) == 1
    kinds = [type(l) for l in graph[0].sublayers()]
    assert Conv2DTranspose in kinds
    net = Net(layers, shape, device="cpu", seed=0)
    assert any(isinstance(l, UpSampling2D) for l in net._all_leaf_layers())
    assert [n for n in net.store.names() if n.startswith("up/")] == ["up/kernel", "up/bias"]
    assert net.store.spec("up/kernel").shape == (8, 3, 3, 8)


def test_sequential_topology_round_trips_through_keras_json():
    layers, shape = layers_from_keras(sequential_decoder())
    net = Net(layers, shape, device="cpu", seed=0)
    cfg = keras_config_from_layers(net.layers_all, net.input_shape)
    classes = [l["class_name"] for l in cfg["config"]["layers"]]
    assert classes[1:3] == ["Conv2DTranspose", "UpSampling2D"]
    again, shape2 = layers_from_keras(json.loads(json.dumps(cfg)))
    assert shape2 == shape
    assert [(type(l).__name__, l.name, l.config()) for l in again] == \
        [(type(l).__name__, l.name, l.config()) for l in net.layers_all]
    c1, c2 = again[1].config(), again[2].config()
    assert c1["kernel_size"] == [3, 3] and c1["strides"] == [2, 2] and c1["padding"] == "same"
    assert c2 == {"size": [2, 2], "interpolation": "nearest"}


def test_other_activations_run_as_their_own_launch_after_the_layer():
    topo = _seq([("Conv2D", {"filters": 3, "kernel_size": [1, 1]}),
                 ("Conv2DTranspose", {"filters": 4, "kernel_size": [2, 2], "strides": [2, 2], "activation": "tanh"}),
                 ("Flatten", {}), ("Dense", {"units": 3})], (3, 3, 2))
    layers, shape = layers_from_keras(topo)
    net = Net(layers, shape, device="cpu", seed=2)
    assert [type(l).__name__ for l in net.exec_layers] == ["Conv2D", "Conv2DTranspose", "Activation", "Dense"]
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 3, 3, 2, generator=g)
    y = torch.randint(0, 3, (4,), generator=g)
    st = net.compute_gradients(x, y)
    P = _params(net)
    h = _conv_tf(x, P["l0/kernel"], P["l0/bias"])
    h = torch.tanh(deconv_torch(h, P["l1/kernel"], P["l1/bias"], (2, 2), (2, 2), "valid"))
    loss = F.cross_entropy(F.linear(h.reshape(4, -1), P["l3/kernel"], P["l3/bias"]), y)
    loss.backward()
    _check_grads(net, P, st, loss, 4)


@pytest.mark.parametrize("topology", ["sequential", "unet"])
def test_whole_model_grads_match_autograd(topology):
    seq = topology == "sequential"
    layers, shape = layers_from_keras(sequential_decoder() if seq else unet_style())
    net = Net(layers, shape, device="cpu", seed=9)
    g = torch.Generator().manual_seed(2)
    B = 5
    x = torch.rand(B, *shape, generator=g)
    with torch.no_grad():  # biases start at zero: make them count
        for s in net.store.specs:
            if s.name.endswith("/bias"):
                net.store[s.name].copy_(torch.randn(s.shape, generator=g) * 0.1)
    P = _params(net)
    if seq:
        y = torch.randint(0, 3, (B,), generator=g)
        h = F.relu(_conv_tf(x, P["l0/kernel"], P["l0/bias"], (2, 2)))
        h = F.relu(deconv_torch(h, P["l1/kernel"], P["l1/bias"], (3, 3), (2, 2), "same"))
        h = h.repeat_interleave(2, 1).repeat_interleave(2, 2)
        h = F.relu(_conv_tf(h, P["l3/kernel"], P["l3/bias"]))
        z = F.linear(h.mean(dim=(1, 2)), P["l5/kernel"], P["l5/bias"])
    else:
        y = torch.randint(0, 5, (B,), generator=g)
        enc = F.relu(_conv_tf(x, P["enc/kernel"], P["enc/bias"]))
        down = F.relu(_conv_tf(enc, P["down/kernel"], P["down/bias"], (2, 2)))
        up = F.relu(deconv_torch(down, P["up/kernel"], P["up/bias"], (3, 3), (2, 2), "same"))
        h = _bilinear2(torch.cat([enc, up], dim=-1))
        h = F.relu(_conv_tf(h, P["dec/kernel"], P["dec/bias"]))
        z = F.linear(h.mean(dim=(1, 2)), P["out/kernel"], P["out/bias"])
    st = net.compute_gradients(x, y)
    loss = F.cross_entropy(z, y)
    loss.backward()
    _check_grads(net, P, st, loss, B)


def test_tfjs_round_trip_keeps_keras_kernel_layout_and_bits(tmp_path):
    from distriflow_amd.checkpoint.tfjs import read_manifest_weights, save_layers_model
    from distriflow_amd.models.distri_model import fetch_model

    layers, shape = layers_from_keras(sequential_decoder())
    net = Net(layers, shape, device="cpu", seed=21)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # every parameter away from its initial value
        for s in net.store.specs:
            net.store[s.name].add_(torch.randn(s.shape, generator=g) * 0.01)
        net.store["l1/kernel"][4, 2, 1, 3] = 1234.5  # engine [cin][kh][kw][f]
    path = save_layers_model(net, str(tmp_path / "ck"))
    with open(path) as f:
        manifest = {w["name"]: w["shape"] for w in json.load(f)["weightsManifest"][0]["weights"]}
    assert manifest["l1/kernel"] == [3, 3, 5, 6] and manifest["l1/bias"] == [5]  # Keras [KH, KW, F, Cin]
    disk = read_manifest_weights(path)
    assert float(disk["l1/kernel"][2, 1, 3, 4]) == 1234.5
    assert torch.equal(torch.from_numpy(disk["l1/kernel"]), net.store["l1/kernel"].permute(1, 2, 3, 0))
    net2 = fetch_model(path, device="cpu")
    assert [type(l).__name__ for l in net2.layers_all] == [type(l).__name__ for l in net.layers_all]
    assert net2.store.names() == net.store.names()
    assert torch.equal(net2.store.master, net.store.master)


def test_unet_style_model_round_trips_every_parameter(tmp_path):
    from distriflow_amd.checkpoint.tfjs import save_layers_model
    from distriflow_amd.models.distri_model import fetch_model

    layers, shape = layers_from_keras(unet_style())
    net = Net(layers, shape, device="cpu", seed=4)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for s in net.store.specs:
            net.store[s.name].add_(torch.randn(s.shape, generator=g) * 0.01)
    # (the exporter writes Sequential topologies; a functional model is saved under the topology it came from)
    path = save_layers_model(net, str(tmp_path / "ck"), topology={"model_config": unet_style()})
    with open(path) as f:
        manifest = {w["name"]: w["shape"] for w in json.load(f)["weightsManifest"][0]["weights"]}
    assert manifest["up/kernel"] == [3, 3, 8, 8] and manifest["dec/kernel"] == [3, 3, 16, 8]
    net2 = fetch_model(path, device="cpu")
    assert net2.store.names() == net.store.names()
    assert torch.equal(net2.store.master, net.store.master)


def test_unsupported_decoder_configs_raise():
    base = {"filters": 4, "kernel_size": [3, 3], "strides": [2, 2]}

    def load(cls, cfg):
        return layers_from_keras(_seq([(cls, cfg)], (8, 8, 2)))

    with pytest.raises(NotImplementedError, match="output_padding"):
        load("Conv2DTranspose", dict(base, output_padding=[1, 1]))
    with pytest.raises(NotImplementedError, match="dilation_rate"):
        load("Conv2DTranspose", dict(base, dilation_rate=[2, 2]))
    with pytest.raises(NotImplementedError, match="channels_first"):
        load("Conv2DTranspose", dict(base, data_format="channels_first"))
    with pytest.raises(NotImplementedError, match="channels_first"):
        load("UpSampling2D", {"size": [2, 2], "data_format": "channels_first"})
    with pytest.raises(NotImplementedError, match="bicubic"):
        load("UpSampling2D", {"size": [2, 2], "interpolation": "bicubic"})
    with pytest.raises(NotImplementedError, match="size"):
        UpSampling2D(1.5)
    # what is supported still loads, output_padding None and dilation 1 spelled out
    layers, _ = load("Conv2DTranspose", dict(base, output_padding=None, dilation_rate=[1, 1]))
    assert isinstance(layers[0], Conv2DTranspose)
    with pytest.raises(ValueError):
        ops.deconv_geometry(1, 0, 4, 2, 2, (3, 3), (1, 1), "same")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_upsample_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """The per-lane channel vectors and accumulators of csrc/upsample.hip are indexed statically; an array
    kept in scratch has faulted a GPU in this project before."""
    out = tmp_path / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    "-I", os.path.join(ROOT, "csrc"), os.path.join(ROOT, "csrc", "upsample.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    names = re.findall(r"^(_Z\S*kernel\S*):", asm, flags=re.M)
    scratch = [int(x) for x in re.findall(r"; ScratchSize: (\d+)", asm)]
    print(dict(zip(names, scratch)))
    assert len(names) >= 10 and len(scratch) >= len(names)
    spilled = [n for n, s in zip(names, scratch) if s > 0]
    assert not spilled, f"kernels with scratch in upsample.hip: {spilled}"
