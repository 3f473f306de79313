"""DepthwiseConv2D, SeparableConv2D and the ReLU layer class of Keras / tf.js LayersModels (MobileNet-style
networks): the CPU fp32 engine against torch autograd on the same graph, the tf.js checkpoint round trip,
and a build-level guard on the kernels (csrc/dwconv.hip).  The GPU kernels themselves are checked against
the same fp32 reference in tests/test_depthwise_gpu.py."""
import json
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from distriflow_amd.models.graph import GraphLayer
from distriflow_amd.models.keras import keras_config_from_layers, layers_from_keras
from distriflow_amd.models.layers import Activation, DepthwiseConv2D, SeparableConv2D
from distriflow_amd.models.net import Net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _seq(layers, input_shape):
    out = []
    for i, (cls, cfg) in enumerate(layers):
        c = dict(cfg, name=cfg.get("name", f"l{i}"))
        if i == 0:
            c["batch_input_shape"] = [None, *input_shape]
        out.append({"class_name": cls, "config": c})
    return {"class_name": "Sequential", "config": {"name": "m", "layers": out}}


def mobilenet_style(dw_cfg):
    """Conv2D -> DepthwiseConv2D -> BatchNormalization -> ReLU(6) -> SeparableConv2D -> GAP -> Dense on 9x9x2.
    The depthwise layer keeps Keras' default bias.  It feeds a training-mode BatchNormalization, so its gradient
    is identically zero (the batch mean removes it): the absolute tolerance here compares that, the cosine of
    the GPU model test cannot, and that test drops the bias (tests/test_depthwise_gpu.py)."""
    return _seq([
        ("Conv2D", {"filters": 8, "kernel_size": [3, 3], "padding": "same", "activation": "relu"}),
        ("DepthwiseConv2D", dict(dw_cfg)),
        ("BatchNormalization", {"momentum": 0.99, "epsilon": 1e-3}),
        ("ReLU", {"max_value": 6.0}),
        ("SeparableConv2D", dict(dw_cfg, filters=12, activation="relu")),
        ("GlobalAveragePooling2D", {}),
        ("Dense", {"units": 5, "activation": "softmax"}),
    ], (9, 9, 2))


DW_CASES = {
    "3x3_s2_same": {"kernel_size": [3, 3], "strides": [2, 2], "padding": "same"},
    "2x3_s21_valid_m2": {"kernel_size": [2, 3], "strides": [2, 1], "padding": "valid", "depth_multiplier": 2},
}


def _clip(v, lo, hi):  # TensorFlow's gradient of relu6 is zero at the corners
    return torch.where((v > lo) & (v < hi), v, v.clamp(lo, hi).detach())


def _conv(h, w, b, pad=0):  # NHWC, engine kernel OHWI
    return F.conv2d(h.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, padding=pad).permute(0, 2, 3, 1)


def _depthwise(h, w, b, cfg):
    """NHWC depthwise conv with the engine's kernel [KH][KW][C*M]: explicit TensorFlow padding (the odd pixel
    bottom / right), then F.conv2d(groups=C)."""
    (kh, kw), (sh, sw) = cfg["kernel_size"], cfg.get("strides", [1, 1])
    B, H, W, C = h.shape
    pads = (0, 0, 0, 0)
    if cfg.get("padding", "valid") == "same":
        th = max((-(-H // sh) - 1) * sh + kh - H, 0)
        tw = max((-(-W // sw) - 1) * sw + kw - W, 0)
        pads = (tw // 2, tw - tw // 2, th // 2, th - th // 2)
    y = F.conv2d(F.pad(h.permute(0, 3, 1, 2), pads), w.permute(2, 0, 1).unsqueeze(1), b, stride=(sh, sw), groups=C)
    return y.permute(0, 2, 3, 1)


def _params(net):
    return {s.name: net.store[s.name].detach().clone().requires_grad_(True) for s in net.store.specs}


def _check_grads(net, P, st, loss, B):
    assert abs(float(st[0]) / B - loss.item()) < 1e-4
    for s in net.store.specs:
        torch.testing.assert_close(net.store.gradient(s.name), P[s.name].grad, rtol=1e-4, atol=1e-5,
                                   msg=lambda m, n=s.name: f"{n}: {m}")


@pytest.mark.parametrize("case", list(DW_CASES))
def test_mobilenet_style_grads_match_autograd(case):
    cfg = DW_CASES[case]
    layers, shape = layers_from_keras(mobilenet_style(cfg))
    assert [type(l) for l in layers[1:5]] == [DepthwiseConv2D, type(layers[2]), Activation, SeparableConv2D]
    net = Net(layers, shape, device="cpu", seed=3)
    M = cfg.get("depth_multiplier", 1)
    assert [s.name for s in net.store.specs] == [
        "l0/kernel", "l0/bias", "l1/depthwise_kernel", "l1/bias", "l2/gamma", "l2/beta", "l4/depthwise_kernel",
        "l4/pointwise_kernel", "l4/bias", "l6/kernel", "l6/bias"]
    kh, kw = cfg["kernel_size"]
    assert net.store.spec("l1/depthwise_kernel").shape == (kh, kw, 8 * M)
    assert net.store.spec("l4/pointwise_kernel").shape == (12, 1, 1, 8 * M * M)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(6, 9, 9, 2, generator=g)
    y = torch.randint(0, 5, (6,), generator=g)
    with torch.no_grad():  # biases start at zero: make them count
        for n in ("l1/bias", "l4/bias"):
            net.store[n].copy_(torch.randn(net.store[n].shape, generator=g) * 0.1)
    st = net.compute_gradients(x, y)
    P = _params(net)
    h = F.relu(_conv(x, P["l0/kernel"], P["l0/bias"], 1))
    h = _depthwise(h, P["l1/depthwise_kernel"], P["l1/bias"], cfg)
    h = F.batch_norm(h.permute(0, 3, 1, 2), None, None, P["l2/gamma"], P["l2/beta"], training=True,
                     eps=1e-3).permute(0, 2, 3, 1)
    h = _clip(h, 0.0, 6.0)
    h = _depthwise(h, P["l4/depthwise_kernel"], None, cfg)
    h = F.relu(_conv(h, P["l4/pointwise_kernel"], P["l4/bias"]))
    z = F.linear(h.mean(dim=(1, 2)), P["l6/kernel"], P["l6/bias"])
    loss = F.cross_entropy(z, y)
    loss.backward()
    assert net.exec_layers[1].out_shape == tuple(_depthwise(torch.zeros(1, 9, 9, 8), torch.zeros(kh, kw, 8 * M),
                                                             None, cfg).shape[1:])
    _check_grads(net, P, st, loss, 6)
    assert net.flops_per_example() > 0


def test_other_activations_run_as_their_own_launch_after_the_layer():
    """A non-relu activation of either layer is split off by the planner, as for Conv2D / Dense."""
    dw = {"kernel_size": [3, 3], "strides": [1, 1], "padding": "same"}
    topo = _seq([("DepthwiseConv2D", dict(dw, activation="tanh")),
                 ("SeparableConv2D", dict(dw, filters=4, activation="elu")),
                 ("Flatten", {}), ("Dense", {"units": 3})], (5, 5, 2))
    layers, shape = layers_from_keras(topo)
    net = Net(layers, shape, device="cpu", seed=2)
    assert [type(l).__name__ for l in net.exec_layers] == ["DepthwiseConv2D", "Activation", "SeparableConv2D",
                                                           "Activation", "Dense"]
    assert not net.exec_layers[0].need_dx and net.exec_layers[2].need_dx
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 5, 5, 2, generator=g)
    y = torch.randint(0, 3, (4,), generator=g)
    st = net.compute_gradients(x, y)
    P = _params(net)
    h = torch.tanh(_depthwise(x, P["l0/depthwise_kernel"], P["l0/bias"], dw))
    h = F.elu(_conv(_depthwise(h, P["l1/depthwise_kernel"], None, dw), P["l1/pointwise_kernel"], P["l1/bias"]))
    loss = F.cross_entropy(F.linear(h.reshape(4, -1), P["l3/kernel"], P["l3/bias"]), y)
    loss.backward()
    _check_grads(net, P, st, loss, 4)


def _functional(layers, input_shape, output):
    out = [{"class_name": "InputLayer", "name": "inp",
            "config": {"name": "inp", "batch_input_shape": [None, *input_shape], "dtype": "float32"},
            "inbound_nodes": []}]
    for cls, name, cfg, ins in layers:
        out.append({"class_name": cls, "name": name, "config": dict(cfg, name=name),
                    "inbound_nodes": [[[i, 0, 0, {}] for i in ins]]})
    return {"class_name": "Model", "config": {"name": "g", "layers": out, "input_layers": [["inp", 0, 0]],
                                              "output_layers": [[output, 0, 0]]}}


def test_inverted_residual_graph_grads_match_autograd():
    """stem -> [1x1 expand -> depthwise 3x3 (relu6) -> 1x1 project] + stem -> [SeparableConv2D] + that -> GAP ->
    Dense: both layers as nodes of the branching region."""
    dw = {"kernel_size": [3, 3], "strides": [1, 1], "padding": "same"}
    topo = _functional([
        ("Conv2D", "stem", {"filters": 4, "kernel_size": [3, 3], "padding": "same", "activation": "relu"}, ["inp"]),
        ("Conv2D", "expand", {"filters": 8, "kernel_size": [1, 1], "activation": "relu"}, ["stem"]),
        ("DepthwiseConv2D", "dw", dict(dw, activation="relu6"), ["expand"]),
        ("Conv2D", "project", {"filters": 4, "kernel_size": [1, 1]}, ["dw"]),
        ("Add", "add1", {}, ["stem", "project"]),
        ("SeparableConv2D", "sep", dict(dw, filters=4, activation="relu"), ["add1"]),
        ("Add", "add2", {}, ["add1", "sep"]),
        ("GlobalAveragePooling2D", "gap", {}, ["add2"]),
        ("Dense", "out", {"units": 3, "activation": "softmax"}, ["gap"]),
    ], (6, 6, 2), "out")
    layers, shape = layers_from_keras(json.loads(json.dumps(topo)))
    graph = [l for l in layers if isinstance(l, GraphLayer)]
    assert len(graph) == 1
    kinds = [type(l) for l in graph[0].sublayers()]
    assert DepthwiseConv2D in kinds and SeparableConv2D in kinds
    net = Net(layers, shape, device="cpu", seed=9)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(5, 6, 6, 2, generator=g)
    y = torch.randint(0, 3, (5,), generator=g)
    with torch.no_grad():  # biases start at zero: make them count
        for n in ("dw/bias", "sep/bias"):
            net.store[n].copy_(torch.randn(net.store[n].shape, generator=g) * 0.1)
    st = net.compute_gradients(x, y)
    P = _params(net)
    stem = F.relu(_conv(x, P["stem/kernel"], P["stem/bias"], 1))
    e = F.relu(_conv(stem, P["expand/kernel"], P["expand/bias"]))
    d = _clip(_depthwise(e, P["dw/depthwise_kernel"], P["dw/bias"], dw), 0.0, 6.0)
    a1 = stem + _conv(d, P["project/kernel"], P["project/bias"])
    s = F.relu(_conv(_depthwise(a1, P["sep/depthwise_kernel"], None, dw), P["sep/pointwise_kernel"], P["sep/bias"]))
    z = F.linear((a1 + s).mean(dim=(1, 2)), P["out/kernel"], P["out/bias"])
    loss = F.cross_entropy(z, y)
    loss.backward()
    _check_grads(net, P, st, loss, 5)


def test_tfjs_round_trip_keeps_names_shapes_and_bits(tmp_path):
    from distriflow_amd.checkpoint.tfjs import load_layers_model_weights, load_topology, save_layers_model

    cfg = {"kernel_size": [3, 3], "strides": [1, 1], "padding": "same", "depth_multiplier": 2}
    layers, shape = layers_from_keras(mobilenet_style(cfg))
    net = Net(layers, shape, device="cpu", seed=21)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # every parameter (biases, gamma / beta too) away from its initial value
        for s in net.store.specs:
            net.store[s.name].add_(torch.randn(s.shape, generator=g) * 0.01)
    path = save_layers_model(net, str(tmp_path / "ck"))
    with open(path) as f:
        manifest = {w["name"]: w["shape"] for w in json.load(f)["weightsManifest"][0]["weights"]}
    assert manifest["l1/depthwise_kernel"] == [3, 3, 8, 2]
    assert manifest["l4/depthwise_kernel"] == [3, 3, 16, 2]
    assert manifest["l4/pointwise_kernel"] == [1, 1, 32, 12]
    assert manifest["l4/bias"] == [12] and manifest["l1/bias"] == [16]
    names = list(manifest)
    assert names.index("l4/depthwise_kernel") + 1 == names.index("l4/pointwise_kernel") == names.index("l4/bias") - 1
    layers2, shape2 = layers_from_keras(load_topology(path))
    net2 = Net(layers2, shape2, device="cpu", seed=99)
    assert not torch.equal(net2.store.master, net.store.master)
    load_layers_model_weights(net2, path)
    assert torch.equal(net2.store.master, net.store.master)
    # the pointwise kernel is HWIO on disk: element [0, 0, i, o] is the engine's [o, 0, 0, i]
    from distriflow_amd.checkpoint.tfjs import read_manifest_weights

    disk = read_manifest_weights(path)
    pw = net.store["l4/pointwise_kernel"]
    assert torch.equal(torch.from_numpy(disk["l4/pointwise_kernel"])[0, 0], pw[:, 0, 0, :].t())
    assert torch.equal(torch.from_numpy(disk["l1/depthwise_kernel"]).reshape(3, 3, 16), net.store["l1/depthwise_kernel"])
    # topology export -> import reproduces the layer configs
    again, shape3 = layers_from_keras(keras_config_from_layers(net.layers_all, net.input_shape))
    assert shape3 == shape
    assert [(type(l).__name__, l.name, l.config()) for l in again] == \
        [(type(l).__name__, l.name, l.config()) for l in net.layers_all]


def test_relu_layer_class():
    def one(cfg):
        topo = _seq([("Dense", {"units": 4}), ("ReLU", cfg), ("Dense", {"units": 2})], (3,))
        return layers_from_keras(topo)[0][1]

    for cfg, act in (({}, "relu"), ({"max_value": None}, "relu"), ({"max_value": 6}, "relu6"),
                     ({"max_value": 6.0, "negative_slope": 0.0, "threshold": 0.0}, "relu6")):
        l = one(cfg)
        assert isinstance(l, Activation) and l.activation == act
    with pytest.raises(NotImplementedError, match="max_value"):
        one({"max_value": 3})
    with pytest.raises(NotImplementedError, match="negative_slope"):
        one({"negative_slope": 0.1})
    with pytest.raises(NotImplementedError, match="threshold"):
        one({"threshold": 1.0})


def test_unsupported_depthwise_configs_still_raise():
    for cls in ("DepthwiseConv2D", "SeparableConv2D"):
        base = {"kernel_size": [3, 3], "filters": 4}
        with pytest.raises(NotImplementedError):
            layers_from_keras(_seq([(cls, dict(base, dilation_rate=[2, 2]))], (8, 8, 2)))
        with pytest.raises(NotImplementedError):
            layers_from_keras(_seq([(cls, dict(base, data_format="channels_first"))], (8, 8, 2)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_dwconv_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """The register windows and accumulators of csrc/dwconv.hip are indexed statically (fully unrolled tap
    loops); an accumulator array kept in scratch has faulted a GPU in this project before."""
    out = tmp_path / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    "-I", os.path.join(ROOT, "csrc"), os.path.join(ROOT, "csrc", "dwconv.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    names = re.findall(r"^(_Z\S*kernel\S*):", asm, flags=re.M)
    scratch = [int(x) for x in re.findall(r"; ScratchSize: (\d+)", asm)]
    assert len(names) >= 6 and len(scratch) >= len(names)
    spilled = [n for n, s in zip(names, scratch) if s > 0]
    assert not spilled, f"kernels with scratch in dwconv.hip: {spilled}"
