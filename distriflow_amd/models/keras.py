"""Keras / tf.js ``LayersModel`` topology <-> engine layers.

Reads the ``modelTopology`` of a tf.js ``model.json`` and writes it back, so a DistriFlow user's model
files load directly.  The reference wraps any ``tf.LayersModel`` fetched by URL
(/root/reference/src/common/utils.ts:236-244, src/common/models.ts:92-100); its shipped model is a
Keras 2.1.4 Sequential (/root/reference/experiment/mnist/model.json:1).  Supported:

* ``Sequential`` models, and functional ``Model`` / ``Functional`` graphs with one input and one output:
  chains, and branching graphs whose branches join in merge layers (Add, Subtract, Multiply, Average,
  Maximum, Minimum, Concatenate on the channel axis) or fan out from one layer to several (the
  branching region runs as one :class:`~distriflow_amd.models.graph.GraphLayer`, models/graph.py);
  the logits layer (the output) must be a Dense fed by a single chain;
* InputLayer, Conv2D (any kernel size / strides pair, 'valid' or 'same' -- an odd 'same' total pads the
  bottom / right, as TensorFlow does), DepthwiseConv2D and SeparableConv2D (same geometries, any
  depth_multiplier; no dilation), Conv2DTranspose (same geometries, kernels smaller than the stride included;
  no output_padding, no dilation), UpSampling2D (integer sizes, nearest or bilinear with Keras' half-pixel
  centres), Dense, Activation (relu, relu6, sigmoid, tanh, elu, selu, softplus, softsign,
  hard_sigmoid, swish / silu, exponential, linear; softmax / sigmoid as the output), the ReLU layer class
  (max_value None or 6, no negative_slope / threshold), MaxPooling2D and
  AveragePooling2D (any pool / strides, 'valid' or 'same'), GlobalAveragePooling2D,
  GlobalMaxPooling2D, Dropout, Flatten, BatchNormalization — channels_last only.
"""
from __future__ import annotations

from ..ops.geometry import pair as _pair
from .graph import GraphLayer, Merge, split_chain
from .layers import (Activation, AveragePooling2D, BatchNorm, Conv2D, Conv2DTranspose, Dense, DepthwiseConv2D, Dropout,
                     Flatten, GlobalAveragePooling2D, GlobalMaxPooling2D, Layer, MaxPooling2D, SeparableConv2D,
                     UpSampling2D)

_MERGES = ("Add", "Subtract", "Multiply", "Average", "Maximum", "Minimum", "Concatenate")


def _inbound_names(lc) -> list:
    """Names of the layers feeding ``lc`` (Keras 2 and Keras 3 JSON); raises for shared layers."""
    nodes = lc.get("inbound_nodes") or []
    if not nodes:
        return []
    if len(nodes) != 1:
        raise NotImplementedError(f"layer {lc['config'].get('name')!r} is applied more than once (shared layer)")
    node = nodes[0]
    if isinstance(node, dict):  # Keras 3 style {"args": [...], "kwargs": {}}
        names = []
        for a in node.get("args", []):
            items = a if isinstance(a, list) else [a]
            names += [x["config"]["keras_history"][0] for x in items if isinstance(x, dict) and "config" in x]
        return names
    return [inb[0] for inb in node]  # Keras 2 style [[name, node_index, tensor_index, kwargs], ...]


def _graph_order(layer_cfgs: list, model_cfg: dict) -> tuple:
    """(configs in topological order, {name: [input names]}) of a one-input, one-output functional
    graph, keeping only what reaches the output."""
    by_name = {lc.get("name") or lc["config"].get("name"): lc for lc in layer_cfgs}
    outs = model_cfg.get("output_layers") or []
    ins = model_cfg.get("input_layers") or []
    if len(outs) != 1:
        raise NotImplementedError("functional models must have exactly one output")
    if len(ins) > 1:
        raise NotImplementedError("functional models must have exactly one input")
    name_of = lambda ref: ref[0] if isinstance(ref, (list, tuple)) else ref  # noqa: E731
    parents = {n: _inbound_names(lc) for n, lc in by_name.items()}
    order, state = [], {}

    def visit(n):  # depth-first post-order from the output
        if state.get(n) == 1:
            raise ValueError("cycle in the layer graph")
        if state.get(n) == 2:
            return
        state[n] = 1
        for p in parents[n]:
            visit(p)
        state[n] = 2
        order.append(n)

    visit(name_of(outs[0]))
    return [by_name[n] for n in order], parents


def _init_name(cfg, key: str = "kernel_initializer"):
    ki = cfg.get(key) or {}
    cls = ki.get("class_name", "VarianceScaling") if isinstance(ki, dict) else str(ki)
    c = ki.get("config", {}) if isinstance(ki, dict) else {}
    if cls in ("GlorotUniform", "glorot_uniform"):
        return "glorot_uniform"
    if cls == "VarianceScaling":
        mode, dist, scale = c.get("mode", "fan_avg"), c.get("distribution", "uniform"), c.get("scale", 1.0)
        if mode == "fan_avg" and "uniform" in dist and scale == 1.0:
            return "glorot_uniform"
        if mode == "fan_in" and scale == 2.0:
            return "he_normal"
        if mode == "fan_in" and scale == 1.0 and "uniform" in dist:
            return "lecun_uniform"
    if cls in ("HeNormal", "he_normal"):
        return "he_normal"
    return "glorot_uniform"


def _make_layer(k: str, c: dict) -> Layer:
    """Engine layer of Keras class ``k`` with config ``c``."""
    name = c.get("name")
    if c.get("data_format", "channels_last") != "channels_last":
        raise NotImplementedError("channels_first layers")
    if k == "Conv2D":
        if tuple(c.get("dilation_rate", [1, 1])) != (1, 1):
            raise NotImplementedError("dilated conv")
        return Conv2D(c["filters"], tuple(c["kernel_size"]), tuple(c.get("strides", [1, 1])), c.get("padding", "valid"),
                      c.get("activation", "linear"), c.get("use_bias", True), name=name,
                      kernel_initializer=_init_name(c))
    if k in ("DepthwiseConv2D", "SeparableConv2D"):
        if _pair(c.get("dilation_rate", [1, 1])) != (1, 1):
            raise NotImplementedError(f"dilated {k}")
        geom = (_pair(c["kernel_size"]), _pair(c.get("strides", [1, 1])), c.get("padding", "valid"),
                int(c.get("depth_multiplier", 1)), c.get("activation", "linear"), c.get("use_bias", True))
        dinit = _init_name(c, "depthwise_initializer")
        if k == "DepthwiseConv2D":
            return DepthwiseConv2D(*geom, name=name, depthwise_initializer=dinit)
        return SeparableConv2D(c["filters"], *geom, name=name, depthwise_initializer=dinit,
                               pointwise_initializer=_init_name(c, "pointwise_initializer"))
    if k == "Conv2DTranspose":
        if c.get("output_padding") is not None:
            raise NotImplementedError(f"Conv2DTranspose {name!r}: output_padding {c['output_padding']!r}")
        if _pair(c.get("dilation_rate", [1, 1])) != (1, 1):
            raise NotImplementedError(f"Conv2DTranspose {name!r}: dilation_rate {c['dilation_rate']!r}")
        return Conv2DTranspose(c["filters"], _pair(c["kernel_size"]), _pair(c.get("strides", [1, 1])),
                               c.get("padding", "valid"), c.get("activation", "linear"), c.get("use_bias", True),
                               name=name, kernel_initializer=_init_name(c))
    if k == "UpSampling2D":
        # Keras' own sampling (half-pixel centres); tf.js' upSampling2d differs for 'bilinear', see PARITY.md
        return UpSampling2D(c.get("size", [2, 2]), c.get("interpolation", "nearest"), name=name)
    if k == "Dense":
        return Dense(c["units"], c.get("activation", "linear"), c.get("use_bias", True), name=name,
                     kernel_initializer=_init_name(c))
    if k == "Activation":
        return Activation(c["activation"], name=name)
    if k == "ReLU":
        # the layer class MobileNet-style models use for relu6; only the two plain forms are implemented
        if float(c.get("negative_slope") or 0.0) != 0.0:
            raise NotImplementedError(f"ReLU layer {name!r}: negative_slope {c['negative_slope']!r}")
        if float(c.get("threshold") or 0.0) != 0.0:
            raise NotImplementedError(f"ReLU layer {name!r}: threshold {c['threshold']!r}")
        mv = c.get("max_value")
        if mv is None:
            return Activation("relu", name=name)
        if float(mv) == 6.0:
            return Activation("relu6", name=name)
        raise NotImplementedError(f"ReLU layer {name!r}: max_value {mv!r} (supported: None, 6)")
    if k in ("MaxPooling2D", "AveragePooling2D"):
        cls_ = MaxPooling2D if k == "MaxPooling2D" else AveragePooling2D
        return cls_(tuple(c.get("pool_size", [2, 2])), c.get("strides"), c.get("padding", "valid"), name=name)
    if k == "GlobalAveragePooling2D":
        return GlobalAveragePooling2D(name=name)
    if k == "GlobalMaxPooling2D":
        return GlobalMaxPooling2D(name=name)
    if k == "Dropout":
        return Dropout(c["rate"], name=name)
    if k == "Flatten":
        return Flatten(name=name)
    if k == "BatchNormalization":
        return BatchNorm(momentum=1.0 - c.get("momentum", 0.99), eps=c.get("epsilon", 1e-3), name=name)
    if k in _MERGES:
        # the axis is checked against the inputs' rank when the graph is built (Merge.build_multi)
        return Merge(k, name=name, axis=int(c.get("axis", -1)) if k == "Concatenate" else -1)
    raise NotImplementedError(f"Keras layer {k}")


def _input_shape_of(lc) -> tuple | None:
    c = lc["config"]
    shp = c.get("batch_input_shape") or c.get("batch_shape")
    return tuple(int(v) for v in shp[1:]) if shp else None


def _graph_layers(order: list, parents: dict) -> tuple:
    """Engine layers of a functional graph: the sequential head and tail as chain layers, the branching
    region in between as one GraphLayer.  Non-relu activations of a Conv2D / Dense INSIDE the branching
    region become their own Activation node (as the chain planner does for chain layers)."""
    input_shape, nodes, value = None, [], {}
    for lc in order:
        k, c = lc["class_name"], lc["config"]
        name = c.get("name")
        if k == "InputLayer" or not parents[name]:
            if k != "InputLayer":
                raise NotImplementedError(f"layer {name!r} has no input")
            input_shape = _input_shape_of(lc)
            value[name] = 0
            continue
        l = _make_layer(k, c)
        srcs = [value[p] for p in parents[name]]
        if isinstance(l, Merge) != (len(srcs) > 1):
            raise NotImplementedError(f"layer {name!r} ({k}) with {len(srcs)} inputs")
        nodes.append((l, srcs))
        value[name] = len(nodes)
    if input_shape is None:
        raise ValueError("the graph has no InputLayer with a batch shape")
    head, mid, tail = split_chain(nodes)
    if mid is None:
        return head, input_shape
    out, newid = [], {0: 0}
    for j, (l, ins) in enumerate(mid, start=1):
        out.append((l, [newid[i] for i in ins]))
        act = getattr(l, "activation", None) if isinstance(l, (Dense, Conv2D, Conv2DTranspose, DepthwiseConv2D,
                                                               SeparableConv2D)) else None
        if act not in (None, "linear", "relu"):
            if act == "softmax":
                raise NotImplementedError("a softmax activation inside a branching region")
            out.append((Activation(act, name=f"{l.name}/{act}", implicit=True), [len(out)]))
        newid[j] = len(out)  # consumers of node j read its activation's output when one was added
    return head + [GraphLayer(out, name="graph")] + tail, input_shape


def layers_from_keras(model_config: dict) -> tuple[list[Layer], tuple]:
    """-> (layers, input_shape HWC/F) from ``modelTopology.model_config`` (or ``modelTopology`` itself)."""
    if "model_config" in model_config:
        model_config = model_config["model_config"]
    cls = model_config.get("class_name")
    cfg = model_config.get("config")
    layer_cfgs = cfg["layers"] if isinstance(cfg, dict) else cfg
    if cls in ("Model", "Functional"):
        return _graph_layers(*_graph_order(layer_cfgs, cfg))
    if cls not in ("Sequential", None):
        raise NotImplementedError(f"model class {cls!r} (supported: Sequential, functional Model)")
    layers: list[Layer] = []
    input_shape = None
    for lc in layer_cfgs:
        if input_shape is None:
            input_shape = _input_shape_of(lc)
        if lc["class_name"] == "InputLayer":
            continue
        l = _make_layer(lc["class_name"], lc["config"])
        if isinstance(l, Merge):
            raise NotImplementedError("a merge layer in a Sequential model")
        layers.append(l)
    if input_shape is None:
        raise ValueError("model_config has no batch_input_shape")
    return layers, input_shape


def optimizer_from_keras(topology: dict) -> dict | None:
    """The optimizer a Keras / tf.js ``modelTopology`` was compiled with, from
    ``training_config.optimizer_config``: ``{"name": "adam" | "sgd", "lr", "betas", "eps", "momentum"}``
    (betas / eps None for SGD, momentum 0.0 for Adam), or None when the topology names no optimizer.
    Both the ``lr`` and the ``learning_rate`` spelling are read.  AMSGrad, a learning-rate ``decay`` and
    other optimizer classes are not implemented and raise instead of training something else."""
    tc = (topology or {}).get("training_config") or {}
    oc = tc.get("optimizer_config")
    if not oc:
        return None
    cls = oc.get("class_name")
    cfg = oc.get("config") or {}
    if cls not in ("Adam", "SGD"):
        raise NotImplementedError(f"Keras optimizer {cls!r} (supported: Adam, SGD)")
    if cfg.get("amsgrad"):
        raise NotImplementedError("Adam with amsgrad=true")
    if float(cfg.get("decay") or 0.0) != 0.0:
        raise NotImplementedError(f"optimizer learning-rate decay {cfg['decay']!r}")
    lr = cfg.get("learning_rate", cfg.get("lr"))
    if lr is None:
        lr = 0.001 if cls == "Adam" else 0.01  # the Keras defaults
    if isinstance(lr, dict):
        raise NotImplementedError("a learning-rate schedule object")
    if cls == "Adam":
        return {"name": "adam", "lr": float(lr), "betas": (float(cfg.get("beta_1", 0.9)), float(cfg.get("beta_2", 0.999))),
                "eps": float(cfg.get("epsilon") or 1e-7), "momentum": 0.0}
    if cfg.get("nesterov"):
        raise NotImplementedError("Keras SGD with nesterov=true from a model.json")
    return {"name": "sgd", "lr": float(lr), "betas": None, "eps": None, "momentum": float(cfg.get("momentum", 0.0))}


_KERAS_LOSSES = {"mean_squared_error": "meanSquaredError", "mse": "meanSquaredError",
                 "mean_absolute_error": "absoluteDifference", "mae": "absoluteDifference",
                 "hinge": "hingeLoss", "huber": "huberLoss", "huber_loss": "huberLoss",
                 "binary_crossentropy": "logLoss", "categorical_crossentropy": "categorical_crossentropy"}


def loss_from_keras(topology: dict) -> str | None:
    """The ``lossesMap`` name of the loss a Keras / tf.js ``modelTopology`` was compiled with, from
    ``training_config.loss``, or None when the topology names none.  ``binary_crossentropy`` maps to
    ``logLoss`` and ``categorical_crossentropy`` to itself: Keras clips the probabilities to
    [eps, 1 - eps] where the tf.js losses add eps inside the logarithm, so the two differ by O(1e-7).
    Any other loss name, and a per-output dict or list of losses, raises instead of training something else."""
    tc = (topology or {}).get("training_config") or {}
    loss = tc.get("loss")
    if loss is None:
        return None
    if isinstance(loss, (dict, list, tuple)):
        raise NotImplementedError(f"per-output losses {loss!r} (one loss name is supported)")
    if loss not in _KERAS_LOSSES:
        raise NotImplementedError(f"Keras loss {loss!r} (supported: {sorted(_KERAS_LOSSES)})")
    return _KERAS_LOSSES[loss]


def keras_config_from_layers(layers: list[Layer], input_shape: tuple, name: str = "sequential") -> dict:
    """Inverse of :func:`layers_from_keras` (Keras 2.x Sequential JSON, as tf.js writes it)."""
    out = []
    first = True
    for l in layers:
        c: dict = {"name": l.name, "trainable": True}
        if first:
            c["batch_input_shape"] = [None, *input_shape]
            c["dtype"] = "float32"
            first = False
        if isinstance(l, Conv2D):
            cls = "Conv2D"
            c.update(l.config())
            c.update({"data_format": "channels_last", "dilation_rate": [1, 1],
                      "kernel_initializer": {"class_name": "VarianceScaling",
                                             "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform",
                                                        "seed": None}},
                      "bias_initializer": {"class_name": "Zeros", "config": {}}})
        elif isinstance(l, Conv2DTranspose):
            cls = "Conv2DTranspose"
            c.update(l.config())
            c.update({"data_format": "channels_last", "dilation_rate": [1, 1], "output_padding": None,
                      "kernel_initializer": {"class_name": "VarianceScaling",
                                             "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform",
                                                        "seed": None}},
                      "bias_initializer": {"class_name": "Zeros", "config": {}}})
        elif isinstance(l, UpSampling2D):
            cls = "UpSampling2D"
            c.update(l.config())
            c["data_format"] = "channels_last"
        elif isinstance(l, (DepthwiseConv2D, SeparableConv2D)):
            cls = type(l).__name__
            glorot = {"class_name": "VarianceScaling",
                      "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform", "seed": None}}
            c.update(l.config())
            c.update({"data_format": "channels_last", "dilation_rate": [1, 1], "depthwise_initializer": glorot,
                      "bias_initializer": {"class_name": "Zeros", "config": {}}})
            if isinstance(l, SeparableConv2D):
                c["pointwise_initializer"] = glorot
        elif isinstance(l, Dense):
            cls = "Dense"
            c.update(l.config())
            c.update({"kernel_initializer": {"class_name": "VarianceScaling",
                                             "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform",
                                                        "seed": None}},
                      "bias_initializer": {"class_name": "Zeros", "config": {}}})
        elif isinstance(l, Activation):
            cls = "Activation"
            c.update(l.config())
        elif isinstance(l, GlobalMaxPooling2D):
            cls = "GlobalMaxPooling2D"
            c["data_format"] = "channels_last"
        elif isinstance(l, MaxPooling2D):
            cls = "AveragePooling2D" if isinstance(l, AveragePooling2D) else "MaxPooling2D"
            c.update(l.config())
            c["data_format"] = "channels_last"
        elif isinstance(l, GlobalAveragePooling2D):
            cls = "GlobalAveragePooling2D"
            c["data_format"] = "channels_last"
        elif isinstance(l, Dropout):
            cls = "Dropout"
            c.update(l.config())
        elif isinstance(l, Flatten):
            cls = "Flatten"
        elif isinstance(l, BatchNorm):
            cls = "BatchNormalization"
            c.update({"momentum": 1.0 - l.momentum, "epsilon": l.eps, "axis": -1})
        else:
            raise NotImplementedError(f"cannot export {type(l).__name__} to Keras JSON")
        out.append({"class_name": cls, "config": c})
    return {"class_name": "Sequential", "config": {"name": name, "layers": out}}
