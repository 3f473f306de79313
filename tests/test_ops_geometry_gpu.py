"""A launch and the plan query that describes it hand the native module the same shape arguments: every layer
takes both from one descriptor (distriflow_amd/ops/geometry.py).  The native module is wrapped in a proxy that
records each call and forwards it; a regular and an irregular Conv2D, a Conv2DTranspose and a Dense run forward
and backward once, then the ops-level queries are issued from the layers' own fields, as the engine and the other
tests issue them."""
from types import SimpleNamespace

import pytest
import torch

from distriflow_amd import native, ops
from distriflow_amd.models.layers import Conv2D, Conv2DTranspose, Dense, dgrad_kpad_of, primary_kpad_of
from distriflow_amd.models.params import ParamStore

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
WS = 1 << 22


class _Recorder:
    def __init__(self, mod, log):
        self._mod, self._log = mod, log

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not callable(fn) or isinstance(fn, type):
            return fn

        def wrapped(*a, **kw):
            self._log.append((name, a, kw))
            return fn(*a, **kw)

        return wrapped


@pytest.fixture
def log(monkeypatch):
    calls = []
    proxy = _Recorder(native.require(), calls)
    monkeypatch.setattr(ops, "_C", lambda: proxy)
    monkeypatch.setattr(native, "get", lambda build_if_missing=None: proxy)
    return calls


def _shapes(call):
    """The shape arguments of a recorded call: (M, N, K, Kpad, geom, mode) of igemm_fwd / conv_plan,
    (M, N, K, ldd, lda, geom, mode) of igemm_wgrad / wgrad_plan."""
    name, a, _ = call
    if name == "igemm_fwd":
        return tuple(a[5:9]) + (a[11], a[12])
    return tuple({"conv_plan": a[:6], "igemm_wgrad": a[5:12], "wgrad_plan": a[:7]}[name])


def _run(layer, in_shape, B, log):
    """Forward and backward of ``layer`` outside a Net (own parameter store, own buffers); returns what it
    launched: the two igemm_fwd calls in order (the forward, then the input gradient) and the igemm_wgrad call."""
    layer.build(in_shape)
    layer.store = ParamStore(layer.specs(), dev, True, seed=3)
    layer.alloc(B, dev, torch.bfloat16, SimpleNamespace(wgrad=torch.empty(WS, dtype=torch.float32, device=dev)))
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B,) + tuple(in_shape), generator=g).to(dev, torch.bfloat16)
    dy = torch.randn((B,) + tuple(layer.out_shape), generator=g).to(dev, torch.bfloat16)
    del log[:]
    layer.forward(x, True)
    dx = layer.backward(dy)
    torch.cuda.synchronize()
    assert torch.isfinite(layer.out.float()).all() and torch.isfinite(dx.float()).all()
    fwd = [c for c in log if c[0] == "igemm_fwd"]
    wg = [c for c in log if c[0] == "igemm_wgrad"]
    assert len(fwd) == 2 and len(wg) == 1, [c[0] for c in log]
    del log[:]
    return fwd, wg[0]


@pytest.mark.parametrize("filters,kernel,strides,in_shape", [(16, 3, 1, (8, 8, 8)), (8, (3, 5), (2, 1), (9, 8, 8))],
                         ids=["regular", "irregular"])
def test_conv2d_launches_and_queries_agree(filters, kernel, strides, in_shape, log):
    B = 2
    l = Conv2D(filters, kernel, strides, "same", "relu", name="c")
    fwd, wg = _run(l, in_shape, B, log)
    assert l.regular == (kernel == 3)
    sizes = (B, *l.in_shape, *l.out_shape)
    ops.conv_plan(*sizes, *l.geom, primary_kpad_of(l))
    ops.conv_plan(*sizes, *l.geom, dgrad_kpad_of(l), dgrad=True)
    ops.wgrad_plan(*sizes, *l.geom, l.use_bias, WS)
    assert [c[0] for c in log] == ["conv_plan", "conv_plan", "wgrad_plan"]
    assert _shapes(fwd[0]) == _shapes(log[0]) and log[0][1][5] == ops.MODE_FWD
    assert _shapes(fwd[1]) == _shapes(log[1]) and log[1][1][5] == ops.MODE_DGRAD
    assert _shapes(wg) == _shapes(log[2])
    assert len(_shapes(wg)[5]) == (9 if l.regular else 11)


def test_conv2d_transpose_launches_and_queries_agree(log):
    B, H, W, Cin, F = 2, 4, 4, 8, 8
    l = Conv2DTranspose(F, 3, 2, "same", "relu", name="t")
    fwd, wg = _run(l, (H, W, Cin), B, log)
    assert l.out_shape == (8, 8, F)
    st = l.store
    plans = ops.deconv_plans(ops.deconv_geometry(B, H, W, Cin, F, (3, 3), (2, 2), "same"), st.weight("t/kernel"),
                             st.weight_t("t/kernel"), has_bias=True, ws_floats=WS)
    assert [c[0] for c in log] == ["conv_plan", "conv_plan", "wgrad_plan"] and set(plans) == {"fwd", "dgrad", "wgrad"}
    assert _shapes(fwd[0]) == _shapes(log[0]) and log[0][1][5] == ops.MODE_DGRAD  # forward: a data-gradient launch
    assert _shapes(fwd[1]) == _shapes(log[1]) and log[1][1][5] == ops.MODE_FWD    # input gradient: a forward launch
    assert _shapes(wg) == _shapes(log[2])
    assert _shapes(log[0])[0] == B * 8 * 8 and _shapes(log[1])[0] == B * H * W


def test_dense_launches_and_query_agree(log):
    B, K, N = 4, 32, 16
    l = Dense(N, "relu", name="d")
    fwd, wg = _run(l, (K,), B, log)
    geom = [1, 1, 1, 1, 1, 1, 1, 1, 0]
    assert _shapes(fwd[0]) == (B, N, K, primary_kpad_of(l), geom, ops.MODE_DIRECT)
    assert _shapes(fwd[1]) == (B, K, N, dgrad_kpad_of(l), geom, ops.MODE_DIRECT)
    ops.dense_wgrad_plan(B, l.in_features, l.units, l.use_bias, WS)
    assert [c[0] for c in log] == ["wgrad_plan"]
    assert _shapes(wg) == _shapes(log[0]) == (B, N, K, N, K, geom, ops.MODE_DIRECT)
