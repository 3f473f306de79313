"""Depthwise conv kernels (csrc/dwconv.hip) exactly: integer data against an fp64 tap-loop reference by
``torch.equal`` (tests/exact_util.py; tests/test_exact_util.py checks the references and the conditions of
exactness of every case without a GPU).  Beyond the shapes of tests/test_depthwise_gpu.py (which keeps the
non-integer data and the rounding paths, at a tolerance) this enters the paths no aligned, small tensor reaches:
the scalar kernels ``vec_ok`` falls back to when an operand is not 16-byte aligned, the grid-stride loops (above
kDwMaxGrid * 256 work items, where a 3x3 lane reloads its weights for another channel vector) and the
kDwMaxSlabs cap of the weight gradient reached through the position count.

x, dy in [-2, 2] and fp32 weights and bias in [-3, 3] hold exact zeros: ``mask > 0`` at mask == 0 and the ReLU of
an exactly zero sum are evaluated.  Every output buffer starts as NaN: an element no thread wrote fails."""
import pytest
import torch

import exact_util as xu
from distriflow_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")

_cache = {}


def _case(case):
    """Data of a case on the device (fp64, the kernels' bf16 / fp32 operands) and its references, computed on the
    device in fp64, once; the conditions of exactness are asserted on them here."""
    if case in _cache:
        return _cache[case]
    d = xu.dw_case(case)
    g = d["geom"]
    c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
    c.update(xd=xu.bf16(d["x"], dev), dyd=xu.bf16(d["dy"], dev), wd=d["w"].float().to(dev), bd=d["b"].float().to(dev))
    for has_b in (False, True):
        pre = xu.dwconv_fwd_ref(c["x"], c["w"], c["b"] if has_b else None, g, False)
        c["y", has_b, False], c["y", has_b, True] = pre, pre.relu()
        xu.assert_exact_output(pre)
    bare = xu.dwconv_dgrad_ref(c["dy"], c["w"], g)
    xu.assert_exact_output(bare)
    c["dx", False], c["dx", True] = bare, xu.join_ref(bare, None, None, c["x"])
    c["gw"], c["gb"], ab = xu.dwconv_wgrad_ref(c["dy"], c["x"], g)
    assert float(ab.max()) < xu.FP32_INT_MAX and float(c["dy"].abs().sum((0, 1, 2)).max()) < xu.FP32_INT_MAX
    fwd, dg, wg, PL = xu.dw_work_items(g)
    print(f"work items: forward {fwd}, data gradient {dg}, weight gradient {wg} at {PL} lanes per slab")
    _cache[case] = c
    return c


def _fwd(c, has_bias, relu, x=None, w=None, bias=None, y=None):
    y = torch.full(c["y", has_bias, relu].shape, NAN, dtype=torch.bfloat16, device=dev) if y is None else y
    b = (c["bd"] if bias is None else bias) if has_bias else None
    ops.dwconv_fwd(c["xd"] if x is None else x, c["wd"] if w is None else w, b, y, c["geom"], relu=relu)
    return y


def _dgrad(c, in_relu, dy=None, w=None, mask=None, dx=None):
    dx = torch.full(c["dx", in_relu].shape, NAN, dtype=torch.bfloat16, device=dev) if dx is None else dx
    m = (c["xd"] if mask is None else mask) if in_relu else None
    ops.dwconv_dgrad(c["dyd"] if dy is None else dy, c["wd"] if w is None else w, dx, c["geom"], mask=m)
    return dx


def _wgrad(c, has_bias, dy=None, x=None, ws=None):
    gw = torch.full(c["gw"].shape, NAN, device=dev)
    gb = torch.full(c["gb"].shape, NAN, device=dev) if has_bias else None
    ws = torch.full((1 << 22,), NAN, device=dev) if ws is None else ws
    ops.dwconv_wgrad(c["dyd"] if dy is None else dy, c["xd"] if x is None else x, gw, gb, ws, c["geom"])
    return gw, gb


def _nan_like_offset(shape, dtype):
    return xu.offset_view(torch.full(shape, NAN, dtype=dtype, device=dev))


def _check_all(c):
    for has_bias in (False, True):
        for relu in (False, True):
            xu.assert_same(_fwd(c, has_bias, relu), c["y", has_bias, relu], f"forward, bias={has_bias} relu={relu}")
    for in_relu in (False, True):
        xu.assert_same(_dgrad(c, in_relu), c["dx", in_relu], f"data gradient, mask={in_relu}")
    for has_bias in (False, True):
        gw, gb = _wgrad(c, has_bias)
        xu.assert_same(gw, c["gw"], f"weight gradient, gb={has_bias}")
        if has_bias:
            xu.assert_same(gb, c["gb"], "bias gradient")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("case", xu.DWCONVS, ids=xu.case_id)
def test_dwconv_fwd_exact(case, has_bias, relu):
    c = _case(case)
    xu.assert_same(_fwd(c, has_bias, relu), c["y", has_bias, relu], "forward")


@pytest.mark.parametrize("in_relu", [False, True])
@pytest.mark.parametrize("case", xu.DWCONVS, ids=xu.case_id)
def test_dwconv_dgrad_exact(case, in_relu):
    c = _case(case)
    xu.assert_same(_dgrad(c, in_relu), c["dx", in_relu], "data gradient")


@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("case", xu.DWCONVS, ids=xu.case_id)
def test_dwconv_wgrad_exact(case, has_bias):
    c = _case(case)
    gw, gb = _wgrad(c, has_bias)
    xu.assert_same(gw, c["gw"], "weight gradient")
    if has_bias:
        xu.assert_same(gb, c["gb"], "bias gradient")


@pytest.mark.parametrize("case", xu.DWCONVS_MISALIGNED, ids=xu.case_id)
def test_dwconv_misaligned_operands_take_the_scalar_kernels(case):
    """One run per operand ``vec_ok`` inspects, with that operand alone one element into a buffer: the launch falls
    back to the scalar kernels and gives the same result."""
    c = _case(case)
    off = xu.offset_view
    for name in ("x", "w", "bias", "y"):
        kw = {"x": dict(x=off(c["xd"])), "w": dict(w=off(c["wd"])), "bias": dict(bias=off(c["bd"])),
              "y": dict(y=_nan_like_offset(c["y", True, True].shape, torch.bfloat16))}[name]
        xu.assert_same(_fwd(c, True, True, **kw), c["y", True, True], f"forward with {name} misaligned")
    for name in ("dy", "w", "mask", "dx"):
        kw = {"dy": dict(dy=off(c["dyd"])), "w": dict(w=off(c["wd"])), "mask": dict(mask=off(c["xd"])),
              "dx": dict(dx=_nan_like_offset(c["dx", True].shape, torch.bfloat16))}[name]
        xu.assert_same(_dgrad(c, True, **kw), c["dx", True], f"data gradient with {name} misaligned")
    for name in ("dy", "x", "ws"):
        kw = {"dy": dict(dy=off(c["dyd"])), "x": dict(x=off(c["xd"])),
              "ws": dict(ws=_nan_like_offset((1 << 20,), torch.float32))}[name]
        gw, gb = _wgrad(c, True, **kw)
        xu.assert_same(gw, c["gw"], f"weight gradient with {name} misaligned")
        xu.assert_same(gb, c["gb"], f"bias gradient with {name} misaligned")


@pytest.mark.parametrize("case", xu.DWCONVS_GRID, ids=xu.case_id)
def test_dwconv_grid_stride_and_slab_cap_exact(case):
    """The smallest shapes whose launches stride their grid or exceed the slab cap (tests/test_exact_util.py asserts
    that they do): every launch, every epilogue."""
    _check_all(_case(case))
    _cache.pop(case)  # the largest tensors of the suite: not kept
