"""The generic implicit-GEMM kernels (csrc/igemm.hip) on irregular conv geometry -- non-square kernels, per-axis
strides, asymmetric Keras 'same' -- exactly: integer data against an fp64 reference by ``torch.equal``
(tests/exact_util.py; tests/test_exact_util.py checks the references and the conditions of exactness of every case
without a GPU).  csrc/conv_plan.hip sends every irregular geometry to the generic family, so these are the only
exact tests of its 11-int geometry, its scalar (LUT) and vector gathers and the generic weight gradient;
tests/test_conv_geometry_gpu.py keeps the non-integer data and the rounding paths, at a tolerance.

Every output buffer starts as NaN: an element no thread wrote fails the comparison."""
import pytest
import torch

import exact_util as xu
from distriflow_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")

# the gather (vector: 8 channels per 16-byte load; else the scalar LUT one) of the forward and the data gradient
# on aligned operands, per case of xu.IRREGULAR_CONVS
VEC = [(True, True), (True, True), (False, True), (True, True), (False, True), (True, True), (False, True), (True, True),
       (True, False)]
CASES = list(zip(xu.IRREGULAR_CONVS, VEC))
IDS = [xu.case_id(c) for c in xu.IRREGULAR_CONVS]

_cache = {}


def _case(case):
    """Data of a case on the device (fp64 and the kernels' bf16 operands), built once."""
    if case not in _cache:
        d = xu.conv_case(case)
        g = d["g"]
        assert not g.regular
        T = g.KH * g.KW
        c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
        c.update({k + "d": xu.bf16(d[k], dev) for k in ("x", "dy", "res", "rmask", "mask")})
        c.update(wp=xu.pad_w(d["w"], dev), wt=xu.pad_wt(d["w"], g.N, T, g.C, dev), bd=d["b"].float().to(dev))
        _cache[case] = c
    return _cache[case]


def _plan_fwd(c, dgrad, **flags):
    g = c["g"]
    p = ops._view_plan(g.dgrad(c["wt"].shape[1]) if dgrad else g.fwd(c["wp"].shape[1]), **flags)
    print(f"{'data gradient' if dgrad else 'forward'}: family {p['family']}, {'vector' if p['vec'] else 'LUT'} gather, "
          f"tile {p['BM']}x{p['BN']}, grid {p['grid']}")
    assert p["family"] == "generic"
    return p


def _fwd(c, x, bias, relu):
    g = c["g"]
    out = torch.full(g.y_shape, NAN, device=dev, dtype=torch.bfloat16)
    ops.conv_fwd(x, c["wp"], c["bd"] if bias else None, out, relu=relu, g=g)
    return out


def _dgrad(c, dy, join):
    g = c["g"]
    dx = torch.full(g.x_shape, NAN, device=dev, dtype=torch.bfloat16)
    kw = dict(mask=c["maskd"], residual=c["resd"], residual_mask=c["rmaskd"]) if join else {}
    ops.conv_dgrad(dy, None, c["wt"], dx, g=g, **kw)
    return dx


def _wgrad(c, dy, x, bias, ws):
    g = c["g"]
    gw = torch.full((g.N, g.KH * g.KW * g.C), NAN, device=dev)
    gb = torch.full((g.N,), NAN, device=dev) if bias else None
    ops.conv_wgrad(dy, x, gw, gb, ws, scale=0.5, g=g)
    return gw, gb


def _fwd_refs(c):
    if "fwd_refs" not in c:
        c["fwd_refs"] = {(bias, relu): xu.conv_fwd_ref(c["x"], c["w"], c["b"] if bias else None, c["g"], relu=relu)
                         for bias, relu in ((True, True), (False, False))}
        for v in c["fwd_refs"].values():
            xu.assert_exact_output(v)
    return c["fwd_refs"]


def _dgrad_refs(c):
    if "dgrad_refs" not in c:
        bare = xu.conv_dgrad_ref(c["dy"], c["w"], c["g"].x_shape, c["g"])
        c["dgrad_refs"] = {False: bare, True: xu.join_ref(bare, c["res"], c["rmask"], c["mask"])}
        for v in c["dgrad_refs"].values():
            xu.assert_exact_output(v)
    return c["dgrad_refs"]


def _wgrad_refs(c):
    if "wgrad_refs" not in c:
        ew, eb, ab = xu.conv_wgrad_ref(c["dy"], c["x"], c["g"])
        assert float(ab.max()) < xu.FP32_INT_MAX and float(c["dy"].abs().sum((0, 1, 2)).max()) < xu.FP32_INT_MAX
        c["wgrad_refs"] = (0.5 * ew, 0.5 * eb)
    return c["wgrad_refs"]


@pytest.mark.parametrize("case,vec", CASES, ids=IDS)
def test_irregular_conv_fwd_exact(case, vec):
    """With bias + ReLU, and bare."""
    c = _case(case)
    assert _plan_fwd(c, False, has_bias=True)["vec"] == vec[0]
    for (bias, relu), exp in _fwd_refs(c).items():
        xu.assert_same(_fwd(c, c["xd"], bias, relu), exp, f"forward, bias={bias} relu={relu}")


@pytest.mark.parametrize("case,vec", CASES, ids=IDS)
def test_irregular_conv_dgrad_exact(case, vec):
    """With mask + residual + residual mask, and bare; pixels no window reads get exactly 0."""
    c = _case(case)
    assert _plan_fwd(c, True, has_mask=True, has_res=True)["vec"] == vec[1]
    for join, exp in _dgrad_refs(c).items():
        xu.assert_same(_dgrad(c, c["dyd"], join), exp, f"data gradient, join={join}")


@pytest.mark.parametrize("case,vec", CASES, ids=IDS)
def test_irregular_conv_wgrad_exact(case, vec):
    """Scale 0.5, with and without the bias gradient, in exactly the workspace the plan wants (the launch fills
    that and nothing past it); a case with splits once more in a workspace of exactly one slab."""
    c = _case(case)
    g = c["g"]
    ew, eb = _wgrad_refs(c)
    for bias in (True, False):
        p = ops._view_wgrad_plan(g.wgrad(), bias, 1 << 24)
        print(f"weight gradient, bias={bias}: family {p['family']}, dvec {p['dvec']} xvec {p['xvec']}, "
              f"{p['splits']} splits, {p['scratch_floats']} scratch floats")
        assert p["family"] == "generic" and not p["capped"]
        assert p["dvec"] == (g.N % 8 == 0) and p["xvec"] == (g.C % 8 == 0)
        ws = torch.full((p["scratch_floats"] + 4096,), NAN, device=dev)
        gw, gb = _wgrad(c, c["dyd"], c["xd"], bias, ws)
        xu.assert_same(gw, ew, f"weight gradient, bias={bias}")
        if bias:
            xu.assert_same(gb, eb, "bias gradient")
        assert torch.isnan(ws[p["scratch_floats"]:]).all(), "wrote past the plan's scratch"
        assert not torch.isnan(ws[:p["scratch_floats"]]).any(), "left some of the plan's scratch unwritten"
        if p["splits"] > 1:
            slab = g.N * (g.KH * g.KW * g.C + (1 if bias else 0))
            assert p["scratch_floats"] == p["splits"] * slab
            one = ops._view_wgrad_plan(g.wgrad(), bias, slab)
            assert one["family"] == "generic" and one["splits"] == 1 and one["capped"]
            gw, gb = _wgrad(c, c["dyd"], c["xd"], bias, torch.full((slab,), NAN, device=dev))
            xu.assert_same(gw, ew, f"weight gradient in one slab, bias={bias}")
            if bias:
                xu.assert_same(gb, eb, "bias gradient in one slab")


def test_irregular_cases_reach_every_generic_path():
    """Both gathers in both directions, dvec / xvec on and off, and a split weight gradient are all in the list."""
    seen = set()
    for case, _ in CASES:
        c = _case(case)
        g = c["g"]
        seen.add(("fwd", ops._view_plan(g.fwd(c["wp"].shape[1]), has_bias=True)["vec"]))
        seen.add(("dgrad", ops._view_plan(g.dgrad(c["wt"].shape[1]), has_mask=True, has_res=True)["vec"]))
        p = ops._view_wgrad_plan(g.wgrad(), True, 1 << 24)
        seen |= {("dvec", p["dvec"]), ("xvec", p["xvec"]), ("split", p["splits"] > 1)}
    assert seen == {(k, v) for k in ("fwd", "dgrad", "dvec", "xvec", "split") for v in (False, True)}


@pytest.mark.parametrize("case", [xu.IRREGULAR_CONVS[0], xu.IRREGULAR_CONVS[5]], ids=[IDS[0], IDS[5]])
def test_irregular_conv_misaligned_operands(case):
    """C = 8 and C = 24 with x, then dy, one element into a buffer: the gather of the launch that reads the
    operand and the weight gradient's xvec / dvec loads take their scalar forms; the same results."""
    c = _case(case)
    xo, dyo = xu.offset_view(c["xd"]), xu.offset_view(c["dyd"])
    for (bias, relu), exp in _fwd_refs(c).items():
        xu.assert_same(_fwd(c, xo, bias, relu), exp, f"forward of a misaligned x, bias={bias} relu={relu}")
    for join, exp in _dgrad_refs(c).items():
        xu.assert_same(_dgrad(c, dyo, join), exp, f"data gradient of a misaligned dy, join={join}")
    ew, eb = _wgrad_refs(c)
    for what, dy, x in (("x", c["dyd"], xo), ("dy", dyo, c["xd"])):
        for bias in (True, False):
            gw, gb = _wgrad(c, dy, x, bias, torch.full((1 << 20,), NAN, device=dev))
            xu.assert_same(gw, ew, f"weight gradient of a misaligned {what}, bias={bias}")
            if bias:
                xu.assert_same(gb, eb, f"bias gradient of a misaligned {what}")
