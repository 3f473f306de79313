"""Conv2DTranspose exactly: integer data against an fp64 reference by ``torch.equal`` (tests/exact_util.py;
tests/test_exact_util.py checks the references and the conditions of exactness of every case without a GPU).

A transposed conv runs the conv kernels with their roles swapped, in epilogue combinations no conv uses: the forward
is a MODE_DGRAD launch with bias and ReLU (on the igemm64 parity-class path a class without a tap holds the bias
alone), the input gradient a MODE_FWD launch with a relu' mask.  Integer data also holds exact zeros, which random
normals never do: ``mask > 0`` at mask == 0 and the ReLU of an exactly zero sum are evaluated here.
tests/test_decoder_gpu.py keeps the non-integer data and the rounding paths, at a tolerance.

Every output buffer starts as NaN: an element no thread wrote fails the comparison."""
import pytest
import torch

import exact_util as xu
from distriflow_amd import ops
from test_decoder_gpu import SUM_CASES

pytestmark = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")
IDS = [xu.case_id(c) for c in xu.DECONVS]
WS_FLOATS = 1 << 22

_cache = {}


def _case(case):
    """Data of a case on the device: fp64, the kernels' bf16 operands and the two padded weight copies, laid out
    as tests/test_decoder_gpu.py::_case lays them out; built once."""
    if case not in _cache:
        d = xu.deconv_case(case)
        G = d["G"]
        c = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
        c.update(xd=xu.bf16(d["x"], dev), dyd=xu.bf16(d["dy"], dev), bd=d["b"].float().to(dev),
                 wp=xu.pad_w(d["w"], dev), wt=xu.pad_wt(d["w"], G.N, G.KH * G.KW, G.C, dev))
        _cache[case] = c
    return _cache[case]


def _plan(c, which, **kw):
    p = ops.deconv_plans(c["geom"], c["wp"], c["wt"], ws_floats=WS_FLOATS, **kw)[which]
    extra = [n for n in ("par", "fast", "vec") if p.get(n)] + ([f"{p['splits']} splits"] if p.get("splits", 1) > 1 else [])
    print(f"{which}: family {p['family']}" + (f" ({', '.join(extra)})" if extra else ""))
    return p


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("case", xu.DECONVS, ids=IDS)
def test_deconv_fwd_exact(case, has_bias, relu):
    c = _case(case)
    _plan(c, "fwd", has_bias=has_bias)
    exp = xu.deconv_fwd_ref(c["x"], c["w"], c["b"] if has_bias else None, c["geom"], relu)
    xu.assert_exact_output(exp)
    y = torch.full(exp.shape, NAN, dtype=torch.bfloat16, device=dev)
    ops.deconv_fwd(c["xd"], c["wp"], c["wt"], c["bd"] if has_bias else None, y, c["geom"], relu=relu)
    xu.assert_same(y, exp, "forward")


@pytest.mark.parametrize("in_relu", [False, True])
@pytest.mark.parametrize("case", xu.DECONVS, ids=IDS)
def test_deconv_dgrad_exact(case, in_relu):
    c = _case(case)
    _plan(c, "dgrad", has_mask=in_relu)
    exp = xu.deconv_dgrad_ref(c["dy"], c["w"], c["geom"], c["x"] if in_relu else None)
    xu.assert_exact_output(exp)
    dx = torch.full(exp.shape, NAN, dtype=torch.bfloat16, device=dev)
    ops.deconv_dgrad(c["dyd"], c["wp"], dx, c["geom"], mask=c["xd"] if in_relu else None)
    xu.assert_same(dx, exp, "input gradient")


@pytest.mark.parametrize("case", xu.DECONVS, ids=IDS)
def test_deconv_wgrad_exact(case):
    """The kernel gradient with the bias gradient (a channel_sum launch) and without."""
    c = _case(case)
    _plan(c, "wgrad")
    ew, eb, ab = xu.deconv_wgrad_ref(c["dy"], c["x"], c["geom"])
    assert float(ab.max()) < xu.FP32_INT_MAX and float(c["dy"].abs().sum((0, 1, 2)).max()) < xu.FP32_INT_MAX
    for with_gb in (True, False):
        gw = torch.full(ew.shape, NAN, device=dev)
        gb = torch.full(eb.shape, NAN, device=dev) if with_gb else None
        ops.deconv_wgrad(c["dyd"], c["xd"], gw, gb, torch.full((WS_FLOATS,), NAN, device=dev), c["geom"])
        xu.assert_same(gw, ew, f"kernel gradient, gb={with_gb}")
        if with_gb:
            xu.assert_same(gb, eb, "bias gradient")


def test_deconv_cases_reach_every_kernel_family():
    """(launch, family, fast, par, vec) over the list, as planned by the build under test."""
    seen = set()
    for case in xu.DECONVS:
        c = _case(case)
        for flags in (dict(), dict(has_bias=True, has_mask=True)):
            for which, p in ops.deconv_plans(c["geom"], c["wp"], c["wt"], ws_floats=WS_FLOATS, **flags).items():
                seen.add((which, p["family"], bool(p.get("fast")), bool(p.get("par")), bool(p.get("vec"))))
    print(sorted(seen))
    want = {("fwd", "generic", False, False, False), ("fwd", "generic", False, False, True),
            ("fwd", "igemm64", False, False, False), ("fwd", "igemm64", True, False, False),
            ("fwd", "igemm64", True, True, False), ("fwd", "halo", False, False, False),
            ("dgrad", "generic", False, False, False), ("dgrad", "generic", False, False, True),
            ("dgrad", "igemm64", False, False, False), ("dgrad", "igemm64", True, False, False),
            ("dgrad", "halo", False, False, False),
            ("wgrad", "generic", False, False, False), ("wgrad", "tr", False, False, False),
            ("wgrad", "halo", False, False, False)}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("M,C", SUM_CASES)
def test_channel_sum_exact(M, C):
    """fp32 sums of integers in [-2, 2]: exact in any order (2 M < 2^24); once more with dy one element into a
    buffer (the scalar loads) and with scale 0.5."""
    dy = xu.ints(xu.gen(M + C), (M, C), -2, 2)
    exp = dy.to(dev).sum(0)
    assert 2 * M < xu.FP32_INT_MAX
    dyd = xu.bf16(dy, dev)
    for what, src, scale in (("aligned", dyd, 1.0), ("misaligned", xu.offset_view(dyd), 1.0), ("scaled", dyd, 0.5)):
        gb = torch.full((C,), NAN, device=dev)
        ops.channel_sum(src, gb, torch.full((1 << 20,), NAN, device=dev), scale=scale)
        xu.assert_same(gb, scale * exp, f"channel_sum, {what}")
