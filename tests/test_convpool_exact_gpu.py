"""csrc/convpool.hip (fused conv + bias + ReLU + 2x2 max-pool: forward, weight gradient, data gradient) against
an fp64 reference by ``torch.equal`` on integer data (tests/exact_util.py), argmax codes and ties included.

Integer data makes a tied window maximum common (and a non-positive one: no gradient), so the tie rule is
exercised on every shape: the first maximum in row-major window order, code = argmax | 4 * (max > 0).  The
backward is fed the REFERENCE's codes, so a wrong code cannot hide from it.

The shapes of ``test_convpool_exact`` come from tests/golden/convpool_cases.json (scripts/convpool_cases.py: one
geometry per distinct value of the three dispatch keys) plus a hand list: the LeNet-5 layers, non-square images,
and two batches large enough that a workgroup stages several images per group and the last group is partial.
"""
import json
import os

import pytest
import torch

import exact_util as xu
from distriflow_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convpool_cases.json")) as _f:
    GENERATED = [(c["B"], c["H"], c["W"], c["C"], c["N"], c["k"], c["pad"]) for c in json.load(_f)["cases"]]

HAND = [  # B, H, W, C, N, k, pad
    (16, 28, 28, 1, 6, 5, 2),     # LeNet conv1 ('same')
    (16, 14, 14, 6, 16, 5, 0),    # LeNet conv2
    (5, 12, 12, 3, 20, 3, 1),     # odd batch, N > 16, partial window tiles
    (3, 10, 10, 16, 8, 3, 0),
    (7, 12, 12, 4, 8, 3, 0),      # data gradient in pair mode with N = 8, partial tiles
    (6, 10, 10, 8, 16, 5, 2),     # data gradient in pair mode, C = 8 fills both column halves
    (3, 8, 12, 3, 6, 3, 1),       # non-square, W > H
    (3, 12, 8, 4, 20, 3, 0),      # non-square, H > W
    # more images than 256 CUs x 8 workgroups: several images per group, a partial last group
    (4100, 10, 10, 3, 8, 3, 0),   # pair mode
    (4100, 14, 14, 6, 16, 5, 0),  # plain mode
]
WS_FLOATS = 1 << 23   # room for one slab per workgroup of the largest case (2048 x 16 x 151 floats)


class Case:
    """Integer data of one geometry and its fp64 reference (on the device); asserts the conditions under which
    every kernel result is exactly representable before anything is compared."""

    def __init__(self, B, H, W, C, N, k, p, x=None):
        assert ops.convpool_supported(H, W, C, k, k, p, N), "not a fused conv+pool geometry"
        self.dims = (B, H, W, C, N, k, p)
        g = xu.gen(3 + B + 3 * H + 5 * W + 7 * C + 11 * N + 13 * k + 17 * p)
        OH, OW = xu.out_hw(H, W, k, 1, p)
        self.pshape = (B, OH // 2, OW // 2, N)
        x = xu.ints(g, (B, H, W, C), -1, 1) if x is None else x.double()
        self.w = xu.sparse_ints(g, (N, k * k * C), -1, 1, xu.weight_density(k * k * C))
        b = xu.ints(g, (N,), -3, 3)
        dp = xu.ints(g, self.pshape, -1, 1)
        self.x, self.dp, self.b = xu.bf16(x, dev), xu.bf16(dp, dev), b.float().to(dev)
        x, w, b, dp = x.to(dev), self.w.to(dev), b.to(dev), dp.to(dev)
        y = xu.conv_fwd_ref(x, w, b, k, 1, p, relu=False)
        xu.assert_exact_output(y)
        m, am = xu.window_argmax(xu.windows(y))
        self.pooled, self.code = m.clamp_min(0), xu.code_convpool(m, am)
        assert (self.code >= 4).any(), "degenerate data: no window passes a gradient"
        self.tied = float(((xu.windows(y) == m.unsqueeze(-1)).sum(-1) > 1).double().mean())
        dconv = xu.unpool_ref(dp, self.code, OH, OW, "convpool")
        self.gw, self.gb, ab = xu.conv_wgrad_ref(dconv, x, k, 1, p)
        assert float(ab.max()) < xu.FP32_INT_MAX and float(dconv.abs().sum((0, 1, 2)).max()) < xu.FP32_INT_MAX
        self.dx = xu.conv_dgrad_ref(dconv, w, (B, H, W, C), k, 1, p)
        xu.assert_exact_output(self.dx)

    def fwd(self, x=None):
        B, H, W, C, N, k, p = self.dims
        out = torch.full(self.pshape, float("nan"), device=dev, dtype=torch.bfloat16)
        code = torch.full(self.pshape, 255, device=dev, dtype=torch.uint8)
        ops.convpool_fwd(self.x if x is None else x, xu.rowpad_w(self.w, k, k, C, H, W, p, dev), self.b, out, code, k, k, p)
        return out, code

    def wgrad(self, x=None, dp=None, code=None, ws_floats=WS_FLOATS):
        B, H, W, C, N, k, p = self.dims
        gw = torch.full((N, k * k * C), float("nan"), device=dev)
        gb = torch.full((N,), float("nan"), device=dev)
        ops.convpool_wgrad(self.x if x is None else x, self.dp if dp is None else dp, self.code if code is None else code,
                           gw, gb, torch.empty(ws_floats, device=dev), k, k, p)
        return gw, gb

    def dgrad(self, dp=None, code=None):
        B, H, W, C, N, k, p = self.dims
        dx = torch.full((B, H, W, C), float("nan"), device=dev, dtype=torch.bfloat16)
        ops.convpool_dgrad(self.dp if dp is None else dp, self.code if code is None else code, self.w.float().to(dev),
                           xu.cp_wt(self.w, k, k, C, H, W, p, dev), dx, k, k, p)
        return dx

    def check_fwd(self, x=None):
        out, code = self.fwd(x)
        assert torch.equal(code, self.code), "argmax codes"
        assert torch.equal(out.double(), self.pooled), "pooled map"

    def check_wgrad(self, **kw):
        gw, gb = self.wgrad(**kw)
        assert torch.equal(gw.double(), self.gw), "weight gradient"
        assert torch.equal(gb.double(), self.gb), "bias gradient"

    def check_dgrad(self, **kw):
        assert torch.equal(self.dgrad(**kw).double(), self.dx), "data gradient"


def _offset(t):
    """The same values as a view that starts one element into a larger buffer (contiguous, misaligned)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 4 != 0
    return v


@pytest.mark.parametrize("B,H,W,C,N,k,p", GENERATED + HAND)
def test_convpool_exact(B, H, W, C, N, k, p):
    """x, dp in {-1, 0, 1}, about 64 non-zero weights in {-1, 1} per reduction, bias in [-3, 3]: the pooled map and
    every code equal the reference; with the reference's codes the weight / bias gradients equal conv_wgrad_ref
    of the unpooled gradient and dx equals conv_dgrad_ref."""
    c = Case(B, H, W, C, N, k, p)
    c.check_fwd()
    c.check_wgrad()
    c.check_dgrad()


def test_convpool_data_has_ties():
    """What makes the tests above a test of the tie rule: a fair share of the reference's windows have a tied
    maximum, and a fair share a non-positive one (no gradient)."""
    c = Case(7, 12, 12, 4, 8, 3, 0)
    assert c.tied > 0.03, c.tied
    assert 0.05 < float((c.code < 4).double().mean()) < 0.95


def test_convpool_wgrad_small_workspace():
    """A workspace of two slabs halves the grid until it fits (8 -> 4 -> 2 workgroups, four images each): the
    same sums; less than one slab is refused."""
    c = Case(8, 12, 12, 3, 20, 3, 1)
    N, Kt = 20, 27 + 1
    c.check_wgrad()
    c.check_wgrad(ws_floats=2 * N * Kt)
    with pytest.raises(RuntimeError):
        c.wgrad(ws_floats=N * Kt - 1)


@pytest.mark.parametrize("H,C,N,k,p", [(28, 1, 6, 5, 2), (12, 3, 6, 3, 1)])
def test_convpool_u8_gather_exact(H, C, N, k, p):
    """The uint8 dataset read through a batch index with repeats (fused gather + cast, scale 1): forward and
    weight gradient equal the reference on the gathered rows."""
    g = xu.gen(H + C)
    data = torch.randint(0, 3, (40, H, H, C), generator=g, dtype=torch.uint8)
    idx = torch.tensor([3, 3, 0, 39, 7, 3, 12, 0, 21])
    c = Case(len(idx), H, H, C, N, k, p, x=data[idx])
    x = ops.GatherRef(data.to(dev), idx.to(dev), 1.0, (H, H, C))
    c.check_fwd(x)
    c.check_wgrad(x=x)


@pytest.mark.parametrize("B,H,W,C,N,k,p", [(5, 12, 12, 4, 8, 3, 0), (6, 10, 10, 8, 16, 5, 2)])
def test_convpool_misaligned_operands(B, H, W, C, N, k, p):
    """Operands that start one element into a buffer.  x: both shapes stage images as 4-element vectors when x
    is aligned, so the view takes the scalar staging, in the forward and the weight gradient.  dp / code: the
    data gradient takes the kernel without the scatter plan; the weight gradient refuses them."""
    c = Case(B, H, W, C, N, k, p)
    assert (W * C) % 4 == 0 and c.x.data_ptr() % 8 == 0
    c.check_fwd()
    c.check_fwd(_offset(c.x))
    c.check_wgrad(x=_offset(c.x))
    c.check_dgrad()
    c.check_dgrad(dp=_offset(c.dp))
    c.check_dgrad(code=_offset(c.code))
    c.check_dgrad(dp=_offset(c.dp), code=_offset(c.code))
    with pytest.raises(RuntimeError):
        c.wgrad(dp=_offset(c.dp))
    with pytest.raises(RuntimeError):
        c.wgrad(code=_offset(c.code))
