"""The fused training-loss kernel (csrc/loss.hip) on the GPU against the fp64 autograd oracle of
tests/loss_oracle.py: every lossesMap kind x output activation x target form over the shapes at which the kernel
changes path, padded leading dimensions, the label clamp, the optional outputs, and an exact comparison on
integer data that pins sign(0) = 0, the strict hinge branch and the Huber seam."""
import pytest
import torch

import exact_util as xu
import loss_oracle as lo
from distriflow_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"


def _run(kind, act, c, gs, dlogits=True, stats=True):
    B, C = c.z.shape
    dl = torch.full((B, C), 7.0, dtype=torch.bfloat16, device=dev) if dlogits else None
    st = torch.zeros(2, device=dev) if stats else None
    ops.loss_grad(c.z.to(dev), c.table.to(dev), kind, act, dl, st, gs, idx=None if c.idx is None else c.idx.to(dev))
    torch.cuda.synchronize()
    return dl, st


@pytest.mark.parametrize("form", lo.FORMS)
@pytest.mark.parametrize("act", lo.ACTS)
@pytest.mark.parametrize("kind", lo.KINDS)
def test_loss_grad_matches_oracle(kind, act, form):
    gs = 0.37
    for B, C in lo.SHAPES:
        if act == "softmax" and C == 1:
            continue  # p == 1 and every gradient is 0: test_softmax_single_class_is_zero
        c = lo.Case(kind, act, form, B, C)
        dl, st = _run(kind, act, c, gs)
        lo.check(kind, act, c, dl, st, gs, what=f"{kind}/{act}/{form} B={B} C={C}")


@pytest.mark.parametrize("kind", lo.KINDS)
def test_softmax_single_class_is_zero(kind):
    z = torch.tensor([[0.3], [-2.0], [4.0]], device=dev)
    for target in (torch.zeros(3, dtype=torch.int32, device=dev), torch.rand(3, 1, device=dev)):
        dl = torch.full((3, 1), 7.0, dtype=torch.bfloat16, device=dev)
        ops.loss_grad(z, target, kind, "softmax", dl, None, 1.0)
        assert torch.equal(dl.float().cpu(), torch.zeros(3, 1))


@pytest.mark.parametrize("B,C", [(257, 10), (5, 33)])
@pytest.mark.parametrize("padded", ["ldl", "ldt", "ldg"])
def test_padded_leading_dimensions(padded, B, C):
    """One of logits / targets / dlogits is a column slice of a wider buffer whose padding holds a sentinel: the
    kernel reads and writes the C columns of a row only."""
    kind, act, gs = "huberLoss", "softmax", 0.5
    c = lo.Case(kind, act, "dense_idx", B, C, seed=3)
    ld = C + 7

    def wide(t, fill, dtype):
        buf = torch.full((t.shape[0], ld), fill, dtype=dtype, device=dev)
        buf[:, :C] = t.to(dev)
        return buf

    zb = wide(c.z, 1e30, torch.float32) if padded == "ldl" else c.z.to(dev)
    tb = wide(c.table, -1e30, torch.float32) if padded == "ldt" else c.table.to(dev)
    gb = torch.full((B, ld if padded == "ldg" else C), -5.0, dtype=torch.bfloat16, device=dev)
    st = torch.zeros(2, device=dev)
    ops.loss_grad(zb[:, :C], tb[:, :C], kind, act, gb[:, :C] if padded == "ldg" else gb, st, gs, idx=c.idx.to(dev))
    torch.cuda.synchronize()
    lo.check(kind, act, c, gb[:, :C], st, gs, what=padded)
    if padded == "ldg":
        assert bool((gb[:, C:] == -5.0).all()), "dlogits padding was written"
    if padded == "ldl":
        assert bool((zb[:, C:] == 1e30).all())
    if padded == "ldt":
        assert bool((tb[:, C:] == -1e30).all())


@pytest.mark.parametrize("B,C", [(9, 5), (6, 40)])
def test_labels_outside_the_row_are_clamped(B, C):
    c = lo.Case("meanSquaredError", "sigmoid", "labels", B, C, out_of_range_labels=True)
    assert int(c.table.max()) >= C and int(c.table.min()) < 0
    dl, st = _run("meanSquaredError", "sigmoid", c, 1.0)
    lo.check("meanSquaredError", "sigmoid", c, dl, st, 1.0)


@pytest.mark.parametrize("B,C", [(9, 5), (6, 40)])
def test_labels_through_idx(B, C):
    c = lo.Case("logLoss", "softmax", "labels", B, C)
    idx = torch.tensor([(3 * i + 1) % B for i in range(B)])
    idx[-1] = idx[0]
    full = c.ref_class.clone()
    c.idx, c.ref_class = idx, full[idx]
    c.t = torch.nn.functional.one_hot(c.ref_class, C).double()
    dl, st = _run("logLoss", "softmax", c, 0.25)
    lo.check("logLoss", "softmax", c, dl, st, 0.25)


@pytest.mark.parametrize("B,C", [(257, 10), (5, 65)])
def test_optional_outputs(B, C):
    kind, act = "sigmoidCrossEntropy", "linear"
    c = lo.Case(kind, act, "dense", B, C)
    dl, _ = _run(kind, act, c, 0.5, stats=False)
    lo.check(kind, act, c, dl, None, 0.5)
    _, st = _run(kind, act, c, 0.5, dlogits=False)
    lo.check(kind, act, c, None, st, 0.5)


@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("kind", ["meanSquaredError", "absoluteDifference", "hingeLoss", "huberLoss"])
def test_exact_on_integer_data(kind, C):
    """Linear output, integer z and t in [-4, 4], grad_scale 2^-3, C a power of two: every gradient is a dyadic
    bf16 value, compared with torch.equal against the closed forms.  Ties included: z == t (sign(0) = 0),
    (2t - 1) z == 1 (the strict hinge branch passes nothing) and |z - t| == 1 (the Huber seam)."""
    g = xu.gen(17 + C)
    B, gs = 37, 2.0 ** -3
    z, t = xu.ints(g, (B, C), -4, 4), xu.ints(g, (B, C), -4, 4)
    z[0, :3], t[0, :3] = torch.tensor([2.0, 1.0, -1.0]), torch.tensor([2.0, 1.0, 0.0])  # d == 0; s z == 1 twice
    z[1, :2], t[1, :2] = torch.tensor([3.0, -2.0]), torch.tensor([2.0, -1.0])           # |d| == 1
    z[2], t[2] = 1.0, 3.0                                                               # every maximum ties
    d, s = z - t, 2 * t - 1
    assert bool((d == 0).any()) and bool((s * z == 1).any()) and bool((d.abs() == 1).any())
    if kind == "meanSquaredError":
        grad, L = 2 * d / C, (d * d).mean(1)
    elif kind == "absoluteDifference":
        grad, L = torch.sign(d) / C, d.abs().mean(1)
    elif kind == "hingeLoss":
        grad, L = torch.where(1 - s * z > 0, -s, torch.zeros_like(s)) / C, torch.relu(1 - s * z).mean(1)
    else:
        grad = torch.where(d.abs() <= 1, d, torch.sign(d)) / C
        L = torch.where(d.abs() <= 1, 0.5 * d * d, d.abs() - 0.5).mean(1)
    want = (gs * grad).to(torch.bfloat16)
    assert torch.equal(want.double(), gs * grad), "the reference gradient is not a bf16 value"
    dl = torch.full((B, C), 7.0, dtype=torch.bfloat16, device=dev)
    st = torch.zeros(2, device=dev)
    ops.loss_grad(z.float().to(dev), t.float().to(dev), kind, "linear", dl, st, gs)
    torch.cuda.synchronize()
    assert torch.equal(dl.cpu(), want)
    assert float(st[0]) == float(L.sum())  # sums of dyadic values: exact in fp32 in any order
    assert float(st[1]) == float((lo.first_argmax(z) == lo.first_argmax(t)).sum())
