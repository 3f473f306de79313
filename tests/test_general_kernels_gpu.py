"""csrc/act.hip against fp32 PyTorch references of the same ops (bf16-rounded inputs): standalone
activations forward / backward, sigmoid cross-entropy, general max / average pooling; plus a general
Keras model (tanh, same-padded pools, sigmoid output) trained on the GPU engine against the CPU fp32
engine, layer for layer.  Reference: tf.LayersModel generality (/root/reference/src/common/utils.ts:236-244)."""
import pytest
import torch
import torch.nn.functional as F

import exact_util as xu
from distriflow_amd import ops

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

ACTS = ["relu", "relu6", "sigmoid", "tanh", "elu", "selu", "softplus", "softsign", "hard_sigmoid", "swish",
        "exponential", "linear"]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("n", [8 * 1001, 999])
def test_act_fwd_bwd(act, n):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(n, generator=g) * 3).to(torch.bfloat16)
    dy = torch.randn(n, generator=g).to(torch.bfloat16)
    xd, dyd = x.to(dev), dy.to(dev)
    y = torch.empty_like(xd)
    ops.act_fwd(xd, y, act)
    ref = ops._act_ref(ops.ACT_KINDS[act], x.float())
    torch.testing.assert_close(y.float().cpu(), ref, rtol=2e-2, atol=2e-2)
    for in_relu in (False, True):
        dx = torch.empty_like(xd)
        ops.act_bwd(xd, dyd, dx, act, in_relu=in_relu)
        xv = x.float().requires_grad_(True)
        (gr,) = torch.autograd.grad(ops._act_ref(ops.ACT_KINDS[act], xv), xv, dy.float())
        if in_relu:
            gr = gr * (x.float() > 0)
        torch.testing.assert_close(dx.float().cpu(), gr, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("B,C", [(1, 1), (300, 10), (257, 37)])
def test_sigmoid_ce(B, C):
    g = torch.Generator().manual_seed(2)
    z = torch.randn(B, C, generator=g) * 4
    y = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    dl = torch.empty(B, C, dtype=torch.bfloat16, device=dev)
    st = torch.zeros(2, device=dev)
    ops.sigmoid_ce(z.to(dev), y.to(dev), dl, st, grad_scale=1.0 / B)
    t = F.one_hot(y.long(), C).float()
    loss = F.binary_cross_entropy_with_logits(z, t, reduction="sum")
    assert abs(float(st[0]) - loss.item()) <= 1e-4 * abs(loss.item()) + 1e-3
    assert float(st[1]) == float((z.argmax(1) == y.long()).sum())
    torch.testing.assert_close(dl.float().cpu(), (torch.sigmoid(z) - t) / B, rtol=1e-2, atol=1e-4)


@pytest.mark.parametrize("H,C,pool,stride,pad,avg", [
    (28, 32, (2, 2), (2, 2), "same", False),
    (13, 8, (3, 3), (2, 2), "same", False),
    (13, 8, (3, 3), (2, 2), "same", True),
    (12, 5, (3, 3), (1, 1), "valid", True),
    (7, 3, (2, 3), (2, 1), "valid", False),
    (9, 16, (9, 9), (9, 9), "valid", False),  # a global max pool
])
def test_pool2d(H, C, pool, stride, pad, avg):
    g = torch.Generator().manual_seed(3)
    B = 3
    x = torch.randn(B, H, H, C, generator=g).relu().to(torch.bfloat16)
    geom = ops.pool_geometry(B, H, H, C, pool, stride, pad)
    OH, OW = geom[4], geom[5]
    y = torch.empty(B, OH, OW, C, dtype=torch.bfloat16, device=dev)
    ops.pool2d_fwd(x.to(dev), y, geom, avg=avg)
    ref = ops._pool_ref(x.float(), geom, avg)
    torch.testing.assert_close(y.float().cpu(), ref, rtol=1e-2, atol=1e-2)
    dy = torch.randn(B, OH, OW, C, generator=g).to(torch.bfloat16)
    for in_relu in (False, True):
        dx = torch.empty(B, H, H, C, dtype=torch.bfloat16, device=dev)
        ops.pool2d_bwd(x.to(dev), dy.to(dev), dx, geom, avg=avg, in_relu=in_relu)
        xv = x.float().requires_grad_(True)
        (gr,) = torch.autograd.grad(ops._pool_ref(xv, geom, avg), xv, dy.float())
        if in_relu:
            if avg:
                gr = gr * (x.float() > 0)
            else:  # a window whose max is not positive passes nothing
                mx = ops._pool_ref(x.float(), geom, False)
                gr = torch.autograd.grad(ops._pool_ref(xv, geom, False), xv, dy.float() * (mx > 0))[0]
        torch.testing.assert_close(dx.float().cpu(), gr, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("H,C,pool,stride,pad", [
    (13, 8, (3, 3), (2, 2), "same"),     # overlapping windows, clipped at the border
    (7, 3, (2, 3), (2, 1), "valid"),     # overlapping along the row only, scalar channels
    (9, 16, (9, 9), (9, 9), "valid"),    # a global max pool
])
def test_pool2d_max_exact_with_ties(H, C, pool, stride, pad):
    """Integer data (x in [-3, 1], dy in [-3, 3]: exact, most windows tied, and of 9 values at most 1 in 8 windows
    has none positive) against the fp64 reference of tests/exact_util.py: each window sends its gradient to its
    first maximum in row-major order, the gradients of overlapping windows sum per input pixel (at most 9 of
    magnitude 3: exact in bf16); with in_relu a window whose maximum is not positive sends nothing."""
    B = 3
    g = xu.gen(H + C)
    geom = ops.pool_geometry(B, H, H, C, pool, stride, pad)
    OH, OW = geom[4], geom[5]
    x, dy = xu.ints(g, (B, H, H, C), -3, 1), xu.ints(g, (B, OH, OW, C), -3, 3)
    exp, m, _, _ = xu.pool_max_ref(x.to(dev), geom)
    xu.assert_exact_output(exp)
    if pool != (9, 9):
        assert 0.05 < float((m <= 0).double().mean()) < 0.95, "in_relu would not be exercised"
    y = torch.full((B, OH, OW, C), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.pool2d_fwd(xu.bf16(x, dev), y, geom, avg=False)
    assert torch.equal(y.double(), exp), "forward"
    for in_relu in (False, True):
        edx = xu.pool_max_bwd_ref(x.to(dev), dy.to(dev), geom, in_relu)
        xu.assert_exact_output(edx)
        dx = torch.full((B, H, H, C), float("nan"), dtype=torch.bfloat16, device=dev)
        ops.pool2d_bwd(xu.bf16(x, dev), xu.bf16(dy, dev), dx, geom, avg=False, in_relu=in_relu)
        assert torch.equal(dx.double(), edx), f"backward, in_relu={in_relu}"


# ---- csrc/layers.hip: add_act, relu_bwd, gap_fwd, gap_bwd.  One grid-stride pass of these launches is 8192
# workgroups of 256 threads = 2 097 152 work items (8-element vectors for the first two, elements for the GAPs).
PASS = 8192 * 256


def _sentinel_out(n):
    buf = torch.full((n + 64,), 1024.0, dtype=torch.bfloat16, device=dev)
    return buf, buf[:n]


@pytest.mark.parametrize("n8", [1, 1000, PASS, PASS + 3])
def test_add_act_and_relu_bwd_exact(n8):
    """Small integers: a + b and its relu are bf16 values, dy * [y > 0] is a selection -- both exact."""
    n = 8 * n8
    a, b = (torch.randint(-100, 101, (n,), device=dev).to(torch.bfloat16) for _ in range(2))
    for relu in (False, True):
        buf, out = _sentinel_out(n)
        ops.add_act(a, b, out, relu)
        exp = a.float() + b.float()
        assert torch.equal(out.float(), exp.relu() if relu else exp)
        assert (buf[n:] == 1024.0).all()
    buf, dx = _sentinel_out(n)
    ops.relu_bwd(a, b, dx)  # y = a (its sign decides), dy = b
    assert torch.equal(dx, torch.where(a.float() > 0, b, torch.zeros_like(b)))
    assert (buf[n:] == 1024.0).all()


def test_add_act_against_fp64_within_one_bf16_ulp():
    g = torch.Generator().manual_seed(5)
    a, b = (torch.randn(8 * 1001, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    out = torch.empty_like(a)
    ops.add_act(a, b, out, True)
    exp = (a.double() + b.double()).relu()
    assert ((out.double() - exp).abs() <= 2.0 ** -7 * exp.abs()).all()


@pytest.mark.parametrize("op", ["add_act", "relu_bwd"])
def test_add_act_relu_bwd_refuse_a_partial_vector(op):
    a, b = (torch.ones(8 * 5 + 3, dtype=torch.bfloat16, device=dev) for _ in range(2))
    out = torch.full_like(a, 1024.0)
    with pytest.raises(RuntimeError):
        ops.add_act(a, b, out, True) if op == "add_act" else ops.relu_bwd(a, b, out)
    torch.cuda.synchronize()
    assert (out == 1024.0).all()


# B, HW, C: C not a multiple of 8; B * C (forward) and B * HW * C (backward) below, at and above one pass
GAPS = [(3, 16, 5), (1, 1, 1), (7, 49, 37), (4096, 4, 512), (2048, 2, 1025), (4, 64, 8192), (5, 64, 8193)]


@pytest.mark.parametrize("B,HW,C", GAPS)
def test_gap_fwd_bwd(B, HW, C):
    """Integers in [-8, 8]: the fp32 sum over HW is exact, so is the division by a power of two (equal to fp64
    after the bf16 rounding of the quotient); HW = 49: within one bf16 ulp of fp64."""
    g = torch.Generator(device=dev).manual_seed(B + HW + C)
    x = torch.randint(-8, 9, (B, HW, 1, C), device=dev, generator=g).to(torch.bfloat16)
    buf, y = _sentinel_out(B * C)
    ops.gap_fwd(x, y.view(B, C))
    exp = x.double().mean(dim=(1, 2))
    if HW & (HW - 1) == 0:
        assert torch.equal(y.view(B, C).double(), exp.to(torch.bfloat16).double())
    else:
        assert ((y.view(B, C).double() - exp).abs() <= (2.0 ** -7 + 2.0 ** -20) * exp.abs()).all()
    assert (buf[B * C:] == 1024.0).all()
    dy = torch.randint(-8, 9, (B, C), device=dev, generator=g).to(torch.bfloat16)
    buf, dx = _sentinel_out(B * HW * C)
    ops.gap_bwd(dy, dx.view(B, HW, 1, C))
    exp = (dy.double() / HW).view(B, 1, C).expand(B, HW, C)
    if HW & (HW - 1) == 0:
        assert torch.equal(dx.view(B, HW, C).double(), exp)
    else:
        assert ((dx.view(B, HW, C).double() - exp).abs() <= (2.0 ** -7 + 2.0 ** -20) * exp.abs()).all()
    assert (buf[B * HW * C:] == 1024.0).all()


def test_general_keras_model_gpu_matches_cpu_engine():
    from distriflow_amd.models.keras import layers_from_keras
    from distriflow_amd.models.net import Net

    topo = {"class_name": "Sequential", "config": {"name": "g", "layers": [
        {"class_name": "Conv2D", "config": {"name": "c1", "filters": 8, "kernel_size": [3, 3], "activation": "tanh",
                                            "padding": "same", "batch_input_shape": [None, 14, 14, 1]}},
        {"class_name": "MaxPooling2D", "config": {"name": "p1", "pool_size": [3, 3], "strides": [2, 2],
                                                  "padding": "same"}},
        {"class_name": "Conv2D", "config": {"name": "c2", "filters": 16, "kernel_size": [3, 3], "activation": "relu"}},
        {"class_name": "AveragePooling2D", "config": {"name": "p2", "pool_size": [2, 2], "padding": "same"}},
        {"class_name": "Flatten", "config": {"name": "f"}},
        {"class_name": "Dense", "config": {"name": "d1", "units": 32, "activation": "elu"}},
        {"class_name": "Dense", "config": {"name": "d2", "units": 6, "activation": "sigmoid"}}]}}
    g = torch.Generator().manual_seed(4)
    x = torch.rand(64, 14, 14, 1, generator=g)
    y = torch.randint(0, 6, (64,), generator=g)
    nets = {}
    for d in ("cpu", "cuda"):
        layers, shape = layers_from_keras(topo)
        nets[d] = Net(layers, shape, device=d, seed=9)
    nets["cuda"].store.master.copy_(nets["cpu"].store.master.to(dev))
    nets["cuda"].store.refresh_compute()
    xb = x.to(torch.bfloat16).float()  # the GPU engine computes on bf16 inputs
    st_c = nets["cpu"].compute_gradients(xb, y)
    st_g = nets["cuda"].compute_gradients(xb.to(dev), y.to(dev))
    torch.cuda.synchronize()
    assert nets["cuda"].final_act == "sigmoid"
    assert abs(float(st_g[0]) - float(st_c[0])) <= 0.02 * abs(float(st_c[0]))
    for s in nets["cpu"].store.specs:
        a = nets["cpu"].store.gradient(s.name).flatten()
        b = nets["cuda"].store.gradient(s.name).flatten().cpu()
        cos = float(F.cosine_similarity(a, b, dim=0))
        assert cos > 0.99, (s.name, cos)
