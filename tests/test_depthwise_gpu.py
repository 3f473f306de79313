"""Depthwise conv kernels (csrc/dwconv.hip) against the fp32 reference (ops/reference.py: F.conv2d(groups=C)
after the explicit TensorFlow padding, gradients by autograd) on bf16-rounded inputs, and a MobileNet-style
model (DepthwiseConv2D, BatchNormalization, ReLU6, SeparableConv2D) on the GPU engine against the CPU fp32
engine and through the trainer's captured step.

Tolerances.  Forward and data gradient are bf16 outputs of fp32 sums: one bf16 rounding is <= 2^-9 relative,
the bound is 1e-2 * max|ref| (5x the rounding unit).  The weight and bias gradients are fp32 sums of exact
products: per element <= 2e-4 * sum |dy| |x| (the same sum over absolute values); the worst-case sequential
bound is n * 2^-24 = 8.6e-5 for the n = 1445 positions of the largest case.

The same kernels on integer data, exactly (torch.equal against fp64), with misaligned operands and shapes large
enough to stride the grid and to reach the slab cap: tests/test_depthwise_exact_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from distriflow_amd import ops
from distriflow_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

# (B, H, W, C, M, kernel, strides, padding)
CASES = [
    (3, 9, 9, 8, 1, (3, 3), (1, 1), "same"),      # one 8-channel vector, halo on all four sides
    (2, 8, 8, 16, 1, (3, 3), (2, 2), "same"),     # even size: TF pads bottom / right only (total 1)
    (2, 9, 9, 16, 1, (3, 3), (2, 2), "same"),     # odd size: one pixel on each side
    (3, 7, 10, 3, 1, (2, 4), (1, 2), "same"),     # scalar channel path, non-square, asymmetric
    (2, 11, 11, 20, 1, (5, 5), (1, 1), "valid"),  # C > 8 and not a multiple of 8
    (2, 9, 11, 4, 2, (3, 3), (1, 1), "same"),     # depth multiplier
    (1, 1, 1, 8, 1, (3, 3), (1, 1), "same"),      # every tap but the centre is padding
    (5, 17, 17, 72, 1, (3, 3), (1, 1), "same"),   # 1445 positions: several workgroups and slabs, > 8 vectors
    # beyond the listed set: the vector path's generic kernels (not 3x3; row stride 3) and a 3x3 'valid'
    # data gradient (padding 2 - 0 of the flipped walk), 10 rows = two row chunks
    (2, 6, 7, 8, 1, (2, 3), (1, 1), "same"),
    (2, 10, 10, 8, 1, (3, 3), (3, 3), "same"),
    (2, 10, 9, 8, 1, (3, 3), (1, 1), "valid"),
    # more than 256 channels: a weight-gradient slab row wider than the workgroup (3x3 and generic kernels), and
    # more than 2048: a second channel block of 256 vectors
    (1, 5, 5, 512, 1, (3, 3), (1, 1), "same"),
    (1, 4, 5, 320, 1, (2, 3), (1, 1), "same"),
    (1, 3, 3, 2056, 1, (3, 3), (2, 2), "same"),
    (1, 3, 4, 150, 2, (2, 2), (1, 1), "valid"),   # scalar path, C*M = 300 > 256: two channel blocks
]
IDS = [f"{c[0]}x{c[1]}x{c[2]}x{c[3]}m{c[4]}_k{c[5][0]}{c[5][1]}_s{c[6][0]}{c[6][1]}_{c[7]}" for c in CASES]

_cache = {}


def _case(case):
    """Inputs (bf16-rounded, as fp32 on the CPU) and every fp32 reference result of a case, computed once."""
    if case in _cache:
        return _cache[case]
    B, H, W, C, M, k, s, pad = case
    geom = ops.dwconv_geometry(B, H, W, C, M, k, s, pad)
    OH, OW = geom[5], geom[6]
    g = torch.Generator().manual_seed(100 + CASES.index(case))
    r16 = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    x = r16(torch.randn(B, H, W, C, generator=g))
    dy = r16(torch.randn(B, OH, OW, C * M, generator=g))
    w = torch.randn(k[0], k[1], C * M, generator=g) * 0.5
    bias = torch.randn(C * M, generator=g)
    d = dict(geom=geom, x=x, dy=dy, w=w, bias=bias)
    for has_b in (False, True):
        for relu in (False, True):
            d["y", has_b, relu] = ref.dwconv_fwd(x, w, bias if has_b else None, geom, relu)
    for in_relu in (False, True):
        d["dx", in_relu] = ref.dwconv_dgrad(dy, w, geom, x if in_relu else None)
    d["gw"], d["gb"] = ref.dwconv_wgrad(dy, x, geom, True)
    d["gw_abs"], d["gb_abs"] = ref.dwconv_wgrad(dy.abs(), x.abs(), geom, True)
    _cache[case] = d
    return d


def _bf(t):
    return t.to(dev, torch.bfloat16).contiguous()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_fwd(case, has_bias, relu):
    d = _case(case)
    want = d["y", has_bias, relu]
    y = torch.full(want.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    ops.dwconv_fwd(_bf(d["x"]), d["w"].to(dev), d["bias"].to(dev) if has_bias else None, y, d["geom"], relu=relu)
    torch.cuda.synchronize()
    err = float((y.float().cpu() - want).abs().max())
    print(f"fwd max err {err:.3e} bound {1e-2 * float(want.abs().max()):.3e}")
    assert err <= 1e-2 * float(want.abs().max())


@pytest.mark.parametrize("in_relu", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_dgrad(case, in_relu):
    d = _case(case)
    want = d["dx", in_relu]
    dx = torch.full(want.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    ops.dwconv_dgrad(_bf(d["dy"]), d["w"].to(dev), dx, d["geom"], mask=_bf(d["x"]) if in_relu else None)
    torch.cuda.synchronize()
    err = float((dx.float().cpu() - want).abs().max())
    print(f"dgrad max err {err:.3e} bound {1e-2 * float(want.abs().max()):.3e}")
    assert err <= 1e-2 * float(want.abs().max())


def _wgrad(d, has_bias, ws):
    gw = torch.full(d["w"].shape, float("nan"), device=dev)
    gb = torch.full(d["bias"].shape, float("nan"), device=dev) if has_bias else None
    ops.dwconv_wgrad(_bf(d["dy"]), _bf(d["x"]), gw, gb, ws, d["geom"])
    torch.cuda.synchronize()
    return gw, gb


@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_wgrad(case, has_bias):
    d = _case(case)
    ws = torch.full((1 << 22,), float("nan"), device=dev)
    gw, gb = _wgrad(d, has_bias, ws)
    ew = (gw.cpu() - d["gw"]).abs()
    print(f"wgrad max err {float(ew.max()):.3e}, max err / bound {float((ew / (2e-4 * d['gw_abs'] + 1e-30)).max()):.3e}")
    assert bool((ew <= 2e-4 * d["gw_abs"]).all())
    if has_bias:
        eb = (gb.cpu() - d["gb"]).abs()
        assert bool((eb <= 2e-4 * d["gb_abs"]).all())


def test_dwconv_wgrad_is_bitwise_reproducible_and_fits_small_workspaces():
    d = _case(CASES[7])
    ws = torch.zeros(1 << 22, device=dev)
    a = _wgrad(d, True, ws)
    ws.fill_(3.0)  # whatever an earlier launch left in the slabs does not matter
    b = _wgrad(d, True, ws)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a workspace of three slabs: fewer workgroups, same sums within the bound; less than one slab is refused
    slab = 10 * 72
    gw, gb = _wgrad(d, True, torch.zeros(3 * slab + 5, device=dev))
    assert bool(((gw.cpu() - d["gw"]).abs() <= 2e-4 * d["gw_abs"]).all())
    assert bool(((gb.cpu() - d["gb"]).abs() <= 2e-4 * d["gb_abs"]).all())
    with pytest.raises(RuntimeError):
        _wgrad(d, True, torch.zeros(slab - 1, device=dev))


# ---------------------------------------------------------------------------------------------- model level
def _topology():
    """The CPU test's MobileNet-style model, except that the depthwise layer has no bias (as in MobileNet): a
    bias that feeds a training-mode BatchNormalization has an identically zero gradient, so the cosine
    criterion below would compare rounding noise.  The depthwise bias is covered by the kernel cases above."""
    dw = {"kernel_size": [3, 3], "padding": "same"}
    cfgs = [("Conv2D", {"filters": 8, "kernel_size": [3, 3], "padding": "same", "activation": "relu"}),
            ("DepthwiseConv2D", dict(dw, strides=[2, 2], use_bias=False)),  # see _topology's docstring
            ("BatchNormalization", {"momentum": 0.99, "epsilon": 1e-3}),
            ("ReLU", {"max_value": 6.0}),
            ("SeparableConv2D", dict(dw, strides=[1, 1], filters=12, activation="relu")),
            ("GlobalAveragePooling2D", {}),
            ("Dense", {"units": 5, "activation": "softmax"})]
    layers = []
    for i, (cls, cfg) in enumerate(cfgs):
        c = dict(cfg, name=f"l{i}")
        if i == 0:
            c["batch_input_shape"] = [None, 9, 9, 2]
        layers.append({"class_name": cls, "config": c})
    return {"class_name": "Sequential", "config": {"name": "m", "layers": layers}}


def _net(device, seed=9):
    from distriflow_amd.models.keras import layers_from_keras
    from distriflow_amd.models.net import Net

    layers, shape = layers_from_keras(_topology())
    return Net(layers, shape, device=device, seed=seed)


def test_mobilenet_style_model_gpu_matches_cpu_engine():
    g = torch.Generator().manual_seed(4)
    x = torch.rand(32, 9, 9, 2, generator=g)
    y = torch.randint(0, 5, (32,), generator=g)
    cpu, gpu = _net("cpu"), _net("cuda")
    with torch.no_grad():  # the bias starts at zero: make it count
        cpu.store["l4/bias"].copy_(torch.randn(12, generator=g) * 0.1)
    gpu.store.master.copy_(cpu.store.master.to(dev))
    gpu.store.refresh_compute()
    xb = x.to(torch.bfloat16).float()  # the GPU engine computes on bf16 inputs
    st_c = cpu.compute_gradients(xb, y)
    st_g = gpu.compute_gradients(xb.to(dev), y.to(dev)).clone()
    torch.cuda.synchronize()
    g1 = gpu.store.grad.clone()
    print(f"loss cpu {float(st_c[0]):.5f} gpu {float(st_g[0]):.5f}")
    assert abs(float(st_g[0]) - float(st_c[0])) <= 0.02 * abs(float(st_c[0]))
    for s in cpu.store.specs:
        a = cpu.store.gradient(s.name).flatten()
        b = gpu.store.gradient(s.name).flatten().cpu()
        cos = float(F.cosine_similarity(a, b, dim=0))
        print(f"{s.name}: cos {cos:.5f}")
        assert cos > 0.99, (s.name, cos)
    gpu.compute_gradients(xb.to(dev), y.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(gpu.store.grad, g1)


def test_mobilenet_style_model_trains_in_the_captured_step():
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer, epoch_permutations

    g = torch.Generator().manual_seed(7)
    labels = torch.randint(0, 5, (256,), generator=g)
    # class c: its own fixed 9x9x2 pattern plus noise
    patterns = torch.rand(5, 9 * 9 * 2, generator=g)
    data = ((0.7 * patterns[labels] + 0.3 * torch.rand(256, 9 * 9 * 2, generator=g)) * 255).to(torch.uint8)
    net = _net("cuda", seed=1)
    tr = DataParallelTrainer(net, lr=0.05)
    tr.bind_dataset(data.to(dev), labels.to(dev, torch.int32), 32, scale=1.0 / 255.0)
    tr.bind_index_stream(epoch_permutations(256, 32, 30, dev, seed=0))
    losses = [float(tr.step()[0].item()) / 32 for _ in range(30)]
    print("losses", [round(v, 4) for v in losses])
    assert tr.graph_mode == "full", getattr(tr, "capture_error", None)  # no launch allocates or synchronises
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses
