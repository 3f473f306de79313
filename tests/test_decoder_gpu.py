"""Conv2DTranspose on the conv kernels with their roles swapped, and the up-sampling / channel-sum kernels
(csrc/upsample.hip), against the fp32 reference (ops/reference.py) on bf16-rounded inputs and weights; then a
U-Net-style model (Conv2D stride 2, Conv2DTranspose stride 2, Concatenate skip, bilinear UpSampling2D) on the
GPU engine against the CPU fp32 engine and through the trainer's captured step.

Kernel families (ops.conv_plan / ops.wgrad_plan, printed per launch).  Forward = a MODE_DGRAD launch, input
gradient = a MODE_FWD launch with the relu' mask, kernel gradient = G's weight gradient:
  forward         generic (scalar LUT gather; vector gather), igemm64 (plain; the FAST gather with a bias on the
                  halo shape; the FAST stride-2 parity classes), halo (the 3x3 / 64-channel shape without a bias)
  input gradient  generic (scalar; vector), igemm64, halo -- each with and without the mask
  kernel gradient generic, tr, halo
Every family applied the bias, the ReLU and the mask in its own epilogue: no extra launch was needed.

Tolerances.  The transposed conv runs the conv kernels, so the criterion is theirs (tests/
test_conv_geometry_gpu.py): max error <= 3e-2 * max|ref|.  channel_sum is an fp32 sum of bf16 values: per
channel <= 2e-4 * sum|dy| (tests/test_depthwise_gpu.py).  Up-sampling: nearest forward copies (bitwise); on
small-integer data every fp32 result is a bf16 value (asserted on the reference first), so nearest backward and
bilinear (2, 2) are exact; other sizes have inexact weights and one bf16 rounding (2^-9): 1e-2 * max|ref|.

The transposed conv and channel_sum on integer data, exactly (torch.equal against fp64), over these cases and
more, with a check that every kernel family is reached: tests/test_deconv_exact_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from distriflow_amd import ops
from distriflow_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

# (B, H, W, Cin, F, kernel, strides, padding)
CASES = [
    (2, 5, 5, 8, 8, (3, 3), (2, 2), "same"),     # asymmetric padding, vector gather
    (2, 4, 6, 3, 5, (3, 3), (2, 2), "valid"),    # scalar LUT gather
    (2, 4, 4, 16, 8, (4, 4), (2, 2), "same"),    # regular geometry, igemm64
    (2, 4, 4, 64, 32, (4, 4), (2, 2), "same"),   # the stride-2 parity-class path
    (2, 8, 8, 64, 64, (3, 3), (1, 1), "same"),   # the halo kernel's shape without bias, igemm64 with bias
    (2, 3, 3, 8, 8, (2, 2), (3, 3), "same"),     # bias-only pixels
    (1, 1, 1, 8, 16, (3, 3), (1, 1), "same"),    # 1x1 input
    (2, 5, 4, 8, 8, (5, 3), (1, 2), "same"),     # non-square kernel, per-axis strides
    (2, 7, 7, 8, 1, (3, 3), (2, 2), "same"),     # F = 1: the input gradient is a one-channel conv with a mask
]
IDS = [f"{c[0]}x{c[1]}x{c[2]}x{c[3]}f{c[4]}_k{c[5][0]}{c[5][1]}_s{c[6][0]}{c[6][1]}_{c[7]}" for c in CASES]

_cache = {}


def _r(a, b):
    return -(-a // b) * b


def _close(got, exp, tol=3e-2):  # tests/test_conv_geometry_gpu.py
    err = (got.float().cpu() - exp.float().cpu()).abs().max().item()
    scale = exp.float().abs().max().item() + 1e-6
    print(f"max err {err:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


def _bf(t):
    return t.to(dev, torch.bfloat16).contiguous()


def _case(case):
    """Inputs (bf16-rounded, fp32 on the CPU), the two padded bf16 weight copies as the parameter store lays them
    out, and every fp32 reference result of a case, computed once."""
    if case in _cache:
        return _cache[case]
    B, H, W, Cin, Fo, k, s, pad = case
    geom = ops.deconv_geometry(*case)
    OH, OW = geom[5], geom[6]
    T = k[0] * k[1]
    g = torch.Generator().manual_seed(300 + CASES.index(case))
    r16 = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    x = r16(torch.randn(B, H, W, Cin, generator=g))
    dy = r16(torch.randn(B, OH, OW, Fo, generator=g))
    w = r16(torch.randn(Cin, T * Fo, generator=g) * 0.2)   # G's OHWI matrix [Cin][KH*KW*F]
    bias = torch.randn(Fo, generator=g)
    wp = torch.zeros(_r(Cin, 16), _r(T * Fo, 32))
    wp[:Cin, :T * Fo] = w
    wt = torch.zeros(_r(Fo, 16), _r(T * Cin, 32))           # dgrad copy: (f, t, cin) <- w[cin, t, f]
    wt[:Fo, :T * Cin] = w.reshape(Cin, T, Fo).permute(2, 1, 0).reshape(Fo, T * Cin)
    d = dict(geom=geom, x=x, dy=dy, w=w, bias=bias, wp=_bf(wp), wt=_bf(wt))
    for has_b in (False, True):
        for relu in (False, True):
            d["y", has_b, relu] = ops.deconv_fwd(x, w, None, bias if has_b else None, torch.empty(B, OH, OW, Fo), geom,
                                                 relu=relu)
    for in_relu in (False, True):
        d["dx", in_relu] = ops.deconv_dgrad(dy, w, torch.empty(B, H, W, Cin), geom, mask=x if in_relu else None)
    d["gw"], d["gb"] = torch.empty(Cin, T * Fo), torch.empty(Fo)
    ops.deconv_wgrad(dy, x, d["gw"], d["gb"], None, geom)
    _cache[case] = d
    return d


def _family(d, which, **kw):
    p = ops.deconv_plans(d["geom"], d["wp"], d["wt"], ws_floats=1 << 22, **kw)[which]
    extra = [n for n in ("par", "fast", "vec") if p.get(n)]
    print(f"{which}: family {p['family']}" + (f" ({', '.join(extra)})" if extra else ""))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_deconv_fwd(case, has_bias, relu):
    d = _case(case)
    _family(d, "fwd", has_bias=has_bias)
    want = d["y", has_bias, relu]
    y = torch.full(want.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    ops.deconv_fwd(_bf(d["x"]), d["wp"], d["wt"], d["bias"].to(dev) if has_bias else None, y, d["geom"], relu=relu)
    torch.cuda.synchronize()
    _close(y, want)


def test_deconv_fwd_bias_only_pixels():
    """2x2 kernel at stride 3: every third output row and column is reached by no tap and holds the bias only."""
    d = _case(CASES[5])
    y = torch.full(d["y", True, False].shape, float("nan"), dtype=torch.bfloat16, device=dev)
    ops.deconv_fwd(_bf(d["x"]), d["wp"], d["wt"], d["bias"].to(dev), y, d["geom"])
    torch.cuda.synchronize()
    b16 = d["bias"].to(torch.bfloat16)
    assert torch.equal(y.cpu()[:, 2::3], b16.expand(2, 3, 9, 8)) and torch.equal(y.cpu()[:, :, 2::3], b16.expand(2, 9, 3, 8))


@pytest.mark.parametrize("in_relu", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_deconv_dgrad(case, in_relu):
    d = _case(case)
    _family(d, "dgrad", has_mask=in_relu)
    want = d["dx", in_relu]
    dx = torch.full(want.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    ops.deconv_dgrad(_bf(d["dy"]), d["wp"], dx, d["geom"], mask=_bf(d["x"]) if in_relu else None)
    torch.cuda.synchronize()
    _close(dx, want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_deconv_wgrad(case):
    d = _case(case)
    _family(d, "wgrad")
    gw = torch.full(d["gw"].shape, float("nan"), device=dev)
    gb = torch.full(d["gb"].shape, float("nan"), device=dev)
    ws = torch.full((1 << 22,), float("nan"), device=dev)
    ops.deconv_wgrad(_bf(d["dy"]), _bf(d["x"]), gw, gb, ws, d["geom"])
    torch.cuda.synchronize()
    _close(gw, d["gw"])
    _close(gb, d["gb"])
    gw.fill_(float("nan"))
    ops.deconv_wgrad(_bf(d["dy"]), _bf(d["x"]), gw, None, ws, d["geom"])  # no bias: the kernel gradient alone
    torch.cuda.synchronize()
    _close(gw, d["gw"])


# ------------------------------------------------------------------------------------------------ channel_sum
# (M, C): one 8-channel vector over two slabs; scalar channels; 9 vectors, many slabs; scalar, two channel
# blocks; vector, two channel blocks
SUM_CASES = [(8192, 8), (117, 5), (1445, 72), (300, 300), (40, 2056)]


@pytest.mark.parametrize("M,C", SUM_CASES)
def test_channel_sum(M, C):
    g = torch.Generator().manual_seed(M + C)
    dy = torch.randn(M, C, generator=g).to(torch.bfloat16)
    want = dy.float().sum(0)
    bound = 2e-4 * dy.float().abs().sum(0)
    ws = torch.zeros(1 << 20, device=dev)
    gb = torch.full((C,), float("nan"), device=dev)
    ops.channel_sum(dy.to(dev), gb, ws)
    torch.cuda.synchronize()
    err = (gb.cpu() - want).abs()
    print(f"max err {float(err.max()):.3e}, max err / bound {float((err / (bound + 1e-30)).max()):.3e}")
    assert bool((err <= bound).all())
    # whatever an earlier launch left in the slabs does not matter: the same bits
    ws.fill_(3.0)
    gb2 = torch.full((C,), float("nan"), device=dev)
    ops.channel_sum(dy.to(dev), gb2, ws)
    torch.cuda.synchronize()
    assert torch.equal(gb, gb2)
    # one slab and a scale; less than one slab is refused
    gb3 = torch.full((C,), float("nan"), device=dev)
    ops.channel_sum(dy.to(dev), gb3, torch.zeros(C, device=dev), scale=0.5)
    torch.cuda.synchronize()
    assert bool(((gb3.cpu() - 0.5 * want).abs() <= 0.5 * bound).all())
    with pytest.raises(RuntimeError):
        ops.channel_sum(dy.to(dev), gb3, torch.zeros(C - 1, device=dev))


# ------------------------------------------------------------------------------------------------ up-sampling
UP_SIZES = [(3, 5, 7, 8, (2, 2)), (2, 4, 4, 3, (3, 2)), (1, 1, 1, 16, (2, 2)), (2, 6, 5, 72, (2, 2)),
            (1, 3, 3, 264, (4, 4))]
UP_IDS = [f"{c[0]}x{c[1]}x{c[2]}x{c[3]}_s{c[4][0]}{c[4][1]}" for c in UP_SIZES]


def _up_data(case, integer):
    B, H, W, C, (sh, sw) = case
    g = torch.Generator().manual_seed(17 + UP_SIZES.index(case))
    if integer:
        x = torch.randint(-7, 8, (B, H, W, C), generator=g).float()
        dy = torch.randint(-3, 4, (B, H * sh, W * sw, C), generator=g).float()
    else:
        x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).float()
        dy = torch.randn(B, H * sh, W * sw, C, generator=g).to(torch.bfloat16).float()
    return x, dy


def _up_fwd(x, size, interp, hpc=True):
    B, H, W, C = x.shape
    y = torch.full((B, H * size[0], W * size[1], C), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.upsample2d_fwd(_bf(x), y, size, interp, hpc)
    torch.cuda.synchronize()
    return y.cpu()


def _up_bwd(dy, x, size, interp, hpc=True, masked=False):
    dx = torch.full(x.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    ops.upsample2d_bwd(_bf(dy), dx, size, interp, hpc, mask=_bf(x) if masked else None)
    torch.cuda.synchronize()
    return dx.cpu()


def _is_bf16(t):
    return torch.equal(t.to(torch.bfloat16).float(), t)


@pytest.mark.parametrize("case", UP_SIZES, ids=UP_IDS)
def test_upsample_nearest_forward_is_bitwise_repeat_interleave(case):
    x, _ = _up_data(case, integer=False)
    size = case[4]
    want = x.to(torch.bfloat16).repeat_interleave(size[0], 1).repeat_interleave(size[1], 2)
    assert torch.equal(_up_fwd(x, size, "nearest"), want)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", UP_SIZES, ids=UP_IDS)
def test_upsample_nearest_backward_is_exact_on_integers(case, masked):
    x, dy = _up_data(case, integer=True)
    size = case[4]
    want = ref.upsample2d_bwd(dy, size, False, True, mask=x if masked else None)
    assert _is_bf16(want)  # a condition on the inputs: every fp32 sum is a bf16 value
    got = _up_bwd(dy, x, size, "nearest", masked=masked)
    assert torch.equal(got.float(), want)
    assert torch.equal(got, _up_bwd(dy, x, size, "nearest", masked=masked))  # the same bits again


@pytest.mark.parametrize("hpc", [True, False], ids=["half_pixel", "legacy"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", [c for c in UP_SIZES if c[4] == (2, 2)],
                         ids=[i for c, i in zip(UP_SIZES, UP_IDS) if c[4] == (2, 2)])
def test_upsample_bilinear_2x2_is_exact_on_integers(case, masked, hpc):
    x, dy = _up_data(case, integer=True)
    size = case[4]
    want_y = ref.upsample2d_fwd(x, size, True, hpc)
    want_dx = ref.upsample2d_bwd(dy, size, True, hpc, mask=x if masked else None)
    assert _is_bf16(want_y) and _is_bf16(want_dx)  # conditions on the inputs (weights are multiples of 1/4)
    assert torch.equal(_up_fwd(x, size, "bilinear", hpc).float(), want_y)
    got = _up_bwd(dy, x, size, "bilinear", hpc, masked=masked)
    assert torch.equal(got.float(), want_dx)
    assert torch.equal(got, _up_bwd(dy, x, size, "bilinear", hpc, masked=masked))


@pytest.mark.parametrize("hpc", [True, False], ids=["half_pixel", "legacy"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", UP_SIZES, ids=UP_IDS)
def test_upsample_bilinear_any_size(case, masked, hpc):
    x, dy = _up_data(case, integer=False)
    size = case[4]
    want_y = ref.upsample2d_fwd(x, size, True, hpc)
    if hpc:  # the reference's own index arithmetic against torch's
        ti = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=tuple(float(v) for v in size), mode="bilinear",
                           align_corners=False).permute(0, 2, 3, 1)
        torch.testing.assert_close(want_y, ti)
    _close(_up_fwd(x, size, "bilinear", hpc), want_y, tol=1e-2)
    want_dx = ref.upsample2d_bwd(dy, size, True, hpc, mask=x if masked else None)
    got = _up_bwd(dy, x, size, "bilinear", hpc, masked=masked)
    _close(got, want_dx, tol=1e-2)
    assert torch.equal(got, _up_bwd(dy, x, size, "bilinear", hpc, masked=masked))


# ---------------------------------------------------------------------------------------------- model level
def _topology():
    """tests/test_decoder_cpu.py's U-Net-style model on a 12x12x2 input."""
    def node(cls, name, cfg, ins):
        return {"class_name": cls, "name": name, "config": dict(cfg, name=name),
                "inbound_nodes": [[[i, 0, 0, {}] for i in ins]]}

    conv = {"kernel_size": [3, 3], "padding": "same", "activation": "relu", "filters": 8}
    layers = [{"class_name": "InputLayer", "name": "inp", "inbound_nodes": [],
               "config": {"name": "inp", "batch_input_shape": [None, 12, 12, 2], "dtype": "float32"}},
              node("Conv2D", "enc", conv, ["inp"]),
              node("Conv2D", "down", dict(conv, strides=[2, 2]), ["enc"]),
              node("Conv2DTranspose", "up", dict(conv, strides=[2, 2]), ["down"]),
              node("Concatenate", "cat", {"axis": -1}, ["enc", "up"]),
              node("UpSampling2D", "ups", {"size": [2, 2], "interpolation": "bilinear"}, ["cat"]),
              node("Conv2D", "dec", conv, ["ups"]),
              node("GlobalAveragePooling2D", "gap", {}, ["dec"]),
              node("Dense", "out", {"units": 5, "activation": "softmax"}, ["gap"])]
    return {"class_name": "Model", "config": {"name": "g", "layers": layers, "input_layers": [["inp", 0, 0]],
                                              "output_layers": [["out", 0, 0]]}}


def _net(device, seed=9):
    from distriflow_amd.models.keras import layers_from_keras
    from distriflow_amd.models.net import Net

    layers, shape = layers_from_keras(_topology())
    return Net(layers, shape, device=device, seed=seed)


def test_unet_style_model_gpu_matches_cpu_engine():
    g = torch.Generator().manual_seed(4)
    x = torch.rand(32, 12, 12, 2, generator=g)
    y = torch.randint(0, 5, (32,), generator=g)
    cpu, gpu = _net("cpu"), _net("cuda")
    with torch.no_grad():  # the biases start at zero: make them count
        for n in ("up/bias", "down/bias"):
            cpu.store[n].copy_(torch.randn(8, generator=g) * 0.1)
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


def test_unet_style_model_trains_in_the_captured_step():
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer, epoch_permutations

    g = torch.Generator().manual_seed(7)
    labels = torch.randint(0, 5, (256,), generator=g)
    # class c: channel 0 at brightness c / 4, channel 1 at 1 - c / 4, plus noise.  The head is a global average
    # pool, which discards position: a class signal in the channel means is what thirty steps can learn (the CPU
    # fp32 engine goes from 1.55 to 0.73 on this data at this rate; per-pixel patterns stay at ln 5)
    level = torch.stack([labels / 4.0, 1.0 - labels / 4.0], dim=1)
    image = level.reshape(256, 1, 2).expand(256, 12 * 12, 2).reshape(256, 12 * 12 * 2)
    data = ((0.7 * image + 0.3 * torch.rand(256, 12 * 12 * 2, generator=g)) * 255).to(torch.uint8)
    net = _net("cuda", seed=1)
    tr = DataParallelTrainer(net, lr=0.2)
    tr.bind_dataset(data.to(dev), labels.to(dev, torch.int32), 32, scale=1.0 / 255.0)
    tr.bind_index_stream(epoch_permutations(256, 32, 30, dev, seed=0))
    losses = [float(tr.step()[0].item()) / 32 for _ in range(30)]
    print("losses", [round(v, 4) for v in losses])
    assert tr.graph_mode == "full", getattr(tr, "capture_error", None)  # no launch allocates or synchronises
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses
