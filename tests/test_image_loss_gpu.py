"""The fused per-pixel loss kernel (csrc/loss_image.hip) on the GPU against the fp64 autograd oracle of
tests/loss_oracle.py (its ``loss64`` / ``act64`` on the [B, E] view of the output map), then exactly on integer
data, then a small autoencoder with a skip connection through the engine, the trainer's captured step and
EngineModel.

Tolerances are the project's own (loss_oracle.check): gradients rtol 1e-2 / atol 1e-4, applied to dz * E against
oracle * E so that the absolute term keeps its meaning for per-element gradients of order 1 (a mean over E
elements scales every gradient by 1/E); the loss sum 1e-3 * |ref| + 1e-3.

Inputs: z is rounded to bf16 first, then moved off the kinks of absoluteDifference (p == t) and hingeLoss
((2t - 1) p == 1) one bf16-exact step at a time, re-rounded after every move; ``_Case`` asserts on the CPU that
every element ends at least ``loss_oracle.MARGIN`` from a kink, so no element is ever excluded from a comparison.
|z| <= 4 keeps a sigmoid output away from saturation, where no move of z could clear a kink."""
import pytest
import torch
import torch.nn.functional as F

import exact_util as xu
import loss_oracle as lo
from distriflow_amd import ops

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

KINDS = lo.KINDS[:6]  # the mean kinds
ACTS = ["linear", "sigmoid"]
FORMS = ["f32", "f32_idx", "u8_idx"]
STEP = 2.0 ** -5      # a bf16-exact move for |z| <= 4 (spacing <= 2^-6)


def _shapes():
    """(B, E): one element; the scalar path with a tail; E = 49; the vector path exact; a partial wave; an image
    that spans two workgroups on the vector and on the scalar path (from the plan, so they follow its constant);
    more images than a 16-bit grid axis holds."""
    P = ops.image_loss_plan(1, 8)["elems_per_wg"]
    return [(1, 1), (3, 27), (3, 49), (2, 128), (2, 200), (2, P + 8), (2, P + 3), (65537, 1)]


def _margin(kind, t, p):
    return (p - t).abs() if kind == "absoluteDifference" else (1.0 - (2.0 * t - 1.0) * p).abs()


class _Case:
    """Inputs of one image_loss_grad call, on the CPU: ``z`` [B][E] of bf16 values (fp32), the target ``table``
    (fp32 [N][E], or uint8 with ``scale``), ``idx`` (or None: N == B) and the rows the call sees, float64 ``t``."""

    def __init__(self, kind, act, form, B, E, seed=0):
        g = xu.gen(7000 * seed + 131 * B + E + 17 * KINDS.index(kind))
        unit = kind == "logLoss" and act == "linear"  # a probability is expected
        z = torch.rand(B, E, generator=g) * 0.9 + 0.05 if unit else (1.5 * torch.randn(B, E, generator=g)).clamp(-4, 4)
        z = z.to(torch.bfloat16).float()
        N = B if form == "f32" else B + 3
        self.idx, self.scale = None, 1.0
        if form != "f32":  # out of order, with repeats
            self.idx = torch.randint(0, N, (B,), generator=g)
            if B > 1:
                self.idx[-1] = self.idx[0]
        if form == "u8_idx":
            self.table = torch.randint(0, 256, (N, E), generator=g, dtype=torch.uint8)
            self.scale = 1.0 / 255.0
            # what the kernel computes: fp32(u8) * fp32(scale)
            full = (self.table.float() * torch.tensor(self.scale, dtype=torch.float32)).double()
        else:
            self.table = torch.rand(N, E, generator=g)
            full = self.table.double()
        self.t = full[self.idx] if self.idx is not None else full
        if kind in ("absoluteDifference", "hingeLoss"):
            for _ in range(64):  # towards zero: it also leaves the flat ends of a sigmoid
                bad = _margin(kind, self.t, lo.act64(z.double(), act)) < 2 * lo.MARGIN
                if not bool(bad.any()):
                    break
                z = torch.where(bad, z + torch.where(z > 0, -STEP, STEP), z).to(torch.bfloat16).float()
            m = float(_margin(kind, self.t, lo.act64(z.double(), act)).min())
            assert m >= lo.MARGIN, f"an element is {m:.2e} from a kink of {kind}"
        assert torch.equal(z.to(torch.bfloat16).float(), z)
        self.z = z


def _oracle(kind, act, c, gs):
    """-> (gs * dL/dz [B][E], sum of the per-example loss), float64: autograd through loss_oracle's formulas."""
    zz = c.z.double().clone().requires_grad_(True)
    L = lo.loss64(kind, c.t, lo.act64(zz, act))
    (g,) = torch.autograd.grad(L.sum(), zz)
    return gs * g, float(L.detach().sum())


def _ws(B, E):
    return torch.full((ops.image_loss_workspace_floats(B, E),), float("nan"), device=dev)


def _run(kind, act, c, gs, want_dz=True, want_stats=True):
    B, E = c.z.shape
    dz = torch.full((B, E), 7.0, dtype=torch.bfloat16, device=dev) if want_dz else None
    st = torch.zeros(2, device=dev) if want_stats else None
    ops.image_loss_grad(c.z.to(dev, torch.bfloat16), c.table.to(dev), kind, act, dz, st, gs,
                        idx=None if c.idx is None else c.idx.to(dev), target_scale=c.scale, workspace=_ws(B, E))
    torch.cuda.synchronize()
    return dz, st


def _check(kind, act, c, dz, st, gs, what=""):
    E = c.z.shape[1]
    ed, el = _oracle(kind, act, c, gs)
    if dz is not None:
        got = dz.double().cpu() * E
        print(f"{what}: max |dz - ref| * E = {float((got - ed * E).abs().max()):.3e}")
        torch.testing.assert_close(got, ed * E, rtol=1e-2, atol=1e-4, msg=lambda m: f"{what} dz: {m}")
    if st is not None:
        got_l = float(st[0])
        print(f"{what}: loss sum {got_l!r} vs {el!r}")
        assert abs(got_l - el) <= 1e-3 * abs(el) + 1e-3, f"{what} loss sum {got_l} vs {el}"
        assert float(st[1]) == 0.0


def test_the_case_preparation_clears_every_kink():
    """On the CPU: the assertion inside ``_Case`` holds for every case the oracle test lists."""
    for kind in ("absoluteDifference", "hingeLoss"):
        for act in ACTS:
            for form in FORMS:
                for B, E in _shapes():
                    _Case(kind, act, form, B, E)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", KINDS)
def test_image_loss_matches_oracle(kind, act, form):
    gs = 0.37
    for B, E in _shapes():
        c = _Case(kind, act, form, B, E)
        dz, st = _run(kind, act, c, gs)
        _check(kind, act, c, dz, st, gs, what=f"{kind}/{act}/{form} B={B} E={E}")


def test_plan_paths():
    P = ops.image_loss_plan(1, 8)["elems_per_wg"]
    assert ops.image_loss_plan(2, 128)["vec"] and not ops.image_loss_plan(2, 128, aligned=False)["vec"]
    assert not ops.image_loss_plan(3, 27)["vec"]
    for E in (P + 8, P + 3):
        p = ops.image_loss_plan(2, E)
        assert p["wgs_per_image"] == 2 and p["grid"] == 4 and p["ws_floats"] == 4 and p["vec"] == (E % 8 == 0)
    p = ops.image_loss_plan(65537, 1)
    assert p["ok"] and p["grid"] == 65537
    assert not ops.image_loss_plan(1 << 30, 2 * P + 1)["ok"]  # the workgroup index would not fit


@pytest.mark.parametrize("which", ["u8_offset3", "f32_odd", "dz_odd"])
def test_misaligned_tables_take_the_scalar_path_and_guards_stay(which):
    """E % 8 == 0 but one base pointer is off its alignment: the launcher falls back to the scalar path and the
    results are right; sentinel-filled guard regions around dz and around the workspace are untouched."""
    kind, act, gs, B, E = "huberLoss", "sigmoid", 0.5, 3, 128
    form = "u8_idx" if which == "u8_offset3" else "f32_idx"
    c = _Case(kind, act, form, B, E, seed=2)
    N = c.table.shape[0]
    off = {"u8_offset3": 3, "f32_odd": 1, "dz_odd": 0}[which]
    store = torch.zeros(N * E + 16, dtype=c.table.dtype, device=dev)
    tab = store[off:off + N * E].view(N, E)
    tab.copy_(c.table.to(dev))
    assert tab.is_contiguous() and tab.storage_offset() == off
    G = 64
    d0 = G + (1 if which == "dz_odd" else 0)
    dzbuf = torch.full((G + B * E + G + 8,), -5.0, dtype=torch.bfloat16, device=dev)
    dz = dzbuf[d0:d0 + B * E].view(B, E)
    assert (dz.data_ptr() % 16 != 0) == (which == "dz_odd")
    assert (tab.data_ptr() % (16 if tab.dtype == torch.float32 else 8) != 0) == (which != "dz_odd")
    nws = ops.image_loss_workspace_floats(B, E)
    wsbuf = torch.full((G + nws + G,), -9.0, device=dev)
    st = torch.zeros(2, device=dev)
    ops.image_loss_grad(c.z.to(dev, torch.bfloat16), tab, kind, act, dz, st, gs, idx=c.idx.to(dev),
                        target_scale=c.scale, workspace=wsbuf[G:G + nws])
    torch.cuda.synchronize()
    _check(kind, act, c, dz, st, gs, what=which)
    assert bool((dzbuf[:d0] == -5.0).all()) and bool((dzbuf[d0 + B * E:] == -5.0).all()), "dz guard written"
    assert bool((wsbuf[:G] == -9.0).all()) and bool((wsbuf[G + nws:] == -9.0).all()), "workspace guard written"


@pytest.mark.parametrize("form", ["f32_idx", "u8_idx"])
def test_indices_outside_the_table_are_clamped(form):
    kind, act, gs, B, E = "meanSquaredError", "linear", 1.0, 4, 200
    c = _Case(kind, act, form, B, E, seed=3)
    N = c.table.shape[0]
    idx = torch.tensor([-4, N + 9, 1, N - 1])
    z, tab = c.z.to(dev, torch.bfloat16), c.table.to(dev)

    def run(ix):
        dz = torch.full((B, E), 7.0, dtype=torch.bfloat16, device=dev)
        st = torch.zeros(2, device=dev)
        ops.image_loss_grad(z, tab, kind, act, dz, st, gs, idx=ix.to(dev), target_scale=c.scale, workspace=_ws(B, E))
        torch.cuda.synchronize()
        return dz, st

    dz_a, st_a = run(idx)
    dz_b, st_b = run(idx.clamp(0, N - 1))
    assert torch.equal(dz_a, dz_b) and torch.equal(st_a, st_b)
    c.idx = idx.clamp(0, N - 1)
    full = (c.table.float() * torch.tensor(c.scale, dtype=torch.float32)).double() if form == "u8_idx" else c.table.double()
    c.t = full[c.idx]
    _check(kind, act, c, dz_a, st_a, gs, what="clamped idx")


@pytest.mark.parametrize("B,E", [(37, 64), (3, 4096)])
@pytest.mark.parametrize("kind", ["meanSquaredError", "absoluteDifference", "huberLoss"])
def test_exact_on_integer_data(kind, B, E):
    """Linear output, integer z in [-4, 4], uint8 targets in [0, 6] with target_scale 1, E and 1 / grad_scale powers
    of two: dz and stats[0] equal the integer arithmetic bit for bit.  d == 0 (sign(0) = 0), |d| == 1 (the Huber
    seam) and |d| > 1 all occur; (3, 4096) spans two workgroups per image."""
    g = xu.gen(23 + E)
    gs = 2.0 ** -3
    z = xu.ints(g, (B, E), -4, 4)
    t8 = torch.randint(0, 7, (B, E), generator=g, dtype=torch.uint8)
    z[0, :4] = torch.tensor([2.0, 3.0, -1.0, 4.0], dtype=torch.float64)
    t8[0, :4] = torch.tensor([2, 2, 0, 0], dtype=torch.uint8)  # d = 0, 1, -1, 4
    t = t8.double()
    d = z - t
    assert bool((d == 0).any()) and bool((d.abs() == 1).any()) and bool((d.abs() > 1).any())
    if kind == "meanSquaredError":
        grad, L = 2 * d / E, (d * d).mean(1)
    elif kind == "absoluteDifference":
        grad, L = torch.sign(d) / E, d.abs().mean(1)
    else:
        grad = torch.where(d.abs() <= 1, d, torch.sign(d)) / E
        L = torch.where(d.abs() <= 1, 0.5 * d * d, d.abs() - 0.5).mean(1)
    want = (gs * grad).to(torch.bfloat16)
    assert torch.equal(want.double(), gs * grad), "the reference gradient is not a bf16 value"
    Lsum = L.sum()
    assert float(torch.tensor(float(Lsum), dtype=torch.float32)) == float(Lsum), "the loss sum is not an fp32 value"
    assert float((d * d).sum()) < 2 ** 23  # every partial sum of dyadic terms stays exact in fp32, in any order
    dz = torch.full((B, E), 7.0, dtype=torch.bfloat16, device=dev)
    st = torch.zeros(2, device=dev)
    ops.image_loss_grad(xu.bf16(z, dev), t8.to(dev), kind, "linear", dz, st, gs, target_scale=1.0, workspace=_ws(B, E))
    torch.cuda.synchronize()
    assert torch.equal(dz.cpu(), want)
    assert float(st[0]) == float(Lsum)
    assert float(st[1]) == 0.0


def test_out_relu_masks_the_gradient_exactly():
    """A model that ends in a fused ReLU: dz is the linear-output gradient where z > 0 and 0 elsewhere."""
    g = xu.gen(5)
    B, E, gs = 3, 72, 0.25
    z = torch.relu(xu.ints(g, (B, E), -3, 4))
    t8 = torch.randint(0, 5, (B, E), generator=g, dtype=torch.uint8)
    args = (xu.bf16(z, dev), t8.to(dev), "meanSquaredError", "linear")
    a = torch.zeros(B, E, dtype=torch.bfloat16, device=dev)
    b = torch.zeros(B, E, dtype=torch.bfloat16, device=dev)
    ops.image_loss_grad(*args, a, None, gs)
    ops.image_loss_grad(*args, b, None, gs, out_relu=True)
    torch.cuda.synchronize()
    assert bool((z == 0).any()) and bool((a.cpu()[z == 0] != 0).any())
    assert torch.equal(b.cpu(), torch.where(z > 0, a.cpu().double(), torch.zeros_like(z)).to(torch.bfloat16))


def test_loss_sum_is_bitwise_reproducible():
    B, E = 64, 28 * 28
    c = _Case("logLoss", "sigmoid", "u8_idx", B, E, seed=5)
    z, tab, idx = c.z.to(dev, torch.bfloat16), c.table.to(dev), c.idx.to(dev)
    out = []
    for fill in (0.0, 3.0):  # whatever an earlier launch left in the workspace does not matter
        st = torch.zeros(2, device=dev)
        ws = torch.full((ops.image_loss_workspace_floats(B, E),), fill, device=dev)
        ops.image_loss_grad(z, tab, "logLoss", "sigmoid", None, st, 1.0, idx=idx, target_scale=c.scale, workspace=ws)
        torch.cuda.synchronize()
        out.append(st.clone())
    assert torch.equal(out[0], out[1]) and float(out[0][0]) > 0
    _check("logLoss", "sigmoid", c, None, out[0], 1.0, what="reproducible")


@pytest.mark.parametrize("B,E", [(3, 49), (2, 2056)])
def test_optional_outputs(B, E):
    kind, act, gs = "sigmoidCrossEntropy", "linear", 0.5
    c = _Case(kind, act, "f32", B, E)
    z, tab = c.z.to(dev, torch.bfloat16), c.table.to(dev)
    # dz=None writes only the stats
    st = torch.zeros(2, device=dev)
    ops.image_loss_grad(z, tab, kind, act, None, st, gs, workspace=_ws(B, E))
    torch.cuda.synchronize()
    _check(kind, act, c, None, st, gs)
    # stats=None leaves the stats buffer (and the workspace) untouched
    keep = torch.full((2,), 5.0, device=dev)
    ws = torch.full((ops.image_loss_workspace_floats(B, E),), -9.0, device=dev)
    dz = torch.full((B, E), 7.0, dtype=torch.bfloat16, device=dev)
    ops.image_loss_grad(z, tab, kind, act, dz, None, gs, workspace=ws)
    torch.cuda.synchronize()
    _check(kind, act, c, dz, None, gs)
    assert bool((keep == 5.0).all()) and bool((ws == -9.0).all())
    # stats accumulate: a second launch adds to them
    ops.image_loss_grad(z, tab, kind, act, None, st, gs, workspace=_ws(B, E))
    torch.cuda.synchronize()
    _, el = _oracle(kind, act, c, gs)
    assert abs(float(st[0]) - 2 * el) <= 2e-3 * abs(el) + 2e-3


def test_the_binding_refuses_instead_of_launching():
    from distriflow_amd import native

    C = native.require()
    B, E = 4, 64
    z = torch.zeros(B, E, dtype=torch.bfloat16, device=dev)
    t = torch.zeros(B, E, device=dev)
    dz = torch.zeros(B, E, dtype=torch.bfloat16, device=dev)
    st = torch.zeros(2, device=dev)
    ws = torch.zeros(B, device=dev)
    idx = torch.zeros(B, dtype=torch.int64, device=dev)
    ok = dict(z=z, targets=t, idx=None, dz=dz, stats=st, workspace=ws, B=B, E=E, kind=0, out_act=0, grad_scale=1.0)
    C.image_loss_grad(**ok)
    bad = [dict(z=z.float()), dict(z=z[:, :32]), dict(targets=t.double()), dict(targets=t[:3]), dict(dz=dz.float()),
           dict(dz=dz[:2]), dict(workspace=ws[:3]), dict(workspace=None), dict(stats=st[:1]), dict(kind=6),
           dict(kind=-1), dict(out_act=1), dict(idx=idx[:3]), dict(idx=idx.int()), dict(E=63), dict(B=0),
           dict(targets=t.cpu())]
    for kw in bad:
        with pytest.raises(RuntimeError):
            C.image_loss_grad(**dict(ok, **kw))
    C.image_loss_grad(**dict(ok, targets=t[:1], idx=idx))  # through idx one row is enough
    with pytest.raises(NotImplementedError, match="per-pixel softmax"):
        ops.image_loss_grad(z, t, "mse", "softmax", dz, None)
    with pytest.raises(NotImplementedError, match="per-pixel softmax"):
        ops.image_loss_grad(z, t, "softmaxCrossEntropy", "linear", dz, None)
    with pytest.raises(ValueError):
        ops.image_loss_grad(z, t, "mse", "linear", None, st)  # stats without a workspace
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- model level
def _topology():
    """A small autoencoder with a skip connection on an 8x8x1 input: Conv2D stride 2, Conv2DTranspose stride 2,
    Concatenate with the input, Conv2D(1, 3, same, sigmoid)."""
    def node(cls, name, cfg, ins):
        return {"class_name": cls, "name": name, "config": dict(cfg, name=name),
                "inbound_nodes": [[[i, 0, 0, {}] for i in ins]]}

    conv = {"kernel_size": [3, 3], "padding": "same", "activation": "relu", "filters": 8}
    layers = [{"class_name": "InputLayer", "name": "inp", "inbound_nodes": [],
               "config": {"name": "inp", "batch_input_shape": [None, 8, 8, 1], "dtype": "float32"}},
              node("Conv2D", "down", dict(conv, strides=[2, 2]), ["inp"]),
              node("Conv2DTranspose", "up", dict(conv, strides=[2, 2]), ["down"]),
              node("Concatenate", "cat", {"axis": -1}, ["inp", "up"]),
              node("Conv2D", "out", dict(conv, filters=1, activation="sigmoid"), ["cat"])]
    return {"class_name": "Model", "config": {"name": "ae", "layers": layers, "input_layers": [["inp", 0, 0]],
                                              "output_layers": [["out", 0, 0]]}}


def _net(device, seed=9, loss="logLoss"):
    from distriflow_amd.models.keras import layers_from_keras
    from distriflow_amd.models.net import Net

    layers, shape = layers_from_keras(_topology())
    return Net(layers, shape, device=device, seed=seed, loss=loss)


def _images(n, seed):
    """Smooth synthetic 8x8 images in [0, 1]: an outer product of two random profiles, which a 3x3 conv net with
    a skip connection reconstructs quickly."""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, 8, 1, generator=g)
    c = torch.rand(n, 1, 8, generator=g)
    return (r * c).reshape(n, 8, 8, 1)


def test_skip_autoencoder_gpu_matches_cpu_engine():
    """The criterion of tests/test_decoder_gpu.py: the loss within 2 %, every gradient's cosine > 0.99, and the
    same bits on a second run."""
    g = torch.Generator().manual_seed(4)
    x = _images(8, 11).to(torch.bfloat16).float()  # the GPU engine computes on bf16 inputs
    cpu, gpu = _net("cpu"), _net("cuda")
    assert gpu.image_output and gpu.final_act == "sigmoid" and tuple(gpu.output_shape) == (8, 8, 1)
    with torch.no_grad():  # the biases start at zero: make them count
        for n in ("up/bias", "down/bias"):
            cpu.store[n].copy_(torch.randn(8, generator=g) * 0.1)
    gpu.store.master.copy_(cpu.store.master.to(dev))
    gpu.store.refresh_compute()
    st_c = cpu.compute_gradients(x, x)
    st_g = gpu.compute_gradients(x.to(dev), x.to(dev)).clone()
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
    st2 = gpu.compute_gradients(x.to(dev), x.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(gpu.store.grad, g1) and torch.equal(st2, st_g)
    # evaluate is the same kernel without dz; predict applies the sigmoid
    loss_g, acc = gpu.evaluate(x, x)
    assert acc == 0.0 and abs(loss_g - float(st_g[0]) / 8) <= 1e-3 * abs(loss_g) + 1e-4
    p = gpu.predict(x)
    assert tuple(p.shape) == (8, 8, 8, 1) and float(p.min()) > 0.0 and float(p.max()) < 1.0


def test_skip_autoencoder_trains_on_its_input_in_the_captured_step():
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer, epoch_permutations

    data = (_images(64, 3).reshape(64, 64) * 255).to(torch.uint8).to(dev)
    rows = epoch_permutations(64, 8, 30, dev, seed=0)

    def trainer(graph):
        tr = DataParallelTrainer(_net("cuda", seed=1), lr=0.5, graph=graph)
        tr.bind_dataset(data, "input", 8, scale=1.0 / 255.0)
        tr.bind_index_stream(rows.clone())
        return tr

    cap, eager = trainer("full"), trainer("none")
    assert torch.equal(cap.net.store.master, eager.net.store.master)
    losses = []
    for _ in range(3):
        losses.append(float(cap.step()[0].item()) / 8)
        le = float(eager.step()[0].item()) / 8
        assert le == losses[-1], (le, losses[-1])
    torch.cuda.synchronize()
    assert cap.graph_mode == "full", getattr(cap, "capture_error", None)  # no launch allocates or synchronises
    assert torch.equal(cap.net.store.master, eager.net.store.master)
    losses += [float(cap.step()[0].item()) / 8 for _ in range(27)]
    print("losses", [round(v, 4) for v in losses])
    assert sum(losses[-5:]) / 5 < losses[0], losses
    # a float table of the same maps trains the same way; a wrong shape is refused
    tr = DataParallelTrainer(_net("cuda", seed=1), lr=0.5)
    with pytest.raises(ValueError, match="target table"):
        tr.bind_dataset(data, torch.zeros(64, 10, device=dev), 8, scale=1.0 / 255.0)
    with pytest.raises(ValueError, match="target_scale"):
        tr.bind_dataset(data, data, 8, scale=1.0 / 255.0)


def test_engine_model_fits_an_autoencoder():
    from distriflow_amd.models.distri_model import EngineModel

    x = _images(16, 21)
    m = EngineModel(_net("cuda", seed=2), {"loss": "logLoss", "learningRate": 0.5}, train_compile_loss=True)
    first = m.evaluate(x, x)
    assert len(first) == 2 and first[1] == 0.0 and first[0] > 0
    for _ in range(10):
        m.update(m.fit(x, x))
    last = m.evaluate(x, x)
    print("evaluate", first, last)
    assert last[1] == 0.0 and last[0] < first[0]
    assert m.output_shape == [8, 8, 1] and tuple(m.predict(x).shape) == (16, 8, 8, 1)
