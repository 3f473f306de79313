"""The reference CNN's fused conv block (csrc/kcnn_fused.hip) against the per-layer kernels it replaces
(conv1 image-resident kernel, conv2 igemm64 with the pooled epilogue, unpool + conv2 weight / data
gradient + conv1 weight gradient).  The fused block computes conv1 on MFMA (the per-layer kernel: VALU FMA
chains), so the 9-tap fp32 sums differ in order: the pooled maps agree to bf16 rounding (a handful of
elements one bf16 step apart, an argmax code flipped where two window values tie within it), the loss and
every gradient to fp32 / bf16 summation order.  The ``*_exact*`` tests compare ``ops.kcnn_fwd`` / ``ops.kcnn_bwd``
themselves with an fp64 reference on integer data by ``torch.equal`` (tests/exact_util.py), ties included."""
import functools

import pytest
import torch

import exact_util as xu
from distriflow_amd import ops

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


def _pair(monkeypatch, seed=3):
    from distriflow_amd.models.layers import KerasConvBlock
    from distriflow_amd.models.zoo import build_model

    f = build_model("keras_cnn", device=dev, seed=seed)
    assert isinstance(f.exec_layers[0], KerasConvBlock)
    monkeypatch.setenv("DISTRIFLOW_DIAG", "kcnn_fused=0")
    p = build_model("keras_cnn", device=dev, seed=seed)
    monkeypatch.delenv("DISTRIFLOW_DIAG")
    assert not isinstance(p.exec_layers[0], KerasConvBlock)
    p.store.set_flat(f.store.master.clone())
    return f, p


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize("B", [64, 200])
def test_kcnn_block_matches_per_layer_path(monkeypatch, B):
    from distriflow_amd.data.synthetic import synthetic_mnist

    f, p = _pair(monkeypatch)
    data, labels = synthetic_mnist(4096, seed=5, device=dev)
    idx = torch.randperm(4096, device=dev)[:B]
    x, y = ops.GatherRef(data, idx, 1 / 255.0, (28, 28, 1)), ops.LabelRef(labels, idx)
    # same dropout masks: the fused step's masks read counter + 1 and its reduce advances the counter at
    # the end; the per-layer step's gather advances it first
    f.step_dev.fill_(5)
    p.step_dev.fill_(5)
    sf = f.compute_gradients(x, y).clone()
    sp = p.compute_gradients(x, y).clone()
    torch.cuda.synchronize()
    assert int(f.step_dev.item()) == 6 and int(p.step_dev.item()) == 6
    of, op = f.exec_layers[0].out, p.exec_layers[1].out  # pooled (+ dropout) map
    assert _rel(of, op) < 2e-3, _rel(of, op)
    assert (of != op).float().mean().item() < 2e-3
    assert (f.exec_layers[0].code != p.exec_layers[1].code).float().mean().item() < 1e-3
    assert abs(float(sf[0]) - float(sp[0])) <= 1e-3 * abs(float(sp[0])) and abs(float(sf[1]) - float(sp[1])) <= 1
    for s in f.store.specs:
        gf, gp = f.store.gradient(s.name), p.store.gradient(s.name)
        assert _rel(gf, gp) < 5e-3, (s.name, _rel(gf, gp))


# ---- exact on integers (tests/exact_util.py): ops.kcnn_fwd / ops.kcnn_bwd against an fp64 reference of the same
# block, argmax codes and ties included.  The forward grid is min(B, 768) and the backward grid min(B, 512), so
# B = 770 gives two forward workgroups a second image and makes 258 backward workgroups store and reload their
# conv2 accumulators between images; the tests above never do either.
@functools.lru_cache(maxsize=None)
def _exact_block(B):
    """Integer data and the fp64 reference of the block at batch B, computed once and shared (never modified):
    x in {0, 1, 2} as rows ``idx`` of a uint8 dataset, w1 / b1 in [-1, 1], about 64 non-zero w2 in {-1, 1} per
    reduction of 288, b2 in [-3, 3], pooled gradient in {-1, 0, 1}."""
    g = xu.gen(B)
    data = torch.randint(0, 3, (B + 30, 28, 28, 1), generator=g, dtype=torch.uint8)
    idx = torch.randperm(B + 30, generator=g)[:B]
    w1, b1 = xu.ints(g, (32, 9), -1, 1), xu.ints(g, (32,), -1, 1)
    w2, b2 = xu.sparse_ints(g, (32, 288), -1, 1, xu.weight_density(288)), xu.ints(g, (32,), -3, 3)
    dyp = xu.ints(g, (B, 12, 12, 32), -1, 1)
    x = data[idx].double().to(dev)
    X1 = xu.conv_fwd_ref(x, w1.to(dev), b1.to(dev), 3, 1, 0, relu=True)
    xu.assert_exact_output(X1)
    y2 = xu.conv_fwd_ref(X1, w2.to(dev), b2.to(dev), 3, 1, 0, relu=False)
    xu.assert_exact_output(y2)
    m, am = xu.window_argmax(xu.windows(y2))
    code = xu.code_relu4(m, am)
    tied = float(((xu.windows(y2) == m.unsqueeze(-1)).sum(-1) > 1).double().mean())
    assert tied > 0.03 and 0.1 < float((code == 4).double().mean()) < 0.5, "the data lost its ties / dead windows"
    dy2 = xu.unpool_ref(dyp.to(dev), code, 24, 24, "relu4")
    del y2
    gw2, gb2, ab2 = xu.conv_wgrad_ref(dy2, X1, 3, 1, 0)
    dX1 = xu.conv_dgrad_ref(dy2, w2.to(dev), X1.shape, 3, 1, 0) * (X1 > 0)
    xu.assert_exact_output(dX1)
    gw1, gb1, ab1 = xu.conv_wgrad_ref(dX1, x, 3, 1, 0)
    sums = (ab1.max(), ab2.max(), dX1.abs().sum((0, 1, 2)).max(), dy2.abs().sum((0, 1, 2)).max())
    assert max(float(s) for s in sums) < xu.FP32_INT_MAX
    return dict(data=data.to(dev), idx=idx.to(dev), w1=xu.pad_w(w1, dev), b1=b1.float().to(dev), w2=xu.pad_w(w2, dev),
                b2=b2.float().to(dev), w2t=xu.pad_wt(w2, 32, 9, 32, dev), dyp=xu.bf16(dyp, dev), pooled=m.clamp_min(0),
                code=code, gw1=gw1, gb1=gb1, gw2=gw2, gb2=gb2)


def _exact_input(r, kind):
    if kind == "u8":
        return ops.GatherRef(r["data"], r["idx"], 1.0, (28, 28, 1))
    return r["data"][r["idx"]].to(torch.bfloat16)


@pytest.mark.parametrize("kind", ["u8", "bf16"])
@pytest.mark.parametrize("B", [3, 770])
def test_kcnn_block_exact_on_integers(B, kind):
    """The pooled map, every argmax code (first maximum in row-major window order, 4 where the maximum is not
    positive) and all four gradients, computed from the reference's codes, equal the fp64 reference; the
    backward advances the step counter by exactly one."""
    r = _exact_block(B)
    x = _exact_input(r, kind)
    out = torch.full((B, 12, 12, 32), float("nan"), dtype=torch.bfloat16, device=dev)
    code = torch.full((B, 12, 12, 32), 255, dtype=torch.uint8, device=dev)
    ops.kcnn_fwd(x, r["w1"], r["b1"], r["w2"], r["b2"], out, code)
    assert torch.equal(code, r["code"]), "argmax codes"
    assert torch.equal(out.double(), r["pooled"]), "pooled map"
    g = {n: torch.full(r[n].shape, float("nan"), device=dev) for n in ("gw1", "gb1", "gw2", "gb2")}
    step = torch.tensor(41, dtype=torch.int64, device=dev)
    slabs = torch.empty(ops.kcnn_slab_floats(B), dtype=torch.float32, device=dev)
    ops.kcnn_bwd(x, r["w1"], r["b1"], r["w2t"], r["dyp"], r["code"], slabs, g["gw1"], g["gb1"], g["gw2"], g["gb2"],
                 step_inc=step)
    for n in ("gw2", "gb2", "gw1", "gb1"):
        assert torch.equal(g[n].double(), r[n]), n
    assert int(step.item()) == 42


@pytest.mark.parametrize("B", [3, 770])
def test_kcnn_fwd_folded_dropout_exact(B):
    """p = 0.5 (scale 2: exact): the pooled map is the reference times the CPU hash twin's mask at step +
    step_add, the codes are those of the undropped map."""
    from distriflow_amd.ops import reference as ref

    r = _exact_block(B)
    assert 2 * float(r["pooled"].max()) <= xu.BF16_INT_MAX
    step = torch.tensor(5, dtype=torch.int64, device=dev)
    keep = ref.dropout_mask(r["pooled"].numel(), 0.5, 99 ^ ((5 + 1) * 0x9E3779B1)).double().view(r["pooled"].shape).to(dev)
    out = torch.full((B, 12, 12, 32), float("nan"), dtype=torch.bfloat16, device=dev)
    code = torch.full((B, 12, 12, 32), 255, dtype=torch.uint8, device=dev)
    ops.kcnn_fwd(_exact_input(r, "u8"), r["w1"], r["b1"], r["w2"], r["b2"], out, code, drop=(0.5, 99, step, 1))
    assert torch.equal(code, r["code"]), "argmax codes"
    assert torch.equal(out.double(), 2 * r["pooled"] * keep), "pooled map"
    assert int(step.item()) == 5


def test_kcnn_block_bf16_batch_input_and_training(monkeypatch):
    """A bf16 batch (no index) takes the same path; a few SGD steps reduce the loss."""
    from distriflow_amd.data.synthetic import synthetic_mnist
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer, epoch_permutations

    f, p = _pair(monkeypatch)
    data, labels = synthetic_mnist(2048, seed=1, device=dev)
    xb = (data[:96].float() / 255.0).to(torch.bfloat16)
    yb = labels[:96]
    f.step_dev.fill_(2)  # masks read 3, then the block's reduce advances the counter
    p.step_dev.fill_(2)  # advanced (torch add) to 3 before the per-layer step reads it
    sf = f.compute_gradients(xb, yb).clone()
    sp = p.compute_gradients(xb, yb).clone()
    torch.cuda.synchronize()
    assert abs(float(sf[0]) - float(sp[0])) <= 1e-3 * abs(float(sp[0]))
    tr = DataParallelTrainer(f, lr=0.05, graph="full")
    tr.bind_dataset(data, labels, 256, scale=1.0 / 255.0)
    tr.bind_index_stream(epoch_permutations(2048, 256, 30, dev, seed=0))
    losses = [float(tr.step()[0].item()) / 256 for _ in range(30)]
    assert tr.graph_mode == "full"
    assert sum(losses[-5:]) < 0.9 * sum(losses[:5]), losses
