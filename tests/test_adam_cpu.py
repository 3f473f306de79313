"""Adam / AdamW on the CPU engine: the store's update against torch.optim, trainer resume with optimizer
state through the launcher's checkpoint path, the Keras optimizer parser and the SGD-only engines."""
import pytest
import torch

from adam_util import BETAS, EPS, LR, STEPS, fixed_grads, rel_err, torch_adam, valid_mask


def _cpu_net(name="mlp_mnist", seed=0):
    from distriflow_amd.models.zoo import build_model

    return build_model(name, device="cpu", seed=seed)


@pytest.mark.parametrize("name", ["adam", "adamw"])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_store_matches_torch_optim(name, wd):
    """5 updates on fixed random gradients (grad_scale 0.25) == torch.optim.Adam / AdamW on the same fp32
    values: allclose at rtol 1e-6, atol 1e-8; the flat buffer's padding stays exactly 0."""
    st = _cpu_net().store
    grads = fixed_grads(st)
    ref = torch_adam(st.master, grads, name, wd, 0.25, torch.float32)
    st.set_optimizer(name, *BETAS, EPS)
    st.set_hyper(LR, 0.0, wd, grad_scale=0.25)
    for g in grads:
        st.grad.copy_(g)
        st.step()
    assert st.adam_t == STEPS
    assert not torch.equal(st.master, ref["w"][0])
    torch.testing.assert_close(st.master, ref["w"][-1], rtol=1e-6, atol=1e-8)
    # the moments cancel (b1 * m + (1 - b1) * g with opposite signs), so their error is measured against the
    # largest magnitude the element took (adam_util.rel_err), at the same 1e-6
    assert rel_err(st.adam_m, ref["m"]) <= 1e-6
    assert rel_err(st.adam_v, ref["v"]) <= 1e-6
    pad = ~valid_mask(st)
    for t in (st.master, st.adam_m, st.adam_v):
        assert torch.equal(t[pad], torch.zeros(int(pad.sum())))


def test_padding_exists_in_some_model():
    """The padding assertion above must look at something: lenet5's flat buffer has alignment padding."""
    st = _cpu_net("lenet5").store
    assert int((~valid_mask(st)).sum()) > 0
    grads = fixed_grads(st, steps=2)
    st.grad[~valid_mask(st)] = 3.0  # garbage in the padding must not reach the state
    st.set_optimizer("adam")
    st.set_hyper(LR, 0.0, 1e-2)
    for g in grads:
        st.grad.copy_(g)
        st.grad[~valid_mask(st)] = 3.0
        st.step()
    pad = ~valid_mask(st)
    for t in (st.master, st.adam_m, st.adam_v):
        assert torch.equal(t[pad], torch.zeros(int(pad.sum())))


def _trainer(net, rows, **opt):
    from distriflow_amd.data.synthetic import synthetic_mnist
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer

    data, labels = synthetic_mnist(256, seed=3, device="cpu")
    tr = DataParallelTrainer(net, lr=1e-3 if opt.get("optimizer") == "adam" else 0.05, graph="none", **opt)
    tr.bind_dataset(data, labels, 32, scale=1.0 / 255.0)
    tr.bind_index_stream(rows)
    return tr


def _opt_tensors(store):
    return {"master": store.master.clone(), **{k: v.clone() for k, v in store.optimizer_state().items()}}


@pytest.mark.parametrize("opt", [{"optimizer": "adam"}, {"optimizer": "sgd", "momentum": 0.9}],
                         ids=["adam", "sgd-momentum"])
def test_trainer_resume_is_bitwise(opt, tmp_path):
    """6 uninterrupted steps == 3 steps, a checkpoint through the launcher's save / resume path into a
    fresh Net, 3 more steps: master and every optimizer tensor bit for bit."""
    from distriflow_amd.checkpoint.store import VersionedStore
    from distriflow_amd.launch import resume_sync_checkpoint, save_sync_checkpoint

    g = torch.Generator().manual_seed(5)
    rows = torch.stack([torch.randperm(256, generator=g)[:32] for _ in range(6)])
    a = _cpu_net()
    tr = _trainer(a, rows, **opt)
    for _ in range(6):
        tr.step()
    want = _opt_tensors(a.store)
    assert len(want) == (4 if opt["optimizer"] == "adam" else 2)

    b = _cpu_net()
    tr = _trainer(b, rows, **opt)
    for _ in range(3):
        tr.step()
    vs = VersionedStore(str(tmp_path))
    vs.setup()
    save_sync_checkpoint(vs, b, epoch=0, step=3)
    assert vs.read_resume()["optimizer"]["name"] == opt["optimizer"]

    c = _cpu_net(seed=11)  # other initial weights: everything must come from the checkpoint
    tr = _trainer(c, rows[3:], **opt)
    assert resume_sync_checkpoint(VersionedStore(str(tmp_path)), c) == 3
    for _ in range(3):
        tr.step()
    got = _opt_tensors(c.store)
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), k
    if opt["optimizer"] == "adam":
        assert c.store.adam_t == 6


def test_resume_refuses_another_optimizer_and_accepts_old_checkpoints(tmp_path):
    from distriflow_amd.checkpoint.store import VersionedStore
    from distriflow_amd.checkpoint.tfjs import save_layers_model
    from distriflow_amd.launch import resume_sync_checkpoint, save_sync_checkpoint

    a = _cpu_net()
    a.store.set_optimizer("adam")
    a.store.set_hyper(1e-3)
    vs = VersionedStore(str(tmp_path / "adam"))
    vs.setup()
    save_sync_checkpoint(vs, a, 0, 1)
    b = _cpu_net()
    b.store.set_hyper(0.05, momentum=0.9)
    with pytest.raises(SystemExit, match="adam"):
        resume_sync_checkpoint(vs, b)
    # a checkpoint from before optimizer state was saved: weights only, resume record without "optimizer"
    old = VersionedStore(str(tmp_path / "old"))
    old.setup()
    v = old.new_version()
    save_layers_model(a, old.path(v))
    old.mark_current(v)
    old.write_resume({"epoch": 0, "step": 4, "version": v})
    c = _cpu_net(seed=3)
    c.store.set_optimizer("adam")
    c.store.set_hyper(1e-3)
    c.store.adam_m.fill_(1.0)
    assert resume_sync_checkpoint(old, c) == 4
    assert torch.equal(c.store.master, a.store.master)
    assert c.store.adam_t == 0 and not c.store.adam_m.any()


def test_optimizer_from_keras():
    from distriflow_amd.models.keras import optimizer_from_keras
    from distriflow_amd.models.zoo import keras_cnn_topology

    oc = optimizer_from_keras(keras_cnn_topology())
    assert oc["name"] == "adam" and oc["momentum"] == 0.0
    assert oc["lr"] == pytest.approx(0.001, rel=1e-6)
    assert oc["betas"] == (pytest.approx(0.9, rel=1e-6), pytest.approx(0.999, rel=1e-6))
    assert oc["eps"] == pytest.approx(1e-7, rel=1e-6)

    def topo(cls, **cfg):
        return {"training_config": {"optimizer_config": {"class_name": cls, "config": cfg}}}

    sgd = optimizer_from_keras(topo("SGD", learning_rate=0.02, momentum=0.9, decay=0.0, nesterov=False))
    assert sgd == {"name": "sgd", "lr": 0.02, "betas": None, "eps": None, "momentum": 0.9}
    assert optimizer_from_keras(topo("SGD", lr=0.5))["lr"] == 0.5
    assert optimizer_from_keras({"model_config": {}}) is None
    with pytest.raises(NotImplementedError):
        optimizer_from_keras(topo("Adam", lr=0.001, amsgrad=True))
    with pytest.raises(NotImplementedError):
        optimizer_from_keras(topo("Adam", lr=0.001, decay=1e-4))
    with pytest.raises(NotImplementedError):
        optimizer_from_keras(topo("RMSprop", lr=0.001))


def test_sgd_only_engines_say_so():
    """The engines whose update is not the store's optimizer launch refuse Adam by name (before touching
    the device, so the check runs anywhere)."""
    from distriflow_amd.parallel.async_ps import AsyncPSTrainer
    from distriflow_amd.parallel.fedavg import FedAvgTrainer
    from distriflow_amd.parallel.fedsgd_ps import FedSGDDeviceTrainer

    net = _cpu_net()
    for cls in (AsyncPSTrainer, FedSGDDeviceTrainer, FedAvgTrainer):
        with pytest.raises(ValueError, match="sgd"):
            cls(net, optimizer="adam")
    assert net.store.optimizer == "sgd"


def test_engine_model_optimizer_keyword():
    from distriflow_amd.models.distri_model import EngineModel

    net = _cpu_net()
    m = EngineModel(net, {"loss": "softmaxCrossEntropy", "learningRate": 1e-3}, optimizer="adam")
    m.fetch_initial()
    g = fixed_grads(net.store, steps=1)[0]
    ref = torch_adam(net.store.master, [g], "adam", 0.0, 1.0, torch.float32)
    m.update_flat(g)
    assert net.store.optimizer == "adam" and net.store.adam_t == 1
    torch.testing.assert_close(net.store.master, ref["w"][-1], rtol=1e-6, atol=1e-8)
    with pytest.raises(ValueError):
        EngineModel(net, optimizer="rmsprop")
