"""One rank of the two-rank Adam test (tests/test_adam_gpu.py): argv = rank world port out_dir."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mp_util import finish, init_rank  # noqa: E402


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dev = init_rank(rank, world, port)
    from distriflow_amd.data.synthetic import synthetic_mnist
    from distriflow_amd.models.zoo import build_model
    from distriflow_amd.parallel.data_parallel import DataParallelTrainer

    B, steps = 32, 3
    g = torch.Generator().manual_seed(5)
    rows = torch.stack([torch.randperm(1024, generator=g)[: B * world] for _ in range(steps)])
    data, labels = synthetic_mnist(1024, seed=3, device=dev)
    net = build_model("mlp_mnist", device=dev, seed=0)
    w0 = net.store.master.cpu()
    tr = DataParallelTrainer(net, lr=1e-3, optimizer="adam", graph="none")
    tr.bind_dataset(data, labels, B, scale=1.0 / 255.0)
    tr.bind_index_stream(rows[:, rank * B:(rank + 1) * B].contiguous().to(dev))
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    tr.check_comm()
    st = net.store
    torch.save({"w0": w0, "w": st.master.cpu(), "m": st.adam_m.cpu(), "v": st.adam_v.cpu(), "t": st.adam_t,
                "launches": tr.step_launches}, os.path.join(out_dir, f"r{rank}.pt"))
    finish()


if __name__ == "__main__":
    main()
