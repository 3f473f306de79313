"""Time of one fused optimizer launch, SGD (sgd_multi) against Adam (adam_multi), on a model's parameters:

    python scripts/adam_launch_time.py [--model resnet18_cifar] [--iters 200]

Event-timed over ``iters`` back-to-back launches (no forward / backward); run it under
``rocprofv3 --kernel-trace --stats`` for the per-kernel table.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet18_cifar")
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    from distriflow_amd.models.zoo import build_model

    net = build_model(args.model, device="cuda:0", seed=0)
    st = net.store
    st.grad.normal_(0.0, 1e-3)
    out = {"model": args.model, "params": net.num_params(), "iters": args.iters}
    st.set_hyper(1e-3)
    out["sgd_us"] = round(timed(st.step, args.iters), 2)
    st.set_hyper(1e-3, momentum=0.9)
    out["sgd_momentum_us"] = round(timed(st.step, args.iters), 2)
    st.set_optimizer("adam")
    st.set_hyper(1e-3)
    out["adam_us"] = round(timed(st.step, args.iters), 2)
    out["adam_over_sgd"] = round(out["adam_us"] / out["sgd_us"], 3)
    assert st.adam_t == args.iters + 10 and bool(torch.isfinite(st.master).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
