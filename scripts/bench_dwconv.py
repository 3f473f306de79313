#!/usr/bin/env python3
"""Time of the three depthwise conv kernels (csrc/dwconv.hip) at MobileNet-sized layers, against PyTorch-ROCm's
F.conv2d(groups=C) forward + backward on channels-last bf16, alternating in one process.

Shapes: B = 256, 56x56x128, 3x3 'same', stride 1 and stride 2.  Per kernel: time per call, the bytes the
algorithm has to move (inputs and outputs once each, the weights once), bytes/s and the share of the HBM
peak (8.0 TB/s, MI355X; a float4 copy reaches 6.29 TB/s of it).  Every timed window ends in a device
synchronise.  Usage: python3 scripts/bench_dwconv.py [--batch 256] [--iters 20] [--rounds 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from distriflow_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


def timed(fn, iters):
    """Seconds per call: a host clock around ``iters`` calls that ends in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_shape(B, H, W, C, stride, iters, rounds):
    dev = torch.device("cuda", 0)
    geom = ops.dwconv_geometry(B, H, W, C, 1, (3, 3), (stride, stride), "same")
    OH, OW = geom[5], geom[6]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, H, W, C, generator=g).to(dev, torch.bfloat16)
    dy = torch.randn(B, OH, OW, C, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(3, 3, C, generator=g) * 0.3).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    gw, gb = torch.empty_like(w), torch.empty_like(bias)
    ws = torch.empty(1 << 22, device=dev)
    # torch: the same tensors as channels-last NCHW views, weights [C][1][3][3] bf16
    xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)
    dyt = dy.permute(0, 3, 1, 2)
    wt = w.permute(2, 0, 1).unsqueeze(1).to(torch.bfloat16).contiguous().requires_grad_(True)
    bt = bias.to(torch.bfloat16).requires_grad_(True)

    def t_fwd():
        with torch.no_grad():
            return F.conv2d(xt, wt, bt, stride=stride, padding=1, groups=C)

    def t_fwd_bwd():
        xt.grad = wt.grad = bt.grad = None
        F.conv2d(xt, wt, bt, stride=stride, padding=1, groups=C).backward(dyt)

    act, out = x.numel() * 2, dy.numel() * 2
    wb = w.numel() * 4 + bias.numel() * 4
    fns = {
        "dwconv_fwd": (lambda: ops.dwconv_fwd(x, w, bias, y, geom), act + out + wb),
        "dwconv_dgrad": (lambda: ops.dwconv_dgrad(dy, w, dx, geom), out + act + w.numel() * 4),
        "dwconv_wgrad": (lambda: ops.dwconv_wgrad(dy, x, gw, gb, ws, geom), out + act + wb),
        "torch_fwd": (t_fwd, act + out + wb // 2),
        "torch_fwd_bwd": (t_fwd_bwd, 0),
    }
    for fn, _ in fns.values():  # warm up every shape the timed windows use (code objects, MIOpen's choice)
        for _ in range(3):
            fn()
    best = {k: float("inf") for k in fns}
    for _ in range(rounds):  # alternate ours and torch's; keep the best round of each
        for k, (fn, _) in fns.items():
            best[k] = min(best[k], timed(fn, iters))
    assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all() and torch.isfinite(gw).all()
    rows = []
    for k, (_, nbytes) in fns.items():
        t = best[k]
        row = {"shape": f"B{B} {H}x{W}x{C} 3x3 s{stride} same", "kernel": k, "us": round(t * 1e6, 1)}
        if nbytes:
            row.update(MB=round(nbytes / 1e6, 1), TBps=round(nbytes / t / 1e12, 3),
                       hbm_peak_share=round(nbytes / t / HBM_PEAK, 3))
        rows.append(row)
    ours = best["dwconv_fwd"] + best["dwconv_dgrad"] + best["dwconv_wgrad"]
    rows.append({"shape": rows[0]["shape"], "kernel": "ours fwd+dgrad+wgrad", "us": round(ours * 1e6, 1),
                 "vs_torch_fwd_bwd": round(ours / best["torch_fwd_bwd"], 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dwconv needs the GPU: a time measured elsewhere says nothing about it")
    for stride in (1, 2):
        for row in bench_shape(a.batch, 56, 56, 128, stride, a.iters, a.rounds):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
