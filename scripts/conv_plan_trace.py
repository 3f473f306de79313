"""Which kernels the conv / dense dispatch launches for the hand list of scripts/conv_plan_fixture.py.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/conv_plan_trace.py --launch
    python scripts/conv_plan_trace.py --reduce DIR > profiles/conv_plan/<table>.txt

``--launch`` runs every entry once, forward and data gradient, each behind a one-element fill that marks
it in the trace.  ``--reduce`` prints one line per kernel: entry, kernel, workgroups, workgroup size, LDS
bytes.  Two builds launch the same kernels exactly when their tables are equal.

``--launch-wgrad`` / ``--reduce-wgrad DIR`` do the same for the weight-gradient hand list (``wgrad_hand_list``),
each entry with the workspace size it names.  Both take the entries whose ``diag`` is the process's
DISTRIFLOW_DIAG (the switches are read once per process), so the list takes one profiler run per value:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/conv_plan_trace.py --launch-wgrad
    DISTRIFLOW_DIAG=halo_groups=1 rocprofv3 ... -d DIR1 -- python scripts/conv_plan_trace.py --launch-wgrad
    (python scripts/conv_plan_trace.py --reduce-wgrad DIR;
     DISTRIFLOW_DIAG=halo_groups=1 python scripts/conv_plan_trace.py --reduce-wgrad DIR1) > <table>.txt
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def launch():
    import torch
    from conv_plan_fixture import hand_list
    from distriflow_amd import native
    m = native.get(build_if_missing=False)
    dev = "cuda"
    jobs = []
    for e in hand_list():
        M, N, K, Kpad = e["M"], e["N"], e["K"], e["Kpad"]
        if e["mode"] == 0:
            lda, geom = e["lda"], [1, 1, 1, 1, 1, 1, 1, 1, 0]
            src = torch.zeros(M * lda, dtype=torch.bfloat16, device=dev)
        else:
            lda, geom = 0, e["geom"]
            src = torch.zeros(M // (geom[3] * geom[4]) * geom[0] * geom[1] * geom[2], dtype=torch.bfloat16, device=dev)
        w = torch.zeros(-(-N // 16) * 16 * Kpad, dtype=torch.bfloat16, device=dev)
        pooled = bool(e.get("pooled"))
        out = torch.zeros((M // 4 if pooled else M) * N, dtype=torch.bfloat16, device=dev)
        kw = {}
        if pooled:
            kw["pool_code"] = torch.zeros(M // 4 * N, dtype=torch.uint8, device=dev)
        if e.get("drop"):
            kw.update(drop_p=0.5, drop_seed=1)
        jobs.append((src, w, None, None, out, M, N, K, Kpad, lda, N, geom, e["mode"], False, 1.0, kw))
    mark = torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    for j in jobs:
        mark.fill_(1.0)
        m.igemm_fwd(*j[:-1], **j[-1])
    torch.cuda.synchronize()


def wgrad_entries():
    from conv_plan_fixture import wgrad_hand_list
    return [e for e in wgrad_hand_list() if e.get("diag", "") == os.environ.get("DISTRIFLOW_DIAG", "")]


def launch_wgrad():
    import torch
    from distriflow_amd import native
    m = native.get(build_if_missing=False)
    dev = "cuda"
    jobs = []
    for e in wgrad_entries():
        M, N, K = e["M"], e["N"], e["K"]
        if e["mode"] == 0:
            geom, nsrc = [1, 1, 1, 1, 1, 1, 1, 1, 0], M * e["lda"]
        else:
            geom = e["geom"]
            nsrc = M // (geom[3] * geom[4]) * geom[0] * geom[1] * geom[2]
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
        jobs.append((z(M * e["ldd"], torch.bfloat16), z(nsrc, torch.bfloat16), z(N * K, torch.float32),
                     z(N, torch.float32) if e["bias"] else None, z(e["ws"], torch.float32), M, N, K, e["ldd"],
                     e["lda"], geom, e["mode"], 1.0))
    mark = torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    for j in jobs:
        mark.fill_(1.0)
        m.igemm_wgrad(*j)
    torch.cuda.synchronize()


def _short(n):
    n = n.replace("void ", "").replace("dfa::", "").replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*\)$", "", n).replace(" ", "")


def reduce_trace(d, names):
    recs = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            wg = int(r["Workgroup_Size_X"]) * int(r.get("Workgroup_Size_Y", 1)) * int(r.get("Workgroup_Size_Z", 1))
            grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1)) * int(r.get("Grid_Size_Z", 1))
            if not r["Kernel_Name"].startswith("__amd_rocclr"):  # (the runtime's own memset of a first-use buffer)
                recs.append((int(r["Start_Timestamp"]), _short(r["Kernel_Name"]), grid // wg, wg, int(r["LDS_Block_Size"])))
    recs.sort()
    marks = [i for i, r in enumerate(recs) if "FillFunctor" in r[1]][-len(names):]
    assert len(marks) == len(names), f"{len(marks)} markers for {len(names)} entries"
    for name, i, j in zip(names, marks, marks[1:] + [len(recs)]):
        for _, kern, grid, wg, lds in recs[i + 1:j]:
            print(f"{name} | {kern} | {grid} | {wg} | {lds}")


def read_table(path):
    """{entry: [[kernel, workgroups, workgroup size, LDS bytes], ...]} of a table --reduce wrote."""
    t = {}
    for line in open(path):
        name, kern, grid, wg, lds = [s.strip() for s in line.split("|")]
        t.setdefault(name, []).append([kern, int(grid), int(wg), int(lds)])
    return t


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--reduce", metavar="DIR")
    ap.add_argument("--launch-wgrad", action="store_true")
    ap.add_argument("--reduce-wgrad", metavar="DIR")
    a = ap.parse_args()
    if a.launch:
        launch()
    if a.launch_wgrad:
        launch_wgrad()
    if a.reduce:
        from conv_plan_fixture import hand_list
        reduce_trace(a.reduce, [e["name"] for e in hand_list()])
    if a.reduce_wgrad:
        reduce_trace(a.reduce_wgrad, [e["name"] for e in wgrad_entries()])
