"""Record tests/golden/convpool_plan.json: what the fused conv+pool path launches over a fixed shape list.

    rocprofv3 --kernel-trace --output-format csv -d DIR/<entry>/<kind> -- \\
        python scripts/convpool_plan_fixture.py --launch <entry> <kind>          # one launch per process
    python scripts/convpool_plan_fixture.py --reduce DIR [--sizes FILE] > profiles/conv_plan/<table>.txt
    python scripts/convpool_plan_fixture.py --write profiles/conv_plan/<table>.txt

The shape list (``entries``): every case of tests/golden/convpool_cases.json at its B = 3, the two conv blocks
of LeNet-5 (the only ones of the zoo models that Net fuses this way) at B in {3, 64, 4096}, and the weight
gradient of test_convpool_wgrad_small_workspace with its two-slab workspace; every other weight gradient gets
2^22 floats, as FusedConvPool.alloc gives it.  ``--launch`` runs one of forward / weight gradient / data
gradient of one entry on zero operands (aligned, so the data gradient takes its staged kernel); ``--reduce``
prints one line per kernel of the traces: entry/kind, kernel with template arguments, workgroups, workgroup
size, LDS bytes, images per group.  Two builds launch the same kernels exactly when their tables are equal.
DISTRIFLOW_DIAG must be unset: cp_wpc and cp_minimgs change the sizing.

The trace's LDS column is the kernel's static segment (0 for the conv+pool kernels, whose LDS is all dynamic),
so the dynamic bytes and the images per group come from ``--sizes``: lines "entry/kind kind imgs grid lds".  For
the commit before the planner, which had no query for them, a throw-away build printed them from its three
launchers, one launch per process as above; for a build with the planner ``--plan-sizes`` prints the same lines
from ops.convpool_plan on a machine with a GPU.  Each line's grid must be the traced one.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "convpool_plan.json")
KINDS = ("fwd", "wgrad", "dgrad")
WS_FLOATS = 1 << 22


def entries():
    def e(name, B, H, W, C, N, k, pad, ws=WS_FLOATS):
        return dict(name=name, B=B, H=H, W=W, C=C, N=N, k=k, pad=pad, ws=ws)

    with open(os.path.join(GOLDEN, "convpool_cases.json")) as f:
        cases = json.load(f)["cases"]
    es = [e("case_h{H}c{C}n{N}k{k}p{pad}".format(**c), *(c[n] for n in ("B", "H", "W", "C", "N", "k", "pad")))
          for c in cases]
    for B in (3, 64, 4096):
        es += [e(f"lenet5_b{B}_conv2d_1", B, 28, 28, 1, 6, 5, 2), e(f"lenet5_b{B}_conv2d_2", B, 14, 14, 6, 16, 5, 0)]
    es.append(e("small_workspace", 8, 12, 12, 3, 20, 3, 1, ws=2 * 20 * 28))
    return es


def launch(name, kind):
    import torch
    from distriflow_amd import ops
    e = next(e for e in entries() if e["name"] == name)
    B, H, W, C, N, k, pad = (e[n] for n in ("B", "H", "W", "C", "N", "k", "pad"))
    assert ops.convpool_supported(H, W, C, k, k, pad, N), e
    PH, PW = (H + 2 * pad - k + 1) // 2, (W + 2 * pad - k + 1) // 2
    z = lambda shape, dt=torch.bfloat16: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    x, dp, code = z((B, H, W, C)), z((B, PH, PW, N)), z((B, PH, PW, N), torch.uint8)
    if kind == "fwd":
        w = z((-(-N // 16) * 16, ops.convpool_fwd_layout(H, W, C, k, k, pad, N)[1]))
        ops.convpool_fwd(x, w, z(N, torch.float32), dp, code, k, k, pad)
    elif kind == "wgrad":
        ops.convpool_wgrad(x, dp, code, z((N, k * k * C), torch.float32), z(N, torch.float32),
                           z(e["ws"], torch.float32), k, k, pad)
    else:
        ops.convpool_dgrad(dp, code, None, z((16, ops.convpool_dgrad_layout(H, W, C, k, k, pad, N)[1])), x, k, k, pad)
    torch.cuda.synchronize()


def reduce_traces(d, sizes):
    import csv
    import glob
    from conv_plan_trace import _short
    size = {}
    if sizes:
        for line in open(sizes):
            name, _, imgs, grid, lds = line.split()
            size[name] = (int(imgs), int(grid), int(lds))
    for e in entries():
        for kind in KINDS:
            rows = []
            for f in glob.glob(os.path.join(d, e["name"], kind, "**", "*kernel_trace.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    kern = _short(r["Kernel_Name"])
                    if kern.startswith(("convpool_", "slab_reduce_")):
                        wg = int(r["Workgroup_Size_X"])
                        rows.append((int(r["Start_Timestamp"]), kern, int(r["Grid_Size_X"]) // wg, wg, int(r["LDS_Block_Size"])))
            assert rows and rows[0][1].startswith(f"convpool_{kind}_kernel"), (e["name"], kind, rows)
            for i, (_, kern, grid, wg, lds) in enumerate(sorted(rows)):
                imgs = ""
                if i == 0 and size:
                    imgs, sgrid, lds = size[f"{e['name']}/{kind}"]
                    assert sgrid == grid, (e["name"], kind, sgrid, grid)
                print(f"{e['name']}/{kind} | {kern} | {grid} | {wg} | {lds} | {imgs}")


def plan_sizes():
    from distriflow_amd import ops
    for e in entries():
        p = ops.convpool_plan(e["H"], e["W"], e["C"], e["k"], e["k"], e["pad"], e["N"], B=e["B"], ws_floats=e["ws"])
        for kind in KINDS:
            print(f"{e['name']}/{kind} {kind} {p[kind]['imgs']} {p[kind]['grid']} {p[kind]['lds']}")


def write(table):
    t = {}
    for line in open(table):
        name, kern, grid, wg, lds, imgs = [c.strip() for c in line.split("|")]
        if name not in t:  # (the first kernel of the launch; a slab reduction may follow)
            t[name] = [kern, int(grid), int(wg), int(lds), int(imgs)]
    es = [dict(e, launch={kind: t[f"{e['name']}/{kind}"] for kind in KINDS}) for e in entries()]
    with open(OUT, "w") as f:
        f.write('{"launch": "per kind [kernel<template arguments>, workgroups, workgroup size, dynamic LDS bytes, images per '
                'group] of the commit before the conv+pool planner, on an MI355X (256 CUs) with no DISTRIFLOW_DIAG switch set; ws: '
                'weight-gradient workspace floats",\n "entries": [\n')
        f.write(",\n".join("  " + json.dumps(e) for e in es))
        f.write("\n]}\n")
    print(f"{len(es)} entries -> {OUT}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", nargs=2, metavar=("ENTRY", "KIND"))
    ap.add_argument("--reduce", metavar="DIR")
    ap.add_argument("--sizes", metavar="FILE")
    ap.add_argument("--plan-sizes", action="store_true")
    ap.add_argument("--write", metavar="TABLE")
    ap.add_argument("--list", action="store_true", help="print 'entry kind' for every launch of the list")
    a = ap.parse_args()
    if a.launch:
        launch(*a.launch)
    if a.list:
        print("\n".join(f"{e['name']} {kind}" for e in entries() for kind in KINDS))
    if a.plan_sizes:
        plan_sizes()
    if a.reduce:
        reduce_traces(a.reduce, a.sizes)
    if a.write:
        write(a.write)
