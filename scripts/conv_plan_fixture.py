"""Record tests/golden/conv_plan.json: the conv / dense launch decisions over a fixed shape list.

    python scripts/conv_plan_fixture.py            # (re)record the query answers, keep recorded launches
    python scripts/conv_plan_fixture.py --launches profiles/conv_plan/<table>.txt   # add the launch table

The shape list is every Conv2D and Dense of lenet5, keras_cnn and resnet18_cifar at B in {1, 4, 32, 256,
1024}, forward and data gradient, plus a hand list that reaches each branch of the dispatch at its
smallest shape (``hand_list``; scripts/conv_plan_trace.py launches it under the profiler).  No GPU needed.

The answers were recorded at the last commit that had the separate shape-only queries
(``igemm_bacc_supported``, ``igemm64_pool_supported``), which is what makes them a reference for the planner
that replaced them.  (The third query, the in-launch BatchNorm statistics tiles, left with that route and is
no longer recorded.)  On a build without those bindings the script keeps every recorded answer (new entries
get none) and only attaches launch tables.

The weight gradients of the same layers are the ``wgrad`` list of the file: every Conv2D / Dense of the three
models with the workspace ``Net.bind`` gives them (their plan is recorded as it is: a pin, the dispatch that
preceded the planner had no query to record) and a hand list with one smallest shape per branch, each with
its workspace size, whose launches at the last commit before the planner are attached with

    python scripts/conv_plan_fixture.py --wgrad-launches profiles/conv_plan/launches_wgrad_parent.txt
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_plan.json")
BATCHES = (1, 4, 32, 256, 1024)
BACC_VARIANTS = list(itertools.product((0, 1), (False, True), (False, True), (False, True)))  # mode two res mask


def r32(v):
    return -(-v // 32) * 32


def conv(name, B, H, W, C, N, k, stride=1, pad=0, **flags):
    """One conv; forward and data-gradient entries.  k / stride / pad: ints or (row, column) pairs."""
    from distriflow_amd import ops
    KH, KW = ops._pair(k)
    OH, OW = ops.conv_out_hw(H, W, KH, KW, stride, pad)
    if "out_hw" in flags:
        OH, OW = flags.pop("out_hw")
    c = dict(B=B, H=H, W=W, C=C, OH=OH, OW=OW, N=N, KH=KH, KW=KW, stride=stride, pad=pad)
    fwd = dict(name=f"{name}/fwd", mode=1, M=B * OH * OW, N=N, K=KH * KW * C, Kpad=r32(KH * KW * C),
               geom=ops._geom(H, W, C, OH, OW, KH, KW, stride, pad), conv=dict(c, Kpad=r32(KH * KW * C), dgrad=False))
    bwd = dict(name=f"{name}/dgrad", mode=2, M=B * H * W, N=C, K=KH * KW * N, Kpad=r32(KH * KW * N),
               geom=ops._geom(OH, OW, N, H, W, KH, KW, stride, pad), conv=dict(c, Kpad=r32(KH * KW * N), dgrad=True))
    fwd.update(flags)
    return [fwd, bwd]


def dense(name, B, K, N, **flags):
    """One dense layer: forward [B][K] -> [B][N] and data gradient [B][N] -> [B][K] (MODE_DIRECT)."""
    fwd = dict(name=f"{name}/fwd", mode=0, M=B, N=N, K=K, Kpad=r32(K), lda=flags.pop("lda", K), geom=None, conv=None)
    bwd = dict(name=f"{name}/dgrad", mode=0, M=B, N=K, K=N, Kpad=r32(N), lda=N, geom=None, conv=None)
    fwd.update(flags)
    return [fwd, bwd]


def model_list():
    es = []
    for B in BATCHES:
        t = f"lenet5/B{B}"
        es += conv(f"{t}/conv2d_1", B, 28, 28, 1, 6, 5, 1, 2) + conv(f"{t}/conv2d_2", B, 14, 14, 6, 16, 5)
        es += dense(f"{t}/dense_1", B, 400, 120) + dense(f"{t}/dense_2", B, 120, 84) + dense(f"{t}/dense_3", B, 84, 10)
        t = f"keras_cnn/B{B}"
        es += conv(f"{t}/conv2d_1", B, 28, 28, 1, 32, 3) + conv(f"{t}/conv2d_2", B, 26, 26, 32, 32, 3)
        es += dense(f"{t}/dense_1", B, 4608, 128) + dense(f"{t}/dense_2", B, 128, 5)
        t = f"resnet18_cifar/B{B}"
        es += conv(f"{t}/stem", B, 32, 32, 3, 64, 3, 1, 1)
        cin, hw = 64, 32
        for stage, (f, s) in enumerate([(64, 1), (128, 2), (256, 2), (512, 2)]):
            for b in range(2):
                st = s if b == 0 else 1
                n = f"{t}/layer{stage + 1}.{b}"
                es += conv(f"{n}/conv1", B, hw, hw, cin, f, 3, st, 1)
                if st != 1 or cin != f:
                    es += conv(f"{n}/proj", B, hw, hw, cin, f, 1, st, 0)
                hw //= st
                es += conv(f"{n}/conv2", B, hw, hw, f, f, 3, 1, 1)
                cin = f
        es += dense(f"{t}/fc", B, 512, 10)
    return es


def hand_list():
    """Each branch of the dispatch at its smallest shape."""
    es = []
    es += conv("halo_c64", 64, 32, 32, 64, 64, 3, 1, 1)                 # 512 tiles: weights-resident kernel
    es += conv("halo_wide", 256, 16, 16, 128, 128, 3, 1, 1)             # 512 tiles x 1 channel tile of 128
    es += conv("halo_narrow_row", 4, 16, 16, 64, 128, 3, 1, 1)          # 8 tiles: 64-channel tiles, a row per step
    es += conv("halo_ks2_fold", 256, 4, 4, 512, 512, 3, 1, 1)           # 256 workgroups: 2 channel-block splits
    es += conv("halo_ks2_big", 480, 4, 4, 512, 512, 3, 1, 1)            # 480 workgroups, still 2 splits
    es += conv("igemm64_128x32", 4, 26, 26, 32, 32, 3)
    es += conv("igemm64_128x64_slow", 4, 16, 16, 8, 64, 3, 1, 1)        # C = 8: no FAST gather
    es += conv("igemm64_128x64_fast", 4, 16, 16, 64, 64, 3)             # pad 0: not the halo kernel
    es += conv("igemm64_128x128", 64, 32, 32, 64, 128, 1)               # 512 tiles of 128 x 128
    es += conv("igemm64_64x128", 4, 16, 16, 64, 128, 1)
    es += conv("igemm64_split2", 256, 8, 8, 256, 512, 3, 2, 1)          # layer4.0 conv1: 256 tiles, 36 k steps
    es += dense("igemm64_split4", 1024, 4608, 512)
    es += dense("igemm64_split16", 32, 9216, 128)
    es += conv("stride2_parity", 4, 16, 16, 64, 128, 3, 2, 1)           # dgrad gathers 128 channels: FAST, classes
    es += conv("stride2_plain", 4, 16, 16, 16, 32, 3, 2, 1)             # dgrad gathers 32 channels: no FAST
    es += conv("pooled", 4, 26, 26, 32, 32, 3, pooled=True)
    es += conv("smallc_c1", 4, 28, 28, 1, 32, 3) + conv("smallc_c1_5x5", 4, 28, 28, 1, 8, 5, 1, 2)
    es += conv("generic_c3", 4, 32, 32, 3, 64, 3, 1, 1)                 # C % 8 != 0: scalar gather
    es += conv("generic_n16", 4, 14, 14, 6, 16, 5) + conv("generic_big_m", 1024, 8, 8, 3, 16, 1)
    # the irregular geometries of test_irregular_conv_geometry_refuses_specialised_paths (generic, vectorised)
    es += conv("irregular_same", 4, 16, 16, 64, 64, 3, 2, (0, 0), out_hw=(8, 8))
    es += conv("irregular_stride", 4, 16, 16, 64, 64, 3, (2, 1), (1, 1))
    es += conv("irregular_3x5", 4, 16, 16, 64, 64, (3, 5), 1, (1, 2))
    es += dense("generic_dropout", 32, 84, 20, drop=True)               # K % 8 != 0: dropout as its own launch
    es += dense("igemm64_dropout", 32, 128, 64, drop=True)              # folded into the epilogue
    es += dense("direct_aligned", 32, 400, 120) + dense("direct_k_unaligned", 32, 84, 10)
    es += dense("direct_lda_unaligned", 32, 120, 84, lda=124)
    return [dict(e, hand=True) for e in es]


def edge_list():
    return conv("empty_batch", 0, 8, 8, 8, 8, 3, 1, 1)                  # M = 0: nothing to launch


def wgrad(name, B, H, W, C, N, k, stride=1, pad=0, bias=False, ws=1 << 24, **flags):
    """The weight gradient of one conv with a workspace of ``ws`` floats."""
    from distriflow_amd import ops
    KH, KW = ops._pair(k)
    OH, OW = flags.pop("out_hw", None) or ops.conv_out_hw(H, W, KH, KW, stride, pad)
    return [dict(name=name, mode=1, M=B * OH * OW, N=N, K=KH * KW * C, ldd=N, lda=0, bias=bias, ws=ws,
                 geom=ops._geom(H, W, C, OH, OW, KH, KW, stride, pad), **flags)]


def wgrad_dense(name, B, K, N, bias=True, ws=1 << 22):
    return [dict(name=name, mode=0, M=B, N=N, K=K, ldd=N, lda=K, bias=bias, ws=ws, geom=None)]


def wgrad_model_list():
    """The layers of model_list(), with their bias and the workspace Net.bind allocates for the model
    (max(2^22, 4 x the largest conv kernel): resnet18_cifar 4 x 512 x 4608)."""
    es = []
    for e in model_list():
        if not e["name"].endswith("/fwd"):
            continue
        name = e["name"][:-4] + "/wgrad"
        resnet = name.startswith("resnet18")
        ws = 4 * 512 * 4608 if resnet else 1 << 22
        if e["conv"] is None:
            es += wgrad_dense(name, e["M"], e["K"], e["N"], ws=ws)
        else:
            c = e["conv"]
            es += wgrad(name, c["B"], c["H"], c["W"], c["C"], c["N"], c["KH"], c["stride"], c["pad"], bias=not resnet, ws=ws)
    return es


def wgrad_hand_list():
    """Each branch of the weight-gradient dispatch at its smallest shape.  ``diag``: the DISTRIFLOW_DIAG the
    entry is planned and launched under (its own process: the switches are read once)."""
    es = []
    es += wgrad("halo_groups2", 4, 16, 16, 64, 64, 3, 1, 1)              # 16 tiles of 64 pixels: 16 splits
    es += wgrad("halo_ws1", 4, 16, 16, 64, 64, 3, 1, 1, ws=1)            # no slab room: one split writes gw
    es += wgrad("halo_ws2slabs", 4, 16, 16, 64, 64, 3, 1, 1, ws=2 * 64 * 576)
    es += wgrad("halo_groups1", 4, 16, 16, 64, 64, 3, 1, 1, diag="halo_groups=1")
    es += wgrad("tr_128x128_32rows", 8, 16, 16, 64, 128, 3, 2, 1)
    es += wgrad("tr_n32", 4, 26, 26, 32, 32, 3)
    es += wgrad("tr_64", 2, 16, 16, 16, 64, 3, 1, 1)
    es += wgrad("tr_bias", 3, 9, 7, 16, 24, 3, 2, 1, bias=True)
    es += wgrad("c1", 4, 28, 28, 1, 32, 3, bias=True, ws=1 << 22)
    es += wgrad("c1_small_ws", 8, 28, 28, 1, 32, 3, bias=True, ws=1000)  # 4 image-pair slabs of 320 do not fit
    es += wgrad("smallc_5x5", 4, 28, 28, 1, 8, 5, 1, 2, bias=True, ws=1 << 22)
    es += wgrad("generic_n16", 4, 14, 14, 6, 16, 5, bias=True, ws=1 << 22)   # C % 8 != 0: no XVEC
    es += wgrad("generic_n32", 4, 8, 8, 3, 32, 3, 1, 1, ws=1 << 22)
    es += wgrad("generic_n64", 4, 32, 32, 3, 64, 3, 1, 1, ws=1 << 22)
    es += wgrad("generic_no_dvec", 4, 28, 28, 1, 6, 5, 1, 2, bias=True, ws=1 << 22)  # N % 8 != 0
    es += wgrad("generic_capped", 8, 14, 14, 6, 16, 5, bias=True, ws=3000)   # 13 splits of 2416 floats wanted
    es += wgrad_dense("direct_aligned", 32, 400, 120) + wgrad_dense("direct_unaligned", 32, 84, 10)
    es += wgrad_dense("direct_no_dvec", 32, 400, 10)                     # XVEC without DVEC
    es += wgrad("irregular_same", 4, 16, 16, 64, 64, 3, 2, (0, 0), out_hw=(8, 8))
    es += wgrad("irregular_stride", 4, 16, 16, 64, 64, 3, (2, 1), (1, 1))
    es += wgrad("irregular_3x5", 4, 16, 16, 64, 64, (3, 5), 1, (1, 2))
    es += wgrad("empty_batch", 0, 8, 8, 8, 8, 3, 1, 1)                   # M = 0: nothing to launch
    return [dict(e, hand=True) for e in es]


def wgrad_plan_of(e, m):
    geom = e["geom"] if e["geom"] is not None else [1, 1, 1, 1, 1, 1, 1, 1, 0]
    return m.wgrad_plan(e["M"], e["N"], e["K"], e["ldd"], e["lda"], geom, e["mode"], e["bias"], e["ws"])


def record(e, m):
    """The parent's answers: the shape-only queries of the native extension (BatchNorm sums, pooling)."""
    geom = e["geom"] if e["geom"] is not None else [1, 1, 1, 1, 1, 1, 1, 1, 0]
    args = (e["M"], e["N"], e["K"], e["Kpad"], geom, e["mode"])
    e["bacc"] = "".join("1" if m.igemm_bacc_supported(*args, bm, two, res, mask) else "0"
                        for bm, two, res, mask in BACC_VARIANTS)
    c = e["conv"]
    if e["mode"] == 1 and c["KH"] == c["KW"] and isinstance(c["stride"], int) and isinstance(c["pad"], int):
        from distriflow_amd import ops  # (the pool query knows regular geometries only: Net asks it for no other)
        e["pool"] = bool(ops.conv_pool_supported(c["H"], c["W"], c["C"], c["KH"], c["KW"], c["stride"], c["pad"], e["N"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", help="reduced launch table (scripts/conv_plan_trace.py --reduce) to attach")
    ap.add_argument("--wgrad-launches", help="the same for the weight-gradient hand list (--reduce-wgrad)")
    a = ap.parse_args()
    from distriflow_amd import native
    m = native.get(build_if_missing=False)
    entries = model_list() + hand_list() + edge_list()
    wentries = wgrad_model_list() + wgrad_hand_list()
    old, wold = {}, {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            j = json.load(f)
        old = {e["name"]: e for e in j["entries"]}
        wold = {e["name"]: e for e in j.get("wgrad", [])}
    for e in entries:
        if hasattr(m, "igemm_bacc_supported"):
            record(e, m)
        else:  # the recorded queries are gone: keep their answers
            for k in ("bacc", "pool"):
                if k in old.get(e["name"], {}):
                    e[k] = old[e["name"]][k]
        if "launch" in old.get(e["name"], {}):
            e["launch"] = old[e["name"]]["launch"]
    if a.launches:
        from conv_plan_trace import read_table
        for name, rows in read_table(a.launches).items():
            next(e for e in entries if e["name"] == name)["launch"] = rows
    wrows = {}
    if a.wgrad_launches:
        from conv_plan_trace import read_table
        wrows = read_table(a.wgrad_launches)
    for e in wentries:
        if e.get("hand"):  # (an entry that launches nothing has no row)
            e["launch"] = wrows.get(e["name"], []) if a.wgrad_launches else wold.get(e["name"], {}).get("launch")
        elif hasattr(m, "wgrad_plan"):
            e["plan"] = wgrad_plan_of(e, m)
        else:
            e["plan"] = wold.get(e["name"], {}).get("plan")
    with open(OUT, "w") as f:
        f.write('{"bacc_variants": "bacc_mode two has_res has_mask, in itertools.product order",\n "entries": [\n')
        f.write(",\n".join("  " + json.dumps(e) for e in entries))
        f.write("\n],\n \"wgrad\": [\n")
        f.write(",\n".join("  " + json.dumps(e) for e in wentries))
        f.write("\n]}\n")
    print(f"{len(entries)} + {len(wentries)} entries -> {OUT}")


if __name__ == "__main__":
    main()
