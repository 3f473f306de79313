"""Host-side launch layouts of the native extension that need no GPU: the LeNet-5 images-per-workgroup
policy (csrc/lenet_fused.hip lenet_ipw / lenet_blocks), the irregular-geometry routing of the conv
dispatch (csrc/bindings_util.h set_conv_geom: only the generic implicit GEMM takes it), the parameter
server's buffer layout (csrc/ps_layout.h), the dense head's error-word offset (csrc/khead.hip) and the
launch plans of the forward / data-gradient and the weight-gradient implicit GEMMs (csrc/conv_plan.hip)."""
import itertools
import json
import os
import shutil
import subprocess
import sys

import pytest

from distriflow_amd import native, ops

m = native.get(build_if_missing=False)
needs_ext = pytest.mark.skipif(m is None, reason="native extension not built")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")


def test_ps_layout_header_is_host_only_and_pinned(tmp_path):
    """csrc/ps_layout.h alone compiles with the host compiler (no HIP, no torch): its static_asserts pin
    every PSCtrl / PSLocal field to its byte offset."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tu = tmp_path / "ps_layout_tu.cpp"
    tu.write_text('#include "ps_layout.h"\n')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", CSRC, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@needs_ext
@pytest.mark.parametrize("B", [1, 32, 33, 1024])
def test_khead_err_offset(B):
    """The error word follows the split-K slabs, dz1, two words per 32-row tile, the tag and the done counter
    (the expression ops.khead_error used to hard-code), and is the workspace's last float."""
    nt = -(-B // 32)
    assert m.khead_err_offset(B) == nt * 8 * 32 * 128 + nt * 32 * 128 // 2 + 2 * nt + 2
    assert m.khead_err_offset(B) == m.khead_ws_floats(B, 4608) - 1
    assert m.khead_supported(4608, 10)


@needs_ext
@pytest.mark.parametrize("B,ipw", [(1, 1), (32, 1), (256, 1), (257, 2), (512, 2), (513, 4), (1024, 4),
                                   (1025, 8), (2048, 8), (2049, 8), (4096, 8), (8192, 8)])
def test_lenet_images_per_workgroup(B, ipw):
    """One workgroup per CU (256) with the fewest images per workgroup, else 8 (the full-batch kernel)."""
    assert ops.lenet_blocks(B) == -(-B // ipw)


@needs_ext
def test_irregular_conv_geometry_refuses_specialised_paths():
    """A regular 3x3 / stride 1 / pad 1 64-channel conv may accumulate BatchNorm sums in the specialised
    kernels' epilogues in both directions; the same conv with asymmetric padding, a (2, 1) stride or a 3x5
    kernel runs on the generic kernel, whose epilogue takes the forward sums only (mode 0)."""
    B, H, W, C, N = 4, 16, 16, 64, 64

    def ok(KH, KW, stride, pad, OH, OW, dgrad):
        Kp = -(-(KH * KW * (N if dgrad else C)) // 32) * 32
        return ops.conv_bacc_ok(B, H, W, C, OH, OW, N, KH, KW, stride, pad, Kp, dgrad=dgrad, mode=1 if dgrad else 0,
                                has_mask=dgrad)

    assert ok(3, 3, 1, 1, 16, 16, True)
    assert not ok(3, 3, 2, (0, 0), 8, 8, True)          # odd 'same' total: pad 0 top / left, 1 bottom / right
    assert not ok(3, 3, (2, 1), (1, 1), 8, 16, True)
    assert not ok(3, 5, 1, (1, 2), 16, 16, True)
    assert ok(3, 5, 1, (1, 2), 16, 16, False)            # generic forward: epilogue sums, mode 0


# ---------------------------------------------------------------------------- conv launch plan
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")
BACC_VARIANTS = list(itertools.product((0, 1), (False, True), (False, True), (False, True)))  # mode two res mask
FAMILY_OF_KERNEL = {"conv3_halo_c64_kernel": "halo_c64", "conv3_halo_kernel": "halo", "igemm64_kernel": "igemm64",
                    "c1_fwd_kernel": "smallc", "smallc_fwd_kernel": "smallc", "igemm_fwd_kernel": "generic"}


def _plan_args(e):
    geom = e["geom"] if e["geom"] is not None else [1, 1, 1, 1, 1, 1, 1, 1, 0]
    return (e["M"], e["N"], e["K"], e["Kpad"], geom, e["mode"]), dict(lda=e.get("lda", 0))


def _check_launch(e, p):
    """The plan against the kernels the parent launched for this entry (name<template flags>, workgroups,
    workgroup size, LDS bytes; profiles/conv_plan/launches_parent.txt)."""
    rows = e["launch"]
    kern, grid, block, _ = rows[0]
    name, _, targs = kern.partition("<")
    t = [{"true": True, "false": False}.get(v, v) for v in targs.rstrip(">").split(",")] if targs else []
    assert p["family"] == FAMILY_OF_KERNEL[name], e["name"]
    if p["family"] == "igemm64":
        want = dict(BM=int(t[0]), BN=int(t[1]), fast=t[6], par=t[7], pool=t[5])
        assert int(t[2]) == e["mode"] and (p["splits"] > 1) == t[4], e["name"]
    elif p["family"] == "halo":
        want = dict(BN=int(t[0]), wide=int(t[0]) == 128, row=t[2])
        assert t[1] == (e["mode"] == 2), e["name"]
    elif p["family"] == "generic":
        want = dict(BM=int(t[0]), BN=int(t[1]), vec=t[5])
        assert int(t[4]) == e["mode"], e["name"]
    else:
        want = {}
    assert {k: p[k] for k in want} == want, e["name"]
    if p["family"] != "smallc":  # (the C = 1 kernels size their own launch)
        assert (p["grid"], p["block"]) == (grid, block), e["name"]
    followers = [r[0] for r in rows[1:]]
    assert followers == ["igemm64_splitk_epilogue_kernel"] * p["combine"] + ["dropout_kernel"] * p["drop_after"], e["name"]


@needs_ext
def test_conv_plan_matches_recorded_decisions():
    """Over every Conv2D / Dense of lenet5, keras_cnn and resnet18_cifar at five batch sizes and a hand list
    that reaches each branch of the dispatch (scripts/conv_plan_fixture.py), the queries answer what the three
    separate query bindings answered before the planner existed (tests/golden/conv_plan.json: BatchNorm sums
    in 16 variants, pooling), and the plan names the kernels, template flags and grids the
    parent build launched on the GPU for the hand list.  The list keeps reaching every family and both values of
    every variant flag."""
    with open(GOLDEN) as f:
        entries = json.load(f)["entries"]
    families, flags, launches, base = set(), {}, 0, []
    for e in entries:
        args, kw = _plan_args(e)
        p = m.conv_plan(*args, pooled=bool(e.get("pooled")), drop=bool(e.get("drop")), **kw)
        plans = [p]
        base.append(p)
        for i, (bm, two, res, mask) in enumerate(BACC_VARIANTS):
            q = m.conv_plan(*args, bacc_mode=bm, two=two, has_res=res, has_mask=mask, **kw)
            assert q["bacc_ok"] == (e["bacc"][i] == "1"), (e["name"], i)
            assert (q["family"] == "invalid") == (not q["bacc_ok"] and e["M"] > 0), (e["name"], i)
            plans.append(q)
        c = e["conv"]
        if c is not None:  # the ops wrappers, as the layers call them
            g = (c["B"], c["H"], c["W"], c["C"], c["OH"], c["OW"], c["N"], c["KH"], c["KW"], c["stride"], c["pad"], c["Kpad"])
            got = "".join("01"[ops.conv_bacc_ok(*g, dgrad=c["dgrad"], mode=bm, two=two, has_res=res, has_mask=mask)]
                          for bm, two, res, mask in BACC_VARIANTS)
            assert got == e["bacc"], e["name"]
            if "pool" in e:
                assert ops.conv_pool_supported(c["H"], c["W"], c["C"], c["KH"], c["KW"], c["stride"], c["pad"],
                                               c["N"]) == e["pool"], e["name"]
        if "launch" in e:
            _check_launch(e, p)
            launches += 1
        for q in plans:
            families.add(q["family"])
            for k in ("fast", "par", "pool", "wide", "row", "fold", "vec", "combine", "drop_after", "bacc_ok"):
                flags.setdefault(k, set()).add(q[k])
            flags.setdefault("split", set()).add(q["splits"] > 1)
            flags.setdefault("ks", set()).add(q["ks"] > 1)
            flags.setdefault("scratch", set()).add(q["splitk_floats"] > 0)
    assert families == {"nop", "invalid", "halo_c64", "halo", "igemm64", "smallc", "generic"}
    assert all(v == {False, True} for v in flags.values()), flags
    assert {q["splits"] for q in base} >= {1, 2, 4, 16}
    assert {(q["BM"], q["BN"]) for q in base if q["family"] == "igemm64"} == {(128, 32), (128, 64), (128, 128), (64, 128)}
    assert launches == 58


@needs_ext
def test_conv_plan_reads_the_diagnostic_switches():
    """DISTRIFLOW_DIAG is read once per process, so a child: with conv_halo=0 a 3x3 / stride 1 / pad 1 conv of
    512 channels (a halo shape, two channel-block splits by default) plans as igemm64, and igemm_splitk=0
    leaves it without split-K scratch."""
    code = ("from distriflow_amd import ops\n"
            "p = ops.conv_plan(256, 4, 4, 512, 4, 4, 512, 3, 3, 1, 1, 4608)\n"
            "print(p['family'], p['splits'], p['splitk_floats'])\n")
    root = os.path.dirname(CSRC)

    def run(diag):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root,
                           env=dict(os.environ, DISTRIFLOW_DIAG=diag))
        assert r.returncode == 0, r.stderr
        return r.stdout.split()

    assert m.conv_plan(4096, 512, 4608, 4608, [4, 4, 512, 4, 4, 3, 3, 1, 1], 1)["family"] == "halo"
    assert run("conv_halo=0") == ["igemm64", "4", str(4 * 4096 * 512)]
    assert run("conv_halo=0,igemm_splitk=0") == ["igemm64", "1", "0"]


# ---------------------------------------------------------------------------- weight-gradient launch plan
WGRAD_FAMILY_OF_KERNEL = {"wgrad_halo_kernel": "halo", "wgrad_tr_kernel": "tr", "c1_wgrad_kernel": "c1",
                          "smallc_wgrad_kernel": "smallc", "igemm_wgrad_kernel": "generic"}
ROOT = os.path.dirname(CSRC)


def _wgrad_args(e):
    geom = e["geom"] if e["geom"] is not None else [1, 1, 1, 1, 1, 1, 1, 1, 0]
    return [e["M"], e["N"], e["K"], e["ldd"], e["lda"], geom, e["mode"], e["bias"], e["ws"]]


def _wgrad_plans_under(diag, calls):
    """DISTRIFLOW_DIAG is read once per process: the plans of ``calls`` (_C.wgrad_plan argument lists) in a child."""
    code = ("import json, sys\nfrom distriflow_amd import native\nm = native.get(build_if_missing=False)\n"
            "print(json.dumps([m.wgrad_plan(*c) for c in json.load(sys.stdin)]))\n")
    r = subprocess.run([sys.executable, "-c", code], input=json.dumps(calls), capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, DISTRIFLOW_DIAG=diag))
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _check_wgrad_launch(e, p):
    """The plan against what the last commit before the planner launched for this entry
    (profiles/conv_plan/launches_wgrad_parent.txt): kernel, template arguments, workgroups, workgroup size, and
    whether a slab_reduce_* launch follows."""
    rows = e["launch"]
    if not rows:
        assert p["family"] == "nop" and e["M"] == 0, e["name"]
        return
    kern, grid, block, _ = rows[0]
    name, _, targs = kern.partition("<")
    t = [{"true": True, "false": False}.get(v, v) for v in targs.rstrip(">").split(",")] if targs else []
    assert p["family"] == WGRAD_FAMILY_OF_KERNEL[name], e["name"]
    if p["family"] == "halo":
        want = dict(groups=int(t[0]))
    elif p["family"] == "tr":
        want = dict(zip(("BN", "BK", "WN", "WK", "BM", "MAXOCC"), map(int, t)))
    elif p["family"] == "generic":
        want = dict(BN=int(t[0]), BK=int(t[1]), WN=int(t[2]), WK=int(t[3]), dvec=t[5], xvec=t[6])
        assert int(t[4]) == e["mode"], e["name"]
    else:
        want = {}
    assert {k: p[k] for k in want} == want, e["name"]
    assert (p["grid"], p["block"]) == (grid, block), e["name"]
    followers = [r[0] for r in rows[1:]]
    assert len(followers) == int(p["reduce"]) and all(f.startswith("slab_reduce_") for f in followers), e["name"]


@needs_ext
def test_wgrad_plan_matches_recorded_launches():
    """For a hand list with one smallest shape per branch of the weight-gradient dispatch, each with its
    workspace size (scripts/conv_plan_fixture.py wgrad_hand_list), the plan names the kernel, template
    arguments, grid and workgroup size that the dispatch launched on the GPU before the planner existed, and
    says whether a slab reduction follows.  The list keeps reaching every family and both values of capped,
    reduce, the halo group count, DVEC and XVEC; the scratch is 0 exactly without a reduction and within the
    workspace wherever the kernel can honour a cap (the C = 1 kernels always write one slab).  Every Conv2D /
    Dense of the three models plans as recorded (a pin of the plan itself)."""
    with open(GOLDEN) as f:
        entries = json.load(f)["wgrad"]
    hand = [e for e in entries if e.get("hand")]
    plans = {e["name"]: m.wgrad_plan(*_wgrad_args(e)) for e in hand if not e.get("diag")}
    for diag in sorted({e["diag"] for e in hand if e.get("diag")}):
        es = [e for e in hand if e.get("diag") == diag]
        plans.update(zip([e["name"] for e in es], _wgrad_plans_under(diag, [_wgrad_args(e) for e in es])))
    seen = {}
    for e in hand:
        p = plans[e["name"]]
        _check_wgrad_launch(e, p)
        assert p["capped"] == (p["scratch_floats"] < p["wanted_floats"]), e["name"]
        assert (p["scratch_floats"] == 0) == (not p["reduce"]), e["name"]
        if p["family"] not in ("c1", "smallc"):
            assert p["scratch_floats"] <= e["ws"], e["name"]
        for k in ("family", "capped", "reduce"):
            seen.setdefault(k, set()).add(p[k])
        if p["family"] in ("halo", "generic"):
            for k in ("groups",) if p["family"] == "halo" else ("dvec", "xvec"):
                seen.setdefault(k, set()).add(p[k])
    assert seen == dict(family={"nop", "halo", "tr", "c1", "smallc", "generic"}, capped={False, True},
                        reduce={False, True}, groups={1, 2}, dvec={False, True}, xvec={False, True}), seen
    assert {e["name"] for e in hand if e["name"].startswith("irregular")} == \
        {"irregular_same", "irregular_stride", "irregular_3x5"}
    assert all(plans[e["name"]]["family"] == "generic" for e in hand if e["name"].startswith("irregular"))
    assert sum(len(e["launch"]) for e in hand) == 38
    assert (plans["halo_ws1"]["splits"], plans["halo_ws2slabs"]["splits"], plans["c1_small_ws"]["family"]) == (1, 2, "smallc")
    models = [e for e in entries if not e.get("hand")]
    assert len(models) == 150
    for e in models:
        assert m.wgrad_plan(*_wgrad_args(e)) == e["plan"], e["name"]


@needs_ext
@pytest.mark.parametrize("model,B", [("lenet5", 4096), ("keras_cnn", 1024), ("resnet18_cifar", 256)])
def test_wgrad_workspace_of_bind_caps_no_layer(model, B):
    """With the workspace Net.bind allocates (max(2^22, 4 x the largest conv kernel) floats) no Conv2D / Dense
    of the three benchmark configurations gets fewer splits than its policy asks for.  ResNet-18 only just:
    its 3x3 64 -> 64 halo layers want 256 slabs of 36 864 floats, exactly 4 x the 512 x 4608 kernel."""
    from distriflow_amd.models.layers import Conv2D, Dense, FusedConvPool
    from distriflow_amd.models.zoo import build_model
    net = build_model(model, device="cpu", seed=0)
    ws = net.wgrad_ws_floats()
    leaves = list(net._all_leaf_layers())
    convs = net.wgrad_layers() + [l.conv for l in leaves if isinstance(l, FusedConvPool)]
    assert convs or model == "lenet5"
    wanted = 0
    for l in convs:
        assert isinstance(l, Conv2D)
        (H, W, C), (OH, OW, N) = l.in_shape, l.out_shape
        p = ops.wgrad_plan(B, H, W, C, OH, OW, N, *l.geom, l.use_bias, ws)
        assert p["family"] != "nop" and not p["capped"], (l.name, p)
        wanted = max(wanted, p["wanted_floats"])
    for l in leaves:
        if isinstance(l, Dense):
            p = ops.dense_wgrad_plan(B, l.in_features, l.units, l.use_bias, ws)
            assert p["family"] == "generic" and not p["capped"], (l.name, p)
    if model == "resnet18_cifar":
        assert wanted == ws == 9437184
        # the sizing is not a bound: a model whose largest 3x3 conv is 64 -> 64 gets 2^22 floats, room for 113
        # slabs; 4096 tiles in splits of 37 are 111
        q = ops.wgrad_plan(B, 32, 32, 64, 32, 32, 64, 3, 3, 1, 1, False, 1 << 22)
        assert q["capped"] and (q["splits"], q["tps"], q["wanted_floats"]) == (111, 37, 9437184)


@needs_ext
def test_wgrad_plan_reads_the_diagnostic_switches():
    """In a child each (the switches are read once per process): with wgrad_halo=0 a 3x3 / stride 1 / pad 1
    conv with C = N = 64 plans as transposed-read, with halo_groups=1 it plans 256-thread workgroups."""
    call = [4 * 16 * 16, 64, 576, 64, 0, [16, 16, 64, 16, 16, 3, 3, 1, 1], 1, False, 1 << 24]
    p = m.wgrad_plan(*call)
    assert (p["family"], p["groups"], p["block"]) == ("halo", 2, 512)
    q = _wgrad_plans_under("wgrad_halo=0", [call])[0]
    assert (q["family"], q["BN"], q["BM"]) == ("tr", 64, 32)
    q = _wgrad_plans_under("halo_groups=1", [call])[0]
    assert (q["family"], q["groups"], q["block"]) == ("halo", 1, 256)


# ---------------------------------------------------------------------------- fused conv+pool dispatch keys
@needs_ext
def test_convpool_cases_cover_their_dispatch_keys():
    """tests/golden/convpool_cases.json (scripts/convpool_cases.py), the shape list of the exact conv+pool tests:
    every case is a supported geometry whose three dispatch keys, read from its plan, are the recorded ones (and
    each launch's instantiation is one of the instantiated list and holds the key's step count), and together the cases reach every key value the file's header lists as covered by the
    enumerated space: forward (pair, channel tiles, k steps), weight gradient (channel tiles, k tiles with the
    bias column), data gradient (pair | vec | scalar, k steps)."""
    with open(os.path.join(os.path.dirname(GOLDEN), "convpool_cases.json")) as f:
        j = json.load(f)
    seen = {"fwd": set(), "wgrad": set(), "dgrad": set()}
    for c in j["cases"]:
        H, W, C, N, k, pad = (c[n] for n in ("H", "W", "C", "N", "k", "pad"))
        p = ops.convpool_plan(H, W, C, k, k, pad, N)
        assert p["ok"] and ops.convpool_supported(H, W, C, k, k, pad, N), c
        for kind in seen:
            v = tuple(p[kind]["key"])
            assert v == tuple(c[kind]), (c, kind, v)
            assert p[kind]["instance"] in p[kind]["instantiated"] and p[kind]["instance"] >= v[-1], (c, kind, p[kind])
            seen[kind].add(v)
    for kind, vals in j["covered"].items():
        assert seen[kind] == {tuple(v) for v in vals}, kind
    # both forward modes, both channel-tile counts everywhere, all three data-gradient kernels
    assert {v[0] for v in seen["fwd"]} == {0, 1} and {v[1] for v in seen["fwd"]} == {1, 2}
    assert {v[0] for v in seen["wgrad"]} == {1, 2} and {v[0] for v in seen["dgrad"]} == {"pair", "vec", "scalar"}


# ---------------------------------------------------------------------------- fused conv+pool launch plan
def _convpool_plan_entries():
    with open(os.path.join(os.path.dirname(GOLDEN), "convpool_plan.json")) as f:
        return json.load(f)["entries"]


def _targs(kernel, name):
    """The template arguments of 'name<a,b,...>' (ints, booleans)."""
    head, _, targs = kernel.partition("<")
    assert head == name, kernel
    return [{"true": True, "false": False}.get(v) if v in ("true", "false") else int(v) for v in targs.rstrip(">").split(",")]


@needs_ext
def test_convpool_plan_names_recorded_kernels():
    """For every entry of tests/golden/convpool_plan.json (scripts/convpool_plan_fixture.py: the cases of
    convpool_cases.json, LeNet-5's two conv blocks at B in {3, 64, 4096}, the small-workspace weight gradient)
    the plan names, for all three launches, the kernel instantiation that the commit before the planner launched
    on the GPU: convpool_fwd_kernel<NT, NK, 4, PAIR>, convpool_wgrad_kernel<NT, KTMAX, 4> and
    convpool_dgrad_kernel<1, NKMAX, VEC, 4, PAIR> (4: the staged variants, which aligned operands take)."""
    entries = _convpool_plan_entries()
    assert len(entries) == 32
    seen = set()
    for e in entries:
        p = ops.convpool_plan(e["H"], e["W"], e["C"], e["k"], e["k"], e["pad"], e["N"])
        assert p["ok"], e["name"]
        f, w, d = p["fwd"], p["wgrad"], p["dgrad"]
        assert _targs(e["launch"]["fwd"][0], "convpool_fwd_kernel") == [f["key"][1], f["instance"], 4, bool(f["key"][0])], e["name"]
        assert _targs(e["launch"]["wgrad"][0], "convpool_wgrad_kernel") == [w["key"][0], w["instance"], 4], e["name"]
        kind = d["key"][0]
        assert _targs(e["launch"]["dgrad"][0], "convpool_dgrad_kernel") == \
            [1, d["instance"], kind != "scalar", 4, kind == "pair"], e["name"]
        assert (kind == "pair") == bool(p["dgrad_pair"]) and bool(f["key"][0]) == bool(p["pair"]), e["name"]
        seen |= {e["launch"][k][0] for k in ("fwd", "wgrad", "dgrad")}
    assert len(seen) == 35   # of the 48 staged instantiations: what the list keeps reaching


@pytest.mark.gpu
def test_convpool_plan_sizes_recorded_launches():
    """Nothing is launched: for every entry of the same list, ops.convpool_plan with the entry's batch and
    weight-gradient workspace gives the workgroups, dynamic LDS bytes and images per group that the commit before
    the planner launched with (recorded on 256 CUs with no DISTRIFLOW_DIAG switch set; cp_wpc and cp_minimgs
    change the sizing), the small workspace halving the weight gradient's grid to two slabs."""
    for e in _convpool_plan_entries():
        p = ops.convpool_plan(e["H"], e["W"], e["C"], e["k"], e["k"], e["pad"], e["N"], B=e["B"], ws_floats=e["ws"])
        for kind in ("fwd", "wgrad", "dgrad"):
            _, grid, block, lds, imgs = e["launch"][kind]
            assert (p[kind]["grid"], p[kind]["lds"], p[kind]["imgs"], block) == (grid, lds, imgs, 256), (e["name"], kind)
        if e["name"] == "small_workspace":
            assert p["wgrad"]["grid"] == 2 and e["ws"] == 2 * e["N"] * (e["k"] * e["k"] * e["C"] + 1)
