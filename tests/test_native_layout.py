"""Host-side launch layouts of the native extension that need no GPU: the LeNet-5 images-per-workgroup
policy (csrc/lenet_fused.hip lenet_ipw / lenet_blocks), the irregular-geometry routing of the conv
dispatch (csrc/bindings_util.h set_conv_geom: only the generic implicit GEMM takes it), the parameter
server's buffer layout (csrc/ps_layout.h), the dense head's error-word offset (csrc/khead.hip) and the
launch plan of the forward / data-gradient implicit GEMMs (csrc/conv_plan.hip)."""
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
