"""The accumulated BatchNorm route at kernel level: the conv epilogues that sum what they store
(csrc/bn_acc.h), ``gap_bwd_bn``, and the consumers ``bn_apply_acc`` / ``bn_dx_acc`` that finalise the sums.

Producers run on integer-valued data (tests/exact_util.py): the stored output, its per-channel sums and their
fp64 replicas are exactly representable, so every comparison with the fp64 reference is ``torch.equal``.  The
conditions under which that holds are asserted on the reference alone, for every case, also by a CPU test
(``test_cases_meet_the_conditions_of_exactness``), so no case is vacuous.  Every case asserts through
``ops.conv_plan`` which kernel variant runs it: a change of the planner's thresholds fails the test instead of
moving the case to another kernel.  No diagnostic switch is set anywhere in this module; the halo kernel's
separate combine launch (ks > 1 without the folded last arriver) is unreachable with default switches and is
not covered.

Consumers run on random bf16 data against fp64, within bounds that follow from the number formats
(``exact_util.assert_within_ulps``, ``assert_close_elem``), none of them measured.
"""
import functools

import pytest
import torch

import exact_util as xu
from distriflow_amd import ops

gpu = pytest.mark.gpu
dev = "cuda"

OUT_SENTINEL = 1024.0       # a bf16 value no exact output reaches (|y| <= 256)
ACC_SENTINEL = 12345.678    # what the replica behind the last one holds
TAIL = 4096                 # sentinel elements behind the output


def _plan_subset(plan, expect):
    return {k: plan[k] for k in expect}


# ---------------------------------------------------------------------------------------------- cases
# name, (B, H, W, C, N, k, stride, pad), bias, what ops.conv_plan(..., bacc_mode=0) must answer.
# The halo kernels take no bias (with one the planner hands the shape to igemm64), so those cases run without.
FWD_CASES = [
    ("generic_bn32_tails", (3, 9, 7, 3, 24, 3, 1, 1), True, dict(family="generic", BM=64, BN=32, grid=3)),
    ("generic_bn16", (2, 14, 14, 6, 16, 5, 1, 0), True, dict(family="generic", BM=64, BN=16, grid=4)),
    ("generic_bn128_n1000", (1, 5, 5, 3, 1000, 1, 1, 0), True, dict(family="generic", BM=64, BN=128, grid=8)),
    ("igemm64_128x32_n16_m189", (3, 9, 7, 8, 16, 3, 1, 1), True,
     dict(family="igemm64", BM=128, BN=32, fast=False, splits=1, grid=2)),
    ("igemm64_128x64_fast_m180", (3, 10, 6, 64, 64, 3, 1, 1), True,
     dict(family="igemm64", BM=128, BN=64, fast=True, splits=1, grid=2)),
    ("igemm64_64x128_fast_1x1_m70", (2, 5, 7, 64, 128, 1, 1, 0), True,
     dict(family="igemm64", BM=64, BN=128, fast=True, splits=1, grid=2)),
    ("igemm64_64x128_n1024", (2, 4, 4, 64, 1024, 1, 1, 0), True,
     dict(family="igemm64", BM=64, BN=128, fast=True, splits=1, grid=8)),
    # 128 x 128 tiles need >= 512 of them.  M = 65 * 1024 is 520 whole tiles; M = 66 * 32 * 31 = 511 tiles + 64 rows
    ("igemm64_128x128", (65, 32, 32, 8, 128, 3, 1, 1), True,
     dict(family="igemm64", BM=128, BN=128, fast=False, splits=1, grid=520)),
    ("igemm64_128x128_m_tail", (66, 32, 31, 8, 128, 3, 1, 1), True,
     dict(family="igemm64", BM=128, BN=128, fast=False, splits=1, grid=512)),
    ("igemm64_splitk8_m48", (3, 4, 4, 256, 512, 3, 1, 1), True,
     dict(family="igemm64", BM=64, BN=128, splits=8, combine=True, grid=32)),
    ("igemm64_splitk16_m48", (3, 4, 4, 512, 512, 3, 1, 1), True,
     dict(family="igemm64", BM=64, BN=128, splits=16, combine=True, grid=64)),
    ("halo_row_one_tile", (2, 8, 8, 64, 64, 3, 1, 1), False,
     dict(family="halo", BN=64, row=True, wide=False, ks=1, combine=False, grid=1)),
    ("halo_ks2_fold", (8, 4, 4, 512, 512, 3, 1, 1), False,
     dict(family="halo", BN=64, ks=2, fold=True, combine=False, grid=16)),
    ("halo_wide", (256, 16, 16, 128, 128, 3, 1, 1), False,
     dict(family="halo", BN=128, wide=True, row=False, ks=1, grid=512)),
    ("halo_c64", (64, 32, 32, 64, 64, 3, 1, 1), False, dict(family="halo_c64", block=512, grid=256)),
    ("halo_c64_partial_last", (260, 16, 16, 64, 64, 3, 1, 1), False, dict(family="halo_c64", block=512, grid=130)),
]

# name, dX (B, H, W, C), dY channels N, k, stride, pad, what ops.conv_plan(dgrad, bacc_mode=1) must answer
BWD_CASES = [
    ("halo_row", (4, 16, 16, 64, 64, 3, 1, 1), dict(family="halo", row=True, ks=1, grid=8)),
    ("igemm64_par_odd", (3, 9, 7, 64, 64, 3, 2, 1), dict(family="igemm64", BM=128, BN=64, fast=True, par=True, grid=4)),
    ("igemm64_par_1x1", (2, 7, 9, 128, 64, 1, 2, 0), dict(family="igemm64", BM=64, BN=128, fast=True, par=True, grid=4)),
    ("igemm64_fast_m70", (2, 5, 7, 64, 128, 1, 1, 0),
     dict(family="igemm64", BM=128, BN=64, fast=True, par=False, splits=1, grid=1)),
    ("igemm64_splitk16", (3, 4, 4, 512, 512, 3, 1, 1), dict(family="igemm64", splits=16, combine=True, grid=64)),
    ("halo_c64", (64, 32, 32, 64, 64, 3, 1, 1), dict(family="halo_c64", block=512, grid=256)),
]

GAP_EXACT = [(3, 16, 64), (5, 4, 512), (2, 64, 8), (1, 1, 1024)]  # B, HW (a power of two: dy / HW is exact), C

_ids = lambda cases: [c[0] for c in cases]  # noqa: E731


def _kpad(K):
    return (K + 31) // 32 * 32


@functools.lru_cache(maxsize=2)
def fwd_data(name):
    """x [B][H][W][C] in {-1, 0, 1}, w [N][K] in {-1, 0, 1} with about 64 entries kept per row, bias in
    [-3, 3]: fp64 on the CPU."""
    idx = _ids(FWD_CASES).index(name)
    B, H, W, C, N, k, s, p = FWD_CASES[idx][1]
    g = xu.gen(100 + idx)
    K = k * k * C
    return (xu.ints(g, (B, H, W, C), -1, 1), xu.sparse_ints(g, (N, K), -1, 1, xu.weight_density(K)),
            xu.ints(g, (N,), -3, 3) if FWD_CASES[idx][2] else None)


@functools.lru_cache(maxsize=2)
def bwd_data(name):
    """Integer operands of a data gradient with the block join and two BatchNorms: fp64 on the CPU.  x in
    [-8, 8], integer means and invstd from {1/2, 1, 2} keep xhat a multiple of 1/2."""
    idx = _ids(BWD_CASES).index(name)
    B, H, W, C, N, k, s, p = BWD_CASES[idx][1]
    OH, OW = xu.out_hw(H, W, k, s, p)
    g = xu.gen(200 + idx)
    K = k * k * N
    d = dict(dy=xu.ints(g, (B, OH, OW, N), -1, 1), w=xu.sparse_ints(g, (N, k * k * C), -1, 1, xu.weight_density(K)),
             mask=xu.ints(g, (B, H, W, C), -1, 1), res=xu.ints(g, (B, H, W, C), -2, 2),
             rmask=xu.ints(g, (B, H, W, C), -1, 1))
    for sfx in ("", "2"):
        d["x" + sfx] = xu.ints(g, (B, H, W, C), -8, 8)
        d["mean" + sfx] = xu.ints(g, (C,), -2, 2)
        d["invstd" + sfx] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)]
    return d


def gap_data(B, HW, C):
    g = xu.gen(300 + B + HW + C)
    return dict(dy=xu.ints(g, (B, C), -4, 4), mask=xu.ints(g, (B, HW, C), -1, 1), x=xu.ints(g, (B, HW, C), -8, 8),
                mean=xu.ints(g, (C,), -2, 2),
                invstd=torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)])


def fwd_reference(name, device):
    """Pre-activation fp64 output [B][OH][OW][N] of a forward case, with the conditions of exactness asserted
    (they hold for relu(y) when they hold for y)."""
    k, s, p = FWD_CASES[_ids(FWD_CASES).index(name)][1][5:]
    x, w, b = fwd_data(name)
    y = xu.conv_fwd_ref(x.to(device), w.to(device), b.to(device) if b is not None else None, k, s, p, False)
    xu.assert_exact_output(y)
    xu.assert_exact_sums(y.reshape(-1, y.shape[-1]))
    return y


def bwd_reference(name, join, device):
    """fp64 (g, xhat, xhat2) of a backward case: g the stored data gradient [B][H][W][C]."""
    shape = BWD_CASES[_ids(BWD_CASES).index(name)][1]
    k, s, p = shape[5:]
    d = {key: v.to(device) for key, v in bwd_data(name).items()}
    g = xu.conv_dgrad_ref(d["dy"], d["w"], shape[:4], k, s, p)
    g = xu.join_ref(g, d["res"] if join else None, d["rmask"] if join else None, d["mask"])
    xh = (d["x"] - d["mean"]) * d["invstd"]
    xh2 = (d["x2"] - d["mean2"]) * d["invstd2"]
    C = shape[3]
    xu.assert_exact_output(g)
    xu.assert_exact_bwd_sums(g.reshape(-1, C), xh.reshape(-1, C))
    xu.assert_exact_bwd_sums(g.reshape(-1, C), xh2.reshape(-1, C))
    return g, xh, xh2


def gap_reference(B, HW, C, device):
    d = {key: v.to(device) for key, v in gap_data(B, HW, C).items()}
    g = (d["dy"] / HW).view(B, 1, C) * (d["mask"] > 0)
    xh = (d["x"] - d["mean"]) * d["invstd"]
    return d, g, xh


# ------------------------------------------------------------------------------- conditions (CPU test)
@pytest.mark.parametrize("kind,name", [pytest.param(kind, c, id=f"{kind}-{c}") for kind, c in
                                       [("fwd", n) for n in _ids(FWD_CASES)] + [("bwd", n) for n in _ids(BWD_CASES)]
                                       + [("gap", c) for c in GAP_EXACT]])
def test_cases_meet_the_conditions_of_exactness(kind, name):
    """Generators + reference of every parametrised producer case, on the CPU: the conditions under which
    ``torch.equal`` is the right assertion hold, so nobody finds out on the GPU that a case was vacuous."""
    if kind == "fwd":
        y = fwd_reference(name, "cpu")
        assert float(y.abs().max()) >= 4, "a forward case whose outputs barely vary tests little"
    elif kind == "bwd":
        for join in (False, True):
            g, xh, _ = bwd_reference(name, join, "cpu")
            assert float(g.abs().max()) >= 4 and float(xh.abs().max()) >= 4
    else:
        B, HW, C = name
        _, g, xh = gap_reference(B, HW, C, "cpu")
        # multiples of 1 / (2 HW): exact in fp32 while 2 HW times the sums stays below 2^24
        assert float(g.abs().max()) * HW <= xu.BF16_INT_MAX
        assert float((g * xh).abs().sum((0, 1)).max()) * 2 * HW < xu.FP32_INT_MAX


# ---------------------------------------------------------------------------------- producers, mode 0
def _out_view(shape):
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + TAIL,), OUT_SENTINEL, dtype=torch.bfloat16, device=dev)
    return buf, buf[:n].view(shape)


def _acc_view(nrep, N, rows=None):
    """[rows][2][N] fp64 (default nrep + 1): the first nrep replicas zero and handed to the launch, the rest at
    the sentinel."""
    buf = torch.full((rows or nrep + 1, 2, N), ACC_SENTINEL, dtype=torch.float64, device=dev)
    buf[:nrep] = 0
    return buf, buf[:nrep]


def _assert_guards(outbuf, n, accbuf, nrep):
    assert (outbuf[n:] == OUT_SENTINEL).all(), "wrote behind the output"
    assert (accbuf[nrep:] == ACC_SENTINEL).all(), "touched a replica beyond nrep"


def _run_fwd_case(name, nrep=8):
    idx = _ids(FWD_CASES).index(name)
    _, (B, H, W, C, N, k, s, p), _, expect = FWD_CASES[idx]
    OH, OW = xu.out_hw(H, W, k, s, p)
    plan = ops.conv_plan(B, H, W, C, OH, OW, N, k, k, s, p, _kpad(k * k * C), bacc_mode=0)
    assert plan["bacc_ok"] and _plan_subset(plan, expect) == expect, plan
    x, w, b = fwd_data(name)
    xd, wd = xu.bf16(x, dev), xu.pad_w(w, dev)
    bd = b.float().to(dev) if b is not None else None
    y0 = fwd_reference(name, dev)
    for relu in (False, True):
        ref = y0.relu() if relu else y0
        r2 = ref.reshape(-1, N)
        S, Q = r2.sum(0), (r2 * r2).sum(0)
        outbuf, out = _out_view((B, OH, OW, N))
        accbuf, acc = _acc_view(nrep, N)
        for launch in (1, 2):  # the epilogue adds: a second launch into the same replicas doubles the sums
            out.fill_(OUT_SENTINEL)
            ops.conv_fwd(xd, wd, bd, out, k, k, s, p, relu, bacc=dict(acc=acc, mode=0))
            assert torch.equal(out.double(), ref), f"relu={relu}: output differs from the fp64 reference"
            assert torch.equal(acc.sum(0)[0], launch * S), f"relu={relu} launch {launch}: sum y"
            assert torch.equal(acc.sum(0)[1], launch * Q), f"relu={relu} launch {launch}: sum y^2"
            _assert_guards(outbuf, out.numel(), accbuf, nrep)


@gpu
@pytest.mark.parametrize("name", _ids(FWD_CASES))
def test_conv_fwd_sums_exact(name):
    """Forward sums S = sum y, Q = sum y^2 of the STORED output, with bias (where the family takes one), relu
    off and on, out and acc views of sentinel-guarded buffers."""
    _run_fwd_case(name)


@gpu
def test_conv_fwd_sums_refused_leave_everything_untouched():
    """N / 4 = 6 does not divide 256: the plan with sums is invalid, the binding raises before any launch."""
    B, H, W, C, N, k, s, p = 3, 9, 7, 16, 24, 3, 2, 1
    OH, OW = xu.out_hw(H, W, k, s, p)
    plan = ops.conv_plan(B, H, W, C, OH, OW, N, k, k, s, p, _kpad(k * k * C), bacc_mode=0)
    assert plan["family"] == "invalid" and not plan["bacc_ok"]
    g = xu.gen(7)
    xd = xu.bf16(xu.ints(g, (B, H, W, C), -1, 1), dev)
    wd = xu.pad_w(xu.ints(g, (N, k * k * C), -1, 1), dev)
    outbuf, out = _out_view((B, OH, OW, N))
    accbuf, acc = _acc_view(8, N)
    acc.fill_(ACC_SENTINEL)
    with pytest.raises(RuntimeError, match="bacc"):
        ops.conv_fwd(xd, wd, None, out, k, k, s, p, False, bacc=dict(acc=acc, mode=0))
    torch.cuda.synchronize()
    assert (outbuf == OUT_SENTINEL).all() and (accbuf == ACC_SENTINEL).all()


# ---------------------------------------------------------------------------------- producers, mode 1
def _run_bwd_case(name, combos=((False, False), (False, True), (True, False), (True, True)), nrep=8):
    idx = _ids(BWD_CASES).index(name)
    _, (B, H, W, C, N, k, s, p), expect = BWD_CASES[idx]
    OH, OW = xu.out_hw(H, W, k, s, p)
    d = bwd_data(name)
    dyd, wt = xu.bf16(d["dy"], dev), xu.pad_wt(d["w"], N, k * k, C, dev)
    t = {key: xu.bf16(d[key], dev) for key in ("mask", "res", "rmask", "x", "x2")}
    v = {key: d[key].float().to(dev) for key in ("mean", "invstd", "mean2", "invstd2")}
    for join in (False, True):
        ref = None
        for two in (False, True):
            if (two, join) not in combos:
                continue
            plan = ops.conv_plan(B, H, W, C, OH, OW, N, k, k, s, p, _kpad(k * k * N), dgrad=True, bacc_mode=1,
                                 two=two, has_res=join, has_mask=True)
            assert plan["bacc_ok"] and _plan_subset(plan, expect) == expect, plan
            if ref is None:
                ref = bwd_reference(name, join, dev)
            g, xh, xh2 = ref
            g2 = g.reshape(-1, C)
            S, Q, Q2 = g2.sum(0), (g2 * xh.reshape(-1, C)).sum(0), (g2 * xh2.reshape(-1, C)).sum(0)
            outbuf, out = _out_view((B, H, W, C))
            accbuf, acc = _acc_view(nrep, C)
            acc2buf, acc2 = _acc_view(nrep, C)
            bacc = dict(acc=acc, mode=1, x=t["x"], mean=v["mean"], invstd=v["invstd"])
            if two:
                bacc.update(acc2=acc2, x2=t["x2"], mean2=v["mean2"], invstd2=v["invstd2"])
            ops.conv_dgrad(dyd, None, wt, out, k, k, s, p, mask=t["mask"], residual=t["res"] if join else None,
                           residual_mask=t["rmask"] if join else None, bacc=bacc)
            what = f"two={two} join={join}"
            assert torch.equal(out.double(), g), f"{what}: dx differs from the fp64 reference"
            assert torch.equal(acc.sum(0)[0], S), f"{what}: sum g"
            assert torch.equal(acc.sum(0)[1], Q), f"{what}: sum g xhat"
            _assert_guards(outbuf, out.numel(), accbuf, nrep)
            if two:
                assert torch.equal(acc2.sum(0)[0], S), f"{what}: sum g of the second BatchNorm"
                assert torch.equal(acc2.sum(0)[1], Q2), f"{what}: sum g xhat2"
            else:
                assert (acc2 == 0).all(), "touched a second accumulator it was not given"
            assert (acc2buf[nrep:] == ACC_SENTINEL).all()


@gpu
@pytest.mark.parametrize("name", _ids(BWD_CASES))
def test_conv_dgrad_sums_exact(name):
    """Backward sums S = sum g, Q = sum g * xhat of the STORED data gradient g (relu' mask, with and without the
    residual join), for one and for two BatchNorms sharing g."""
    _run_bwd_case(name)


# ------------------------------------------------------------------------------------------ replicas
@gpu
@pytest.mark.parametrize("nrep", [1, 3, 8, 16])
@pytest.mark.parametrize("name", ["igemm64_128x64_fast_m180", "halo_row_one_tile", "igemm64_splitk8_m48"])
def test_replica_counts(name, nrep):
    """Any replica count in [1, 16]: the replica sum is exact, no replica beyond nrep is touched (the buffer
    always has 17)."""
    idx = _ids(FWD_CASES).index(name)
    _, (B, H, W, C, N, k, s, p), _, _ = FWD_CASES[idx]
    OH, OW = xu.out_hw(H, W, k, s, p)
    x, w, b = fwd_data(name)
    ref = fwd_reference(name, dev)
    r2 = ref.reshape(-1, N)
    outbuf, out = _out_view((B, OH, OW, N))
    accbuf, acc = _acc_view(nrep, N, rows=17)
    ops.conv_fwd(xu.bf16(x, dev), xu.pad_w(w, dev), b.float().to(dev) if b is not None else None, out, k, k, s, p,
                 False, bacc=dict(acc=acc, mode=0))
    assert torch.equal(out.double(), ref)
    assert torch.equal(acc.sum(0)[0], r2.sum(0)) and torch.equal(acc.sum(0)[1], (r2 * r2).sum(0))
    _assert_guards(outbuf, out.numel(), accbuf, nrep)


@gpu
@pytest.mark.parametrize("nrep", [1, 3, 8, 16])
def test_replica_counts_backward_halo(nrep):
    _run_bwd_case("halo_row", combos=((True, True),), nrep=nrep)


# ---------------------------------------------------------------------------------------- gap_bwd_bn
@gpu
@pytest.mark.parametrize("B,HW,C", GAP_EXACT)
def test_gap_bwd_bn_exact(B, HW, C):
    d, g, xh = gap_reference(B, HW, C, dev)
    nrep = 8
    outbuf, dx = _out_view((B, HW, 1, C))
    accbuf, acc = _acc_view(nrep, C)
    ops.gap_bwd_bn(xu.bf16(d["dy"], dev), xu.bf16(d["mask"], dev).view(B, HW, 1, C), dx, acc,
                   xu.bf16(d["x"], dev), d["mean"].float(), d["invstd"].float())
    assert torch.equal(dx.double().view(B, HW, C), g)
    assert torch.equal(acc.sum(0)[0], g.sum((0, 1))) and torch.equal(acc.sum(0)[1], (g * xh).sum((0, 1)))
    _assert_guards(outbuf, dx.numel(), accbuf, nrep)


@gpu
def test_gap_bwd_bn_hw49():
    """HW = 49: dy / HW is rounded.  dx within one bf16 ulp of fp64 (2^-7 |ref|, plus 2^-20 |ref| for the fp32
    reciprocal and product); the sums are those of the STORED dx, summed in fp32 by one workgroup per 4-channel
    group over at most all B * HW rows: n * 2^-24 * sum |terms| with n = B * HW + 1 (the product g * xhat
    rounds once more)."""
    B, HW, C = 4, 49, 64
    d, g, xh = gap_reference(B, HW, C, dev)
    accbuf, acc = _acc_view(8, C)
    outbuf, dx = _out_view((B, 7, 7, C))
    ops.gap_bwd_bn(xu.bf16(d["dy"], dev), xu.bf16(d["mask"], dev).view(B, 7, 7, C), dx, acc, xu.bf16(d["x"], dev),
                   d["mean"].float(), d["invstd"].float())
    got = dx.double().view(B, HW, C)
    err, bound = (got - g).abs(), (2.0 ** -7 + 2.0 ** -20) * g.abs()
    print(f"gap_bwd_bn HW=49: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert (err <= bound).all()
    n = B * HW + 1
    for i, terms in enumerate((got, got * xh)):
        e, bnd = (acc.sum(0)[i] - terms.sum((0, 1))).abs(), n * 2.0 ** -24 * terms.abs().sum((0, 1))
        print(f"  sum {i}: max err {float(e.max()):.3g}, smallest bound {float(bnd.min()):.3g}")
        assert (e <= bnd).all()
    _assert_guards(outbuf, dx.numel(), accbuf, 8)


# ----------------------------------------------------------------------------------------- consumers
MOM32 = float(torch.tensor(0.1, dtype=torch.float32))   # the kernels take momentum and eps as fp32
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))
_within_ulps, _close_elem = xu.assert_within_ulps, xu.assert_close_elem


def _split(total, nrep):
    return xu.split_replicas(total, nrep, ACC_SENTINEL)


def _dirty(nrep, C):
    buf = torch.full((nrep + 1, 2, C), ACC_SENTINEL, dtype=torch.float64, device=dev)
    buf[:nrep] = torch.randn(nrep, 2, C, dtype=torch.float64, device=dev) + 3
    return buf, buf[:nrep]


def _stats64(acc, M):
    """(mean, biased var, unbiased var, invstd) in fp64 of what the replicas hold (summed in replica order)."""
    S, Q = acc[:, 0].sum(0), acc[:, 1].sum(0)
    m = S / M
    var = (Q / M - m * m).clamp_min(0)
    return m, var, var * (M / (M - 1)) if M > 1 else var, 1 / torch.sqrt(var + EPS32)


def _check_fin(M, acc, mean, invstd, rm0, rv0, rm, rv, what):
    m, var, unb, inv = _stats64(acc, M)
    _within_ulps(mean, m, 2, what + " mean")
    assert ((invstd.double() - inv).abs() <= 2.0 ** -20 * inv).all(), what + " invstd"
    _within_ulps(rm, (1 - MOM32) * rm0.double() + MOM32 * m, 2, what + " running mean")
    _within_ulps(rv, (1 - MOM32) * rv0.double() + MOM32 * unb, 2, what + " running var")
    return m, inv


CONS_C = [8, 64, 512, 1024]      # the three channels-per-thread instantiations (C <= 256, <= 512, else)
CONS_M = [1, 3, 1000, 40000]     # below, inside and beyond one batch of the grid-stride loop
CONS_NREP = [1, 8, 9, 16]        # 9 crosses the 8-replica load chunk


def _bn_input(M, C, shift=0.5):
    x = (torch.randn(M, C, device=dev) * 2 + shift).to(torch.bfloat16)
    x[:, 1 % C] = 1.5   # a constant channel: variance 0, eps alone decides invstd
    return x


@gpu
@pytest.mark.parametrize("nrep", CONS_NREP)
@pytest.mark.parametrize("M", CONS_M)
@pytest.mark.parametrize("C", CONS_C)
def test_bn_apply_acc_against_fp64(C, M, nrep):
    torch.manual_seed(C + M + nrep)
    x, r = _bn_input(M, C), _bn_input(M, C, -1.0)
    xd, rd = x.double(), r.double()
    vec = lambda lo=0.0: torch.randn(C, device=dev) + lo  # noqa: E731
    gamma, beta, rgamma, rbeta = torch.rand(C, device=dev) + 0.5, vec(), torch.rand(C, device=dev) + 0.5, vec()
    accbuf, acc = _split(torch.stack([xd.sum(0), (xd * xd).sum(0)]), nrep)
    raccbuf, racc = _split(torch.stack([rd.sum(0), (rd * rd).sum(0)]), nrep)
    acc0, racc0 = accbuf.clone(), raccbuf.clone()
    for res in ("none", "plain", "bn"):
        for relu in (False, True):
            what = f"res={res} relu={relu}"
            zbuf, zero = _dirty(nrep, C)
            rzbuf, rzero = _dirty(nrep, C)
            mean, invstd, rmean, rinvstd = (torch.full((C,), float("nan"), device=dev) for _ in range(4))
            rm0, rv0, rrm0, rrv0 = vec(), torch.rand(C, device=dev) + 0.5, vec(), torch.rand(C, device=dev) + 0.5
            rm, rv, rrm, rrv = rm0.clone(), rv0.clone(), rrm0.clone(), rrv0.clone()
            ybuf, y = _out_view((M, C))
            rbn = [rgamma, rbeta, racc, rzero, rmean, rinvstd, rrm, rrv] if res == "bn" else None
            ops.bn_apply_acc(x, y, gamma, beta, acc, zero, mean, invstd, rm, rv, relu=relu,
                             residual=None if res == "none" else r, rbn=rbn, momentum=0.1, eps=1e-5)
            m, inv = _check_fin(M, acc, mean, invstd, rm0, rv0, rm, rv, what)
            a, b = xd * (inv * gamma.double()), m * inv * gamma.double()
            ref, terms = a - b + beta.double(), a.abs() + b.abs() + beta.double().abs()
            if res == "plain":
                ref, terms = ref + rd, terms + rd.abs()
            if res == "bn":
                mr, invr = _check_fin(M, racc, rmean, rinvstd, rrm0, rrv0, rrm, rrv, what + " residual")
                ra, rb = rd * (invr * rgamma.double()), mr * invr * rgamma.double()
                ref, terms = ref + ra - rb + rbeta.double(), terms + ra.abs() + rb.abs() + rbeta.double().abs()
                assert (rzero == 0).all() and (rzbuf[nrep] == ACC_SENTINEL).all(), what + ": residual zero"
            else:
                assert torch.isnan(rmean).all() and torch.equal(rrm, rrm0), what + ": touched the residual BN"
            _close_elem(y, ref.relu() if relu else ref, terms, what + " y")
            assert (ybuf[y.numel():] == OUT_SENTINEL).all(), what + ": wrote behind y"
            assert (zero == 0).all() and (zbuf[nrep] == ACC_SENTINEL).all(), what + ": zero"
            assert torch.equal(accbuf, acc0) and torch.equal(raccbuf, racc0), what + ": acc changed"


@gpu
@pytest.mark.parametrize("nrep", CONS_NREP)
@pytest.mark.parametrize("M", CONS_M)
@pytest.mark.parametrize("C", CONS_C)
def test_bn_dx_acc_against_fp64(C, M, nrep):
    torch.manual_seed(2 * C + M + nrep)
    x = _bn_input(M, C)
    g = torch.randn(M, C, device=dev).to(torch.bfloat16)
    xd, gd = x.double(), g.double()
    gamma, mean, invstd = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5
    ga, mu, isd = gamma.double(), mean.double(), invstd.double()
    xh = (xd - mu) * isd
    S, Q = gd.sum(0), (gd * xh).sum(0)
    accbuf, acc = _split(torch.stack([S, Q]), nrep)
    acc0 = accbuf.clone()
    zbuf, zero = _dirty(nrep, C)
    dgamma, dbeta, coef = (torch.full((n,), float("nan"), device=dev) for n in (C, C, 3 * C))
    dxbuf, dx = _out_view((M, C))
    ops.bn_dx_acc(x, g, dx, acc, zero, gamma, mean, invstd, dgamma, dbeta, coef, gscale=0.5)
    Sr, Qr = acc[:, 0].sum(0), acc[:, 1].sum(0)
    k1 = ga * isd
    k2, k3 = -k1 * isd * (Qr / M), k1 * (mu * isd * (Qr / M) - Sr / M)
    _within_ulps(dbeta, 0.5 * Sr, 2, "dbeta")
    _within_ulps(dgamma, 0.5 * Qr, 2, "dgamma")
    _within_ulps(coef, torch.cat([k1, k2, k3]), 2, "coef")
    _close_elem(dx, k1 * gd + k2 * xd + k3, (k1 * gd).abs() + (k2 * xd).abs() + k3.abs(), "dx")
    assert (dxbuf[dx.numel():] == OUT_SENTINEL).all()
    assert (zero == 0).all() and (zbuf[nrep] == ACC_SENTINEL).all()
    assert torch.equal(accbuf, acc0), "acc changed"


# --------------------------------------------------------------------------------------------- chain
@gpu
def test_chain_twice_on_the_same_buffers():
    """producer forward -> bn_apply_acc -> producer backward (mode 1, with the mean / invstd just written) ->
    bn_dx_acc, twice on the same accumulators without clearing anything by hand: each consumer clears the other
    direction's sums (the protocol BatchNorm in models/layers.py relies on), so the second round equals the
    first."""
    name = "igemm64_128x64_fast_m180"
    B, H, W, C, N, k, s, p = FWD_CASES[_ids(FWD_CASES).index(name)][1]
    M, nrep = B * H * W, 8
    x, w, b = fwd_data(name)
    xd, wd, bd = xu.bf16(x, dev), xu.pad_w(w, dev), b.float().to(dev)
    g0 = xu.gen(11)
    dy2 = xu.bf16(xu.ints(g0, (B, H, W, N), -1, 1), dev)
    w2t = xu.pad_wt(xu.sparse_ints(g0, (N, k * k * N), -1, 1, xu.weight_density(k * k * N)), N, k * k, N, dev)
    gamma, beta = torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev)
    acc_all = torch.zeros(2, nrep, 2, N, dtype=torch.float64, device=dev)
    acc_f, acc_b = acc_all[0], acc_all[1]
    rm, rv = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    y, z, g, dx = (torch.empty(B, H, W, N, dtype=torch.bfloat16, device=dev) for _ in range(4))
    rounds = []
    for _ in range(2):
        mean, invstd, dgamma, dbeta = (torch.full((N,), float("nan"), device=dev) for _ in range(4))
        coef = torch.full((3 * N,), float("nan"), device=dev)
        ops.conv_fwd(xd, wd, bd, y, k, k, s, p, False, bacc=dict(acc=acc_f, mode=0))
        ops.bn_apply_acc(y.view(M, N), z.view(M, N), gamma, beta, acc_f, acc_b, mean, invstd, rm, rv, relu=True)
        ops.conv_dgrad(dy2, None, w2t, g, k, k, s, p, mask=z,
                       bacc=dict(acc=acc_b, mode=1, x=y, mean=mean, invstd=invstd))
        ops.bn_dx_acc(y.view(M, N), g.view(M, N), dx.view(M, N), acc_b, acc_f, gamma, mean, invstd, dgamma, dbeta, coef)
        assert (acc_f == 0).all() and (acc_b != 0).any()
        rounds.append([t.clone() for t in (mean, invstd, dgamma, dbeta, dx, z, g)])
    yref = fwd_reference(name, dev)
    m64 = yref.reshape(-1, N).mean(0)
    _within_ulps(rounds[0][0], m64, 2, "chain mean")
    for a, b2, what in zip(rounds[0], rounds[1], ("mean", "invstd", "dgamma", "dbeta", "dx", "z", "g")):
        assert not torch.isnan(a.float()).any() and torch.equal(a, b2), f"second round's {what} differs"
