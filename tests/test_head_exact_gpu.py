"""The two fused dense-head kernels (csrc/khead.hip: khead_train + khead_wgrad; csrc/mlphead.hip: head_train),
called directly, against the fp64 reference of tests/exact_util.py.

Exact tests.  On integer data with a saturated softmax (exact_util.head_ints / head_ref) every output of both
kernels is exactly representable, so each one is compared with ``torch.equal``: a wrong row of a partly filled
tile, a slab summed twice, a stale tail column in a transposed operand or a bias column from the wrong tile fails
the comparison outright.  Every test first asserts the conditions of exactness on the reference
(exact_util.assert_exact_head; tests/test_exact_util.py asserts them for every shape without a GPU).  Every
output buffer is poisoned before each launch (NaN, or a finite sentinel where the weight-gradient launch would sum
it), and the khead workspace is the one ``Net`` allocates: zeroed words, here with NaN in the slab and
published-dZ1 regions.

Stage tests.  The integer data saturates the softmax, so its arithmetic is tested on random bf16 data, stage by
stage: every stage is compared with an fp64 evaluation fed by the KERNEL'S OWN upstream output, so exactly one
rounding separates the two.  bf16 outputs: exact_util.assert_close_elem (one bf16 ulp + 2^-20 sum |terms|); fp32
logits and weight gradients: 2^-20 sum |terms|.  The softmax stage uses __expf, __logf and 1.f / s, whose error is
not derived but measured against fp64 on the kernel's logits, on an MI355X, over the listed cases:

  * P_ERR: the error of (p - onehot) left once the one bf16 rounding of dZ_last (half a bf16 ulp of the stored
    value) is taken off.  Measured 0, 3.516e-09 (khead 70 x 4608) and 0; bound = 4 x the worst = 1.4064e-08.
  * LOSS_ERR: the error of a 16-row loss partial, per row of the partial.  Measured 1.635e-07 (khead 200 x 512),
    8.612e-08 (khead 70 x 4608) and 2.458e-07 (mlphead); bound = 4 x the worst = 9.832e-07.

The kernels and the test data are deterministic, so these figures repeat from run to run; the raw error of
dZ_last / grad_scale, its bf16 rounding included, is 1.9e-3 (half a bf16 ulp of 0.5).
"""
import pytest
import torch
import torch.nn.functional as F

import exact_util as xu
from distriflow_amd import native, ops

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

GS = xu.HEAD_GRAD_SCALE
SENTINEL = 77.0       # finite, a bf16 value, above every activation of the integer data
# 4 x the worst value measured on an MI355X over the stage cases below (the figures: the docstring above)
P_ERR = 4 * 3.516e-09
LOSS_ERR = 4 * 2.458e-07

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _full(shape, value, dtype=torch.float32):
    return torch.full(tuple(shape), value, device=dev, dtype=dtype)


def _cpu(t):
    return t.detach().double().cpu()


def _eq(name, got, exp):
    got, exp = _cpu(got), exp.double()
    assert got.shape == exp.shape, f"{name}: shape {tuple(got.shape)} != {tuple(exp.shape)}"
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{name}: {len(bad)} of {got.numel()} entries differ, first at {i}: "
                             f"got {got[i].item()!r}, expected {exp[i].item()!r}")


def _dev_f32(t):
    return None if t is None else t.float().to(dev)


# ------------------------------------------------------------------------------------------------ khead
class KHead:
    """Operands and buffers of one Dense(K -> 128, ReLU) [-> Dropout] -> Dense(C) head for ops.khead_train /
    ops.khead_wgrad; :meth:`launch` poisons every output, runs both and returns the outputs on the CPU."""

    def __init__(self, d, drop=None, dp=True, dp_mask=True, logits=True, dp_scale=0.5, grad_scale=GS):
        self.B, self.K = d["x"].shape
        self.C = d["dims"][-1]
        self.ldt = xu._r32(self.B)
        W1, W2 = d["W"]
        self.p = xu.bf16(d["x"], dev)
        self.w1, self.w1t = xu.pad_w(W1, dev), xu.pad_wt(W1, xu.KHEAD_N1, 1, self.K, dev)
        self.w2, self.w2t = xu.pad_w(W2, dev), xu.pad_wt(W2, self.C, 1, xu.KHEAD_N1, dev)
        assert self.w2.shape == (16, 128) and self.w2t.shape == (128, 32)
        self.b1, self.b2 = _dev_f32(d["b"][0]), _dev_f32(d["b"][1])
        self.labels = d["labels"].to(dev)
        self.idx = None if d["idx"] is None else d["idx"].to(dev)
        self.step = torch.tensor([drop[2]], dtype=torch.int64, device=dev) if drop else None
        self.drop = (drop[0], drop[1], self.step) if drop else None
        self.dh_scale = 1.0 / (1.0 - drop[0]) if drop else 1.0
        self.want_dp, self.dp_mask, self.want_logits = dp, dp_mask, logits
        self.dp_scale, self.grad_scale = dp_scale, grad_scale
        # the workspace as Net allocates it (zeros); the slab and published-dZ1 regions poisoned
        nt = (self.B + 31) // 32
        self.ws = torch.zeros(ops.khead_ws_floats(self.B, self.K), dtype=torch.float32, device=dev)
        self.ws[:nt * 8 * 32 * 128 + nt * 32 * 128 // 2] = float("nan")
        assert nt * 8 * 32 * 128 + nt * 32 * 128 // 2 + 2 * nt + 2 == native.require().khead_err_offset(self.B)

    def launch(self):
        B, K, C, ldt, N1 = self.B, self.K, self.C, self.ldt, xu.KHEAD_N1
        bf = torch.bfloat16
        pT, h1T = _full((K, ldt), SENTINEL, bf), _full((N1, ldt), SENTINEL, bf)
        dz1T, dz2T = _full((N1, ldt), SENTINEL, bf), _full((C, ldt), SENTINEL, bf)
        nan = float("nan")
        dp = _full((B, K), nan, bf) if self.want_dp else None
        logits = _full((B, C), nan) if self.want_logits else None
        loss_part, stats = _full((2 * ((B + 15) // 16),), nan), _full((2,), nan)
        gw1, gb1, gw2, gb2 = _full((N1, K), nan), _full((N1,), nan), _full((C, N1), nan), _full((C,), nan)
        ops.khead_train(self.p, pT, dp, self.w1, self.w1t, self.b1, self.w2, self.w2t, self.b2, h1T, dz1T, dz2T,
                        logits, self.labels, self.idx, self.grad_scale, loss_part, self.ws, drop=self.drop,
                        dh_scale=self.dh_scale, dp_scale=self.dp_scale, dp_mask=self.dp_mask)
        ops.khead_wgrad(pT, h1T, dz1T, dz2T, gw1, gb1 if self.b1 is not None else None, gw2,
                        gb2 if self.b2 is not None else None, B, K, C, loss_part, stats)
        torch.cuda.synchronize()
        assert ops.khead_error(self.ws, B) == 0, "a row tile's flag wait timed out"
        return {"xT": _cpu(pT), "hT": [_cpu(h1T)], "dzT": [_cpu(dz1T), _cpu(dz2T)],
                "dx": None if dp is None else _cpu(dp), "logits": None if logits is None else _cpu(logits),
                "gw": [_cpu(gw1), _cpu(gw2)],
                "gb": [_cpu(gb1) if self.b1 is not None else None, _cpu(gb2) if self.b2 is not None else None],
                "loss_part": _cpu(loss_part).view(-1, 2), "stats": _cpu(stats)}


# --------------------------------------------------------------------------------------------- mlphead
class MlpHead:
    """Operands and buffers of a Dense chain for ops.head_train.  The kernel's contract: the caller zeroes the
    tail columns [B, round32(B)) of xT / hT / dzT and the kernel writes valid rows only; columns [0, B) hold a
    sentinel before each launch."""

    def __init__(self, d, x_relu=False, dx_scale=1.0, grad_scale=GS):
        self.dims = d["dims"]
        self.B, self.nl, self.ldt = d["x"].shape[0], len(d["W"]), xu._r32(d["x"].shape[0])
        self.x = xu.bf16(d["x"], dev)
        self.w = [xu.pad_w(w, dev) for w in d["W"]]
        self.wt = [xu.pad_wt(w, w.shape[0], 1, w.shape[1], dev) for w in d["W"]]
        self.b = [_dev_f32(b) for b in d["b"]]
        self.labels = d["labels"].to(dev)
        self.idx = None if d["idx"] is None else d["idx"].to(dev)
        self.x_relu, self.dx_scale, self.grad_scale = x_relu, dx_scale, grad_scale

    def _transposed(self, rows):
        t = torch.zeros(rows, self.ldt, device=dev, dtype=torch.bfloat16)
        t[:, :self.B] = SENTINEL
        return t

    def launch(self, phases=(3,)):
        B, dims, nl = self.B, self.dims, self.nl
        nan = float("nan")
        gw = [_full((dims[l + 1], dims[l]), nan) for l in range(nl)]
        gb = [_full((dims[l + 1],), nan) for l in range(nl)]
        hT = [self._transposed(dims[l + 1]) for l in range(nl - 1)] + [None]
        dzT = [self._transposed(dims[l + 1]) for l in range(nl)]
        xT = self._transposed(dims[0])
        dx, logits = _full((B, dims[0]), nan, torch.bfloat16), _full((B, dims[-1]), nan)
        loss_part, stats = _full((2 * ((B + 15) // 16),), nan), _full((2,), nan)
        for ph in phases:
            ops.head_train(self.w, self.wt, self.b, gw, gb, hT, dzT, list(dims[:-1]), list(dims[1:]), self.x,
                           self.x_relu, xT, dx, logits, self.labels, self.idx, self.grad_scale, loss_part, stats,
                           phases=ph, dx_scale=self.dx_scale)
        torch.cuda.synchronize()
        return {"xT": _cpu(xT), "hT": [_cpu(t) for t in hT[:-1]], "dzT": [_cpu(t) for t in dzT], "dx": _cpu(dx),
                "logits": _cpu(logits), "gw": [_cpu(t) for t in gw], "gb": [_cpu(t) for t in gb],
                "loss_part": _cpu(loss_part).view(-1, 2), "stats": _cpu(stats)}


# ------------------------------------------------------------------------------------- the exact comparison
def _padT(t, ldt):
    """fp64 [B][N] -> [N][ldt], zero in the tail columns."""
    out = torch.zeros(t.shape[1], ldt, dtype=torch.float64)
    out[:, :t.shape[0]] = t.t()
    return out


def _assert_exact(out, ref, what):
    """Every output against the reference with torch.equal; the transposed operands over ALL of [rows][round32(B)]:
    columns [0, B) overwritten, columns [B, round32(B)) exactly zero (the weight-gradient launch sums them)."""
    B = ref["logits"].shape[0]
    ldt = xu._r32(B)
    if out["logits"] is not None:
        _eq(f"{what} logits", out["logits"], ref["logits"])
    _eq(f"{what} xT", out["xT"], _padT(ref["acts"][0], ldt))
    for l, t in enumerate(out["hT"]):
        _eq(f"{what} hT[{l}]", t, _padT(ref["acts"][l + 1], ldt))
    for l, t in enumerate(out["dzT"]):
        _eq(f"{what} dzT[{l}]", t, _padT(ref["dz"][l], ldt))
    if out["dx"] is not None:
        _eq(f"{what} dx", out["dx"], ref["dx"])
    for l in range(len(out["gw"])):
        _eq(f"{what} gw[{l}]", out["gw"][l], ref["gw"][l])
        if out["gb"][l] is not None:
            _eq(f"{what} gb[{l}]", out["gb"][l], ref["gb"][l])
    _eq(f"{what} loss_part", out["loss_part"], ref["loss_part"])
    _eq(f"{what} stats", out["stats"], ref["stats"])


def _khead_ref(case, **kw):
    def make():
        d, ref = xu.khead_case(*case, **kw)
        xu.assert_exact_head(ref)
        return d, ref
    return _cached(("khead", case, tuple(sorted(kw.items()))), make)


def _kid(c):
    return f"B{c[0]}_K{c[1]}_C{c[2]}" + ("_drop" if c[3] else "") + ("_idx" if c[4] else "")


@pytest.mark.parametrize("case", xu.KHEAD_CASES, ids=_kid)
def test_khead_exact(case):
    """khead_train + khead_wgrad, twice on the same workspace (the launch tag advances and the tickets reset on the
    device, with no host-side counter), every output re-poisoned in between."""
    d, ref = _khead_ref(case)
    h = KHead(d, drop=xu.HEAD_DROP if case[3] else None)
    _assert_exact(h.launch(), ref, "first launch")
    _assert_exact(h.launch(), ref, "second launch")


@pytest.mark.parametrize("case,cap", [((96, 512, 10, False, False), 8),     # G = 8: three jobs per workgroup
                                      ((160, 256, 10, False, False), 16)],  # 40 jobs on 16: an uneven last round
                         ids=["B96_K512_cap8", "B160_K256_cap16"])
def test_khead_exact_with_a_capped_grid(case, cap):
    """A persistent grid smaller than the job count: every workgroup takes further jobs and reuses its LDS after
    the tag hand-off."""
    d, ref = _khead_ref(case)
    C = native.require()
    try:
        C.khead_set_grid_cap(cap)
        h = KHead(d)
        _assert_exact(h.launch(), ref, "first launch")
        _assert_exact(h.launch(), ref, "second launch")
    finally:
        C.khead_set_grid_cap(0)


def test_khead_refuses_a_grid_below_one_row_tile():
    """With fewer than 8 workgroups the 8 jobs of a row tile could not run together: nothing is launched."""
    d, _ = _khead_ref((96, 512, 10, False, False))
    C = native.require()
    try:
        C.khead_set_grid_cap(4)
        with pytest.raises(RuntimeError):
            KHead(d).launch()
    finally:
        C.khead_set_grid_cap(0)


@pytest.mark.parametrize("variant", ["dp_none", "no_bias", "no_dp_mask", "no_logits"])
def test_khead_exact_variants(variant):
    case = (40, 512, 10, False, False)
    if variant == "no_bias":
        d, ref = _khead_ref(case, bias=False)
        h = KHead(d)
        assert h.b1 is None and h.b2 is None
    elif variant == "no_dp_mask":
        d, ref = _khead_ref(case, dp_mask=False)
        h = KHead(d, dp_mask=False)
    else:
        d, ref = _khead_ref(case)
        h = KHead(d, dp=variant != "dp_none", logits=variant != "no_logits")  # dp None: the owner's other P^T branch
    out = h.launch()
    assert (out["dx"] is None) == (variant == "dp_none") and (out["logits"] is None) == (variant == "no_logits")
    _assert_exact(out, ref, variant)
    _assert_exact(h.launch(), ref, variant + ", second launch")


def test_khead_supported_and_refusals():
    assert not ops.khead_supported(384, 10) and not ops.khead_supported(5632, 10) and not ops.khead_supported(256, 17)
    assert ops.khead_supported(5376, 16) and ops.khead_supported(256, 1)
    d = xu.head_ints(xu.gen(0), 8, (384, xu.KHEAD_N1, 10))
    with pytest.raises(RuntimeError):   # refused by the binding: nothing is launched
        KHead(d).launch()


# ---------------------------------------------------------------------------------------- mlphead, exact
def _mid(c):
    return f"B{c[0]}_" + "x".join(map(str, c[1]))


def _mlp_ref(case):
    def make():
        d, ref = xu.mlphead_case(*case)
        xu.assert_exact_head(ref)
        return d, ref
    return _cached(("mlp", case), make)


@pytest.mark.parametrize("case", xu.MLPHEAD_CASES, ids=_mid)
def test_mlphead_exact(case):
    d, ref = _mlp_ref(case)
    h = MlpHead(d, x_relu=case[3], dx_scale=case[4])
    _assert_exact(h.launch(), ref, "phases=3")


def test_mlphead_exact_in_two_launches():
    case = xu.MLPHEAD_CASES[0]
    d, ref = _mlp_ref(case)
    _assert_exact(MlpHead(d).launch(phases=(1, 2)), ref, "phases=1 then 2")


# ------------------------------------------------------------------------------- the first-maximum rule
TIE_ROWS = [([200, 200, 0, 72], 0), ([200, 200, 0, 72], 1), ([8, 96, 3, 96], 1), ([8, 96, 3, 96], 3),
            ([0, 5, 130, 130], 2), ([0, 5, 130, 130], 3), ([7, 7, 7, 7], 0), ([7, 7, 7, 7], 2), ([1, 2, 3, 4], 3)]


def _tie_data(B, K, hidden):
    """Hand-built integer rows whose logits ARE the first four inputs (identity weights, no bias): a two-way (or
    four-way) tie at the maximum with the label on the first or a later tied position."""
    rows = [TIE_ROWS[i % len(TIE_ROWS)] for i in range(B)]
    x = torch.zeros(B, K, dtype=torch.float64)
    x[:, :4] = torch.tensor([r for r, _ in rows], dtype=torch.float64)
    y = torch.tensor([lab for _, lab in rows], dtype=torch.int32)
    dims = (K,) + tuple(hidden) + (4,)
    W = []
    for l in range(len(dims) - 1):
        w = torch.zeros(dims[l + 1], dims[l], dtype=torch.float64)
        w[:4, :4] = torch.eye(4, dtype=torch.float64)
        W.append(w)
    logits = x[:, :4]
    am = xu.window_argmax(logits)[1]       # the strict-> scan
    correct = torch.zeros((B + 15) // 16 * 16, dtype=torch.float64)
    correct[:B] = (am == y.long()).double()
    d = {"dims": dims, "x": x, "W": W, "b": [None] * len(W), "labels": y, "idx": None}
    return d, logits, correct.view(-1, 16).sum(1)


@pytest.mark.parametrize("kernel", ["khead", "mlphead"])
def test_correct_counts_the_first_maximum_on_ties(kernel):
    if kernel == "khead":
        d, logits, correct = _tie_data(40, 256, (xu.KHEAD_N1,))
        out = KHead(d).launch()
    else:
        d, logits, correct = _tie_data(40, 16, ())
        out = MlpHead(d).launch()
    assert 0 < float(correct.sum()) < 40
    _eq("logits", out["logits"], logits)
    _eq("correct per 16 rows", out["loss_part"][:, 1], correct)
    _eq("correct", out["stats"][1], correct.sum())


# --------------------------------------------------------------------- real softmax values, stage by stage
def _rand_head(seed, B, dims, with_idx=False):
    """Random bf16 inputs and weights, fp32 biases (all as fp64 on the CPU)."""
    g = xu.gen(seed)
    r16 = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    nl = len(dims) - 1
    W = [r16(torch.randn(dims[l + 1], dims[l], generator=g) / dims[l] ** 0.5) for l in range(nl)]
    b = [(torch.randn(dims[l + 1], generator=g) * 0.1).float().double() for l in range(nl)]
    table = torch.randint(0, dims[-1], (3 * B if with_idx else B,), generator=g, dtype=torch.int32)
    idx = torch.randperm(3 * B, generator=g)[:B] if with_idx else None
    return {"dims": tuple(dims), "x": r16(torch.randn(B, dims[0], generator=g)), "W": W, "b": b, "labels": table,
            "idx": idx, "y": (table[idx] if with_idx else table).long()}


def _half_ulp_bf16(v):
    """Half a bf16 ulp of the stored value v (the most its one rounding can have moved it)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 8)


def _assert_stages(out, d, gs, what, keep=None, dh_scale=1.0, x_relu=False, dx_scale=1.0):
    """Each stage against fp64 on the kernel's own upstream output; returns the measured softmax-stage errors
    (P_ERR, LOSS_ERR of the module docstring) after asserting their bounds."""
    W, b, y = d["W"], d["b"], d["y"]
    nl, B, C = len(W), d["x"].shape[0], d["dims"][-1]
    ldt = xu._r32(B)
    assert torch.equal(out["xT"], _padT(d["x"], ldt)), f"{what}: xT"
    for t in out["hT"] + out["dzT"]:
        assert torch.equal(t[:, B:], torch.zeros_like(t[:, B:])), f"{what}: tail columns not zero"
    acts = [d["x"]] + [t[:, :B].t() for t in out["hT"]]
    dz = [t[:, :B].t() for t in out["dzT"]]
    eps32 = 2.0 ** -20
    for l in range(nl - 1):                                  # hidden activations from the kernel's previous one
        h = (acts[l] @ W[l].t() + b[l]).relu()
        terms = acts[l].abs() @ W[l].abs().t() + b[l].abs()
        if keep is not None and l == nl - 2:
            h, terms = h * keep * dh_scale, terms * keep * dh_scale
        xu.assert_close_elem(acts[l + 1], h, terms, f"{what}: h{l + 1}")
    z = out["logits"]                                        # logits from the kernel's last activation
    zr = acts[-1] @ W[-1].t() + b[-1]
    zt = acts[-1].abs() @ W[-1].abs().t() + b[-1].abs()
    assert ((z - zr).abs() <= eps32 * zt).all(), f"{what}: logits {float(((z - zr).abs() / zt).max()):.3g} x terms"
    # the softmax stage from the kernel's logits
    p = torch.softmax(z, dim=1)
    g = (p - F.one_hot(y, C).double()) * gs
    err = ((dz[-1] - g).abs() - _half_ulp_bf16(dz[-1])).clamp_min(0) / gs
    p_err = float(err.max())
    rows = torch.zeros((B + 15) // 16 * 16, dtype=torch.float64)
    rows[:B] = torch.logsumexp(z, dim=1) - z.gather(1, y[:, None])[:, 0]
    nrows = torch.tensor([min(16, B - 16 * q) for q in range((B + 15) // 16)], dtype=torch.float64)
    part = rows.view(-1, 16).sum(1)
    loss_err = float(((out["loss_part"][:, 0] - part).abs() / nrows).max())
    print(f"{what}: softmax stage: p error beyond the bf16 rounding {p_err:.3e} (bound {P_ERR:.3e}), "
          f"loss error per row {loss_err:.3e} (bound {LOSS_ERR:.3e}), "
          f"raw max |dz/gs - (p - onehot)| {float(((dz[-1] - g).abs() / gs).max()):.3e}")
    assert p_err <= P_ERR, f"{what}: p error {p_err:.3e} > {P_ERR:.3e}"
    assert loss_err <= LOSS_ERR, f"{what}: loss error per row {loss_err:.3e} > {LOSS_ERR:.3e}"
    am = xu.window_argmax(z)[1]
    corr = torch.zeros_like(rows)
    corr[:B] = (am == y).double()
    assert torch.equal(out["loss_part"][:, 1], corr.view(-1, 16).sum(1)), f"{what}: correct per 16 rows"
    lp = out["loss_part"]
    assert abs(float(out["stats"][0] - lp[:, 0].sum())) <= eps32 * float(lp[:, 0].abs().sum()), f"{what}: loss total"
    assert float(out["stats"][1]) == float(lp[:, 1].sum()), f"{what}: correct total"
    for l in range(nl - 1, 0, -1):                           # hidden dZ from the kernel's dZ above and activation
        s = dh_scale if (keep is not None and l == nl - 1) else 1.0
        r = (dz[l] @ W[l]) * (acts[l] > 0) * s
        xu.assert_close_elem(dz[l - 1], r, dz[l].abs() @ W[l].abs() * s, f"{what}: dz{l - 1}")
    if out["dx"] is not None:                                # dX from the kernel's dZ0
        r = dz[0] @ W[0] * dx_scale
        if x_relu:
            r = r * (d["x"] > 0)
        xu.assert_close_elem(out["dx"], r, dz[0].abs() @ W[0].abs() * dx_scale, f"{what}: dx")
    for l in range(nl):                                      # gW, gb from the kernel's transposed operands
        r, t = dz[l].t() @ acts[l], dz[l].abs().t() @ acts[l].abs()
        assert ((out["gw"][l] - r).abs() <= eps32 * t).all(), f"{what}: gw{l}"
        assert ((out["gb"][l] - dz[l].sum(0)).abs() <= eps32 * dz[l].abs().sum(0)).all(), f"{what}: gb{l}"
    return p_err, loss_err


@pytest.mark.parametrize("B,K,C,drop", [(200, 512, 10, False), (70, 4608, 10, True)],
                         ids=["B200_K512", "B70_K4608_drop"])
def test_khead_stages_on_random_data(B, K, C, drop):
    from distriflow_amd.ops import reference

    d = _rand_head(11 + K, B, (K, xu.KHEAD_N1, C), with_idx=drop)
    spec = xu.HEAD_DROP if drop else None
    keep = None
    if drop:
        keep = reference.dropout_mask(B * xu.KHEAD_N1, spec[0], spec[1] ^ (spec[2] * 0x9E3779B1)).double().view(B, -1)
    gs = 1.0 / 64
    h = KHead(d, drop=spec, grad_scale=gs)
    for n in ("first", "second"):
        _assert_stages(h.launch(), d, gs, f"khead {B}x{K} {n} launch", keep=keep, dh_scale=h.dh_scale, x_relu=True,
                       dx_scale=0.5)


def test_mlphead_stages_on_random_data():
    B, dims = 50, (64, 48, 32, 10)
    d = _rand_head(7, B, dims)
    gs = 1.0 / 64
    _assert_stages(MlpHead(d, x_relu=True, grad_scale=gs).launch(), d, gs, "mlphead 50 x (64, 48, 32, 10)", x_relu=True)

