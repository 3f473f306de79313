"""fp64 oracle and input preparation for the ``ops.loss_grad`` tests (CPU and GPU).

The oracle is torch autograd in float64 through float64 restatements of the ``distriflow_amd/losses.py``
formulas (``losses.py`` itself casts to fp32; ``tests/test_loss_grad_cpu.py`` ties the two together).

The gradient is discontinuous at |p - t| = 0 (absoluteDifference), at 1 - (2t - 1) p = 0 (hingeLoss) and at
the 1e-7 clamp (categorical cross-entropy): fp32 and fp64 may fall on different sides there.  ``case`` prepares
every input on the CPU so that no element is within 1e-3 of a kink and asserts it, so no element is ever
excluded from a comparison.
"""
import torch
import torch.nn.functional as F

import exact_util as xu

KINDS = ["meanSquaredError", "absoluteDifference", "hingeLoss", "huberLoss", "logLoss", "sigmoidCrossEntropy",
         "softmaxCrossEntropy", "categorical_crossentropy"]
ACTS = ["linear", "softmax", "sigmoid"]
FORMS = ["labels", "dense", "dense_idx"]
# (B, C): one element; a small odd case; across a 256-thread workgroup; the row-per-thread / wave-per-row switch
# with a partial last workgroup of 4 rows; the lane-stride boundary; several strides
SHAPES = [(1, 1), (5, 3), (257, 10), (5, 32), (5, 33), (3, 64), (3, 65), (2, 200)]
MARGIN = 1e-3


def act64(z, act):
    return torch.softmax(z, dim=1) if act == "softmax" else (torch.sigmoid(z) if act == "sigmoid" else z)


def loss64(kind, t, p):
    """Per-example loss [B] of ``kind`` on float64 targets ``t`` and outputs ``p`` [B][C]."""
    if kind in ("meanSquaredError", "mse"):
        return ((t - p) ** 2).mean(1)
    if kind == "absoluteDifference":
        return (t - p).abs().mean(1)
    if kind == "hingeLoss":
        return torch.relu(1.0 - (2.0 * t - 1.0) * p).mean(1)
    if kind == "huberLoss":
        d = (p - t).abs()
        return torch.where(d <= 1.0, 0.5 * d * d, d - 0.5).mean(1)
    if kind == "logLoss":
        return (-(t * torch.log(p + 1e-7) + (1 - t) * torch.log(1 - p + 1e-7))).mean(1)
    if kind == "sigmoidCrossEntropy":
        return (p.clamp_min(0) - p * t + torch.log1p(torch.exp(-p.abs()))).mean(1)
    if kind == "softmaxCrossEntropy":
        return -(t * F.log_softmax(p, dim=1)).sum(1)
    if kind in ("categorical_crossentropy", "categoricalCrossentropy"):
        return -(t * torch.log(p.clamp(1e-7, 1.0))).sum(1)
    raise KeyError(kind)


def first_argmax(v):
    """Index of the first maximum of every row (an explicit strict scan, tests/exact_util.py)."""
    return xu.window_argmax(v)[1]


def oracle(kind, act, z, t, ref_class, grad_scale):
    """-> (grad_scale * dL/dz [B][C], sum of the per-example loss, number correct), all float64 / int."""
    zz = z.double().clone().requires_grad_(True)
    L = loss64(kind, t.double(), act64(zz, act))
    (g,) = torch.autograd.grad(L.sum(), zz)
    return grad_scale * g, float(L.detach().sum()), int((first_argmax(z.double()) == ref_class).sum())


def _margin(kind, t, p):
    if kind == "absoluteDifference":
        return (p - t).abs()
    return (1.0 - (2.0 * t - 1.0) * p).abs()  # hingeLoss


class Case:
    """Inputs of one ``loss_grad`` call on the CPU: logits ``z`` [B][C] fp32; the target ``table`` (int32 [N] or
    fp32 [N][C]) with ``idx`` (int64 [B], or None: N == B); the rows the call sees as float64 ``t`` [B][C] and
    their class ``ref_class`` [B]."""

    def __init__(self, kind, act, form, B, C, seed=0, out_of_range_labels=False):
        g = xu.gen(1000 * seed + 31 * B + C)
        unit = kind in ("logLoss", "categorical_crossentropy") and act == "linear"
        z = torch.rand(B, C, generator=g) * 0.9 + 0.05 if unit else 1.5 * torch.randn(B, C, generator=g)
        N = B if form != "dense_idx" else B + 3
        self.idx = None
        if form == "dense_idx":  # out of order, with repeats
            self.idx = torch.randint(0, N, (B,), generator=g)
            if B > 1:
                self.idx[-1] = self.idx[0]
        rows = self.idx if self.idx is not None else torch.arange(B)
        kinked = kind in ("absoluteDifference", "hingeLoss")
        if form == "labels":
            y = torch.randint(0, C, (N,), generator=g, dtype=torch.int32)
            if out_of_range_labels:
                y[::2] = C + 5
                y[1::3] = -3
            self.table = y
            self.ref_class = y.long().clamp(0, C - 1)[rows]
            t = F.one_hot(self.ref_class, C).double()
            if kinked and act == "linear":  # move z off the kinks (z == t, (2t - 1) z == 1)
                for _ in range(8):
                    bad = _margin(kind, t, z.double()) < 2 * MARGIN
                    z = torch.where(bad, z + 0.01, z)
            elif kinked:  # bounded outputs: the kinks lie on the boundary of the range, never inside it
                p32 = act64(z, act)
                assert bool(((p32 > 0) & (p32 < 1)).all()), "fp32 outputs must lie strictly inside (0, 1)"
        else:
            tab = torch.rand(N, C, generator=g)
            if kinked:  # move t off the kinks; rows the call never reads are moved too (harmless)
                p_rows = act64(z.double(), act)
                for _ in range(8):
                    moved = False
                    for b in range(B):  # a table row read by several batch rows must clear all of them
                        r = int(rows[b])
                        bad = _margin(kind, tab[r].double(), p_rows[b]) < 2 * MARGIN
                        if bool(bad.any()):
                            tab[r] = torch.where(bad, tab[r] + torch.where(tab[r] > 0.5, -0.01, 0.01), tab[r])
                            moved = True
                    if not moved:
                        break
            self.table = tab
            t = tab[rows].double()
            self.ref_class = first_argmax(t)
        self.z, self.t = z.float(), t
        p = act64(self.z.double(), act)
        if kinked and (form != "labels" or act == "linear"):
            m = float(_margin(kind, t, p).min())
            assert m >= MARGIN, f"an element is {m:.2e} from a kink of {kind}"
        if kind == "categorical_crossentropy" and not (act == "softmax" and C == 1):
            assert float(p.min()) >= 1e-6 and float(p.max()) < 1.0, "outputs must stay inside the clamp"


def check(kind, act, case, dl, stats, grad_scale, what=""):
    """The project's tolerances for these quantities (test_softmax_ce, test_sigmoid_ce)."""
    ed, el, ec = oracle(kind, act, case.z, case.t, case.ref_class, grad_scale)
    if dl is not None:
        torch.testing.assert_close(dl.double().cpu(), ed, rtol=1e-2, atol=1e-4, msg=lambda m: f"{what} dlogits: {m}")
    if stats is not None:
        got_l, got_c = float(stats[0]), float(stats[1])
        assert abs(got_l - el) <= 1e-3 * abs(el) + 1e-3, f"{what} loss sum {got_l} vs {el}"
        assert got_c == ec, f"{what} correct {got_c} vs {ec}"
