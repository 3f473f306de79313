"""Integer-valued test data and an fp64 reference for the exact kernel tests.

With inputs, weights and bias taken from small integers every product, every fp32 partial sum in any order,
every bf16-rounded output and every fp32 / fp64 accumulator of a conv / dense kernel is exactly representable,
so ``torch.equal`` against an fp64 reference is the right assertion: no tolerance hides a wrong row, tap, tail
or replica.  That holds under conditions on the REFERENCE (``assert_exact_*`` below), which every test asserts
before it compares anything; they are conditions, not tolerances.

The reference is ``F.unfold`` / ``F.fold`` + matmul in float64, in batch chunks.  It does not go through
``ops.reference``: that casts to fp32, and an fp32 library conv may pick a Winograd-class algorithm, which is
not exact on integers.

Everything is generated on the CPU from a seeded generator (the same values with and without a GPU) and moved
to ``device`` afterwards.
"""
import torch
import torch.nn.functional as F

BF16_INT_MAX = 256        # every integer of magnitude <= 256 is a bf16 value
FP32_INT_MAX = 1 << 24    # every integer of magnitude <= 2^24 is an fp32 value


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo, hi):
    """Integers in [lo, hi] as float64 (CPU)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def sparse_ints(g, shape, lo, hi, density):
    """Integers in [lo, hi], each kept with probability ``density`` (else 0), as float64 (CPU)."""
    v = ints(g, shape, lo, hi)
    if density >= 1.0:
        return v
    return v * (torch.rand(tuple(shape), generator=g) < density)


def weight_density(K, terms=64):
    """Density that leaves about ``terms`` non-zero weights in a reduction of length K."""
    return min(1.0, terms / K)


def bf16(t, device):
    """fp64 integers -> bf16 on ``device``; the values must survive the cast."""
    b = t.to(torch.bfloat16)
    assert torch.equal(b.double(), t), "not bf16 values"
    return b.to(device)


def _r(a, b):
    return (a + b - 1) // b * b


def pad_w(w2d, device):
    """fp64 [N][K] -> zero padded bf16 [Npad16][Kpad32] (the forward compute layout)."""
    N, K = w2d.shape
    out = torch.zeros(_r(N, 16), _r(K, 32), dtype=torch.bfloat16)
    out[:N, :K] = w2d.to(torch.bfloat16)
    return out.to(device)


def pad_wt(w2d, N, T, Ci, device):
    """fp64 [N][T*Ci] -> data-gradient layout bf16 [Ci_pad16][pad32(T*N)] with (ci, t, n) <- w[n, t, ci]."""
    w3 = w2d.view(N, T, Ci).permute(2, 1, 0).reshape(Ci, T * N)
    out = torch.zeros(_r(Ci, 16), _r(T * N, 32), dtype=torch.bfloat16)
    out[:Ci, :T * N] = w3.to(torch.bfloat16)
    return out.to(device)


def _chunk(B, per_image_elems, budget=1 << 25):
    return max(1, min(B, budget // max(1, per_image_elems)))


def conv_fwd_ref(x, w, bias, k, s, p, relu):
    """fp64 NHWC conv: x [B][H][W][C], w [N][k*k*C] with column (ky, kx, c), bias [N] or None -> [B][OH][OW][N]."""
    B, H, W, C = x.shape
    N = w.shape[0]
    OH, OW = out_hw(H, W, k, s, p)
    # F.unfold orders a column (c, ky, kx)
    wu = w.view(N, k, k, C).permute(0, 3, 1, 2).reshape(N, C * k * k).double()
    out = torch.empty(B, OH, OW, N, dtype=torch.float64, device=x.device)
    step = _chunk(B, C * k * k * OH * OW)
    for b0 in range(0, B, step):
        xc = x[b0:b0 + step].double().permute(0, 3, 1, 2)
        cols = F.unfold(xc, k, padding=p, stride=s)          # [b][C*k*k][OH*OW]
        y = torch.matmul(wu, cols)                           # [b][N][OH*OW]
        out[b0:b0 + step] = y.permute(0, 2, 1).reshape(-1, OH, OW, N)
    if bias is not None:
        out += bias.double()
    return out.relu_() if relu else out


def conv_dgrad_ref(dy, w, xshape, k, s, p):
    """fp64 data gradient of :func:`conv_fwd_ref`: dy [B][OH][OW][N] -> [B][H][W][C] (no epilogue)."""
    B, H, W, C = xshape
    N = w.shape[0]
    OH, OW = out_hw(H, W, k, s, p)
    wu = w.view(N, k, k, C).permute(0, 3, 1, 2).reshape(N, C * k * k).double()
    out = torch.empty(B, H, W, C, dtype=torch.float64, device=dy.device)
    step = _chunk(B, C * k * k * OH * OW)
    for b0 in range(0, B, step):
        g = dy[b0:b0 + step].double().reshape(-1, OH * OW, N).permute(0, 2, 1)   # [b][N][L]
        cols = torch.matmul(wu.t(), g)                                           # [b][C*k*k][L]
        dx = F.fold(cols, (H, W), k, padding=p, stride=s)                        # [b][C][H][W]
        out[b0:b0 + step] = dx.permute(0, 2, 3, 1)
    return out


def conv_wgrad_ref(dy, x, k, s, p):
    """fp64 weight / bias gradient: gw [N][k*k*C] with column (ky, kx, c), gb [N]; also the per-element
    sum of |dy * x| (the exactness condition of the weight gradient)."""
    B, H, W, C = x.shape
    N = dy.shape[-1]
    OH, OW = out_hw(H, W, k, s, p)
    gw = torch.zeros(N, C * k * k, dtype=torch.float64, device=x.device)
    ab = torch.zeros_like(gw)
    step = _chunk(B, C * k * k * OH * OW)
    for b0 in range(0, B, step):
        cols = F.unfold(x[b0:b0 + step].double().permute(0, 3, 1, 2), k, padding=p, stride=s)  # [b][CKK][L]
        g = dy[b0:b0 + step].double().reshape(-1, OH * OW, N).permute(0, 2, 1)                 # [b][N][L]
        gw += torch.matmul(g, cols.transpose(1, 2)).sum(0)
        ab += torch.matmul(g.abs(), cols.abs().transpose(1, 2)).sum(0)
    reorder = lambda t: t.view(N, C, k, k).permute(0, 2, 3, 1).reshape(N, k * k * C)  # noqa: E731
    return reorder(gw), dy.double().reshape(-1, N).sum(0), reorder(ab)


def join_ref(dx, res, rmask, mask):
    """The data gradient's epilogue: (dx + res * [rmask > 0]) * [mask > 0]."""
    if res is not None:
        dx = dx + (res.double() * (rmask.double() > 0) if rmask is not None else res.double())
    if mask is not None:
        dx = dx * (mask.double() > 0)
    return dx


# ---------------------------------------------------------------------------- conditions of exactness
def assert_exact_output(y):
    """A bf16 (or fp32) output of integers: |y| <= 256 elementwise."""
    assert torch.equal(y, y.round()), "reference is not integer valued"
    assert float(y.abs().max()) <= BF16_INT_MAX, f"max |y| = {float(y.abs().max())} > {BF16_INT_MAX}"


def assert_exact_sums(y2d):
    """Forward sums of y [M][N]: per channel sum |y| and sum y^2 below 2^24 (every fp32 partial is exact)."""
    sa, sq = float(y2d.abs().sum(0).max()), float((y2d * y2d).sum(0).max())
    assert sa < FP32_INT_MAX and sq < FP32_INT_MAX, f"sum|y| = {sa}, sum y^2 = {sq}: not below 2^24"


def assert_exact_bwd_sums(g2d, xhat2d):
    """Backward sums of g [M][N] with xhat a multiple of 1/2: per channel sum |g| < 2^24, sum |g xhat| < 2^23."""
    assert torch.equal(2 * xhat2d, (2 * xhat2d).round()), "xhat is not a multiple of 1/2"
    sa, sq = float(g2d.abs().sum(0).max()), float((g2d * xhat2d).abs().sum(0).max())
    assert sa < FP32_INT_MAX and sq < (1 << 23), f"sum|g| = {sa}, sum|g xhat| = {sq}: too large to be exact"


# ------------------------------------------------------- bounds of the non-integer (consumer) comparisons
ULP32 = 2.0 ** -23   # one fp32 ulp of v is at most 2^-23 |v|


def assert_within_ulps(got, ref64, ulps, what):
    """``got`` (fp32) equals the fp32 rounding of the fp64 value ``ref64`` to ``ulps`` fp32 ulps."""
    err, bound = (got.double() - ref64).abs(), ulps * ULP32 * ref64.abs() + 1e-38
    assert (err <= bound).all(), f"{what}: {float((err / bound).max()):.2f} x the bound of {ulps} fp32 ulps"


def assert_close_elem(got, ref64, terms64, what):
    """|got - ref| <= 2^-7 |ref| + 2^-20 * (sum of the absolute terms of ref): one bf16 ulp for a rounding
    flip, plus the fp32 evaluation error."""
    err, bound = (got.double() - ref64).abs(), 2.0 ** -7 * ref64.abs() + 2.0 ** -20 * terms64
    assert (err <= bound).all(), f"{what}: {float((err / bound.clamp_min(1e-300)).max()):.2f} x the bound"


def split_replicas(total, nrep, sentinel):
    """fp64 sums [2][C] -> a [nrep + 1][2][C] buffer whose first nrep replicas sum to them (split at random, with
    cancellation) and whose last holds ``sentinel``; returns (buffer, view of the nrep replicas)."""
    buf = torch.full((nrep + 1,) + tuple(total.shape), sentinel, dtype=torch.float64, device=total.device)
    f = torch.rand((nrep,) + tuple(total.shape), dtype=torch.float64, device=total.device) * 2 - 0.5
    f[-1] = 1 - f[:-1].sum(0)
    buf[:nrep] = f * total
    return buf, buf[:nrep]
