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


def rowpad_w(w2d, KH, KW, C, H, W, pad, device):
    """[N][KH*KW*C] -> fused conv+pool forward layout bf16 [Npad16][Kpad2]: column ky*RLp + kx*Cp + c with the
    kernel's channel stride Cp; pair layout (N <= 8) additionally holds in rows 8+n the kernel of channel n
    shifted right by one column (RLp = round8((KW+1)*Cp))."""
    from distriflow_amd import ops
    N = w2d.shape[0]
    Cp, kp, pair = ops.convpool_fwd_layout(H, W, C, KH, KW, pad, N)
    RLp = _r((KW + (1 if pair else 0)) * Cp, 8)
    out = torch.zeros(_r(N, 16), kp, dtype=torch.bfloat16, device=w2d.device)
    w4 = w2d.view(N, KH, KW, C).to(torch.bfloat16)
    for ky in range(KH):
        for kx in range(KW):
            out[:N, ky * RLp + kx * Cp: ky * RLp + kx * Cp + C] = w4[:, ky, kx]
            if pair:
                out[8:8 + N, ky * RLp + (kx + 1) * Cp: ky * RLp + (kx + 1) * Cp + C] = w4[:, ky, kx]
    return out.to(device)


def cp_wt(w2d, KH, KW, C, H, W, pad, device):
    """[N][KH*KW*C] -> fused conv+pool data-gradient layout: the plain [Cpad16][K2pad] layout of :func:`pad_wt`,
    or the pair layout [16][round32(KH*(KW+1)*N)] (row c: tap (a, b) = W[n][KH-1-a][KW-1-b][c]; row 8+c: the
    same shifted by one column, W[n][KH-1-a][KW-b][c])."""
    from distriflow_amd import ops
    N = w2d.shape[0]
    pair, k2p = ops.convpool_dgrad_layout(H, W, C, KH, KW, pad, N)
    if not pair:
        return pad_wt(w2d, N, KH * KW, C, device)
    out = torch.zeros(16, k2p, dtype=torch.bfloat16, device=w2d.device)
    w4 = w2d.view(N, KH, KW, C).to(torch.bfloat16)
    for a in range(KH):
        for b in range(KW + 1):
            col = (a * (KW + 1) + b) * N
            if b < KW:
                out[:C, col:col + N] = w4[:, KH - 1 - a, KW - 1 - b, :].t()
            if b >= 1:
                out[8:8 + C, col:col + N] = w4[:, KH - 1 - a, KW - b, :].t()
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


# ------------------------------------------------------------------------------------- max-pool, ties included
# The tie rule every argmax kernel documents: the FIRST maximum in row-major window order (j = dy * P + dx).
def windows(y, P=2):
    """[B][OH][OW][N] -> [B][OH//P][OW//P][N][P*P] in row-major window order; rows / columns past the last whole
    window are dropped."""
    B, OH, OW, N = y.shape
    PH, PW = OH // P, OW // P
    return y[:, :PH * P, :PW * P].reshape(B, PH, P, PW, P, N).permute(0, 1, 3, 5, 2, 4).reshape(B, PH, PW, N, P * P)


def window_argmax(win):
    """win [..., P*P] in row-major window order -> (max, index of the first maximum): an explicit scan with a
    strict ``>``, so nothing rests on the tie behaviour of ``torch.max``."""
    m = win[..., 0].clone()
    am = torch.zeros(m.shape, dtype=torch.int64, device=win.device)
    for j in range(1, win.shape[-1]):
        v = win[..., j]
        better = v > m
        m = torch.where(better, v, m)
        am = torch.where(better, torch.full_like(am, j), am)
    return m, am


def code_convpool(m, am):
    """csrc/convpool.hip: argmax | 4 * (max > 0)."""
    return (am | ((m > 0).to(torch.int64) << 2)).to(torch.uint8)


def code_relu4(m, am):
    """csrc/kcnn_fused.hip, the igemm64 POOL epilogue and unpool2: argmax, or 4 (no gradient) when max <= 0."""
    return torch.where(m > 0, am, torch.full_like(am, 4)).to(torch.uint8)


def unpool_ref(dyp, code, OH, OW, convention):
    """fp64 full-resolution gradient [B][OH][OW][N] of a 2x2 max-pool from the pooled gradient and the codes of
    ``convention`` ('convpool' | 'relu4'); zero outside the windows and where the code passes nothing."""
    B, PH, PW, N = code.shape
    c = code.long()
    if convention == "convpool":
        pos, live = c & 3, (c & 4) > 0
    elif convention == "relu4":
        pos, live = c.clamp_max(3), c < 4
    else:
        raise ValueError(convention)
    g = dyp.double().reshape(B, PH, PW, N) * live
    out = torch.zeros(B, OH, OW, N, dtype=torch.float64, device=code.device)
    for j in range(4):
        out[:, j // 2:2 * PH:2, j % 2:2 * PW:2] = g * (pos == j)
    return out


def pool_max_ref(x, geom):
    """General max-pool of x [B][H][W][C] over ``geom`` (``ops.pool_geometry``): windows clipped to the image, any
    stride, overlap allowed.  -> (y [B][OH][OW][C] fp64 with 0 for an empty window, max, row and column of the
    first maximum in row-major scan order; row -1 for an empty window)."""
    B, H, W, C, OH, OW, ph, pw, sh, sw, pt, pl = geom
    x = x.double()
    dev = x.device
    m = torch.full((B, OH, OW, C), float("-inf"), dtype=torch.float64, device=dev)
    ah = torch.full((B, OH, OW, C), -1, dtype=torch.int64, device=dev)
    aw = ah.clone()
    oh, ow = torch.arange(OH, device=dev), torch.arange(OW, device=dev)
    for i in range(ph):
        for j in range(pw):
            hh, ww = oh * sh - pt + i, ow * sw - pl + j
            inside = ((hh >= 0) & (hh < H))[:, None] & ((ww >= 0) & (ww < W))[None, :]
            v = x[:, hh.clamp(0, H - 1)][:, :, ww.clamp(0, W - 1)]
            better = inside[None, :, :, None] & (v > m)
            m = torch.where(better, v, m)
            ah = torch.where(better, hh[None, :, None, None].expand_as(ah), ah)
            aw = torch.where(better, ww[None, None, :, None].expand_as(aw), aw)
    return torch.where(ah >= 0, m, torch.zeros_like(m)), m, ah, aw


def pool_max_bwd_ref(x, dy, geom, relu):
    """fp64 gradient of :func:`pool_max_ref`: every window sends its gradient to its first maximum, gradients sum
    per input pixel; with ``relu`` a window whose maximum is not positive sends nothing."""
    B, H, W, C, OH, OW = geom[:6]
    _, m, ah, aw = pool_max_ref(x, geom)
    live = (ah >= 0) & (m > 0) if relu else ah >= 0
    b = torch.arange(B, device=m.device)[:, None, None, None]
    c = torch.arange(C, device=m.device)[None, None, None, :]
    flat = ((b * H + ah.clamp_min(0)) * W + aw.clamp_min(0)) * C + c
    dx = torch.zeros(B * H * W * C, dtype=torch.float64, device=m.device)
    dx.index_add_(0, flat.reshape(-1), (dy.double().reshape(B, OH, OW, C) * live).reshape(-1))
    return dx.view(B, H, W, C)


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
