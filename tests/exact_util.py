"""Integer-valued test data and an fp64 reference for the exact kernel tests.

With inputs, weights and bias taken from small integers every product, every fp32 partial sum in any order,
every bf16-rounded output and every fp32 / fp64 accumulator of a conv / dense kernel is exactly representable,
so ``torch.equal`` against an fp64 reference is the right assertion: no tolerance hides a wrong row, tap, tail
or replica.  That holds under conditions on the REFERENCE (``assert_exact_*`` below), which every test asserts
before it compares anything; they are conditions, not tolerances.

The reference is ``F.unfold`` / ``F.fold`` + matmul in float64, in batch chunks.  It does not go through
``ops.reference``: that casts to fp32, and an fp32 library conv may pick a Winograd-class algorithm, which is
not exact on integers.  The conv references take one (k, s, p) or a ``ConvGeom`` (per-axis kernel and strides,
top / left padding, the bottom / right padding the output size implies); the transposed conv is that conv with
the roles swapped, the depthwise conv a loop over its taps.

Everything is generated on the CPU from a seeded generator (the same values with and without a GPU) and moved
to ``device`` afterwards.
"""
import torch
import torch.nn.functional as F

from distriflow_amd.ops import geometry
from distriflow_amd.ops.geometry import ConvGeom, DeconvGeom, DwGeom, pad_after

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


def conv_geom(xshape, N, k, s=1, p=0):
    """The ``ConvGeom`` of a conv reference: ``k`` is a ConvGeom already (``s``, ``p`` unused), or the kernel k /
    (kh, kw) with strides s / (sh, sw) and the symmetric padding p / (ph, pw)."""
    if isinstance(k, ConvGeom):
        return k
    B, H, W, C = xshape
    OH, OW = geometry.out_hw(H, W, k, s, p)
    return ConvGeom.of(B, H, W, C, OH, OW, N, *geometry.pair(k), s, p)


def _padded_hw(g):
    """Size of the padded image the windows of ``g`` tile exactly (they read nothing past it)."""
    return (g.OH - 1) * g.sh + g.KH, (g.OW - 1) * g.sw + g.KW


def _unfold(xc, g):
    """NCHW fp64 -> the columns [b][C*KH*KW][OH*OW] of ``g``'s windows: top / left padding (pt, pl), the bottom /
    right padding the output size implies (negative: trailing pixels that no window reads are cropped)."""
    xp = F.pad(xc, (g.pl, pad_after(g.W, g.OW, g.KW, g.sw, g.pl), g.pt, pad_after(g.H, g.OH, g.KH, g.sh, g.pt)))
    assert tuple(xp.shape[2:]) == _padded_hw(g)
    return F.unfold(xp, (g.KH, g.KW), stride=(g.sh, g.sw))


def _w_unfold(w, g):
    """[N][KH*KW*C] with column (ky, kx, c) -> fp64 [N][C*KH*KW] in F.unfold's column order (c, ky, kx)."""
    return w.view(g.N, g.KH, g.KW, g.C).permute(0, 3, 1, 2).reshape(g.N, g.C * g.KH * g.KW).double()


def conv_fwd_ref(x, w, bias, k, s=1, p=0, relu=False):
    """fp64 NHWC conv: x [B][H][W][C], w [N][KH*KW*C] with column (ky, kx, c), bias [N] or None -> [B][OH][OW][N].
    ``k, s, p``: see :func:`conv_geom`."""
    B = x.shape[0]
    g = conv_geom(x.shape, w.shape[0], k, s, p)
    wu = _w_unfold(w, g)
    out = torch.empty(B, g.OH, g.OW, g.N, dtype=torch.float64, device=x.device)
    step = _chunk(B, wu.shape[1] * g.OH * g.OW)
    for b0 in range(0, B, step):
        cols = _unfold(x[b0:b0 + step].double().permute(0, 3, 1, 2), g)   # [b][C*KH*KW][OH*OW]
        y = torch.matmul(wu, cols)                                        # [b][N][OH*OW]
        out[b0:b0 + step] = y.permute(0, 2, 1).reshape(-1, g.OH, g.OW, g.N)
    if bias is not None:
        out += bias.double()
    return out.relu_() if relu else out


def conv_dgrad_ref(dy, w, xshape, k, s=1, p=0):
    """fp64 data gradient of :func:`conv_fwd_ref`: dy [B][OH][OW][N] -> [B][H][W][C] (no epilogue); exactly 0 at
    the pixels no window reads."""
    B = xshape[0]
    g = conv_geom(xshape, w.shape[0], k, s, p)
    wu = _w_unfold(w, g)
    PH, PW = _padded_hw(g)
    hh, ww = min(g.H, PH - g.pt), min(g.W, PW - g.pl)   # the rows / columns of the image inside the padded one
    out = torch.zeros(B, g.H, g.W, g.C, dtype=torch.float64, device=dy.device)
    step = _chunk(B, wu.shape[1] * g.OH * g.OW)
    for b0 in range(0, B, step):
        gy = dy[b0:b0 + step].double().reshape(-1, g.OH * g.OW, g.N).permute(0, 2, 1)   # [b][N][L]
        cols = torch.matmul(wu.t(), gy)                                                 # [b][C*KH*KW][L]
        dx = F.fold(cols, (PH, PW), (g.KH, g.KW), stride=(g.sh, g.sw))                  # [b][C][PH][PW]
        out[b0:b0 + step, :hh, :ww] = dx[:, :, g.pt:g.pt + hh, g.pl:g.pl + ww].permute(0, 2, 3, 1)
    return out


def conv_wgrad_ref(dy, x, k, s=1, p=0):
    """fp64 weight / bias gradient: gw [N][KH*KW*C] with column (ky, kx, c), gb [N]; also the per-element
    sum of |dy * x| (the exactness condition of the weight gradient)."""
    B = x.shape[0]
    N = dy.shape[-1]
    g = conv_geom(x.shape, N, k, s, p)
    CK = g.C * g.KH * g.KW
    gw = torch.zeros(N, CK, dtype=torch.float64, device=x.device)
    ab = torch.zeros_like(gw)
    step = _chunk(B, CK * g.OH * g.OW)
    for b0 in range(0, B, step):
        cols = _unfold(x[b0:b0 + step].double().permute(0, 3, 1, 2), g)                        # [b][CKK][L]
        gy = dy[b0:b0 + step].double().reshape(-1, g.OH * g.OW, N).permute(0, 2, 1)            # [b][N][L]
        gw += torch.matmul(gy, cols.transpose(1, 2)).sum(0)
        ab += torch.matmul(gy.abs(), cols.abs().transpose(1, 2)).sum(0)
    reorder = lambda t: t.view(N, g.C, g.KH, g.KW).permute(0, 2, 3, 1).reshape(N, CK)  # noqa: E731
    return reorder(gw), dy.double().reshape(-1, N).sum(0), reorder(ab)


# ------------------------------------------------------------------------------------------ transposed conv
# A Conv2DTranspose is the conv G = DeconvGeom.G with the roles swapped (ops/geometry.py): x [B][H][W][Cin] is G's
# output gradient, the layer's output [B][OH][OW][F] G's input, w = G's matrix [Cin][KH*KW*F].
def deconv_fwd_ref(x, w, bias, dgeom, relu):
    """fp64 [relu](G's data gradient of x + bias) -> [B][OH][OW][F]."""
    G = DeconvGeom(*dgeom).G
    y = conv_dgrad_ref(x.reshape(G.y_shape), w, G.x_shape, G)
    if bias is not None:
        y += bias.double()
    return y.relu_() if relu else y


def deconv_dgrad_ref(dy, w, dgeom, mask=None):
    """fp64 G(dy) * [mask > 0] -> [B][H][W][Cin]."""
    G = DeconvGeom(*dgeom).G
    return join_ref(conv_fwd_ref(dy.reshape(G.x_shape), w, None, G), None, None, mask)


def deconv_wgrad_ref(dy, x, dgeom):
    """fp64 kernel gradient [Cin][KH*KW*F] (G's, with x and dy exchanged, no bias column), gb [F] = sum dy, and
    the per-element sum of |x * dy|."""
    G = DeconvGeom(*dgeom).G
    gw, _, ab = conv_wgrad_ref(x.reshape(G.y_shape), dy.reshape(G.x_shape), G)
    return gw, dy.double().reshape(-1, G.C).sum(0), ab


# ------------------------------------------------------------------------------------------- depthwise conv
# Weights [KH][KW][C*M], output channel co reads input channel co // M.  A loop over the KH*KW taps on shifted,
# strided slices of the padded image: no library conv.
def _dw_pads(g):
    return g.pl, pad_after(g.W, g.OW, g.KW, g.sw, g.pl), g.pt, pad_after(g.H, g.OH, g.KH, g.sh, g.pt)


def _dw_taps(g):
    """(kh, kw, row slice, column slice) of every tap: the padded pixels the OH x OW windows read at that tap."""
    for kh in range(g.KH):
        for kw in range(g.KW):
            yield kh, kw, slice(kh, kh + (g.OH - 1) * g.sh + 1, g.sh), slice(kw, kw + (g.OW - 1) * g.sw + 1, g.sw)


def _dw_source(x, g):
    """x [B][H][W][C] -> fp64 padded / cropped [B][PH][PW][C*M] with channel co = input channel co // M."""
    xp = F.pad(x.double(), (0, 0) + _dw_pads(g))
    assert tuple(xp.shape[1:3]) == _padded_hw(g)
    return xp.repeat_interleave(g.M, dim=3) if g.M > 1 else xp


def dwconv_fwd_ref(x, w, bias, geom, relu=False):
    g = DwGeom(*geom)
    xs, w = _dw_source(x, g), w.double()
    y = torch.zeros(x.shape[0], g.OH, g.OW, g.C * g.M, dtype=torch.float64, device=x.device)
    for kh, kw, rows, cols in _dw_taps(g):
        y += xs[:, rows, cols] * w[kh, kw]
    if bias is not None:
        y += bias.double()
    return y.relu_() if relu else y


def dwconv_dgrad_ref(dy, w, geom, mask=None):
    """fp64 [B][H][W][C]: every tap's dy * w scattered to the pixel it read, summed over the M outputs of a
    channel; exactly 0 at pixels no window reads; * [mask > 0]."""
    g = DwGeom(*geom)
    B, (PH, PW) = dy.shape[0], _padded_hw(g)
    dy, w = dy.double().reshape(B, g.OH, g.OW, g.C * g.M), w.double()
    dp = torch.zeros(B, PH, PW, g.C * g.M, dtype=torch.float64, device=dy.device)
    for kh, kw, rows, cols in _dw_taps(g):
        dp[:, rows, cols] += dy * w[kh, kw]
    dp = dp.view(B, PH, PW, g.C, g.M).sum(-1)
    hh, ww = min(g.H, PH - g.pt), min(g.W, PW - g.pl)
    dx = torch.zeros(B, g.H, g.W, g.C, dtype=torch.float64, device=dy.device)
    dx[:, :hh, :ww] = dp[:, g.pt:g.pt + hh, g.pl:g.pl + ww]
    return join_ref(dx, None, None, mask.reshape(dx.shape) if mask is not None else None)


def dwconv_wgrad_ref(dy, x, geom):
    """fp64 gw [KH][KW][C*M], gb [C*M], and the per-element sum of |dy * x|."""
    g = DwGeom(*geom)
    xs, dy = _dw_source(x, g), dy.double().reshape(x.shape[0], g.OH, g.OW, g.C * g.M)
    gw = torch.zeros(g.KH, g.KW, g.C * g.M, dtype=torch.float64, device=x.device)
    ab = torch.zeros_like(gw)
    for kh, kw, rows, cols in _dw_taps(g):
        prod = xs[:, rows, cols] * dy
        gw[kh, kw], ab[kh, kw] = prod.sum((0, 1, 2)), prod.abs().sum((0, 1, 2))
    return gw, dy.sum((0, 1, 2)), ab


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


# ------------------------------------------------------------------- dense heads with a saturated softmax
# A Dense chain + softmax cross-entropy is exact on integers once the softmax saturates: the last layer has
# weights in 2048 * {-1, 0, 1} and the bias 128 * perm(16)[:C], so the logits of a row are congruent to distinct
# multiples of 128 modulo 2048: pairwise >= 128 apart, the maximum unique.  exp(z - max) for z - max <= -104
# is below 2^-150, exactly 0 in fp32, so sum = 1, 1 / sum = 1, log(sum) = 0 and the kernel must produce exactly
# dZ_last = grad_scale * (onehot(argmax) - onehot(y)), row loss = max - z_y, correct = [argmax == y].
def _r32(n):
    return _r(n, 32)


def head_ints(g, B, dims, with_idx=False, bias=True):
    """Integer data of the head ``dims[0] -> ... -> dims[-1]`` (C = dims[-1] <= 16 classes): x in [-1, 2], hidden
    weights in {-1, 0, 1} with about 48 non-zeros per row, hidden bias in [-3, 3], dense last-layer weights in
    2048 * {-1, 0, 1} with the bias 128 * perm(16)[:C].  ``with_idx``: the labels are a table of 3 B rows read
    through an index vector.  ``bias=False``: no bias anywhere; the distinct multiples of 128 then reach the
    logits through a unit that is 1 in every row (x[:, 0] = 1, row 0 of each hidden layer passes it on, column 0
    of the last layer holds 128 * perm(16)[:C])."""
    nl, C = len(dims) - 1, dims[-1]
    x = ints(g, (B, dims[0]), -1, 2)
    W, b = [], []
    for l in range(nl):
        K, N = dims[l], dims[l + 1]
        if l < nl - 1:
            W.append(sparse_ints(g, (N, K), -1, 1, weight_density(K, 48)))
            b.append(ints(g, (N,), -3, 3))
        else:
            W.append(2048.0 * ints(g, (N, K), -1, 1))
            b.append(128.0 * torch.randperm(16, generator=g)[:C].double())
    if not bias:
        x[:, 0] = 1
        for l in range(nl - 1):
            W[l][0] = 0
            W[l][0, 0] = 1
        W[-1][:, 0] = b[-1]
        b = [None] * nl
    table = torch.randint(0, C, (3 * B if with_idx else B,), generator=g, dtype=torch.int32)
    idx = torch.randperm(3 * B, generator=g)[:B] if with_idx else None
    return {"dims": tuple(dims), "x": x, "W": W, "b": b, "labels": table, "idx": idx,
            "y": (table[idx] if with_idx else table).long()}


def head_ref(d, grad_scale, drop=None, dh_scale=1.0, x_relu=False, dx_scale=1.0):
    """fp64 reference of everything a fused head kernel writes for the data ``d`` of :func:`head_ints`, with the
    softmax saturated (see above; :func:`assert_exact_head` asserts that it is).

    ``drop = (p, seed, step)``: a dropout folded after the LAST hidden layer, mask
    ``reference.dropout_mask(B * N, p, seed ^ (step * 0x9E3779B1))`` over [B][N], forward * 1 / (1 - p), backward
    * ``dh_scale``.  ``x_relu``: relu' of the input on dx.  ``dx_scale`` multiplies dx.

    -> dict: acts (x and every hidden activation), pre_drop, logits, dz (per layer), dx, gw, gb, gw_terms,
    logit_terms, loss_rows, loss_part [ceil(B/16)][2], stats [2], argmax."""
    from distriflow_amd.ops import reference

    x, W, b, y = d["x"], d["W"], d["b"], d["y"]
    nl, B, C = len(W), x.shape[0], W[-1].shape[0]
    acts, pre_drop, keep = [x], None, None
    for l in range(nl - 1):
        h = (acts[-1] @ W[l].t() + (b[l] if b[l] is not None else 0)).relu()
        if drop is not None and l == nl - 2:
            p, seed, step = drop
            keep = reference.dropout_mask(B * h.shape[1], p, seed ^ (step * 0x9E3779B1)).double().view(B, -1)
            pre_drop, h = h, h * keep / (1.0 - p)
        acts.append(h)
    logits = acts[-1] @ W[-1].t() + (b[-1] if b[-1] is not None else 0)
    logit_terms = acts[-1].abs() @ W[-1].abs().t() + (b[-1].abs() if b[-1] is not None else 0)
    mx, am = window_argmax(logits)          # the strict-> scan: first maximum
    zy = logits.gather(1, y[:, None])[:, 0]
    loss_rows, correct = mx - zy, (am == y).double()
    dz = [None] * nl
    dz[-1] = grad_scale * (F.one_hot(am, C).double() - F.one_hot(y, C).double())
    for l in range(nl - 1, 0, -1):
        dz[l - 1] = (dz[l] @ W[l]) * (acts[l] > 0) * (dh_scale if (keep is not None and l == nl - 1) else 1.0)
    dx = dz[0] @ W[0]
    if x_relu:
        dx = dx * (x > 0)
    dx = dx * dx_scale
    nb = (B + 15) // 16
    part = torch.zeros(nb * 16, 2, dtype=torch.float64)
    part[:B, 0], part[:B, 1] = loss_rows, correct
    part = part.view(nb, 16, 2).sum(1)
    return {"acts": acts, "pre_drop": pre_drop, "logits": logits, "logit_terms": logit_terms, "argmax": am,
            "dz": dz, "dx": dx, "gw": [dz[l].t() @ acts[l] for l in range(nl)], "gb": [dz[l].sum(0) for l in range(nl)],
            "gw_terms": [dz[l].abs().t() @ acts[l].abs() for l in range(nl)], "loss_rows": loss_rows,
            "loss_terms": mx.abs() + zy.abs(), "loss_part": part, "stats": part.sum(0)}


def _unit(t):
    """The largest power of two 2^-k (0 <= k <= 24) of which every entry of t is a multiple."""
    for k in range(25):
        if torch.equal(t * 2.0 ** k, (t * 2.0 ** k).round()):
            return 2.0 ** -k
    raise AssertionError("not a dyadic fraction with at most 24 fractional bits")


def assert_exact_head(ref):
    """The conditions under which a head kernel must reproduce ``ref`` (:func:`head_ref`) bit for bit.  C = 1 is the
    one case whose gradients are all exactly zero (argmax = y = 0); it is held to that instead of to a density."""
    C = ref["logits"].shape[1]
    # activations: integers <= 256 (<= 128 before a dropout's * 2)
    for h in ref["acts"]:
        assert_exact_output(h)
    if ref["pre_drop"] is not None:
        assert float(ref["pre_drop"].abs().max()) <= 128, "pre-dropout activation above 128"
    # saturation: the top-2 gap of every row
    if C > 1:
        top = ref["logits"].topk(2, dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        assert gap >= 104, f"top-2 logit gap {gap} < 104: the softmax does not saturate"
    # logits and loss sums: multiples of 128, exact in fp32 while (sum |terms|) / 128 < 2^24
    assert torch.equal(ref["logits"] / 128, (ref["logits"] / 128).round()), "logits are not multiples of 128"
    assert float(ref["logit_terms"].max()) / 128 < FP32_INT_MAX, "logit terms too large"
    assert float(ref["loss_terms"].sum()) / 128 < FP32_INT_MAX, "loss terms too large"
    # weight / bias gradients: fp32 sums of multiples of a power of two, sum |dz h| / unit < 2^24 per element
    for l, (dz, terms) in enumerate(zip(ref["dz"], ref["gw_terms"])):
        u = min(_unit(dz), 1.0)
        assert float(terms.max()) < FP32_INT_MAX, f"layer {l}: sum |dz h| not below 2^24"
        assert float(terms.max()) / u < FP32_INT_MAX, f"layer {l}: sum |dz h| / {u} not below 2^24"
        assert float(dz.abs().sum(0).max()) / u < FP32_INT_MAX, f"layer {l}: sum |dz| / {u} not below 2^24"
    # every bf16 output is a bf16 value
    for name, t in [("dx", ref["dx"])] + [(f"dz{l}", t) for l, t in enumerate(ref["dz"])]:
        assert torch.equal(t.to(torch.bfloat16).double(), t), f"{name} is not representable in bf16"
    # the comparison sees something: >= 5 % of each gradient non-zero (C = 1: all exactly zero)
    for name, t in [("dx", ref["dx"])] + [(f"gw{l}", t) for l, t in enumerate(ref["gw"])] + \
                   [(f"gb{l}", t) for l, t in enumerate(ref["gb"])]:
        nz = float((t != 0).double().mean())
        if C == 1:
            assert nz == 0, f"{name}: a one-class head has zero gradients"
        else:
            assert nz >= 0.05, f"{name}: only {100 * nz:.1f} % non-zero"


# The shapes of tests/test_head_exact_gpu.py, each the smallest that reaches its path; tests/test_exact_util.py
# asserts the conditions above for every one of them without a GPU.
KHEAD_N1 = 128
HEAD_GRAD_SCALE = 2.0 ** -11           # dZ_last = +-2^-11, dZ_last W_last an integer in [-2, 2]
HEAD_DROP = (0.5, 0x5EED, 5)           # (p, seed, step)
# (B, K, C, dropout, labels through idx)
KHEAD_CASES = [
    (1, 256, 1, False, False),         # one row, KS = 1 (waves 2, 3 idle in the dP phase), C = 1: zero gradients
    (33, 256, 10, False, False),       # a second row tile with a single valid row
    (70, 512, 10, True, True),         # dropout 0.5, dh_scale 2, labels through idx
    (100, 1536, 16, False, False),     # KS = 6 = PF exactly, C = 16
    (47, 1792, 3, True, False),        # KS = 7 = PF + 1
    (96, 3072, 10, False, False),      # KS = 12 = 2 PF, B a multiple of 32
    (40, 3328, 10, False, False),      # KS = 13: the second trip of the ping-pong loop
    (200, 4608, 10, True, True),       # the <18> instantiation
    (40, 5376, 10, True, False),       # the largest supported K (KS = 21)
    (1040, 256, 10, False, False),     # 264 jobs > 256 workgroups; 33 batch steps in the weight gradient
]
# (B, dims, labels through idx, x_relu, dx_scale)
MLPHEAD_CASES = [
    (50, (64, 48, 32, 10), False, False, 1.0),     # the last block has 2 rows
    (19, (400, 120, 84, 10), True, True, 1.0),     # the LeNet-5 head
    (96, (784, 10), False, False, 1.0),            # a single layer
    (33, (30, 16), False, False, 1.0),             # D0 % 8 != 0: the scalar staging path; C = 16
    (300, (200, 100, 10), False, False, 0.5),      # 19 blocks: the loss reduction spans lane rounds
    (16, (256, 128, 1), False, False, 1.0),        # C = 1
]


def khead_case(B, K, C, drop, with_idx, bias=True, dp_mask=True, seed=0):
    """(data, reference) of a khead case: Dense(K -> 128, ReLU) [-> Dropout 0.5] -> Dense(C), dP scaled by 0.5."""
    d = head_ints(gen(1000 * seed + B + K + C), B, (K, KHEAD_N1, C), with_idx, bias)
    ref = head_ref(d, HEAD_GRAD_SCALE, HEAD_DROP if drop else None, 2.0 if drop else 1.0, dp_mask, 0.5)
    return d, ref


def mlphead_case(B, dims, with_idx, x_relu, dx_scale, seed=0):
    d = head_ints(gen(1000 * seed + B + sum(dims)), B, dims, with_idx)
    return d, head_ref(d, HEAD_GRAD_SCALE, x_relu=x_relu, dx_scale=dx_scale)


# ------------------------------------------------ irregular, transposed and depthwise convs: cases and data
# tests/test_conv_geometry_exact_gpu.py, tests/test_deconv_exact_gpu.py and tests/test_depthwise_exact_gpu.py run
# these on the GPU; tests/test_exact_util.py asserts the references and the conditions of exactness for every
# case without one.
# (B, H, W, C, N, kernel, strides, padding): none is ``ConvGeom.regular``, so all take the generic kernels
IRREGULAR_CONVS = [
    (4, 9, 8, 8, 16, (3, 5), (2, 1), "same"),
    (4, 16, 16, 16, 32, (3, 3), (2, 2), "same"),
    (3, 7, 10, 3, 8, (2, 4), (1, 2), "same"),      # LUT gather forward
    (2, 9, 11, 8, 24, (1, 3), (3, 2), "valid"),
    (2, 12, 6, 5, 40, (5, 1), (1, 1), "same"),     # LUT gather forward
    # padding symmetric in one axis only; C = 24: the 32-wide K step crosses taps; M = 108: a partial 64-row
    # tile; N = 72: a partial 128-wide tile
    (3, 11, 12, 24, 72, (3, 3), (2, 2), "same"),
    (5, 7, 7, 1, 8, (2, 2), (3, 3), "same"),       # C = 1; stride > kernel: unread pixels must get dx = 0
    (2, 10, 10, 40, 136, (3, 2), (1, 1), "same"),  # two 128-wide tiles, the second 8 wide; two wgrad splits
    (2, 6, 9, 8, 5, (2, 2), (1, 2), "valid"),      # N = 5: LUT data gradient, weight gradient without dvec
]
# (B, H, W, Cin, F, kernel, strides, padding) of a Conv2DTranspose: the nine of tests/test_decoder_gpu.py, then
DECONVS = [
    (2, 5, 5, 8, 8, (3, 3), (2, 2), "same"),
    (2, 4, 6, 3, 5, (3, 3), (2, 2), "valid"),
    (2, 4, 4, 16, 8, (4, 4), (2, 2), "same"),
    (2, 4, 4, 64, 32, (4, 4), (2, 2), "same"),
    (2, 8, 8, 64, 64, (3, 3), (1, 1), "same"),
    (2, 3, 3, 8, 8, (2, 2), (3, 3), "same"),
    (1, 1, 1, 8, 16, (3, 3), (1, 1), "same"),
    (2, 5, 4, 8, 8, (5, 3), (1, 2), "same"),
    (2, 7, 7, 8, 1, (3, 3), (2, 2), "same"),
    (5, 7, 5, 64, 16, (3, 3), (2, 2), "valid"),    # parity classes of unequal size (15x11 output), partial tiles
    (5, 8, 8, 64, 32, (4, 4), (2, 2), "same"),     # a parity class spans 2.5 row tiles; wgrad tr with 2 splits
    (2, 3, 4, 64, 8, (1, 1), (2, 2), "valid"),     # three of the four parity classes have no tap: bias only
    (2, 5, 3, 128, 64, (4, 4), (2, 2), "same"),    # two 64-channel blocks per tap; input gradient igemm64 FAST
    (3, 5, 5, 24, 40, (3, 3), (2, 2), "same"),     # generic vector gather with Cin = 24
    (2, 6, 6, 16, 8, (2, 2), (2, 2), "valid"),     # kernel = stride: every output pixel has exactly one tap
    (2, 3, 5, 64, 64, (3, 3), (1, 1), "valid"),    # FAST stride 1 in both directions
]
# (B, H, W, C, M, kernel, strides, padding) of a DepthwiseConv2D: the fifteen of tests/test_depthwise_gpu.py
DWCONVS = [
    (3, 9, 9, 8, 1, (3, 3), (1, 1), "same"),
    (2, 8, 8, 16, 1, (3, 3), (2, 2), "same"),
    (2, 9, 9, 16, 1, (3, 3), (2, 2), "same"),
    (3, 7, 10, 3, 1, (2, 4), (1, 2), "same"),
    (2, 11, 11, 20, 1, (5, 5), (1, 1), "valid"),
    (2, 9, 11, 4, 2, (3, 3), (1, 1), "same"),
    (1, 1, 1, 8, 1, (3, 3), (1, 1), "same"),
    (5, 17, 17, 72, 1, (3, 3), (1, 1), "same"),
    (2, 6, 7, 8, 1, (2, 3), (1, 1), "same"),
    (2, 10, 10, 8, 1, (3, 3), (3, 3), "same"),
    (2, 10, 9, 8, 1, (3, 3), (1, 1), "valid"),
    (1, 5, 5, 512, 1, (3, 3), (1, 1), "same"),
    (1, 4, 5, 320, 1, (2, 3), (1, 1), "same"),
    (1, 3, 3, 2056, 1, (3, 3), (2, 2), "same"),
    (1, 3, 4, 150, 2, (2, 2), (1, 1), "valid"),
]
DWCONVS_MISALIGNED = [DWCONVS[0], DWCONVS[8]]      # the 3x3 vector kernels and the generic vector kernels
# the smallest shapes whose launches stride their grid (csrc/dwconv.hip: kDwMaxGrid * 256 = 524288 work items)
DW_GRID_ITEMS = 2048 * 256
DWCONVS_GRID = [
    # 525312 walks of CC = 9 channel vectors, 524288 mod 9 = 2: the second pass reloads another vector's weights
    # (3x3 forward, data gradient, weight gradient; the weight gradient's 58368 walks / PL = 28 exceed 1024 slabs)
    (114, 2, 512, 72, 1, (3, 3), (1, 1), "same"),
    (4, 64, 64, 33, 2, (3, 3), (1, 1), "same"),    # generic scalar kernels, M = 2: 1081344 / 540672 items
    (2, 23, 23, 128, 2, (2, 2), (1, 1), "same"),   # CO = 256: PL = 1, 1058 positions > 1024 slabs
]


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}x{c[4]}_k{c[5][0]}{c[5][1]}_s{c[6][0]}{c[6][1]}_{c[7]}"


def _case_seed(c):
    return sum((i + 1) * int(v) for i, v in enumerate(c[:5])) + 31 * c[5][0] + 37 * c[5][1] + 41 * c[6][0] + 43 * c[6][1]


def conv_case(case):
    """Integer data of an igemm conv case (the values of ``test_conv_exact_on_integers``): x, dy, mask, rmask in
    {-1, 0, 1}, res in [-2, 2], w [N][KH*KW*C] in {-1, 0, 1} with about 64 non-zeros per reduction, bias in
    [-3, 3].  -> dict with the ConvGeom ``g`` (CPU fp64)."""
    g = ConvGeom.build(*case)
    r = gen(_case_seed(case))
    T = g.KH * g.KW
    return {"g": g, "x": ints(r, g.x_shape, -1, 1), "dy": ints(r, g.y_shape, -1, 1),
            "w": sparse_ints(r, (g.N, T * g.C), -1, 1, weight_density(T * max(g.C, g.N))), "b": ints(r, (g.N,), -3, 3),
            "res": ints(r, g.x_shape, -2, 2), "rmask": ints(r, g.x_shape, -1, 1), "mask": ints(r, g.x_shape, -1, 1)}


def deconv_case(case):
    """Integer data of a transposed conv case, as :func:`conv_case`: x [B][H][W][Cin] (also the relu' mask of the
    input gradient, as the layer passes it), dy [B][OH][OW][F], w = G's matrix [Cin][KH*KW*F], bias [F]; ``geom``
    is the DeconvGeom."""
    G = ConvGeom.transposed(*case)
    r = gen(_case_seed(case) + 1)
    T = G.KH * G.KW
    return {"geom": G.t_geom, "G": G, "x": ints(r, G.y_shape, -1, 1), "dy": ints(r, G.x_shape, -1, 1),
            "w": sparse_ints(r, (G.N, T * G.C), -1, 1, weight_density(T * max(G.C, G.N))), "b": ints(r, (G.C,), -3, 3)}


def dw_case(case):
    """Integer data of a depthwise case: x (also the relu' mask), dy in [-2, 2], fp32 weights [KH][KW][C*M] and
    bias in [-3, 3]: |y| <= KH*KW * 6 + 3 and |dx| <= KH*KW * M * 6."""
    g = DwGeom.build(*case)
    r = gen(_case_seed(case) + 2)
    CO = g.C * g.M
    return {"geom": g, "x": ints(r, (g.B, g.H, g.W, g.C), -2, 2), "dy": ints(r, (g.B, g.OH, g.OW, CO), -2, 2),
            "w": ints(r, (g.KH, g.KW, CO), -3, 3), "b": ints(r, (CO,), -3, 3)}


def dw_work_items(geom):
    """Work items of the forward, data-gradient and weight-gradient launches of csrc/dwconv.hip on aligned
    operands: (image, 8-row chunk, column, channel vector) walks on the 3x3 vector kernels, else one per output
    vector / element; weight gradient: walks / positions, and the position lanes per workgroup PL."""
    g = DwGeom(*geom)
    vec = g.M == 1 and g.C % 8 == 0
    CO, k3 = g.C * g.M, g.KH == 3 and g.KW == 3
    cu = CO // 8 if vec else CO
    chunks = lambda n: -(-n // 8)  # noqa: E731
    fwd = g.B * chunks(g.OH) * g.OW * cu if vec and k3 and g.sh <= 2 else g.B * g.OH * g.OW * cu
    dg = g.B * chunks(g.H) * g.W * (g.C // 8) if vec and k3 and (g.sh, g.sw) == (1, 1) else \
        g.B * g.H * g.W * (g.C // 8 if vec else g.C)
    wg = g.B * chunks(g.OH) * g.OW if vec and k3 and g.sh <= 2 else g.B * g.OH * g.OW
    return fwd, dg, wg, 256 // min(cu, 256)


def zero_share(t):
    return float((t == 0).double().mean())


def offset_view(t):
    """The same values as a view that starts one element into a larger buffer: contiguous, not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def assert_same(got, exp, what):
    """``torch.equal(got, exp)`` (exp fp64; a NaN left in ``got`` differs), naming the first differing index."""
    got = got.double()
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(exp.shape)}"
    if not torch.equal(got, exp):
        bad = got != exp
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {exp.numel()} elements differ, the first at {i}: "
                             f"got {float(got[i])}, expected {float(exp[i])}")
