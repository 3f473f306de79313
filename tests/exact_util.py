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
