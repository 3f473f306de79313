"""Functional ops of the training engine.

GPU tensors run the hand-written gfx950 kernels of ``distriflow_amd._C`` (no fallback: a missing
extension raises); CPU tensors run the fp32 reference in :mod:`.reference` (CPU plumbing config
and numerics oracle).  All ops write into caller-provided output buffers so that the engine can
preallocate everything once and capture the whole training step into a hipGraph.

Weight arguments:
  * ``w``  — compute weights [Npad][Kpad] (GPU: zero-padded bf16 copy; CPU: fp32 master view [N][K])
  * ``wt`` — dgrad weights [Cin_pad][pad(KH*KW*N)] (GPU only; the CPU path derives it from ``w``)
"""
from __future__ import annotations

import torch

from .. import native
from ..diagnostics import on as _diag_on
from . import reference as ref
from .geometry import (MODE_DGRAD, MODE_DIRECT, MODE_FWD, ConvGeom, ConvPoolGeom, DeconvGeom,  # noqa: F401
                       DenseGeom, DwGeom, PoolGeom, UpGeom, out_hw, window)
from .geometry import pair as _pair


class _DebugSync:
    """``DISTRIFLOW_DEBUG_SYNC=1``: every kernel entry point is followed by a device
    synchronize outside graph capture, so an asynchronous fault or a race between streams is reported
    at the op that caused it (combine with ``AMD_SERIALIZE_KERNEL=3`` set before the first HIP call)."""

    def __init__(self, mod):
        self._mod = mod

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not callable(fn) or isinstance(fn, type):
            return fn

        def wrapped(*args, **kw):
            out = fn(*args, **kw)
            if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
                try:
                    torch.cuda.synchronize()
                except RuntimeError as e:
                    raise RuntimeError(f"distriflow_amd kernel '{name}' failed: {e}") from e
            return out

        return wrapped


_DEBUG = None


def _C():
    global _DEBUG
    mod = native.require()
    if _DEBUG is None:
        import os

        _DEBUG = os.environ.get("DISTRIFLOW_DEBUG_SYNC", "0") == "1"
    return _DebugSync(mod) if _DEBUG else mod


def graph_upload(g) -> bool:
    """hipGraphUpload of a captured ``torch.cuda.CUDAGraph`` on the current stream: the graph's launch
    resources are staged on the device at capture time, so its first replay (often the first one inside a
    timed region) costs what every later one does.  An optimisation only: a graph the runtime will not
    upload (returns False) is replayed as it is."""
    try:
        _C().graph_upload(int(g.raw_cuda_graph_exec()))
        return True
    except (RuntimeError, AttributeError):
        return False


def _geom(SH=1, SW=1, SC=1, OH=1, OW=1, KH=1, KW=1, stride=1, pad=0):
    """Native conv geometry list (:meth:`ConvGeom.geom`) of a source [SH][SW][SC] and an output OH x OW."""
    return ConvGeom.of(0, SH, SW, SC, OH, OW, 0, KH, KW, stride, pad).geom()


def conv_out_hw(H, W, KH, KW, stride, pad):
    """Output size of a conv with symmetric padding ``pad`` = p or (ph, pw) and ``stride`` = s or (sh, sw)."""
    return out_hw(H, W, (KH, KW), stride, pad)


def same_padding(H, W, KH, KW, stride):
    """Keras / TF 'same' (:func:`geometry.window`).  Returns ((OH, OW), (top, left))."""
    OH, OW, pt, pl = window(H, W, (KH, KW), stride, "same")
    return (OH, OW), (pt, pl)


def _conv_geom(xs, ys, KH, KW, stride, pad) -> ConvGeom:
    """The conv from shape ``xs`` = [B][H][W][C] to ``ys`` = [B][OH][OW][N]."""
    return ConvGeom.of(*xs, *ys[1:], KH, KW, stride, pad)


# ----------------------------------------------------------------------------------- dense
def _drop_kw(drop) -> dict:
    """Keyword arguments of a folded dropout ``(p, seed, step[, step_add])`` for the native launchers."""
    if drop is None:
        return {}
    return {"drop_p": float(drop[0]), "drop_seed": int(drop[1]), "drop_step": drop[2],
            "drop_step_add": int(drop[3]) if len(drop) > 3 else 0}


def dense_fwd(x, w, bias, out, relu=False, drop=None):
    """out[B][N] = act(x[B][K] @ W^T + b); out may be bf16 or fp32 (logits).  ``drop = (p, seed, step)``:
    a Dropout that follows, folded into the epilogue (the mask of :func:`dropout` on ``out``)."""
    if x.is_cuda:
        g = DenseGeom(x.shape[0], x.shape[-1], out.shape[-1])
        _C().igemm_fwd(x, w, bias, None, out, *g.fwd(w.shape[1]), relu, 1.0, **_drop_kw(drop))
    else:
        out.copy_(ref.dense_fwd(x, w, bias, relu))
        if drop is not None:
            dropout(out, out, drop[0], drop[1], step=drop[2], step_add=drop[3] if len(drop) > 3 else 0)
    return out


def dense_dgrad(dy, w, wt, out, mask=None, alpha=1.0):
    """out[B][K] = alpha * (dy[B][N] @ W) * relu'(mask)."""
    g = DenseGeom(dy.shape[0], out.shape[-1], dy.shape[-1])
    if dy.is_cuda:
        _C().igemm_fwd(dy, wt, None, mask, out, *g.dgrad(wt.shape[1]), False, float(alpha))
    else:
        out.copy_(ref.dense_dgrad(dy, w, g.K, mask) * alpha)
    return out


def dense_wgrad(dy, x, gw, gb, workspace=None, scale=1.0):
    """gw[N][K] = dy^T x * scale ; gb[N] = sum_b dy * scale."""
    if dy.is_cuda:
        _C().igemm_wgrad(dy, x, gw, gb, workspace, *DenseGeom(dy.shape[0], x.shape[-1], dy.shape[-1]).wgrad(), scale)
    else:
        g, b = ref.dense_wgrad(dy, x, gb is not None)
        gw.copy_(g.reshape(gw.shape) * scale)
        if gb is not None:
            gb.copy_(b * scale)


# ----------------------------------------------------------------------------------- conv2d
def _bacc_kwargs(bacc):
    """igemm launch arguments of epilogue-accumulated BatchNorm sums (kernels.h BnAcc, csrc/bn_acc.h):
    ``bacc`` = dict(acc=[nrep][2][N] float64, mode=0) or dict(acc, mode=1, x, mean, invstd[, acc2, x2, mean2,
    invstd2]) -- mode 1 with the BatchNorm input(s) at the output's positions."""
    if bacc is None:
        return {}
    kw = dict(bacc=bacc["acc"], bacc_mode=int(bacc.get("mode", 0)))
    if kw["bacc_mode"] == 1:
        kw["bacc_in"] = [bacc["x"], bacc["mean"], bacc["invstd"]]
        if bacc.get("acc2") is not None:
            kw.update(bacc2=bacc["acc2"], bacc2_in=[bacc["x2"], bacc["mean2"], bacc["invstd2"]])
    return kw


def conv_plan(B, H, W, C, OH, OW, N, KH, KW, stride, pad, Kpad, dgrad=False, **flags) -> dict:
    """The launch plan (csrc/conv_plan.hip: kernel family, variant, grid, scratch) of the conv
    forward, or of the data gradient with output [B][H][W][C]; {} without the native extension."""
    g = ConvGeom.of(B, H, W, C, OH, OW, N, KH, KW, stride, pad)
    return _view_plan(g.dgrad(Kpad) if dgrad else g.fwd(Kpad), **flags)


def _view_plan(view, **flags) -> dict:
    """csrc/conv_plan.hip's plan of the ``igemm_fwd`` launch that takes ``view`` (a geometry.GemmView)."""
    m = native.get(build_if_missing=False)
    return m.conv_plan(*view.plan, **flags) if m is not None else {}


def conv_bacc_ok(B, H, W, C, OH, OW, N, KH, KW, stride, pad, Kpad, dgrad=False, mode=0, two=False,
                 has_res=False, has_mask=False) -> bool:
    """Can the conv launch (forward, or the data gradient with output [B][H][W][C]) accumulate BatchNorm
    sums of its output in its epilogue?"""
    p = conv_plan(B, H, W, C, OH, OW, N, KH, KW, stride, pad, Kpad, dgrad, bacc_mode=int(mode), two=bool(two),
                  has_res=bool(has_res), has_mask=bool(has_mask))
    return bool(p.get("bacc_ok", False))


def conv_fwd(x, w, bias, out, KH=None, KW=None, stride=1, pad=0, relu=False, bacc=None, g=None):
    """NHWC conv: out[B][OH][OW][N]; w = [Npad][Kpad] with K = KH*KW*C.  ``g``: the layer's ConvGeom, in place
    of KH / KW / stride / pad.
    ``bacc``: the consuming BatchNorm's sums are accumulated by the epilogue (:func:`_bacc_kwargs`)."""
    g = g or _conv_geom(x.shape, out.shape, KH, KW, stride, pad)
    if x.is_cuda:
        _C().igemm_fwd(x, w, bias, None, out, *g.fwd(w.shape[1]), relu, 1.0, **_bacc_kwargs(bacc))
    else:
        out.copy_(ref.conv_fwd(x, w, bias, g.KH, g.KW, g.stride, g.pad, relu, out_hw=(g.OH, g.OW)))
    return out


def conv_pool_supported(H, W, C, KH, KW, stride, pad, N, Kpad=None) -> bool:
    """Conv + 2x2 max-pool in the igemm64 epilogue (pooled map + argmax codes only).  ``Kpad``: the row length
    of the weight copy the launch will read (default: the plain layout's, K rounded up to 32)."""
    if stride != 1 or N % 8:
        return False
    g = ConvGeom.of(1, H, W, C, *conv_out_hw(H, W, KH, KW, stride, pad), N, KH, KW, stride, pad)
    Kpad = -(-g.KH * g.KW * g.C // 32) * 32 if Kpad is None else Kpad
    return bool(_view_plan(g.fwd(Kpad), pooled=True).get("pool", False))


def conv_pool_fwd(x, w, bias, out, code, KH=None, KW=None, stride=1, pad=0, relu=True, drop=None, g=None):
    """conv(+bias, ReLU) then 2x2 max-pool [then a folded dropout]: ``out`` = pooled [B][OH/2][OW/2][N],
    ``code`` = argmax position 0..3 per pooled element (4 = no gradient)."""
    B, PH, PW, N = out.shape
    g = g or _conv_geom(x.shape, (B, 2 * PH, 2 * PW, N), KH, KW, stride, pad)
    if x.is_cuda:
        _C().igemm_fwd(x, w, bias, None, out, *g.fwd(w.shape[1]), relu, 1.0, pool_code=code, **_drop_kw(drop))
    else:
        y = ref.conv_fwd(x, w, bias, g.KH, g.KW, g.stride, g.pad, relu).to(out.dtype).float()
        win = y.reshape(B, PH, 2, PW, 2, N).permute(0, 1, 3, 5, 2, 4).reshape(B, PH, PW, N, 4)
        mx, am = win.max(dim=-1)  # first max
        if relu:
            am = torch.where(mx > 0, am, torch.full_like(am, 4))
        out.copy_(mx)
        code.copy_(am.to(torch.uint8))
        if drop is not None:
            dropout(out, out, drop[0], drop[1], step=drop[2], step_add=drop[3] if len(drop) > 3 else 0)
    return out


def unpool2(dyp, code, dy):
    """dy [B][OH][OW][N]: each pooled gradient at the window position its code names."""
    if dy.is_cuda:
        _C().unpool2(dyp.contiguous(), code, dy)
    else:
        B, OH, OW, N = dy.shape
        g = dyp.float().reshape(B, OH // 2, OW // 2, N, 1)
        sel = (code.long().reshape(B, OH // 2, OW // 2, N, 1) == torch.arange(4).reshape(1, 1, 1, 1, 4)).float()
        full = (g * sel).reshape(B, OH // 2, OW // 2, N, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, OH, OW, N)
        dy.copy_(full)
    return dy


def kcnn_supported() -> bool:
    m = native.get(build_if_missing=False)
    return m is not None and hasattr(m, "kcnn_fwd")


def _kc_in(x):
    if isinstance(x, GatherRef):
        return x.data, x.idx, x.scale
    return x, None, 1.0


def kcnn_fwd(x, w1, b1, w2, b2, out, code, drop=None):
    """The reference CNN's conv block forward on GPU (csrc/kcnn_fused.hip): conv1 + ReLU, conv2 + ReLU,
    2x2 max-pool [+ folded dropout] -> pooled ``out`` [B][12][12][32] and argmax ``code``.  ``x``: a
    :class:`GatherRef` (uint8 dataset rows, read in-kernel) or a bf16 batch [B][28][28][1]."""
    src, idx, scale = _kc_in(x)
    dkw = _drop_kw(drop)
    _C().kcnn_fwd(src, idx, float(scale), int(out.shape[0]), w1, b1, int(w1.shape[1]), w2, b2, out, code, **dkw)
    return out


def kcnn_slab_floats(B: int) -> int:
    return int(_C().kcnn_slab_floats(int(B)))


def kcnn_bwd(x, w1, b1, w2t, dyp, code, slabs, g_w1, g_b1, g_w2, g_b2, step_inc=None):
    """Both conv weight gradients of the block from the pooled gradient ``dyp`` (one backward launch +
    one deterministic slab reduction, which also advances ``step_inc``)."""
    src, idx, scale = _kc_in(x)
    _C().kcnn_bwd(src, idx, float(scale), int(dyp.shape[0]), w1, b1, int(w1.shape[1]), w2t, dyp.contiguous(), code,
                  slabs, g_w1, g_b1, g_w2, g_b2, step_inc=step_inc)


def conv_dgrad(dy, w, wt, out, KH=None, KW=None, stride=1, pad=0, mask=None, residual=None, residual_mask=None,
               bacc=None, g=None):
    """dX (NHWC [B][H][W][C]) of a conv whose output gradient is dy [B][OH][OW][N].

    Epilogue (ResNet block join): dX = (conv^T dy + residual * [residual_mask > 0]) * [mask > 0].
    ``bacc`` (mode 1): dX is the output gradient of a BatchNorm; its backward sums are accumulated by
    the epilogue (:func:`_bacc_kwargs`)."""
    g = g or _conv_geom(out.shape, dy.shape, KH, KW, stride, pad)
    if dy.is_cuda:
        _C().igemm_fwd(dy, wt, None, mask, out, *g.dgrad(wt.shape[1]), False, 1.0, residual, residual_mask,
                       **_bacc_kwargs(bacc))
    else:
        dx = ref.conv_dgrad(dy, w, out.shape, g.KH, g.KW, g.stride, g.pad, None)
        if residual is not None:
            r = residual.float().reshape(dx.shape)
            if residual_mask is not None:
                r = r * (residual_mask.float().reshape(dx.shape) > 0)
            dx = dx + r
        if mask is not None:
            dx = dx * (mask.float().reshape(dx.shape) > 0)
        out.copy_(dx)
    return out


def wgrad_plan(B, H, W, C, OH, OW, N, KH, KW, stride, pad, with_bias, ws_floats) -> dict:
    """The launch plan (csrc/conv_plan.hip wgrad_plan: kernel family, tile, splits, grid, the floats it writes
    into a workspace of ``ws_floats``) of :func:`conv_wgrad`; {} without the native extension.  A workspace
    smaller than ``wanted_floats`` gives fewer splits (``capped``): another summation order."""
    return _view_wgrad_plan(ConvGeom.of(B, H, W, C, OH, OW, N, KH, KW, stride, pad).wgrad(), with_bias, ws_floats)


def _view_wgrad_plan(view, with_bias, ws_floats) -> dict:
    """csrc/conv_plan.hip's plan of the ``igemm_wgrad`` launch that takes ``view`` (a geometry.WgradView)."""
    m = native.get(build_if_missing=False)
    return m.wgrad_plan(*view, bool(with_bias), int(ws_floats)) if m is not None else {}


def dense_wgrad_plan(B, K, N, with_bias, ws_floats) -> dict:
    """:func:`wgrad_plan` of :func:`dense_wgrad` (x [B][K], dy [B][N])."""
    return _view_wgrad_plan(DenseGeom(B, K, N).wgrad(), with_bias, ws_floats)


def conv_wgrad(dy, x, gw, gb, workspace, KH=None, KW=None, stride=1, pad=0, scale=1.0, g=None):
    g = g or _conv_geom(x.shape, dy.shape, KH, KW, stride, pad)
    if dy.is_cuda:
        _C().igemm_wgrad(dy, x, gw, gb, workspace, *g.wgrad(), scale)
    else:
        g, b = ref.conv_wgrad(dy, x, g.KH, g.KW, g.stride, g.pad, gb is not None)
        gw.copy_(g.reshape(gw.shape) * scale)
        if gb is not None:
            gb.copy_(b * scale)


# ----------------------------------------------------------------------------------- pooling etc.
def maxpool_fwd(x, out, P, drop=None):
    """``drop = (p, seed, step)``: a Dropout that follows, folded in (same mask as :func:`dropout`)."""
    B, H, W, C = x.shape
    if x.is_cuda:
        dkw = _drop_kw(drop)
        _C().maxpool_fwd(x, out, B, H, W, C, P, **dkw)
    else:
        out.copy_(ref.maxpool_fwd(x, P))
        if drop is not None:
            dropout(out, out, drop[0], drop[1], step=drop[2], step_add=drop[3] if len(drop) > 3 else 0)
    return out


def maxpool_bwd(x, dy, dx, P, relu_fused=False):
    B, H, W, C = x.shape
    if x.is_cuda:
        _C().maxpool_bwd(x, dy, dx, B, H, W, C, P, relu_fused)
    else:
        dx.copy_(ref.maxpool_bwd(x, dy, P, relu_fused))
    return dx


def softmax_ce(logits, labels, dlogits=None, stats=None, grad_scale=1.0):
    """Fused softmax-cross-entropy: dlogits = (softmax - onehot) * grad_scale; stats += [loss_sum, #correct]."""
    B, C = logits.shape
    if logits.is_cuda:
        ldg = dlogits.shape[-1] if dlogits is not None else C
        _C().softmax_ce(logits, labels, dlogits, stats, B, C, C, ldg, grad_scale)
    else:
        loss, corr, dl = ref.softmax_ce(logits, labels, grad_scale)
        if dlogits is not None:
            dlogits.copy_(dl)
        if stats is not None:
            stats[0] += loss
            stats[1] += corr


def dropout(x, out, p, seed, mask=None, step=None, step_add=0):
    """out = x * keep(seed ^ step, i) / (1 - p) [* relu'(mask)]; ``step`` is a device int64 scalar."""
    if x.is_cuda:
        if step_add:
            raise ValueError("step_add is for folded dropouts only")
        _C().dropout(x, out, p, seed, mask, step)
    else:
        s = seed ^ ((int(step.item()) + step_add) * 0x9E3779B1 if step is not None else 0)
        out.copy_(ref.dropout(x, p, s, mask).reshape(out.shape))
    return out


def gather_batch(data, labels, idx, out, out_labels, scale=1.0, step_inc=None):
    """out[b] = data[idx[b]] (uint8 -> bf16 * scale on the fly); out_labels[b] = labels[idx[b]].
    ``step_inc``: a device int64 counter the launch advances by one (the engine's dropout step)."""
    B = idx.shape[0]
    row = out[0].numel()
    if out.is_cuda:
        _C().gather_batch(data, labels, idx, out, out_labels, B, row, scale, step_inc=step_inc)
    else:
        if step_inc is not None:
            step_inc.add_(1)
        out.copy_((data.index_select(0, idx).float() * scale).reshape(out.shape))
        if labels is not None:
            out_labels.copy_(labels.index_select(0, idx))
    return out


def add_act(a, b, out, relu=False):
    if a.is_cuda:
        _C().add_act(a, b, out, relu)
    else:
        r = a.float() + b.float()
        out.copy_(torch.relu(r) if relu else r)
    return out


# ---- Keras merge layers of branching graphs (csrc/merge.hip); codes match kernels.h kMerge*
MERGE_KINDS = {"Add": 0, "Subtract": 1, "Multiply": 2, "Average": 3, "Maximum": 4, "Minimum": 5, "Concatenate": 6}


def _merge_ref(kind: int, xs):
    xs = [x.float() for x in xs]
    if kind == 6:
        return torch.cat(xs, dim=-1)
    out = xs[0].clone()
    for x in xs[1:]:
        if kind in (0, 3):
            out = out + x
        elif kind == 1:
            out = out - x
        elif kind == 2:
            out = out * x
        elif kind == 4:
            out = torch.maximum(out, x)
        else:
            out = torch.minimum(out, x)
    return out / len(xs) if kind == 3 else out


def merge_fwd(inputs, out, kind: str):
    """out = merge(inputs) over the last axis layout [..., C] (one launch on GPU)."""
    k = MERGE_KINDS[kind]
    if out.is_cuda:
        _C().merge_fwd([x.contiguous() for x in inputs], out, k)
    else:
        out.copy_(_merge_ref(k, inputs).to(out.dtype))
    return out


def merge_bwd(inputs, dy, grads, kind: str):
    """grads[i] = d merge / d inputs[i] * dy (Maximum / Minimum: to the first input holding the extreme)."""
    k = MERGE_KINDS[kind]
    if dy.is_cuda:
        _C().merge_bwd([x.contiguous() for x in inputs], dy.contiguous(), list(grads), k)
        return grads
    if k == 6:
        off = 0
        for x, g in zip(inputs, grads):
            w = x.shape[-1]
            g.copy_(dy[..., off:off + w])
            off += w
        return grads
    if k in (4, 5):  # first extreme wins, as the kernel
        xs = [x.float() for x in inputs]
        ext = _merge_ref(k, inputs)
        taken = torch.zeros_like(ext, dtype=torch.bool)
        for x, g in zip(xs, grads):
            hit = (x == ext) & ~taken
            taken |= hit
            g.copy_(torch.where(hit, dy.float(), torch.zeros_like(ext)).to(g.dtype))
        return grads
    xs = [x.float().detach().requires_grad_(True) for x in inputs]
    y = _merge_ref(k, xs)
    gs = torch.autograd.grad(y, xs, dy.float())
    for g, v in zip(grads, gs):
        g.copy_(v.to(g.dtype))
    return grads


# ---- generic Keras layers (csrc/act.hip); codes match kernels.h ActKind
ACT_KINDS = {"linear": 0, None: 0, "relu": 1, "relu6": 2, "sigmoid": 3, "tanh": 4, "elu": 5, "selu": 6,
             "softplus": 7, "softsign": 8, "hard_sigmoid": 9, "hardSigmoid": 9, "swish": 10, "silu": 10,
             "exponential": 11}


def _act_ref(kind: int, x):
    import torch.nn.functional as F

    def clip(v, lo, hi):  # TensorFlow's gradient of a clipped activation: zero AT the corners too
        return torch.where((v > lo) & (v < hi), v, v.clamp(lo, hi).detach())

    f = {0: lambda v: v, 1: F.relu, 2: lambda v: clip(v, 0.0, 6.0), 3: torch.sigmoid, 4: torch.tanh, 5: F.elu,
         6: F.selu, 7: F.softplus, 8: F.softsign, 9: lambda v: clip(0.2 * v + 0.5, 0.0, 1.0), 10: F.silu,
         11: torch.exp}[kind]
    return f(x)


def act_fwd(x, out, activation):
    """out = act(x) for the Keras activations in ACT_KINDS (one streaming launch on GPU)."""
    kind = ACT_KINDS[activation]
    if x.is_cuda:
        _C().act_fwd(x.contiguous(), out, kind)
    else:
        out.copy_(_act_ref(kind, x.float()).to(out.dtype))
    return out


def act_bwd(x, dy, dx, activation, in_relu=False):
    """dx = dy * act'(x) [* relu'(x) when x is itself a fused-ReLU output]."""
    kind = ACT_KINDS[activation]
    if x.is_cuda:
        _C().act_bwd(x.contiguous(), dy.contiguous(), dx, kind, bool(in_relu))
    else:
        xv = x.float().detach().requires_grad_(True)
        y = _act_ref(kind, xv)
        (g,) = torch.autograd.grad(y, xv, dy.float())
        if in_relu:
            g = g * (x.float() > 0)
        dx.copy_(g.to(dx.dtype))
    return dx


def sigmoid_ce(logits, labels, dlogits=None, stats=None, grad_scale=1.0):
    """Sigmoid cross-entropy on logits vs one-hot(labels), summed over classes: dlogits = (sigmoid(z) -
    onehot) * grad_scale; stats += [loss_sum, #correct (argmax)]."""
    B, C = logits.shape
    if logits.is_cuda:
        ldg = dlogits.shape[-1] if dlogits is not None else C
        _C().sigmoid_ce(logits, labels.to(torch.int32), dlogits, stats, B, C, C, ldg, grad_scale)
    else:
        z = logits.float()
        t = torch.nn.functional.one_hot(labels.long().clamp(0, C - 1), C).float()
        loss = (z.clamp_min(0) - z * t + torch.log1p(torch.exp(-z.abs()))).sum()
        if dlogits is not None:
            dlogits.copy_(((torch.sigmoid(z) - t) * grad_scale).to(dlogits.dtype))
        if stats is not None:
            stats[0] += loss
            stats[1] += (z.argmax(1) == labels.long()).float().sum()
    return stats


pool_geometry = PoolGeom.build  # (B, H, W, C, pool, strides, padding) of a Keras/TF pooling layer ('valid' | 'same')


def _pool_ref(x, g, avg):
    F, g = torch.nn.functional, PoolGeom(*g)
    xf = x.float().permute(0, 3, 1, 2)
    pads, win = (g.pl, max(g.pr, 0), g.pt, max(g.pb, 0)), ((g.ph, g.pw), (g.sh, g.sw))
    if avg:
        ones = torch.ones(1, 1, g.H, g.W, dtype=xf.dtype, device=xf.device)
        num = F.avg_pool2d(F.pad(xf, pads), *win, divisor_override=1)
        cnt = F.avg_pool2d(F.pad(ones, pads), *win, divisor_override=1)
        y = num / cnt.clamp_min(1.0)
    else:
        y = F.max_pool2d(F.pad(xf, pads, value=float("-inf")), *win)
    return y[:, :, :g.OH, :g.OW].permute(0, 2, 3, 1)


def pool2d_fwd(x, out, geom, avg=False):
    """General 2-D pooling (max / average; any window, stride and 'valid' / 'same' padding), NHWC."""
    if x.is_cuda:
        _C().pool2d_fwd(x.contiguous(), out, [int(v) for v in geom], bool(avg))
    else:
        out.copy_(_pool_ref(x, geom, avg).reshape(out.shape).to(out.dtype))
    return out


def pool2d_bwd(x, dy, dx, geom, avg=False, in_relu=False):
    if x.is_cuda:
        _C().pool2d_bwd(x.contiguous(), dy.contiguous(), dx, [int(v) for v in geom], bool(avg), bool(in_relu))
    else:
        xv = x.float().detach().requires_grad_(True)
        y = _pool_ref(xv, geom, avg)
        (g,) = torch.autograd.grad(y, xv, dy.float().reshape(y.shape))
        if in_relu:
            g = g * (x.float() > 0)
        dx.copy_(g.reshape(dx.shape).to(dx.dtype))
    return dx


# ---- depthwise convolution (csrc/dwconv.hip): fp32 kernel [KH][KW][C*M], output channel co reads input co // M
dwconv_geometry = DwGeom.build  # (B, H, W, C, M, kernel, strides, padding) of a Keras DepthwiseConv2D


def dwconv_fwd(x, w, bias, out, geom, relu=False):
    """out = [relu](bias + depthwise conv of NHWC ``x`` with ``w`` [KH][KW][C*M] fp32)."""
    if x.is_cuda:
        _C().dwconv_fwd(x.contiguous(), w, bias, out, [int(v) for v in geom], bool(relu))
    else:
        out.copy_(ref.dwconv_fwd(x, w, bias, geom, relu).reshape(out.shape).to(out.dtype))
    return out


def dwconv_dgrad(dy, w, dx, geom, mask=None):
    """dx = (transposed depthwise conv of dy) * relu'(mask)."""
    if dy.is_cuda:
        _C().dwconv_dgrad(dy.contiguous(), w, mask, dx, [int(v) for v in geom])
    else:
        dx.copy_(ref.dwconv_dgrad(dy, w, geom, mask).reshape(dx.shape).to(dx.dtype))
    return dx


def dwconv_wgrad(dy, x, gw, gb, workspace, geom):
    """gw [KH][KW][C*M] = sum over (b, oh, ow) of dy * x; gb [C*M] = sum dy (None: no bias).  fp32, the same
    bits for the same inputs (``workspace``: fp32 slab scratch, GPU only)."""
    if dy.is_cuda:
        _C().dwconv_wgrad(dy.contiguous(), x.contiguous(), gw, gb, workspace, [int(v) for v in geom])
    else:
        w, b = ref.dwconv_wgrad(dy, x, geom, gb is not None)
        gw.copy_(w.reshape(gw.shape))
        if gb is not None:
            gb.copy_(b)
    return gw


# ---- transposed convolution: the data gradient of a conv G with the same kernel size, strides and padding;
# kernel = G's OHWI matrix [Cin][KH*KW*F].  The conv kernels run it with their roles swapped (ConvGeom.t_fwd).
def deconv_geometry(B, H, W, Cin, F, kernel, strides, padding):
    """The DeconvGeom [B, H, W, Cin, F, OH, OW, KH, KW, sh, sw, pt, pl] of a Keras Conv2DTranspose."""
    return ConvGeom.transposed(B, H, W, Cin, F, kernel, strides, padding).t_geom


def deconv_plans(geom, w, wt, has_bias=False, has_mask=False, ws_floats=0) -> dict:
    """The kernel families (csrc/conv_plan.hip) the three launches of a transposed conv take: ``fwd`` (a
    MODE_DGRAD launch), ``dgrad`` (a MODE_FWD launch) and ``wgrad``; {} without the native extension.  A bias
    changes the forward's plan (the halo kernel refuses one)."""
    if native.get(build_if_missing=False) is None:
        return {}
    G = DeconvGeom(*geom).G
    return {"fwd": _view_plan(G.t_fwd(int(wt.shape[1])), has_bias=bool(has_bias)),
            "dgrad": _view_plan(G.t_dgrad(int(w.shape[1])), has_mask=bool(has_mask)),
            "wgrad": _view_wgrad_plan(G.t_wgrad(), False, ws_floats)}


def deconv_fwd(x, w, wt, bias, out, geom, relu=False):
    """out [B][OH][OW][F] = [relu](transposed conv of NHWC ``x`` + bias).  ``w``: the kernel [Cin][KH*KW*F]
    (CPU) ; ``wt``: its dgrad-layout bf16 copy [Fpad][pad(KH*KW*Cin)] (GPU)."""
    G = DeconvGeom(*geom).G
    if x.is_cuda:
        _C().igemm_fwd(x, wt, bias, None, out, *G.t_fwd(wt.shape[1]), bool(relu), 1.0)
    else:
        y = ref.conv_dgrad(x.reshape(G.y_shape), w, G.x_shape, G.KH, G.KW, G.stride, G.pad)
        if bias is not None:
            y = y + bias.float()
        if relu:
            y = torch.relu(y)
        out.copy_(y.reshape(out.shape))
    return out


def deconv_dgrad(dy, w, dx, geom, mask=None):
    """dx [B][H][W][Cin] = G(dy) * relu'(mask): the forward of the conv G on the output gradient."""
    G = DeconvGeom(*geom).G
    if dy.is_cuda:
        _C().igemm_fwd(dy, w, None, mask, dx, *G.t_dgrad(w.shape[1]), False, 1.0)
    else:
        g = ref.conv_fwd(dy.reshape(G.x_shape), w, None, G.KH, G.KW, G.stride, G.pad, False, out_hw=(G.OH, G.OW))
        if mask is not None:
            g = g * (mask.float().reshape(g.shape) > 0)
        dx.copy_(g.reshape(dx.shape))
    return dx


def channel_sum(dy, gb, workspace, scale=1.0):
    """gb [C] = scale * sum over every leading position of dy [..][C], fp32, the same bits for the same inputs
    (``workspace``: fp32 slab scratch of at least C floats, GPU only)."""
    C = dy.shape[-1]
    if dy.is_cuda:
        _C().channel_sum(dy.contiguous(), gb, workspace, dy.numel() // C, C, float(scale))
    else:
        gb.copy_(dy.float().reshape(-1, C).sum(0) * scale)
    return gb


def deconv_wgrad(dy, x, gw, gb, workspace, geom):
    """gw [Cin][KH*KW*F]: G's kernel gradient with x in the output-gradient slot and dy in the input slot (no
    bias column: it would sum x); gb [F] = sum over positions of dy (None: no bias)."""
    G = DeconvGeom(*geom).G
    conv_wgrad(x.reshape(G.y_shape), dy.reshape(G.x_shape), gw, None, workspace, g=G)
    if gb is not None:
        channel_sum(dy.reshape(-1, G.C), gb, workspace)
    return gw


# ---- up-sampling (csrc/upsample.hip)
UPSAMPLE_KINDS = ("nearest", "bilinear")


def upsample2d_fwd(x, out, size, interpolation="nearest", half_pixel_centers=True):
    """out [B][H*sh][W*sw][C]: every pixel repeated ('nearest'), or 'bilinear' sampling at
    src = (dst + o) / s - o with o = 0.5 (``half_pixel_centers``, Keras / TF2) or 0 (tf.js)."""
    g = UpGeom(*x.shape, *_pair(size))
    bil = UPSAMPLE_KINDS.index(interpolation) == 1
    if x.is_cuda:
        _C().upsample2d_fwd(x.contiguous(), out, list(g), bil, bool(half_pixel_centers))
    else:
        out.copy_(ref.upsample2d_fwd(x, (g.sh, g.sw), bil, half_pixel_centers).reshape(out.shape))
    return out


def upsample2d_bwd(dy, dx, size, interpolation="nearest", half_pixel_centers=True, mask=None):
    """dx [B][H][W][C] = (sum of the dy pixels that read the pixel, weighted) * relu'(mask)."""
    g = UpGeom(*dx.shape, *_pair(size))
    bil = UPSAMPLE_KINDS.index(interpolation) == 1
    if dy.is_cuda:
        _C().upsample2d_bwd(dy.contiguous(), mask, dx, list(g), bil, bool(half_pixel_centers))
    else:
        dx.copy_(ref.upsample2d_bwd(dy.reshape(g.B, g.H * g.sh, g.W * g.sw, g.C), (g.sh, g.sw), bil,
                                    half_pixel_centers, mask))
    return dx


def relu_bwd(y, dy, dx):
    if y.is_cuda:
        _C().relu_bwd(y, dy, dx)
    else:
        dx.copy_((dy.float().reshape(y.shape) * (y.float() > 0)).reshape(dx.shape))
    return dx


def gap_fwd(x, out):
    B, H, W, C = x.shape
    if x.is_cuda:
        _C().gap_fwd(x, out, B, H * W, C)
    else:
        out.copy_(x.float().mean(dim=(1, 2)))
    return out


def gap_bwd(dy, dx):
    B, H, W, C = dx.shape
    if dy.is_cuda:
        _C().gap_bwd(dy, dx, B, H * W, C)
    else:
        dx.copy_((dy.float() / (H * W)).view(B, 1, 1, C).expand(B, H, W, C))
    return dx


BN_COUNTERS = 64  # ticket counters of one BN statistics launch: 1 global + 1 per group of 16 (<= 1008) workgroups


def bn_workspace_floats(C: int) -> int:
    """fp32 workspace of a BN statistics launch of any M: <= 1024 partial slabs + <= 64 group slabs of [2][C]."""
    return (1024 + 64) * 2 * C


def bn_stats_fwd(x2d, mean, invstd, run_mean, run_var, ws, counter, momentum=0.1, eps=1e-5):
    """Training batch statistics of x2d [M][C] -> mean, invstd; running statistics updated in place.
    GPU: one launch (csrc/bn.hip; ``counter`` = int32 last-arriver ticket, zero between launches)."""
    M, C = x2d.shape
    if x2d.is_cuda:
        _C().bn_stats_fwd(x2d, mean, invstd, run_mean, run_var, ws, counter, M, C, momentum, eps)
    else:
        mu = x2d.float().mean(0)
        var = x2d.float().var(0, unbiased=False)
        mean.copy_(mu)
        invstd.copy_(torch.rsqrt(var + eps))
        if run_mean is not None:
            unb = var * M / max(M - 1, 1)
            run_mean.mul_(1 - momentum).add_(mu * momentum)
            run_var.mul_(1 - momentum).add_(unb * momentum)


def bn_apply(x2d, y2d, gamma, beta, mean, invstd, relu=False, residual=None, residual_bn=None, eval_mode=False,
             eps=1e-5):
    """y = act(bn(x) [+ r | + bn_r(r)]): ``residual_bn`` = (gamma, beta, mean, invstd) of the residual's BN
    (ResNet projection shortcut).  ``eval_mode``: mean / invstd are the running mean / variance."""
    M, C = x2d.shape
    if x2d.is_cuda:
        rg = rb = rm = ri = None
        if residual_bn is not None:
            rg, rb, rm, ri = residual_bn
        _C().bn_apply(x2d, y2d, gamma, beta, mean, invstd, residual, rg, rb, rm, ri, M, C, relu, eval_mode, eps)
    else:
        def aff(x, g, b, m, v):
            inv = torch.rsqrt(v + eps) if eval_mode else v
            return (x.float() - m) * inv * g + b

        y = aff(x2d, gamma, beta, mean, invstd)
        if residual is not None:
            r = residual.reshape(M, C)
            y = y + (aff(r, *residual_bn) if residual_bn is not None else r.float())
        y2d.copy_(torch.relu(y) if relu else y)
    return y2d


def bn_apply_acc(x2d, y2d, gamma, beta, acc, zero, mean, invstd, run_mean, run_var, relu=False, residual=None,
                 rbn=None, momentum=0.1, eps=1e-5):
    """Training y = act(bn(x) [+ r | + bn_r(r)]) with the batch statistics finalised from the producing
    conv's accumulated sums ``acc`` (csrc/bn.hip bn_apply_acc): writes mean / invstd / running statistics
    and clears ``zero`` (the other direction's accumulator).  ``rbn``: the residual's BatchNorm as
    [gamma, beta, acc, zero, mean, invstd, run_mean, run_var] (its statistics finalised the same way)."""
    M, C = x2d.shape
    z = zero if zero is not None else None
    rb = list(rbn) if rbn is not None else []
    if rb and rb[3] is None:
        rb[3] = torch.empty(0, dtype=torch.float64, device=x2d.device)
    _C().bn_apply_acc(x2d, y2d, gamma, beta, acc, z, mean, invstd, run_mean, run_var, residual, rb, M, C, relu,
                      momentum, eps)
    return y2d


def bn_dx_acc(x2d, g2d, dx2d, acc, zero, gamma, mean, invstd, dgamma, dbeta, coef, gscale=1.0):
    """dx = k1 g + k2 x + k3 with the coefficients finalised from the producer's backward sums ``acc``
    (csrc/bn.hip bn_dx_acc); also writes dgamma, dbeta (x gscale) and coef, and clears ``zero``."""
    M, C = x2d.shape
    _C().bn_dx_acc(x2d, g2d, dx2d, acc, zero, gamma, mean, invstd, dgamma, dbeta, coef, M, C, gscale)
    return dx2d


def gap_bwd_bn(dy, mask, dx, acc, x, mean, invstd):
    """GAP backward with relu'(mask) and the BatchNorm backward sums of dx (``x`` = that BN's input)."""
    B, H, W, C = dx.shape
    _C().gap_bwd_bn(dy.contiguous(), mask, dx, B, H * W, C, acc, [x, mean, invstd])
    return dx


def bn_dx(x2d, g2d, dx2d, coef):
    """dx = k1 g + k2 x + k3 per channel (coef [3][C] from a finalised backward statistics pass)."""
    M, C = x2d.shape
    if x2d.is_cuda:
        _C().bn_dx(x2d, None, g2d, dx2d, coef, M, C)
    else:
        dx2d.copy_(coef[:C] * g2d.float() + coef[C:2 * C] * x2d.float() + coef[2 * C:3 * C])
    return dx2d


def bn_bwd(x2d, mask2d, dy2d, dx2d, gamma, mean, invstd, dgamma, dbeta, ws, coef, counter, gscale=1.0):
    """Backward of y = bn(x): dx, dgamma, dbeta (scaled by gscale) from dy; g = dy * (mask > 0) when a
    mask (relu' source) is given.  GPU: statistics launch (which also writes the dx coefficients) + dx pass."""
    M, C = x2d.shape
    if x2d.is_cuda:
        _C().bn_stats_bwd(x2d, mask2d, dy2d, gamma, mean, invstd, dgamma, dbeta, coef, ws, counter, M, C, gscale)
        _C().bn_dx(x2d, mask2d, dy2d, dx2d, coef, M, C)
    else:
        g = dy2d.float() * (mask2d.float() > 0) if mask2d is not None else dy2d.float()
        dx, sg, sb = ref.batchnorm_bwd(x2d, g, gamma, mean, invstd)
        dx2d.copy_(dx)
        dgamma.copy_(sg * gscale)
        dbeta.copy_(sb * gscale)
    return dx2d


# ----------------------------------------------------------------------------------- fused conv+pool
class GatherRef:
    """A batch that has not been materialised: rows ``idx`` of an HBM-resident uint8 dataset, scaled.
    The first layer reads it directly (fused gather + cast); other consumers call :meth:`materialise`."""

    def __init__(self, data, idx, scale, shape):
        self.data, self.idx, self.scale = data, idx, scale
        self.shape = (idx.shape[0],) + tuple(shape)
        self.device = data.device
        self.is_cuda = data.is_cuda

    def materialise(self, out, step_inc=None):
        return gather_batch(self.data, None, self.idx, out, None, self.scale, step_inc=step_inc)


class LabelRef:
    """Labels of a batch that has not been gathered: ``labels[idx]`` (consumers that can read through
    the index vector — the fused head — never materialise it)."""

    def __init__(self, labels, idx):
        self.labels, self.idx = labels, idx
        self.shape = (idx.shape[0],)

    def materialise(self, out):
        return gather_labels(self.labels, self.idx, out)


class TargetRef:
    """Dense fp32 targets of a batch that has not been gathered: ``targets[idx]`` ([N, C] table, int64
    batch indices).  :func:`loss_grad` reads through the index vector, so no gather launch exists.

    For an image output (:func:`image_loss_grad`) the table is [N, ...] of the output's shape, fp32 or uint8;
    a uint8 table is read as ``u8 * scale`` (the HBM dataset itself as an autoencoder's target)."""

    def __init__(self, targets, idx, scale: float = 1.0):
        self.targets, self.idx, self.scale = targets, idx, float(scale)
        self.shape = (idx.shape[0],) + tuple(targets.shape[1:])


def head_supported() -> bool:
    m = native.get(build_if_missing=False)
    return m is not None and hasattr(m, "head_train")


def head_train(w, wt, b, gw, gb, hT, dzT, K, N, x, x_relu, xT, dx, logits, labels, idx, grad_scale, loss_part,
               stats, phases=3, dx_scale=1.0):
    """Fused dense head on GPU (csrc/mlphead.hip): forward + softmax-CE + backward of a Dense chain.
    phases bit 1: forward, loss, backward data chain (dx, logits, H^T/dZ^T); bit 2: weight/bias
    gradients gw/gb (batch-mean scaled via grad_scale) and stats.  Each phase is one launch on the
    current stream, so the two can be placed on different streams."""
    _C().head_train(list(w), list(wt), list(b), list(gw), list(gb), list(hT), list(dzT), list(K), list(N),
                    x.reshape(x.shape[0], -1) if x.is_contiguous() else x.contiguous().reshape(x.shape[0], -1),
                    bool(x_relu), xT, dx, logits, labels, idx, float(grad_scale), loss_part, stats, int(phases),
                    dx_scale=float(dx_scale))


def khead_supported(K: int, C: int) -> bool:
    m = native.get(build_if_missing=False)
    return m is not None and hasattr(m, "khead_train") and bool(m.khead_supported(int(K), int(C)))


def khead_ws_floats(B: int, K: int) -> int:
    return int(_C().khead_ws_floats(int(B), int(K)))


def khead_error(ws: torch.Tensor, B: int) -> int:
    """The dense-head launch's sticky error word (csrc/khead.hip): non-zero after a row tile's flag wait timed
    out (its results invalid).  ``ws``: the launch's workspace (ops.khead_ws_floats floats)."""
    off = int(_C().khead_err_offset(int(B)))  # (layout: csrc/khead.hip khead_err_offset)
    return int(ws[off:off + 1].view(torch.int32).item())


def khead_train(p, pT, dp, w1, w1t, b1, w2, w2t, b2, h1T, dz1T, dz2T, logits, labels, idx, grad_scale, loss_part, ws,
                drop=None, dh_scale=1.0, dp_scale=1.0, dp_mask=False):
    """The reference CNN's dense head on GPU (csrc/khead.hip): dense1 (K -> 128, ReLU, folded ``drop``),
    dense2 (128 -> C) and softmax-CE, forward + loss + both data gradients in ONE launch (split-K over 8
    workgroups per 32 batch rows).  Writes logits, the loss partials, dP (``dp``) and the weight-gradient
    operands P^T / H1^T / dZ1^T / dZ2^T that :func:`head_train` (phases=2) turns into gw / gb / stats."""
    dk = _drop_kw(drop)
    _C().khead_train(p.reshape(p.shape[0], -1), pT, dp, w1, w1t, b1, w2, w2t, b2, dk.get("drop_p", 0.0),
                     dk.get("drop_seed", 0), dk.get("drop_step"), dk.get("drop_step_add", 0), float(dh_scale),
                     float(dp_scale), bool(dp_mask), h1T, dz1T, dz2T, logits, labels, idx, float(grad_scale),
                     loss_part, ws)


def khead_wgrad(pT, h1T, dz1T, dz2T, gw1, gb1, gw2, gb2, B, K, C, loss_part, stats):
    """Weight / bias gradients of the :func:`khead_train` head from its transposed operands, and the
    loss partials -> stats (one launch, csrc/khead.hip)."""
    _C().khead_wgrad(pT, h1T, dz1T, dz2T, gw1, gb1, gw2, gb2, int(B), int(K), int(C), loss_part, stats)


METRIC_KINDS = {"meanSquaredError": 0, "mse": 0, "absoluteDifference": 1, "hingeLoss": 2, "huberLoss": 3,
                "logLoss": 4, "sigmoidCrossEntropy": 5, "softmaxCrossEntropy": 6, "categorical_crossentropy": 7,
                "categoricalCrossentropy": 7}


def _out_act_code(out_act) -> int:
    """0 linear, 1 softmax, 2 sigmoid, from the code itself, an activation name, or a final_softmax bool."""
    if out_act in ("linear", None):
        return 0
    if out_act in ("softmax", "sigmoid"):
        return 1 if out_act == "softmax" else 2
    if isinstance(out_act, (bool, int)) and 0 <= int(out_act) <= 2:
        return int(out_act)
    raise ValueError(f"unknown output activation {out_act!r}")


def _ld(t, C):
    """Leading dimension of a [rows][C] matrix: a contiguous tensor or a column slice of a wider buffer."""
    return int(t.stride(0)) if t.dim() == 2 and t.shape[0] > 1 and not t.is_contiguous() else int(t.shape[-1])


def _loss_terms(kind: int, p, t):
    """Per-element loss terms and dL/dp of METRIC_KINDS ``kind`` on outputs ``p`` vs targets ``t`` (the
    closed forms of csrc/loss.hip; rows sum to the per-example loss)."""
    C = p.shape[1]
    d = p - t
    if kind == 0:
        return d * d / C, 2 * d / C
    if kind == 1:
        return d.abs() / C, torch.sign(d) / C
    if kind == 2:
        s = 2 * t - 1
        m = 1 - s * p
        return m.clamp_min(0) / C, torch.where(m > 0, -s, torch.zeros_like(s)) / C
    if kind == 3:
        a = d.abs()
        return torch.where(a <= 1, 0.5 * d * d, a - 0.5) / C, torch.where(a <= 1, d, torch.sign(d)) / C
    if kind == 4:
        eps = 1e-7
        return (-(t * torch.log(p + eps) + (1 - t) * torch.log(1 - p + eps)) / C,
                (-t / (p + eps) + (1 - t) / (1 - p + eps)) / C)
    if kind == 5:
        return (p.clamp_min(0) - p * t + torch.log1p(torch.exp(-p.abs()))) / C, (torch.sigmoid(p) - t) / C
    if kind == 6:
        return -t * torch.log_softmax(p, dim=1), torch.softmax(p, dim=1) * t.sum(1, keepdim=True) - t
    eps = 1e-7
    inside = (p >= eps) & (p <= 1)
    return -t * torch.log(p.clamp(eps, 1.0)), torch.where(inside, -t / p, torch.zeros_like(p))


def loss_grad(logits, target, loss: str, out_act, dlogits=None, stats=None, grad_scale=1.0, idx=None):
    """Any ``lossesMap`` loss (a key of METRIC_KINDS) on ``act(logits)``, fp32 ``logits`` [B][C], in one launch
    (csrc/loss.hip): dlogits = grad_scale * dL/dlogits (bf16 on the GPU, rows of ``dlogits.shape[-1]`` elements);
    stats += [sum of the per-example loss, #correct].  ``target``: an int tensor [.] of classes (one-hot, clamped
    to the row) or a float tensor [., C] of dense targets; row b reads ``target[idx[b]]`` when ``idx`` (int64 [B])
    is given.  ``out_act``: "linear" | "softmax" | "sigmoid" (or 0 / 1 / 2).  Correct: argmax logits == the
    class, or == argmax of the dense target (first maximum).  ``logits`` / ``target`` / ``dlogits`` may be column
    slices ``buf[:, :C]`` of wider buffers.  The CPU path is the same closed forms in fp32 torch."""
    kind = METRIC_KINDS[loss]
    act = _out_act_code(out_act)
    B, C = logits.shape
    dense = target.is_floating_point()
    if dense and (target.dim() != 2 or target.shape[1] != C):
        raise ValueError(f"dense targets must be [., {C}], got {tuple(target.shape)}")
    if idx is None and target.shape[0] < B:
        raise ValueError(f"{target.shape[0]} target rows for {B} rows of logits")
    if logits.is_cuda:
        if dense:
            lab, tgt = None, (target if target.dtype == torch.float32 else target.float())
        else:
            lab, tgt = (target if target.dtype == torch.int32 else target.to(torch.int32)), None
        _C().loss_grad(logits, lab, tgt, idx, dlogits, stats, B, C, _ld(logits, C), _ld(tgt, C) if dense else C,
                       _ld(dlogits, C) if dlogits is not None else C, kind, act, float(grad_scale))
        return stats
    z = logits.float()
    tt = target if idx is None else target.index_select(0, idx.long().clamp(0, target.shape[0] - 1))
    tt = tt[:B]
    if dense:
        t = tt.float()
        ref_class = t.argmax(1)
    else:
        ref_class = tt.long().view(-1).clamp(0, C - 1)
        t = torch.nn.functional.one_hot(ref_class, C).float()
    p = torch.softmax(z, dim=1) if act == 1 else (torch.sigmoid(z) if act == 2 else z)
    terms, g = _loss_terms(kind, p, t)
    if dlogits is not None:
        dz = p * (g - (g * p).sum(1, keepdim=True)) if act == 1 else (g * p * (1 - p) if act == 2 else g)
        dlogits[:, :C].copy_((dz * grad_scale).to(dlogits.dtype))
    if stats is not None:
        stats[0] += terms.sum()
        stats[1] += (z.argmax(1) == ref_class).float().sum()
    return stats


IMAGE_LOSS_KINDS = 6  # the mean kinds of METRIC_KINDS, codes 0..5, are defined per pixel


def image_loss_plan(B: int, E: int, aligned: bool = True) -> dict:
    """The launch plan of :func:`image_loss_grad` for ``B`` images of ``E`` elements (csrc/loss_image.hip
    image_loss_plan, the function its launcher reads; needs no GPU): ``ok``, ``vec`` (a lane owns 8 adjacent
    elements; needs ``E % 8 == 0`` and ``aligned`` base pointers), ``threads``, ``elems_per_wg``,
    ``wgs_per_image``, ``grid`` and ``ws_floats`` (the fp32 workspace the loss sum needs)."""
    return dict(_C().image_loss_plan(int(B), int(E), bool(aligned)))


def image_loss_workspace_floats(B: int, E: int) -> int:
    return int(image_loss_plan(B, E)["ws_floats"])


def _image_loss_codes(loss: str, out_act):
    kind = METRIC_KINDS[loss]
    act = _out_act_code(out_act)
    if act == 1 or kind >= IMAGE_LOSS_KINDS:
        raise NotImplementedError(f"per-pixel softmax and class-map targets are not supported: loss {loss!r} with "
                                  f"output activation {out_act!r} on an image output (use one of the mean losses "
                                  f"{sorted(k for k, v in METRIC_KINDS.items() if v < IMAGE_LOSS_KINDS)} on a "
                                  f"linear or sigmoid output)")
    return kind, act


def image_loss_grad(z, target, loss: str, out_act, dz=None, stats=None, grad_scale=1.0, idx=None, target_scale=1.0,
                    workspace=None, out_relu=False):
    """A mean ``lossesMap`` loss (METRIC_KINDS codes 0..5) between ``act(z)`` and a target map, for a model whose
    output is an image: ``z`` [B, ...] (bf16 on the GPU, any trailing shape, viewed as [B][E]), per-example loss
    L_b = mean over the E elements.  dz = grad_scale * dL_b/dz (same shape as ``z``); stats[0] += sum_b L_b
    (stats[1], the accuracy count, is not defined for an image and is left alone).  ``target``: an fp32 table
    [N, ...], or a uint8 table read as ``u8 * target_scale``; image b reads ``target[idx[b]]`` (``idx`` int64 [B],
    clamped to the table) or row b.  ``out_act``: "linear" | "sigmoid".  ``out_relu``: ``z`` is the output of a
    fused ReLU (a model that ends in one), whose relu' (z > 0) multiplies dz.  One streaming launch on the GPU
    (csrc/loss_image.hip) plus the fixed-order sum of its per-workgroup partials in ``workspace`` (fp32,
    :func:`image_loss_workspace_floats`; required with ``stats``): the loss sum is bitwise reproducible.  The CPU
    path is the same closed forms in fp32 torch."""
    kind, act = _image_loss_codes(loss, out_act)
    B = int(z.shape[0])
    E = int(z.numel() // max(B, 1))
    if target.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"image targets must be fp32 or uint8, got {target.dtype}")
    if target.dim() < 1 or target.numel() % E or target.numel() // E != target.shape[0]:
        raise ValueError(f"image targets must be [N, ...] with {E} elements per row, got {tuple(target.shape)}")
    N = int(target.shape[0])
    if N < (1 if idx is not None else B):
        raise ValueError(f"{N} target rows for {B} images")
    if dz is not None and dz.numel() != z.numel():
        raise ValueError(f"dz must have the shape of z {tuple(z.shape)}, got {tuple(dz.shape)}")
    if z.is_cuda:
        if stats is not None and workspace is None:
            raise ValueError("image_loss_grad: stats needs a workspace (ops.image_loss_workspace_floats)")
        _C().image_loss_grad(z, target, idx, dz, stats, workspace if stats is not None else None, B, E, kind, act,
                             float(grad_scale), float(target_scale), bool(out_relu))
        return stats
    zz = z.reshape(B, E).float()
    tab = target.reshape(N, E)
    tt = (tab if idx is None else tab.index_select(0, idx.long().clamp(0, N - 1)))[:B]
    t = tt.float() * float(target_scale) if target.dtype == torch.uint8 else tt
    p = torch.sigmoid(zz) if act == 2 else zz
    terms, g = _loss_terms(kind, p, t)
    if dz is not None:
        d = g * p * (1 - p) if act == 2 else g
        if out_relu:
            d = d * (zz > 0)
        dz.copy_((d * grad_scale).to(dz.dtype).reshape(dz.shape))
    if stats is not None:
        stats[0] += terms.sum()
    return stats


def classifier_metrics(z, labels, loss: str, softmax, out):
    """[sum over the batch of the compiled loss, number correct] of fp32 model outputs ``z`` [B][C]
    against int labels (one launch on GPU, csrc/metrics.hip).  ``softmax``: the model output is
    softmax(z).  Returns ``out`` (device [2]); CPU uses the torch loss registry."""
    if z.is_cuda:
        # softmax: False / True (model ends in softmax) or the output activation name ("sigmoid")
        out_act = 2 if softmax == "sigmoid" else (1 if softmax in (True, "softmax") else 0)
        _C().classifier_metrics(z.contiguous(), labels.to(torch.int32).contiguous(), METRIC_KINDS[loss], out_act,
                                out)
        return out
    from ..losses import accuracy, get_loss

    if softmax == "sigmoid":
        p = torch.sigmoid(z.float())
    else:
        p = torch.softmax(z.float(), dim=1) if softmax in (True, "softmax") else z.float()
    onehot = torch.nn.functional.one_hot(labels.long(), z.shape[1]).float()
    out[0] = get_loss(loss)(onehot, p).sum()
    out[1] = accuracy(labels, p).sum()
    return out


def lenet_supported() -> bool:
    m = native.get(build_if_missing=False)
    return m is not None and hasattr(m, "lenet_train")


def lenet_frag_bytes() -> int:
    return int(_C().lenet_frag_bytes())


def lenet_blocks(B: int) -> int:
    return int(_C().lenet_blocks(int(B)))


_LENET_TABLES = {}


def lenet_dc2_class(oy: int, ox: int) -> int:
    """Bank class (physical row mod 8) of conv2 output position (oy, ox) in the dC2 block; also defined
    outside the 10x10 map, where it names the zero row a "no tap" lane of the data gradient reads."""
    return ((ox >> 1) + 7 * oy + 4 * (ox & 1)) % 8


def lenet_conv2_tables():
    """Host (numpy) form of the fused LeNet-5 kernel's conv2 index tables; ``t`` is the window-order row
    (window * 4 + position) of a conv2 output position inside an image's 104-row block, t = 100 .. 103 padding.
    ``place`` [104] -- t -> physical row of the image's dC2 block: position (oy, ox) lies at a row of class
    lenet_dc2_class(oy, ox) (rows class + 8 j, filled in t order), the padding rows take the rows left over;
    ``ftab`` [98][2][16] u8 -- conv2 data gradient: for pool1 pixel pair (y, X2), k-half and step s, the
    physical row of the position (oy, ox) = (y - ky, 2 X2 + 1 - u) it gathers, (ky, u) = divmod(2 s + half, 6);
    outside the map (and for the unused step 15) the zero code 128 + class: row ``class`` of the zero block;
    ``rowpix`` [104] -- physical row -> pool1 pixel of its position's window corner inside the image (the
    padding rows: pixel 0, read against a zero gradient);
    ``winpix`` [104] -- t -> the same pixel (conv2 forward, whose rows stay in window order)."""
    import numpy as np

    pos = {}
    for oy in range(10):
        for ox in range(10):
            pos[(((oy >> 1) * 5 + (ox >> 1)) << 2) + ((oy & 1) << 1) + (ox & 1)] = (oy, ox)
    place = np.full(104, -1, dtype=np.int64)
    fill = [0] * 8
    for t in range(100):
        c = lenet_dc2_class(*pos[t])
        place[t] = c + 8 * fill[c]
        fill[c] += 1
    assert max(fill) <= 13
    place[100:] = sorted(set(range(104)) - set(place[:100].tolist()))
    winpix = np.zeros(104, dtype=np.int64)
    for t, (oy, ox) in pos.items():
        winpix[t] = oy * 14 + ox
    rowpix = np.zeros(104, dtype=np.int64)
    rowpix[place] = winpix
    ft = np.zeros((98, 2, 16), dtype=np.uint8)
    for yx in range(98):
        y, X2 = divmod(yx, 7)
        for hf in range(2):
            for s in range(16):
                ky, u = divmod(2 * s + hf, 6)
                oy, ox = y - ky, 2 * X2 + 1 - u
                if ky < 5 and 0 <= oy < 10 and 0 <= ox < 10:
                    t = (((oy >> 1) * 5 + (ox >> 1)) << 2) + ((oy & 1) << 1) + (ox & 1)
                    ft[yx, hf, s] = place[t]
                else:
                    ft[yx, hf, s] = 128 + lenet_dc2_class(oy, ox)
    return place, ft, rowpix, winpix


def lenet_tables(device):
    """Constant index tables of the fused LeNet-5 kernel (built once per device, from lenet_conv2_tables):
    ``ftab`` [98][2][16] u8 -- phase F's gather table (physical dC2 rows and zero codes);
    ``pxtab`` [832 + 104] i16 -- [0, 832): physical dC2 row (image * 104 + row) -> pool1 pixel index
    image * 196 + rowpix[row], which phase E reads in physical row order; [832, 936): entry t =
    winpix[t] | place[t] << 8, the per-image tables of phase B (low byte) and phase D (high byte);
    ``frag`` -- scratch for the per-step conv and dense weight fragments (written by the kernel's prep launch)."""
    key = str(device)
    if key not in _LENET_TABLES:
        import numpy as np

        place, ft, rowpix, winpix = lenet_conv2_tables()
        px = np.concatenate([(np.arange(8)[:, None] * 196 + rowpix[None, :]).reshape(-1),
                             winpix | (place << 8)]).astype(np.int16)
        nbytes = int(_C().lenet_frag_bytes())
        _LENET_TABLES[key] = (torch.from_numpy(ft.reshape(-1)).to(device), torch.from_numpy(px).to(device),
                              torch.zeros(nbytes, dtype=torch.uint8, device=device))
    return _LENET_TABLES[key]


def lenet_dense_part_floats(B: int) -> int:
    return int(_C().lenet_dense_part_floats(int(B)))


def lenet_train(x, labels, conv, dense_w, dense_b, conv_grads, dense_gw, dense_gb, hT, dzT, conv_part,
                dense_part, loss_part, stats, grad_scale, frag=None, prep=True, snap=None, conv_mom=(), sgd=None):
    """Whole-network LeNet-5 training step on GPU (csrc/lenet_fused.hip, 2 launches): fills every
    gradient and ``stats`` = [loss sum, correct].  ``x``: bf16 batch [B,28,28,1] or a :class:`GatherRef`
    over a uint8 dataset; ``labels``: int32 [B] or a :class:`LabelRef` through the same indices.
    ``conv`` / ``dense_w`` / ``dense_b``: views of the fp32 master (the kernel reads every weight matrix
    from the fragment buffer; the prep launch builds it from these)."""
    if isinstance(x, GatherRef):
        src, idx, scale = x.data, x.idx, x.scale
    else:
        src, idx, scale = x.contiguous(), None, 1.0
    if isinstance(labels, LabelRef):
        lab, lidx = labels.labels, labels.idx
        if idx is None:
            idx = lidx
    else:
        lab = labels if labels.dtype == torch.int32 else labels.to(torch.int32)
    B = x.shape[0]
    ftab, pxtab, scratch = lenet_tables(stats.device)
    # ``frag``: the fragment buffer the optimizer rebuilds (ParamStore.lenet_frag), refreshed by the prep
    # launch only when ``prep``; None = prep into scratch.  It holds the conv and the dense fragments.
    # ``snap`` [2][2550]: the reduce kernel stores the conv kernels' weights and momentum (``conv_mom``)
    # there for the optimizer's rebuild.
    _C().lenet_train(src, idx, float(scale), lab, list(conv), list(dense_w), list(dense_b),
                     list(conv_grads), list(dense_gw), list(dense_gb), list(hT), list(dzT), conv_part, dense_part,
                     loss_part, stats, scratch if frag is None else frag, ftab, pxtab, int(B), float(grad_scale),
                     prep=bool(prep) or frag is None, snap=snap, conv_mom=list(conv_mom),
                     red_succ=_diag_on("lenet_succ"), **(sgd or {}))


def lenet_red_error(dense_part) -> int:
    """Sticky error word of the LeNet-5 reduce launch's granule hand-off (non-zero: a wait timed out)."""
    o = int(_C().lenet_red_err_offset())  # (layout: csrc/lenet_fused.hip lenet_red_bind_scratch)
    return int(dense_part[o:o + 1].view(torch.int32)[0].item())


def convpool_plan(H, W, C, KH, KW, pad, N, B=0, ws_floats=0) -> dict:
    """csrc/kernels.h CPPlan as a dict: ``ok``, the weight layouts, and per launch (``fwd``, ``wgrad``, ``dgrad``)
    the dispatch ``key``, the ``instance`` picked from the ``instantiated`` list and, with ``B`` on a GPU machine,
    ``imgs`` per group, ``grid`` and ``lds`` bytes (nothing is launched)."""
    return _C().convpool_plan(H, W, C, KH, KW, pad, N, B=B, ws_floats=ws_floats)


def convpool_supported(H, W, C, KH, KW, pad, N) -> bool:
    return native.get(build_if_missing=False) is not None and convpool_plan(H, W, C, KH, KW, pad, N)["ok"]


def convpool_fwd_layout(H, W, C, KH, KW, pad, N):
    """(channel stride Cp, row length Kpad2, pair) of the fused conv+pool forward weight layout."""
    return tuple(convpool_plan(H, W, C, KH, KW, pad, N)[k] for k in ("Cp", "Kpad2", "pair"))


def convpool_dgrad_layout(H, W, C, KH, KW, pad, N):
    """(pair, row length K2pad) of the fused conv+pool data-gradient weight layout."""
    return tuple(convpool_plan(H, W, C, KH, KW, pad, N)[k] for k in ("dgrad_pair", "K2pad"))


_cp_in = _kc_in


def convpool_fwd(x, w, bias, out, code, KH, KW, pad):
    """Fused conv(stride 1) + bias + ReLU + maxpool 2x2 -> pooled map ``out`` and argmax ``code``."""
    if x.is_cuda:
        src, idx, scale = _cp_in(x)
        _C().convpool_fwd(src, idx, scale, w, bias, out, code, list(ConvPoolGeom(*x.shape, KH, KW, pad, out.shape[-1])))
    else:
        if isinstance(x, GatherRef):
            x = (x.data.index_select(0, x.idx).float() * x.scale).reshape(x.shape)
        p, c = ref.convpool_fwd(x, w, bias, KH, KW, pad)
        out.copy_(p)
        if code is not None:
            code.copy_(c)
    return out


def convpool_wgrad(x, dp, code, gw, gb, workspace, KH, KW, pad, defer: list | None = None):
    """``defer``: a list to which the GPU path appends its split-m slab reduction instead of launching
    it; run them all with :func:`flush_slab_reductions` (one launch, bit-identical results)."""
    if code.is_cuda:
        src, idx, scale = _cp_in(x)
        g = ConvPoolGeom(*x.shape, KH, KW, pad, code.shape[-1])
        S = _C().convpool_wgrad(src, idx, scale, dp, code, gw, gb, workspace, list(g), defer is not None)
        if defer is not None and S > 0:
            K = g.KH * g.KW * g.C
            defer.append((workspace, gw.reshape(-1), gb, g.N, K, K + 1, int(S), 1.0))
    else:
        if isinstance(x, GatherRef):
            x = (x.data.index_select(0, x.idx).float() * x.scale).reshape(x.shape)
        g, b = ref.convpool_wgrad(x, dp, code, KH, KW, pad)
        gw.copy_(g.reshape(gw.shape))
        if gb is not None:
            gb.copy_(b)


def flush_slab_reductions(pending: list):
    """One launch for the deferred slab reductions in ``pending`` (emptied)."""
    for i in range(0, len(pending), 8):
        _C().slab_reduce_multi(pending[i:i + 8])
    pending.clear()


def convpool_dgrad(dp, code, w, wt, dx, KH, KW, pad):
    if code.is_cuda:
        _C().convpool_dgrad(dp, code, wt, dx, list(ConvPoolGeom(*dx.shape, KH, KW, pad, code.shape[-1])))
    else:
        dx.copy_(ref.convpool_dgrad(dp, code, w, dx.shape, KH, KW, pad))
    return dx


def gather_labels(labels, idx, out):
    if out.is_cuda:
        _C().gather_labels(labels, idx, out)
    else:
        out.copy_(labels.index_select(0, idx))
    return out
