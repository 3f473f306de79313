"""Shapes of the sliding-window and GEMM launches, each stated once (pure Python, nothing native).

A layer builds one descriptor per batch size; the launch and every query about it (csrc/conv_plan.hip) take
their shape arguments from the same method of it, so the two cannot drift apart.  The int lists the native
bindings read are these tuples' fields in order: ``list(g)``."""
from __future__ import annotations

from collections import namedtuple

MODE_DIRECT, MODE_FWD, MODE_DGRAD = 0, 1, 2


def pair(v, default=None):
    if v is None:
        return default
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def out_hw(H, W, kernel, strides, pads):
    """Output size under symmetric padding ``pads`` = p or (ph, pw)."""
    (kh, kw), (sh, sw), (ph, pw) = pair(kernel), pair(strides), pair(pads)
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


def pad_after(n_in, n_out, k, s, before):
    """Bottom / right padding that ``n_out`` windows imply (negative: trailing pixels no window reads)."""
    return (n_out - 1) * s + k - n_in - before


def window(H, W, kernel, strides, padding, keras_only=None):
    """(OH, OW, pt, pl) of a ``kernel`` window sliding over H x W.  ``padding``: 'valid'; Keras / TF 'same'
    (output ceil(in / stride), total padding max((out - 1) * s + k - in, 0), the odd pixel bottom / right); or
    an explicit symmetric p / (ph, pw).  ``keras_only``: the name of an op that takes the two words only."""
    (kh, kw), (sh, sw) = pair(kernel), pair(strides)
    if isinstance(padding, str) and padding not in ("valid", "same") or keras_only and not isinstance(padding, str):
        raise ValueError(f"{keras_only or 'window'} padding {padding!r}")
    if padding == "same":
        OH, OW = -(-H // sh), -(-W // sw)
        pt, pl = max(pad_after(H, OH, kh, sh, 0), 0) // 2, max(pad_after(W, OW, kw, sw, 0), 0) // 2
    else:
        pt, pl = (0, 0) if padding == "valid" else pair(padding)
        OH, OW = out_hw(H, W, (kh, kw), (sh, sw), (pt, pl))
    if OH < 1 or OW < 1:
        raise ValueError(f"window {kh}x{kw} / strides {sh},{sw} / padding {padding!r} does not fit a {H}x{W} input")
    return OH, OW, pt, pl


# The shape arguments of ``igemm_fwd``, in its order; ``plan``: those of ``conv_plan``.
GemmView = namedtuple("GemmView", "M N K Kpad lda ldc geom mode")
GemmView.plan = property(lambda v: (v.M, v.N, v.K, v.Kpad, v.geom, v.mode))
# The shape arguments of ``igemm_wgrad`` and of ``wgrad_plan``, in their order.
WgradView = namedtuple("WgradView", "M N K ldd lda geom mode")


class ConvGeom(namedtuple("ConvGeom", "B H W C OH OW N KH KW sh sw pt pl")):
    """A conv from [B][H][W][C] to [B][OH][OW][N]: per-axis strides, top / left padding (the bottom / right
    padding is whatever the output size implies: asymmetric Keras 'same')."""

    @classmethod
    def of(cls, B, H, W, C, OH, OW, N, KH, KW, stride=1, pad=0):
        """From the sizes and ``stride`` = s or (sh, sw), ``pad`` = p or (top, left), as the conv ops take them."""
        return cls(*(int(v) for v in (B, H, W, C, OH, OW, N, KH, KW)), *pair(stride), *pair(pad))

    @classmethod
    def build(cls, B, H, W, C, N, kernel, strides, padding):
        OH, OW, pt, pl = window(H, W, kernel, strides, padding)
        return cls.of(B, H, W, C, OH, OW, N, *pair(kernel), strides, (pt, pl))

    @classmethod
    def transposed(cls, B, H, W, Cin, F, kernel, strides, padding):
        """The conv G of a Keras Conv2DTranspose from [B][H][W][Cin] to ``F`` filters: G maps the layer's output
        (G.H x G.W x F: H*sh + max(KH - sh, 0) rows for 'valid', H*sh for 'same') back to its input, with the
        same kernel size, strides and padding (no output_padding, no dilation)."""
        (kh, kw), (sh, sw) = pair(kernel), pair(strides)
        if min(int(B), int(H), int(W), int(Cin), int(F), kh, kw, sh, sw) < 1:
            raise ValueError(f"transposed conv: kernel {kh}x{kw} / strides {sh},{sw} / {F} filters on {H}x{W}x{Cin}")
        if padding not in ("valid", "same"):
            raise ValueError(f"transposed conv padding {padding!r}")
        grow = (0, 0) if padding == "same" else (max(kh - sh, 0), max(kw - sw, 0))
        g = cls.build(B, H * sh + grow[0], W * sw + grow[1], F, Cin, (kh, kw), (sh, sw), padding)
        if (g.OH, g.OW) != (H, W):
            raise ValueError(f"transposed conv: no {kh}x{kw} / {sh},{sw} {padding!r} conv maps {g.H}x{g.W} to {H}x{W}")
        return g

    args = property(lambda g: (*g[:9], g.stride, g.pad), doc="What :meth:`of` takes.")
    x_shape = property(lambda g: (g.B, g.H, g.W, g.C))
    y_shape = property(lambda g: (g.B, g.OH, g.OW, g.N))
    stride = property(lambda g: (g.sh, g.sw))
    pad = property(lambda g: (g.pt, g.pl))

    @property
    def symmetric(self) -> bool:
        """The padding is (pt, pl) on both sides: the output size confirms it."""
        return (self.OH, self.OW) == out_hw(self.H, self.W, (self.KH, self.KW), self.stride, self.pad)

    @property
    def regular(self) -> bool:
        """Square kernel, one stride, one symmetric padding (csrc set_conv_geom makes the same test): what the
        fused and specialised kernels match on."""
        return self.KH == self.KW and self.sh == self.sw and self.pt == self.pl and self.symmetric

    def geom(self, swap=False):
        """The native geometry list, source side first (``swap``: the data gradient reads the output side):
        9 ints when row and column stride / padding agree, else 11."""
        src, dst = (self.H, self.W, self.C), (self.OH, self.OW, self.N)
        if swap:
            src, dst = dst, src
        g = [*src, *dst[:2], self.KH, self.KW, self.sh, self.pt]
        return g if (self.sh, self.pt) == (self.sw, self.pl) else g + [self.sw, self.pl]

    def fwd(self, Kpad) -> GemmView:
        return GemmView(self.B * self.OH * self.OW, self.N, self.KH * self.KW * self.C, Kpad, 0, self.N, self.geom(),
                        MODE_FWD)

    def dgrad(self, Kpad) -> GemmView:
        return GemmView(self.B * self.H * self.W, self.C, self.KH * self.KW * self.N, Kpad, 0, self.C,
                        self.geom(swap=True), MODE_DGRAD)

    def wgrad(self) -> WgradView:
        M, N, K = self.fwd(0)[:3]
        return WgradView(M, N, K, N, 0, self.geom(), MODE_FWD)

    # A Conv2DTranspose runs G's three launches with their roles swapped: its forward is G's data gradient, its
    # input gradient G's forward, its kernel gradient G's with x and dy exchanged (x is G's output gradient).
    t_fwd, t_dgrad, t_wgrad = dgrad, fwd, wgrad
    t_geom = property(lambda g: DeconvGeom(g.B, g.OH, g.OW, g.N, g.C, g.H, g.W, *g[7:]))


# A Keras Conv2DTranspose from [B][H][W][Cin] to [B][OH][OW][F], as ``ops.deconv_*`` take it; ``G``: its conv.
DeconvGeom = namedtuple("DeconvGeom", "B H W Cin F OH OW KH KW sh sw pt pl")
DeconvGeom.G = property(lambda d: ConvGeom(d.B, d.OH, d.OW, d.F, d.H, d.W, d.Cin, *d[7:]))

default_geom = ConvGeom.of(0, 1, 1, 1, 1, 1, 0, 1, 1).geom  # () -> the list of a launch without a geometry: MODE_DIRECT


class DenseGeom(namedtuple("DenseGeom", "B K N")):
    """y [B][N] = x [B][K] @ W^T: plain GEMMs (MODE_DIRECT) with the row lengths as leading dimensions."""

    def fwd(self, Kpad) -> GemmView:
        return GemmView(self.B, self.N, self.K, Kpad, self.K, self.N, default_geom(), MODE_DIRECT)

    def dgrad(self, Kpad) -> GemmView:
        return GemmView(self.B, self.K, self.N, Kpad, self.N, self.K, default_geom(), MODE_DIRECT)

    def wgrad(self) -> WgradView:
        return WgradView(self.B, self.N, self.K, self.N, self.K, default_geom(), MODE_DIRECT)


class PoolGeom(namedtuple("PoolGeom", "B H W C OH OW ph pw sh sw pt pl")):
    """A Keras / TF pooling layer ('valid' | 'same'); the list of ``pool2d_fwd`` / ``pool2d_bwd``."""

    @classmethod
    def build(cls, B, H, W, C, pool, strides, padding):
        OH, OW, pt, pl = window(H, W, pool, strides, padding, "pooling")
        return cls(int(B), int(H), int(W), int(C), OH, OW, *pair(pool), *pair(strides), pt, pl)

    pb = property(lambda g: pad_after(g.H, g.OH, g.ph, g.sh, g.pt))
    pr = property(lambda g: pad_after(g.W, g.OW, g.pw, g.sw, g.pl))


class DwGeom(namedtuple("DwGeom", "B H W C M OH OW KH KW sh sw pt pl")):
    """A Keras DepthwiseConv2D with ``M`` filters per channel ('valid' | 'same'); the list of ``dwconv_*``."""

    @classmethod
    def build(cls, B, H, W, C, M, kernel, strides, padding):
        if M < 1:
            raise ValueError(f"depthwise conv: {M} filters per channel")
        OH, OW, pt, pl = window(H, W, kernel, strides, padding, "depthwise conv")
        return cls(int(B), int(H), int(W), int(C), int(M), OH, OW, *pair(kernel), *pair(strides), pt, pl)


# UpSampling2D of [B][H][W][C] by (sh, sw): the list of ``upsample2d_*``; and the list of the fused conv (stride 1,
# symmetric ``pad``) + 2x2 max-pool kernels (csrc/convpool.hip).
UpGeom = namedtuple("UpGeom", "B H W C sh sw")
ConvPoolGeom = namedtuple("ConvPoolGeom", "B H W C KH KW pad N")
