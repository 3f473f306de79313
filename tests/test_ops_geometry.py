"""distriflow_amd/ops/geometry.py: the descriptors' GEMM views against the raw arguments the call sites derived
by hand before the module existed (tests/golden/conv_plan.json), and the window arithmetic against the shapes
torch's own convolutions produce.  No GPU, no extension."""
import itertools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from distriflow_amd.ops.geometry import ConvGeom, DenseGeom, default_geom, pad_after, window

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")) as f:
    GOLDEN = json.load(f)
STRIDES = list(itertools.product((1, 2, 3), repeat=2))


def _conv(c):
    return ConvGeom.of(*(c[k] for k in ("B", "H", "W", "C", "OH", "OW", "N", "KH", "KW", "stride", "pad")))


def test_golden_forward_and_data_gradient_views():
    convs = [e for e in GOLDEN["entries"] if e["conv"] is not None]
    assert len(convs) == 286 and sum(e["conv"]["dgrad"] for e in convs) == 143
    for e in convs:
        c = e["conv"]
        v = _conv(c).dgrad(c["Kpad"]) if c["dgrad"] else _conv(c).fwd(c["Kpad"])
        assert v.plan == (e["M"], e["N"], e["K"], e["Kpad"], e["geom"], e["mode"]), e["name"]
        assert (v.lda, v.ldc, v.mode) == (0, e["N"], 2 if c["dgrad"] else 1), e["name"]
    dense = [e for e in GOLDEN["entries"] if e["mode"] == 0]
    assert len(dense) == 74 and all(e["conv"] is None and e["geom"] is None for e in dense)
    contiguous = 0
    for e in dense:  # x [M][K] -> [M][N]; the data gradient is the same GEMM with the layer's K and N exchanged
        fwd = e["name"].endswith("/fwd")
        assert fwd or e["name"].endswith("/dgrad"), e["name"]
        d = DenseGeom(e["M"], e["K"], e["N"]) if fwd else DenseGeom(e["M"], e["N"], e["K"])
        v = d.fwd(e["Kpad"]) if fwd else d.dgrad(e["Kpad"])
        assert v.plan == (e["M"], e["N"], e["K"], e["Kpad"], [1, 1, 1, 1, 1, 1, 1, 1, 0], 0), e["name"]
        assert (v.lda, v.ldc) == (e["K"], e["N"]), e["name"]
        contiguous += e["lda"] == v.lda
    assert contiguous == 73  # (one hand entry reads a column slice of a wider buffer: lda 124 for K 120)


def test_golden_weight_gradient_views():
    by_name = {e["name"]: e for e in GOLDEN["entries"]}
    paired = 0
    for w in GOLDEN["wgrad"]:
        want = tuple(w[k] for k in ("M", "N", "K", "ldd", "lda", "geom", "mode"))
        if w["geom"] is None:
            assert tuple(DenseGeom(w["M"], w["K"], w["N"]).wgrad()) == want[:5] + (default_geom(), 0), w["name"]
            continue
        stem = w["name"][:-len("/wgrad")] if w["name"].endswith("/wgrad") else w["name"]
        e = by_name.get(stem + "/fwd")
        if e is not None:  # the layer of the same model / batch / name
            g = _conv(e["conv"])
            paired += 1
        else:  # a hand entry of the weight gradient alone: the layer its own geometry list describes
            H, W, C, OH, OW, KH, KW, s, p = w["geom"][:9]
            sw, pl = w["geom"][9:] or (s, p)
            g = ConvGeom.of(w["M"] // (OH * OW), H, W, C, OH, OW, w["N"], KH, KW, (s, sw), (p, pl))
        assert tuple(g.wgrad()) == want, w["name"]
    assert len(GOLDEN["wgrad"]) == 173 and sum(w["geom"] is None for w in GOLDEN["wgrad"]) == 33 and paired >= 120


@pytest.mark.parametrize("padding", ["valid", "same"])
@pytest.mark.parametrize("strides", STRIDES, ids=lambda s: f"s{s[0]}{s[1]}")
def test_window_gives_the_shape_torch_convolves_to(strides, padding):
    sh, sw = strides
    for H, W, kh, kw in itertools.product(range(1, 11), range(1, 11), range(1, 6), range(1, 6)):
        if padding == "valid" and (kh > H or kw > W):
            with pytest.raises(ValueError):
                window(H, W, (kh, kw), strides, padding)
            continue
        OH, OW, pt, pl = window(H, W, (kh, kw), strides, padding)
        th, tw = max(pad_after(H, OH, kh, sh, 0), 0), max(pad_after(W, OW, kw, sw, 0), 0)
        if padding == "same":
            assert (OH, OW, pt, pl) == (-(-H // sh), -(-W // sw), th // 2, tw // 2)
        else:
            assert (pt, pl, th, tw) == (0, 0, 0, 0)
        x = F.pad(torch.ones(1, 1, H, W), (pl, tw - pl, pt, th - pt))
        y = F.conv2d(x, torch.ones(1, 1, kh, kw), stride=strides)
        assert tuple(y.shape[2:]) == (OH, OW), (H, W, kh, kw)


def test_window_explicit_padding_and_errors():
    assert window(8, 8, 3, 2, 1) == (4, 4, 1, 1)
    assert window(9, 8, (3, 5), (2, 1), (1, 2)) == (5, 8, 1, 2)
    for bad in ("full", "SAME"):
        with pytest.raises(ValueError):
            window(8, 8, 3, 1, bad)
    with pytest.raises(ValueError):
        window(8, 8, 3, 1, 1, keras_only="pooling")
    with pytest.raises(ValueError):
        window(2, 8, 5, 1, 1)


@pytest.mark.parametrize("strides", STRIDES, ids=lambda s: f"s{s[0]}{s[1]}")
def test_transposed_view(strides):
    sh, sw = strides
    for H, W, kh, kw in itertools.product(range(1, 7), range(1, 7), range(1, 5), range(1, 5)):
        g = ConvGeom.transposed(2, H, W, 3, 5, (kh, kw), strides, "valid")
        # Keras gives H * sh + max(KH - sh, 0) rows, torch (H - 1) * sh + KH: the same but for a kernel smaller
        # than its stride, where Keras keeps the sh - KH trailing rows no tap reaches (torch: output_padding)
        y = F.conv_transpose2d(torch.ones(1, 1, H, W), torch.ones(1, 1, kh, kw), stride=strides,
                               output_padding=(max(sh - kh, 0), max(sw - kw, 0)))
        assert (g.H, g.W) == tuple(y.shape[2:]), (H, W, kh, kw)
        s = ConvGeom.transposed(2, H, W, 3, 5, (kh, kw), strides, "same")
        assert (s.H, s.W) == (H * sh, W * sw)
        for t, pad in ((g, "valid"), (s, "same")):  # G's own forward window maps the output back to the input
            assert window(t.H, t.W, (kh, kw), strides, pad) == (H, W, t.pt, t.pl) == (t.OH, t.OW, t.pt, t.pl)
            assert (t.B, t.C, t.N, t.KH, t.KW, t.sh, t.sw) == (2, 5, 3, kh, kw, sh, sw)
            # the layer's three launches are G's data gradient, forward and weight gradient
            assert t.t_fwd(96) == t.dgrad(96) and t.t_dgrad(64) == t.fwd(64) and t.t_wgrad() == t.wgrad()
            assert t.t_fwd(96).plan[:3] == (2 * t.H * t.W, 5, kh * kw * 3) and t.t_fwd(96).mode == 2
            # the list ops.deconv_* take: the layer's own view [B, H, W, Cin, F, OH, OW, KH, KW, sh, sw, pt, pl]
            assert t.t_geom == (2, H, W, 3, 5, t.H, t.W, kh, kw, sh, sw, t.pt, t.pl) and t.t_geom.G == t
    with pytest.raises(ValueError):
        ConvGeom.transposed(1, 0, 4, 2, 2, (3, 3), (1, 1), "same")
    with pytest.raises(ValueError):
        ConvGeom.transposed(1, 4, 4, 2, 2, (3, 3), (1, 1), 1)


def test_descriptor_lists_and_regular():
    g = ConvGeom.build(2, 8, 8, 3, 4, 3, 2, "same")  # odd total: pad 0 top / left, 1 bottom / right
    assert (g.OH, g.OW, g.pad) == (4, 4, (0, 0)) and not g.symmetric and not g.regular
    r = ConvGeom.build(2, 8, 8, 3, 4, 3, 2, 1)
    assert r.regular and r.geom() == [8, 8, 3, 4, 4, 3, 3, 2, 1] and r.geom(swap=True) == [4, 4, 4, 8, 8, 3, 3, 2, 1]
    i = ConvGeom.build(2, 9, 8, 3, 4, (3, 5), (2, 1), "same")
    assert not i.regular and i.symmetric and i.geom() == [9, 8, 3, 5, 8, 3, 5, 2, 1, 1, 2]
    assert list(i) == [2, 9, 8, 3, 5, 8, 4, 3, 5, 2, 1, 1, 2]
