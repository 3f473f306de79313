"""The reference helpers of tests/exact_util.py themselves (CPU): the tie rule the max-pool helpers encode, the two
code conventions, agreement with torch's own pooling where no tie is possible; the saturated-head reference against
fp64 autograd of the same chain with the real softmax, and its exactness conditions at every shape the GPU tests use;
the conv (any ConvGeom), transposed conv and depthwise conv references against a four-loop tap sum and ops.reference,
and the conditions of exactness of every case of the irregular, transposed and depthwise exact GPU tests."""
import pytest
import torch

import exact_util as xu
from distriflow_amd import ops
from distriflow_amd.ops import reference as ref


def test_window_argmax_takes_the_first_maximum():
    win = torch.tensor([[1., 3., 3., 2.], [0., 0., 0., 0.], [-2., -1., -1., -3.], [5., 1., 5., 5.], [1., 2., 3., 4.]]).double()
    m, am = xu.window_argmax(win)
    assert m.tolist() == [3, 0, -1, 5, 4] and am.tolist() == [1, 0, 1, 0, 3]
    assert xu.code_convpool(m, am).tolist() == [5, 0, 1, 4, 7]
    assert xu.code_relu4(m, am).tolist() == [1, 4, 4, 0, 3]


def test_windows_are_row_major_and_drop_the_remainder():
    y = torch.arange(5 * 7, dtype=torch.float64).view(1, 5, 7, 1)
    w = xu.windows(y)
    assert w.shape == (1, 2, 3, 1, 4)
    assert w[0, 1, 2, 0].tolist() == [y[0, 2, 4, 0], y[0, 2, 5, 0], y[0, 3, 4, 0], y[0, 3, 5, 0]]


def test_unpool_ref_places_by_code():
    dyp = torch.tensor([2., 3., 5., 7.]).view(1, 1, 4, 1)
    full = xu.unpool_ref(dyp, torch.tensor([1, 4, 3, 2], dtype=torch.uint8).view(1, 1, 4, 1), 3, 9, "relu4")
    assert full.shape == (1, 3, 9, 1) and float(full.abs().sum()) == 2 + 5 + 7
    assert full[0, 0, 1, 0] == 2 and full[0, 1, 5, 0] == 5 and full[0, 1, 6, 0] == 7
    full = xu.unpool_ref(dyp, torch.tensor([5, 1, 7, 4], dtype=torch.uint8).view(1, 1, 4, 1), 2, 8, "convpool")
    assert float(full.abs().sum()) == 2 + 5 + 7
    assert full[0, 0, 1, 0] == 2 and full[0, 1, 5, 0] == 5 and full[0, 0, 6, 0] == 7


def test_pool_max_ref_agrees_with_torch_without_ties_and_sums_overlaps():
    g = xu.gen(1)
    B, H, W, C = 2, 9, 7, 3
    x = torch.randperm(B * H * W * C, generator=g).double().view(B, H, W, C) - 100
    for pool, stride, pad in (((3, 3), (2, 2), "same"), ((2, 3), (2, 1), "valid"), ((2, 2), (2, 2), "valid")):
        geom = ops.pool_geometry(B, H, W, C, pool, stride, pad)
        y = xu.pool_max_ref(x, geom)[0]
        assert torch.equal(y, ops._pool_ref(x, geom, False).double())
        dy = xu.ints(g, y.shape, -3, 3)
        xv = x.clone().requires_grad_(True)
        (gr,) = torch.autograd.grad(ops._pool_ref(xv, geom, False), xv, dy.float())
        assert torch.equal(xu.pool_max_bwd_ref(x, dy, geom, False), gr.double())
    # all equal: every window's first element is its top-left pixel inside the image
    geom = ops.pool_geometry(1, 4, 4, 1, (3, 3), (1, 1), "same")
    dx = xu.pool_max_bwd_ref(torch.zeros(1, 4, 4, 1), torch.ones(1, 4, 4, 1), geom, False)
    assert dx[0, :, :, 0].tolist() == [[4, 2, 2, 0], [2, 1, 1, 0], [2, 1, 1, 0], [0, 0, 0, 0]]
    assert float(xu.pool_max_bwd_ref(torch.zeros(1, 4, 4, 1), torch.ones(1, 4, 4, 1), geom, True).abs().sum()) == 0


# ------------------------------------------------------------------------------- the saturated-head reference
def _autograd_head(d, grad_scale, drop, x_relu, dx_scale):
    """fp64 autograd of the same chain with the REAL softmax (F.cross_entropy)."""
    x = d["x"].clone().requires_grad_(True)
    W = [w.clone().requires_grad_(True) for w in d["W"]]
    b = [None if v is None else v.clone().requires_grad_(True) for v in d["b"]]
    h, nl = x, len(W)
    for l in range(nl):
        h = h @ W[l].t() + (b[l] if b[l] is not None else 0)
        if l < nl - 1:
            h = h.relu()
            if drop is not None and l == nl - 2:
                keep = ref.dropout_mask(h.numel(), drop[0], drop[1] ^ (drop[2] * 0x9E3779B1)).double().view_as(h)
                h = h * keep / (1 - drop[0])
    loss = torch.nn.functional.cross_entropy(h, d["y"], reduction="sum")
    (loss * grad_scale).backward()
    dx = x.grad * (d["x"] > 0) if x_relu else x.grad
    return h.detach(), loss.detach(), dx * dx_scale, [w.grad for w in W], [None if v is None else v.grad for v in b]


def _check_ref_against_autograd(d, r, drop, x_relu, dx_scale):
    xu.assert_exact_head(r)
    logits, loss, dx, gw, gb = _autograd_head(d, xu.HEAD_GRAD_SCALE, drop, x_relu, dx_scale)
    tight = dict(rtol=0, atol=1e-40)   # the two differ by the fp64 exp tail alone (<= e^-104)
    assert torch.equal(r["logits"], logits)
    torch.testing.assert_close(r["stats"][0], loss, **tight)
    torch.testing.assert_close(r["dx"], dx, **tight)
    for l in range(len(gw)):
        torch.testing.assert_close(r["gw"][l], gw[l], **tight)
        if gb[l] is not None:
            torch.testing.assert_close(r["gb"][l], gb[l], **tight)
    assert float(r["stats"][1]) == float((logits.argmax(1) == d["y"]).sum())
    assert torch.equal(r["loss_part"].sum(0), r["stats"])


@pytest.mark.parametrize("case", xu.KHEAD_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_head_ref_matches_autograd_khead_cases(case):
    d, r = xu.khead_case(*case)
    _check_ref_against_autograd(d, r, xu.HEAD_DROP if case[3] else None, True, 0.5)
    assert r["dx"].shape == (case[0], case[1]) and len(r["loss_part"]) == (case[0] + 15) // 16


@pytest.mark.parametrize("case", xu.MLPHEAD_CASES, ids=lambda c: f"{c[0]}-" + "x".join(map(str, c[1])))
def test_head_ref_matches_autograd_mlphead_cases(case):
    d, r = xu.mlphead_case(*case)
    _check_ref_against_autograd(d, r, None, case[3], case[4])


def test_head_ref_without_bias_and_mask():
    d, r = xu.khead_case(40, 512, 10, False, False, bias=False, dp_mask=False)
    assert all(v is None for v in d["b"])
    _check_ref_against_autograd(d, r, None, False, 0.5)


def test_head_ref_takes_the_first_maximum_and_its_conditions_bite():
    d, r = xu.khead_case(33, 256, 10, False, False)
    assert torch.equal(r["argmax"], r["logits"].argmax(1))  # unique maxima: any rule agrees
    bad = dict(r, logits=r["logits"].clone())
    bad["logits"][5] = 128.0 * torch.tensor([3., 3, 0, 0, 0, 0, 0, 0, 0, 0])
    with pytest.raises(AssertionError, match="gap"):
        xu.assert_exact_head(bad)
    bad = dict(r, dx=r["dx"] + 1.0 / 1024)
    with pytest.raises(AssertionError, match="bf16"):
        xu.assert_exact_head(bad)


# ------------------------------------------------------- irregular, transposed and depthwise conv references
# Each reference against (1) a direct four-loop tap sum written here, by torch.equal, and (2) ops.reference (fp32,
# tied to Keras semantics by tests/test_conv_geometry.py) on the same integers with atol = 1e-3: two integer
# results that differ at all differ by at least 1, so that is a condition, not a tolerance.  Then the conditions
# under which the GPU tests may compare by torch.equal, for every case they run.
INT = dict(atol=1e-3, rtol=0)
# lower bounds on the share of exact zeros (igemm data: masks in {-1, 0, 1} are zero a third of the time; depthwise
# masks in [-2, 2] a fifth; a pre-ReLU sum of some tens of terms of +-1 is zero a few percent of the time)
MASK_ZEROS_IGEMM, MASK_ZEROS_DW, SUM_ZEROS = 0.25, 0.15, 0.01


def _tap_loop(x, w4, dy, g):
    """Forward, data gradient and weight gradient of a conv by the definition: y[b, oh, ow, n] = sum over (kh, kw)
    with ih = oh*sh - pt + kh and iw = ow*sw - pl + kw inside the image of x[b, ih, iw, :] . w4[n, kh, kw, :]."""
    B = x.shape[0]
    y, dx, gw = torch.zeros(B, g.OH, g.OW, g.N).double(), torch.zeros(B, g.H, g.W, g.C).double(), torch.zeros_like(w4)
    for oh in range(g.OH):
        for ow in range(g.OW):
            for kh in range(g.KH):
                for kw in range(g.KW):
                    ih, iw = oh * g.sh - g.pt + kh, ow * g.sw - g.pl + kw
                    if 0 <= ih < g.H and 0 <= iw < g.W:
                        y[:, oh, ow] += x[:, ih, iw] @ w4[:, kh, kw].t()
                        dx[:, ih, iw] += dy[:, oh, ow] @ w4[:, kh, kw]
                        gw[:, kh, kw] += dy[:, oh, ow].t() @ x[:, ih, iw]
    return y, dx, gw.reshape(g.N, -1)


def _check_conv_refs(g, x, w, b, dy):
    """The three conv references of the ConvGeom ``g`` on x [B][H][W][C], dy [B][OH][OW][N], w [N][KH*KW*C]."""
    y, dx, gw = _tap_loop(x, w.view(g.N, g.KH, g.KW, g.C), dy, g)
    ry, rdx = xu.conv_fwd_ref(x, w, None, g), xu.conv_dgrad_ref(dy, w, g.x_shape, g)
    rgw, rgb, rab = xu.conv_wgrad_ref(dy, x, g)
    assert torch.equal(ry, y) and torch.equal(rdx, dx) and torch.equal(rgw, gw)
    assert torch.equal(rgb, dy.reshape(-1, g.N).sum(0)) and bool((rab >= rgw.abs()).all())
    assert torch.equal(xu.conv_fwd_ref(x, w, b, g, relu=True), (y + b).relu())
    geo = (g.KH, g.KW, g.stride, g.pad)
    torch.testing.assert_close(ry, ref.conv_fwd(x.float(), w.float(), None, *geo, False, out_hw=(g.OH, g.OW)).double(), **INT)
    torch.testing.assert_close(rdx, ref.conv_dgrad(dy.float(), w.float(), g.x_shape, *geo).double(), **INT)
    ow_, ob_ = ref.conv_wgrad(dy.float(), x.float(), *geo)
    torch.testing.assert_close(rgw, ow_.double(), **INT)
    torch.testing.assert_close(rgb, ob_.double(), **INT)
    return ry, rdx, rab


def test_conv_refs_keep_their_k_s_p_form():
    """Existing callers pass one k, one s, one symmetric p: the same values as torch's own unfold with padding p,
    trailing pixels that no window reads included ((9 + 2 - 3) % 2 == 0 but (8 + 2 - 3) % 2 != 0)."""
    r = xu.gen(3)
    for (B, H, W, C, N, k, s, p) in ((2, 9, 8, 3, 4, 3, 2, 1), (2, 7, 6, 2, 5, 4, 2, 1), (1, 6, 6, 3, 2, 2, 3, 0)):
        x, w = xu.ints(r, (B, H, W, C), -2, 2), xu.ints(r, (N, k * k * C), -2, 2)
        OH, OW = xu.out_hw(H, W, k, s, p)
        dy = xu.ints(r, (B, OH, OW, N), -2, 2)
        g = xu.conv_geom(x.shape, N, k, s, p)
        assert (g.OH, g.OW) == (OH, OW) and g.pad == (p, p)
        y, dx, gw = _tap_loop(x, w.view(N, k, k, C), dy, g)
        assert torch.equal(xu.conv_fwd_ref(x, w, None, k, s, p, False), y)
        assert torch.equal(xu.conv_dgrad_ref(dy, w, (B, H, W, C), k, s, p), dx)
        assert torch.equal(xu.conv_wgrad_ref(dy, x, k, s, p)[0], gw)


def test_conv_dgrad_ref_is_zero_where_no_window_reads():
    """A 2x2 kernel at stride 3 under 'same': every third row and column is read by no window."""
    d = xu.conv_case((5, 7, 7, 1, 8, (2, 2), (3, 3), "same"))
    g = d["g"]
    assert (g.OH, g.OW, g.pt, g.pl) == (3, 3, 0, 0)
    dx = xu.conv_dgrad_ref(d["dy"], d["w"], g.x_shape, g)
    assert float(dx[:, 2::3].abs().sum()) == 0 and float(dx[:, :, 2::3].abs().sum()) == 0 and float(dx.abs().sum()) > 0


@pytest.mark.parametrize("case", xu.IRREGULAR_CONVS, ids=xu.case_id)
def test_irregular_conv_refs_and_conditions(case):
    d = xu.conv_case(case)
    g, x, w, b, dy = d["g"], d["x"], d["w"], d["b"], d["dy"]
    assert not g.regular
    y, dx, ab = _check_conv_refs(g, x, w, b, dy)
    for t in (y, y + b, dx, xu.join_ref(dx, d["res"], d["rmask"], d["mask"])):
        xu.assert_exact_output(t)
    assert float(ab.max()) < xu.FP32_INT_MAX and float(dy.abs().sum((0, 1, 2)).max()) < xu.FP32_INT_MAX
    print(f"max |y| {float((y + b).abs().max())}, max |dx| {float(dx.abs().max())}; zeros: mask "
          f"{xu.zero_share(d['mask']):.3f} rmask {xu.zero_share(d['rmask']):.3f} y + b {xu.zero_share(y + b):.3f}")
    assert min(xu.zero_share(d["mask"]), xu.zero_share(d["rmask"])) >= MASK_ZEROS_IGEMM
    assert xu.zero_share(y + b) >= SUM_ZEROS
    # the mask rule bites: somewhere mask == 0 sits on a non-zero gradient
    assert bool(((d["mask"] == 0) & (dx + d["res"] * (d["rmask"] > 0) != 0)).any())


@pytest.mark.parametrize("case", xu.DECONVS, ids=xu.case_id)
def test_deconv_refs_and_conditions(case):
    d = xu.deconv_case(case)
    G, x, w, b, dy = d["G"], d["x"], d["w"], d["b"], d["dy"]
    assert tuple(d["geom"]) == tuple(ops.deconv_geometry(*case))
    # the conv G on (its input = dy, its output gradient = x), then the roles swapped
    gy, gdx, _ = _check_conv_refs(G, dy, w, torch.zeros(G.N).double(), x)
    y = xu.deconv_fwd_ref(x, w, None, d["geom"], False)
    assert torch.equal(y, gdx.reshape(y.shape))
    assert torch.equal(xu.deconv_fwd_ref(x, w, b, d["geom"], True), (gdx + b).relu())
    assert torch.equal(xu.deconv_dgrad_ref(dy, w, d["geom"], None), gy)
    assert torch.equal(xu.deconv_dgrad_ref(dy, w, d["geom"], x), gy * (x > 0))
    gw, gb, ab = xu.deconv_wgrad_ref(dy, x, d["geom"])
    assert torch.equal(gw, xu.conv_wgrad_ref(x, dy, G)[0]) and torch.equal(gb, dy.reshape(-1, G.C).sum(0))
    # ops' own CPU path of the three launches
    oy = ops.deconv_fwd(x.float(), w.float(), None, b.float(), torch.empty(y.shape), d["geom"])
    odx = ops.deconv_dgrad(dy.float(), w.float(), torch.empty(gy.shape), d["geom"], mask=x.float())
    torch.testing.assert_close(y + b, oy.double(), **INT)
    torch.testing.assert_close(gy * (x > 0), odx.double(), **INT)
    ogw, ogb = torch.empty(gw.shape), torch.empty(G.C)
    ops.deconv_wgrad(dy.float(), x.float(), ogw, ogb, None, d["geom"])
    torch.testing.assert_close(gw, ogw.double(), **INT)
    torch.testing.assert_close(gb, ogb.double(), **INT)
    for t in (y, y + b, gy):
        xu.assert_exact_output(t)
    assert float(ab.max()) < xu.FP32_INT_MAX and float(dy.abs().sum((0, 1, 2)).max()) < xu.FP32_INT_MAX
    print(f"max |y| {float((y + b).abs().max())}, max |dx| {float(gy.abs().max())}; zeros: mask {xu.zero_share(x):.3f} "
          f"y + b {xu.zero_share(y + b):.3f}")
    if x.numel() >= 512:
        assert xu.zero_share(x) >= MASK_ZEROS_IGEMM
    if y.numel() >= 512:
        assert xu.zero_share(y + b) >= SUM_ZEROS
    assert bool(((x == 0) & (gy != 0)).any()) or x.numel() < 64


def test_case_lists_begin_with_the_tolerance_tests_cases():
    import test_decoder_gpu
    import test_depthwise_gpu
    import test_conv_geometry_gpu

    assert xu.DECONVS[:9] == test_decoder_gpu.CASES and len(xu.DECONVS) == 16
    assert xu.DWCONVS == test_depthwise_gpu.CASES and len(xu.DWCONVS) == 15
    assert xu.IRREGULAR_CONVS[:5] == test_conv_geometry_gpu.GEOMS and len(xu.IRREGULAR_CONVS) == 9


def _dw_tap_loop(x, w, dy, g):
    B, CO = x.shape[0], g.C * g.M
    xr = x.repeat_interleave(g.M, dim=3)   # channel co reads input co // M
    y, dxr, gw = torch.zeros(B, g.OH, g.OW, CO).double(), torch.zeros(B, g.H, g.W, CO).double(), torch.zeros_like(w)
    for oh in range(g.OH):
        for ow in range(g.OW):
            for kh in range(g.KH):
                for kw in range(g.KW):
                    ih, iw = oh * g.sh - g.pt + kh, ow * g.sw - g.pl + kw
                    if 0 <= ih < g.H and 0 <= iw < g.W:
                        y[:, oh, ow] += xr[:, ih, iw] * w[kh, kw]
                        dxr[:, ih, iw] += dy[:, oh, ow] * w[kh, kw]
                        gw[kh, kw] += (dy[:, oh, ow] * xr[:, ih, iw]).sum(0)
    return y, dxr.view(B, g.H, g.W, g.C, g.M).sum(-1), gw


def _check_dw_refs(d):
    g, x, w, b, dy = d["geom"], d["x"], d["w"], d["b"], d["dy"]
    y, dx, gw = _dw_tap_loop(x, w, dy, g)
    ry, rdx = xu.dwconv_fwd_ref(x, w, None, g), xu.dwconv_dgrad_ref(dy, w, g)
    rgw, rgb, rab = xu.dwconv_wgrad_ref(dy, x, g)
    assert torch.equal(ry, y) and torch.equal(rdx, dx) and torch.equal(rgw, gw)
    assert torch.equal(rgb, dy.sum((0, 1, 2))) and bool((rab >= rgw.abs()).all())
    assert torch.equal(xu.dwconv_fwd_ref(x, w, b, g, True), (y + b).relu())
    assert torch.equal(xu.dwconv_dgrad_ref(dy, w, g, x), dx * (x > 0))
    torch.testing.assert_close(ry + b, ref.dwconv_fwd(x.float(), w.float(), b.float(), g).double(), **INT)
    torch.testing.assert_close(rdx * (x > 0), ref.dwconv_dgrad(dy.float(), w.float(), g, x.float()).double(), **INT)
    ow_, ob_ = ref.dwconv_wgrad(dy.float(), x.float(), g, True)
    torch.testing.assert_close(rgw, ow_.double(), **INT)
    torch.testing.assert_close(rgb, ob_.double(), **INT)
    return ry, rdx, rab


@pytest.mark.parametrize("case", xu.DWCONVS, ids=xu.case_id)
def test_dwconv_refs_and_conditions(case):
    d = xu.dw_case(case)
    g, x, b, dy = d["geom"], d["x"], d["b"], d["dy"]
    y, dx, ab = _check_dw_refs(d)
    T = g.KH * g.KW
    assert float((y + b).abs().max()) <= T * 6 + 3 <= xu.BF16_INT_MAX and float(dx.abs().max()) <= T * g.M * 6 <= xu.BF16_INT_MAX
    for t in (y, y + b, dx):
        xu.assert_exact_output(t)
    assert float(ab.max()) < xu.FP32_INT_MAX and float(dy.abs().sum((0, 1, 2)).max()) < xu.FP32_INT_MAX
    print(f"max |y| {float((y + b).abs().max())}, max |dx| {float(dx.abs().max())}; zeros: mask {xu.zero_share(x):.3f} "
          f"y + b {xu.zero_share(y + b):.3f}")
    if x.numel() >= 512:
        assert xu.zero_share(x) >= MASK_ZEROS_DW and xu.zero_share(y + b) >= SUM_ZEROS
        assert bool(((x == 0) & (dx != 0)).any())


@pytest.mark.parametrize("M", [1, 2])
def test_dwconv_refs_with_a_depth_multiplier_and_unread_pixels(M):
    """M = 1 and M = 2 on a geometry with asymmetric 'same' padding, and on one whose stride exceeds the kernel."""
    for case in ((2, 8, 7, 3, M, (3, 2), (2, 1), "same"), (2, 7, 7, 2, M, (2, 2), (3, 3), "same")):
        _, dx, _ = _check_dw_refs(xu.dw_case(case))
    assert float(dx[:, 2::3].abs().sum()) == 0 and float(dx[:, :, 2::3].abs().sum()) == 0 and float(dx.abs().sum()) > 0


@pytest.mark.parametrize("case", xu.DWCONVS_GRID, ids=xu.case_id)
def test_dwconv_grid_stride_cases_stride_and_stay_exact(case):
    """The large cases, bounded from the value ranges alone (x, dy in [-2, 2], w, bias in [-3, 3]): |y| <= 9*6 + 3,
    |dx| <= 9*M*6, every weight-gradient sum below 4 * positions; and each launch it is there for does stride."""
    g = ops.dwconv_geometry(*case)
    T, P = g.KH * g.KW, g.B * g.OH * g.OW
    assert T * 6 + 3 <= xu.BF16_INT_MAX and T * g.M * 6 <= xu.BF16_INT_MAX and 4 * P < xu.FP32_INT_MAX
    assert g.B * max(g.H * g.W * g.C, g.OH * g.OW * g.C * g.M) <= 10 << 20
    fwd, dg, wg, PL = xu.dw_work_items(g)
    print(f"work items: forward {fwd}, data gradient {dg}, weight gradient {wg} at {PL} lanes per slab")
    if case == xu.DWCONVS_GRID[0]:
        assert fwd == dg == 525312 > xu.DW_GRID_ITEMS and xu.DW_GRID_ITEMS % (g.C // 8) == 2
        assert PL == 28 and -(-wg // PL) > 1024
    elif case == xu.DWCONVS_GRID[1]:
        assert (fwd, dg) == (1081344, 540672) and dg > xu.DW_GRID_ITEMS
    else:
        assert PL == 1 and wg == 1058 > 1024
