"""The reference helpers of tests/exact_util.py themselves (CPU): the tie rule the max-pool helpers encode, the two
code conventions, agreement with torch's own pooling where no tie is possible; the saturated-head reference against
fp64 autograd of the same chain with the real softmax, and its exactness conditions at every shape the GPU tests use."""
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
