"""The max-pool reference helpers of tests/exact_util.py themselves (CPU): the tie rule they encode, the two code
conventions, and agreement with torch's own pooling where no tie is possible."""
import torch

import exact_util as xu
from distriflow_amd import ops


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
