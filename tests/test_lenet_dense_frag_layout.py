"""Layout of the fused LeNet-5 step's dense weight fragments (csrc/lenet_frag.h), from the position maps
alone (no GPU): six matrices -- forward [N][K] and transposed [K][N] of the three dense layers -- behind
the 37 conv fragments of the fragment buffer, each as [tile of 16 rows][k-step of 32 columns] fragments of
64 lanes x 8 bf16."""
import torch

NK = [(120, 400), (84, 120), (10, 84)]
CONV_ELEMS = 37 * 64 * 8


def _maps():
    from distriflow_amd import native

    m = native.require()
    return [m.lenet_dense_frag_map(l) for l in range(3)], int(m.lenet_frag_bytes()) // 2


def test_every_weight_has_one_position_and_no_two_matrices_overlap():
    maps, total = _maps()
    seen = torch.zeros(total, dtype=torch.int32)
    for l, (fwd, tr) in enumerate(maps):
        N, K = NK[l]
        assert tuple(fwd.shape) == (N, K) and tuple(tr.shape) == (K, N)
        for mp in (fwd, tr):
            flat = mp.reshape(-1)
            assert int(flat.min()) >= CONV_ELEMS, "a dense element inside the conv fragments"
            assert int(flat.max()) < total, "a dense element outside lenet_frag_bytes()"
            assert flat.unique().numel() == flat.numel(), "two weights of one matrix share a position"
            seen.index_add_(0, flat, torch.ones_like(flat, dtype=torch.int32))
    assert int(seen.max()) == 1, "two matrices overlap"
    assert int(seen[:CONV_ELEMS].sum()) == 0
    assert int(seen.sum()) == 2 * sum(n * k for n, k in NK)


def test_forward_and_transposed_maps_cover_the_same_weights():
    """tr[k][n] is the transposed position of the weight whose forward position is fwd[n][k]; both follow
    the MFMA operand rule: row r, reduction column c -> fragment (r / 16) * KS + c / 32 of the matrix's
    range, lane 16 * ((c % 32) / 8) + r % 16, element c % 8."""
    maps, _ = _maps()
    starts = {}
    for l, (fwd, tr) in enumerate(maps):
        N, K = NK[l]
        for name, mp, R, C in (("fwd", fwd, N, K), ("tr", tr, K, N)):
            KS = (C + 31) // 32
            f0 = int(mp[0, 0]) // 512
            starts[(l, name)] = (f0, ((R + 15) // 16) * KS)
            r = torch.arange(R).view(R, 1).expand(R, C)
            c = torch.arange(C).view(1, C).expand(R, C)
            want = ((f0 + (r // 16) * KS + c // 32) * 64 + 16 * ((c % 32) // 8) + r % 16) * 8 + c % 8
            assert torch.equal(mp, want), f"layer {l} {name}"
    # the ranges in buffer order, back to back behind the conv fragments
    order = [(0, "fwd"), (1, "fwd"), (2, "fwd"), (2, "tr"), (1, "tr"), (0, "tr")]
    at = 37
    for key in order:
        f0, n = starts[key]
        assert f0 == at, f"{key} starts at fragment {f0}, expected {at}"
        at += n
    assert at * 512 == _maps()[1]
    assert [starts[k][1] for k in order] == [104, 24, 3, 6, 24, 100]


def test_activation_block_layout_is_a_permutation():
    """Transposed activation buffers [rows][ldt]: blocks of 16 rows x 32 columns in [row tile][k-step] order,
    piece (col % 32) / 8, row r % 16, element col % 8 -- a permutation of the buffer's elements in which the
    8 columns of a piece are consecutive and the 16 rows of a tile 16 bytes apart."""
    from distriflow_amd import native

    m = native.require()
    for rows, ldt in ((16, 32), (96, 64), (400, 160)):
        mp = m.lenet_act_map(rows, ldt)
        assert tuple(mp.shape) == (rows, ldt)
        assert torch.equal(mp.reshape(-1).sort().values, torch.arange(rows * ldt))
        r = torch.arange(rows).view(rows, 1).expand(rows, ldt)
        c = torch.arange(ldt).view(1, ldt).expand(rows, ldt)
        want = (((r // 16) * (ldt // 32) + c // 32) * 64 + 16 * ((c % 32) // 8) + r % 16) * 8 + c % 8
        assert torch.equal(mp, want)
