"""LDS layout of the conv2 output gradient (dC2) in the fused LeNet-5 train kernel (csrc/lenet_fused.hip), from
its index tables alone (no GPU): position (oy, ox) of an image lies at physical row ``place[t]`` of the image's
104-row block, a row of bank class ((ox >> 1) + 7 oy + 4 (ox & 1)) mod 8, and a data-gradient lane without a tap
reads the zero-block row of the class its out-of-range position would have had
(distriflow_amd.ops.lenet_conv2_tables, replayed by scripts/lds_sim.py)."""
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the 16-lane sets a ds_read_b128 is served in (lane = 16 g + i); in phase F the lanes with even g read the
# first 16 bytes of their row and the lanes with odd g the second 16 bytes: 8 lanes each
SERVICE = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
           list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
           list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
           list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
FPERM = [0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 4, 5, 6, 7]  # A row (pixel pair) of lane i in phase F


def _tables():
    from distriflow_amd import ops

    return ops.lenet_conv2_tables()


def _cls(oy, ox):
    return ((ox >> 1) + 7 * oy + 4 * (ox & 1)) % 8


def _trow(oy, ox):
    return (((oy >> 1) * 5 + (ox >> 1)) << 2) + ((oy & 1) << 1) + (ox & 1)


def _sim():
    spec = importlib.util.spec_from_file_location("lds_sim", os.path.join(ROOT, "scripts", "lds_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_place_is_a_bijection_with_the_formulas_classes():
    from distriflow_amd import ops

    place = _tables()[0]
    assert sorted(place.tolist()) == list(range(104))
    for oy in range(10):
        for ox in range(10):
            assert place[_trow(oy, ox)] % 8 == _cls(oy, ox) == ops.lenet_dc2_class(oy, ox), (oy, ox)
    assert sorted(_trow(oy, ox) for oy in range(10) for ox in range(10)) == list(range(100))


def test_ftab_names_the_placed_row_or_a_zero_code_of_the_positions_class():
    place, ft, _, _ = _tables()
    assert ft.shape == (98, 2, 16) and ft.dtype == np.uint8
    for yx in range(98):
        y, X2 = divmod(yx, 7)
        for hf in range(2):
            for s in range(16):
                ky, u = divmod(2 * s + hf, 6)
                oy, ox = y - ky, 2 * X2 + 1 - u
                e = int(ft[yx, hf, s])
                if ky < 5 and 0 <= oy < 10 and 0 <= ox < 10:
                    assert e == place[_trow(oy, ox)], (yx, hf, s)
                else:
                    assert e == 128 + _cls(oy, ox), (yx, hf, s)


def test_rows_served_together_are_distinct_mod_8():
    """Phase F, one workgroup of 8 images: 49 tiles x 15 steps x 4 service groups, each two sets of 8 lanes that
    read the same 16-byte half.  A set whose distinct rows are distinct mod 8 is conflict-free; the model
    (scripts/lds_sim.py) prices the rest at 96 conflict cycles of 3036, which is also what the committed
    output says."""
    _, ft, _, _ = _tables()
    bad_groups = total = 0
    for mt in range(49):
        for s in range(15):
            for grp in SERVICE:
                total += 1
                bad = False
                for half in range(2):
                    rows = []
                    for lane in grp:
                        i, g = lane & 15, lane >> 4
                        if (g & 1) != half:
                            continue
                        img, rem = divmod(16 * mt + FPERM[i], 98)
                        e = int(ft[rem, g >> 1, s])
                        # (block, row): a zero code's row in the zero block has its class; lanes that read
                        # the same row of the same block share one access
                        rows.append((img if e < 128 else -1, e & 127))
                    assert len(rows) == 8
                    bad |= len({r % 8 for _, r in set(rows)}) < len(set(rows))
                bad_groups += bad
    assert total == 49 * 15 * 4
    sim = _sim()
    ph = sim.Phase("F")
    sim.phase_f(ph)
    assert (ph.cyc, ph.cyc - ph.ideal) == (3036, 96)
    # every group with a repeated class costs at least one conflict cycle
    assert bad_groups <= ph.cyc - ph.ideal, bad_groups
    old = sim.Phase("F before")
    sim.phase_f(old, diag=False, perm=False)
    assert (old.cyc, old.cyc - old.ideal) == (5772, 2832)
    text = open(os.path.join(ROOT, "profiles", "lenet_conv2_layout", "lds_sim.txt")).read()
    m = re.search(r"^F conv2 dgrad \(A reads\)\s+instr\s+735\s+LDS cycles\s+(\d+)\s+conflict\s+(\d+)", text, flags=re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (3036, 96)


def test_model_tables_and_phase_e_reads():
    """The model replays the tables the kernel is given; phase E's dC2 reads in physical row order are
    conflict-free."""
    sim = _sim()
    sim.check_tables()
    a, b, x = sim.Phase("a"), sim.Phase("b"), sim.Phase("x")
    sim.phase_e(a, b, x)
    assert (a.cyc, a.cyc - a.ideal) == (416, 0)
    assert (b.cyc, b.cyc - b.ideal) == (2536, 1184)


def test_row_to_pixel_tables_invert_place():
    import torch

    from distriflow_amd import ops

    place, ft, rowpix, winpix = _tables()
    for oy in range(10):
        for ox in range(10):
            t = _trow(oy, ox)
            assert winpix[t] == oy * 14 + ox and rowpix[place[t]] == oy * 14 + ox
    assert (winpix[100:] == 0).all() and (rowpix[place[100:]] == 0).all()
    # what the kernel is given
    ftab, pxtab, _ = ops.lenet_tables(torch.device("cpu"))
    assert ftab.dtype == torch.uint8 and torch.equal(ftab, torch.from_numpy(ft.reshape(-1)))
    assert pxtab.dtype == torch.int16 and pxtab.numel() == 832 + 104
    px = pxtab.numpy().astype(np.int64)
    for img in range(8):
        assert (px[img * 104 + place] == img * 196 + winpix).all()
    assert ((px[832:] & 255) == winpix).all() and ((px[832:] >> 8) == place).all()
